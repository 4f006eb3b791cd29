"""CPU: the proof that the checks of tests/test_gpu_attn_edges.py can fail, and that a correct kernel passes them.

For every case of the GPU file's tables (tests/attn_bounds.py: ATTN_CASES, XATTN_CASES), on the same seeded
inputs:
  * the bf16 emulation of the kernels' documented rounding points stays within C E on every element of
    every output (and within EMUL_MAX, the recorded maximum C is twice of);
  * every applicable mutant (a deliberately wrong algorithm, float64) exceeds C E on each output named for
    it in MUTANT_OUTPUTS, separately in every group of the launch in which it changes anything: a kernel
    with that bug at that length would fail the GPU check.
The float64 reference itself is checked against float64 autograd, and the attention entry points must
reject a q / k / v column offset that is no multiple of 8 before any launch.
"""

import os

import numpy as np
import pytest
import torch

import attn_bounds as ab

OUTS = ("o", "dq", "dk", "dv")
_ids = lambda c: c.name  # noqa: E731


def _emulation_ratios(variant_fn, case):
    ex, em = variant_fn(case), variant_fn(case, "emul")
    return {n: ab.assert_within(em[n], ex[n], ex["E_" + n], f"{case.name} emulated {n}") for n in OUTS}


@pytest.mark.parametrize("case", ab.ATTN_CASES, ids=_ids)
def test_attn_emulation_within_bound(case):
    for n, r in _emulation_ratios(ab.attn_variant, case).items():
        assert r <= ab.EMUL_MAX, f"{case.name} {n}: emulation ratio {r:.4f} above the recorded maximum {ab.EMUL_MAX}"


@pytest.mark.parametrize("case", ab.XATTN_CASES, ids=_ids)
def test_xattn_emulation_within_bound(case):
    for n, r in _emulation_ratios(ab.xattn_variant, case).items():
        assert r <= ab.EMUL_MAX, f"{case.name} {n}: emulation ratio {r:.4f} above the recorded maximum {ab.EMUL_MAX}"


def test_recorded_constant():
    """C = 2 EMUL_MAX, and EMUL_MAX is the measured maximum over every case, rounded up to 3 places."""
    worst = max(max(_emulation_ratios(fn, c).values())
                for fn, cases in ((ab.attn_variant, ab.ATTN_CASES), (ab.xattn_variant, ab.XATTN_CASES)) for c in cases)
    assert ab.C == 2 * ab.EMUL_MAX
    assert ab.EMUL_MAX - 1e-3 <= worst <= ab.EMUL_MAX, worst


@pytest.mark.parametrize("case", ab.ATTN_CASES, ids=_ids)
def test_attn_mutants_caught(case):
    ex = ab.attn_variant(case)
    muts = ab.attn_mutants(case)
    assert "M5" in muts and ("M3" in muts) == (0 < case.fblk < max(l for n, l in case.groups if n))
    assert ("M4" in muts) == (case.p > 0)
    for m in muts:
        mu = ab.attn_variant(case, m)
        checked = 0
        for g, (nseq, L) in enumerate(case.groups):
            if not nseq or not ab.mutant_applies(case, m, L):
                continue
            t0 = min(t for gg, t, _ in ab.attn_sequences(case) if gg == g)
            sl = slice(t0, t0 + nseq * L)
            for n in ab.MUTANT_OUTPUTS[m]:
                r = float(ab.ratio(mu[n][sl], ex[n][sl], ex["E_" + n][sl]).max())
                assert r > ab.C, f"{case.name}: {m} moves {n} of the length-{L} group by {r:.3g} E only (C = {ab.C})"
            checked += 1
        assert checked


@pytest.mark.parametrize("case", ab.XATTN_CASES, ids=_ids)
def test_xattn_mutants_caught(case):
    ex = ab.xattn_variant(case)
    assert ("M6" in ab.xattn_mutants(case)) == (case.N >= 2) and ("M7" in ab.xattn_mutants(case)) == (case.nq > 16)
    for m in ab.xattn_mutants(case):
        mu = ab.xattn_variant(case, m)
        for n in ab.MUTANT_OUTPUTS[m]:
            r = float(ab.ratio(mu[n], ex[n], ex["E_" + n]).max())
            assert r > ab.C, f"{case.name}: {m} moves {n} by {r:.3g} E only (C = {ab.C})"


def test_tables_cover_the_edges():
    """The lengths, frame blocks and cross-attention shapes the tables must contain."""
    names = {c.name for c in ab.ATTN_CASES} | {c.name for c in ab.XATTN_CASES}
    assert len(names) == len(ab.ATTN_CASES) + len(ab.XATTN_CASES)
    for hd in (32, 64, 80, 88):
        dense = [c for c in ab.ATTN_CASES if c.hd == hd and not c.fblk and not c.p]
        lens = {l for c in dense for n, l in c.groups if n}
        assert {1, 32, 33, 63, 64, 65, 127, 128, 129, 256, 257} <= lens
        assert any(n == 0 for c in dense for n, l in c.groups) and all(len(c.groups) <= 4 for c in dense)
        assert {c.fblk for c in ab.ATTN_CASES if c.hd == hd and c.fblk and not c.p} == {1, 32, 64, 43, 129, 1000}
        assert {bool(c.fblk) for c in ab.ATTN_CASES if c.hd == hd and c.p == 0.2} == {False, True}
    assert any(c.hd == 32 and c.groups == ((1, 255),) for c in ab.ATTN_CASES)
    for hd in (32, 64, 88, 128):
        assert {(c.B, c.nq, c.N) for c in ab.XATTN_CASES if c.hd == hd} == {
            (2, 1, 1), (2, 1, 63), (1, 3, 64), (2, 16, 65), (1, 17, 129), (1, 32, 64), (2, 33, 130)}


@pytest.mark.parametrize("name", ["dense0-hd32", "fc43-hd64", "drop-hd80", "dropfc43-hd88"])
def test_reference_matches_autograd(name):
    """The closed-form float64 reference (O, lse, dQ, dK, dV) against float64 autograd of
    softmax(mask(s Q K^T)) o Z V on the same operands."""
    case = next(c for c in ab.ATTN_CASES if c.name == name)
    qkv, do = ab.attn_inputs(case)
    T, H, hd = ab.attn_tokens(case), case.H, case.hd
    D = H * hd
    q, k, v = (qkv[:, i * D:(i + 1) * D].double().reshape(T, H, hd).requires_grad_(True) for i in range(3))
    outs = []
    for _, t0, L in ab.attn_sequences(case):
        qq, kk, vv = (x[t0:t0 + L].transpose(0, 1) for x in (q, k, v))
        s = (qq @ kk.transpose(-1, -2)) * hd ** -0.5
        if case.fblk:
            f = torch.arange(L) // case.fblk
            s = s.masked_fill(f[None, :] > f[:, None], float("-inf"))
        p = torch.softmax(s, -1)
        if case.p:
            rows = (np.arange(t0, t0 + L)[None, :] * H + np.arange(H)[:, None]).reshape(-1)
            keep = ab.vj_dropout_mask_ref(case.seed, rows, np.arange(L), case.p).reshape(H, L, L)
            p = p * torch.from_numpy(keep).double() / (1 - case.p)
        outs.append((p @ vv).transpose(0, 1))
    o = torch.cat(outs, 0)
    o.backward(do.double().reshape(T, H, hd))
    ex = ab.attn_variant(case)
    for n, got in (("o", o.detach()), ("dq", q.grad), ("dk", k.grad), ("dv", v.grad)):
        assert (got.reshape(T, D) - ex[n]).abs().max().item() < 1e-12, n
        assert bool((ex["E_" + n] >= 0).all())


def test_xattn_reference_matches_autograd():
    case = next(c for c in ab.XATTN_CASES if c.name == "x2-33-130-hd64")
    q, kv, do = ab.xattn_inputs(case)
    B, nq, N, H, hd = case.B, case.nq, case.N, case.H, case.hd
    D = H * hd
    qf, kvf = q.double().requires_grad_(True), kv.double().requires_grad_(True)
    qh = qf.reshape(B, nq, H, hd).permute(0, 2, 1, 3)
    kvh = kvf.reshape(B, N, 2, H, hd).permute(2, 0, 3, 1, 4)
    s = (qh @ kvh[0].transpose(-1, -2)) * hd ** -0.5
    o = (torch.softmax(s, -1) @ kvh[1]).transpose(1, 2).reshape(B * nq, D)
    o.backward(do.double())
    ex = ab.xattn_variant(case)
    for n, got in (("o", o.detach()), ("dq", qf.grad), ("dk", kvf.grad[:, :D]), ("dv", kvf.grad[:, D:])):
        assert (got - ex[n]).abs().max().item() < 1e-12, n
    assert (torch.logsumexp(s, -1).reshape(B * H, nq).detach() - ex["lse"]).abs().max().item() < 1e-12


def _library():
    from vjepa2_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        from vjepa2_amd.build import build

        build(verbose=False)
    return _lib


@pytest.mark.parametrize("offs", [(4, 128, 256), (0, 132, 256), (0, 128, 260), (0, 128, 257), (-8, 128, 256)])
def test_attn_rejects_misaligned_offsets(offs):
    """q, k and v rows are read in 16-B pieces from column off + h * hd: an offset that is no non-negative
    multiple of 8 is an argument error, reported before any launch (null operands: nothing can run)."""
    _lib = _library()
    lib = _lib.load()
    T, H, hd = 10, 2, 64
    groups = (_lib.int_array([1]), _lib.int_array([T]))
    rc = lib.vj_attn_fwd_ex(T, H, hd, None, 392, *offs, None, 128, None, 0.125, 1, *groups, 0, 0.0, 0, None)
    assert rc != 0 and "column offsets" in _lib.last_error(), _lib.last_error()
    rc = lib.vj_attn_bwd_ex(T, H, hd, None, 392, *offs, None, 128, None, 128, None, None, 392, 0.125, 1, *groups,
                            None, 0, 0, 0, None, None, 0, 0.0, 0, None)
    assert rc != 0 and "column offsets" in _lib.last_error(), _lib.last_error()
    rc = lib.vj_attn_fwd(T, H, hd, None, 392, *offs, None, 128, None, 0.125, 1, *groups, None)
    assert rc != 0 and "column offsets" in _lib.last_error(), _lib.last_error()
