"""Float64 references, componentwise rounding bounds, a bf16 emulation and deliberately wrong variants
("mutants") of the attention kernels (vj_attn_fwd_ex / vj_attn_bwd_ex, vj_xattn_fwd / vj_xattn_bwd).
A helper, not collected: tests/test_attn_bounds.py (CPU) proves on it that the bounds hold for the
documented rounding points and that every mutant breaks them; tests/test_gpu_attn_edges.py holds the
kernels to the same bounds on the same inputs.

Reference: plain float64 attention on the bf16-rounded operands, per (sequence, head), with an optional
frame-causal mask (key j visible to query i iff j // fblk <= i // fblk) and an optional dropout scale
matrix Z = keep / (1 - p) (vj_dropout_mask_ref: mask row = token * H + head, column = key in sequence).
With P = softmax(s Q K^T), Pz = P o Z, s the softmax scale and u = 2^-8:

    O  = Pz V                 E_O  = u (|O| + Pz |V|)
    d  = rowsum(dO o O)       E_d  = rowsum(|dO| o (u |O| + E_O))        (the kernels form d from the bf16 O)
    dS = P o (Z o dO V^T - d) E_dS = u |dS| + P E_d
    dQ = s dS K               E_dQ = u |dQ| + s E_dS |K|
    dK = s dS^T Q             E_dK = u |dK| + s E_dS^T |Q|
    dV = Pz^T dO              E_dV = u (|dV| + Pz^T |dO|)

first-order in the rounding points the kernels document: P and dS become bf16 MFMA operands, O, dQ, dK and
dV are stored as bf16, d is formed from the stored O. vj_xattn keeps P and dS in f32 and rounds only its
outputs; it is held to the same bounds (looser than it needs by the P and dS terms).

An output passes when |got - exact| <= C E on every element. C is not tuned on a kernel: `emulate` redoes
the float64 math with .bfloat16() at each rounding point above (vj_xattn: at the outputs and the stored O
only), and C = 2 x the largest |emulated - exact| / E over every case of the tables below; the factor 2
covers what the emulation leaves out (f32 accumulation order, the hardware exp2, the f32 softmax scale).
Measured on the CPU over ATTN_CASES and XATTN_CASES (head dims 32 / 64 / 80 / 88 / 128, lengths 1 ... 257,
dense, frame-causal from fblk = 1 on, dropout 0.2):

    largest emulation ratio   0.9016 (dV, frame-causal fblk = 32, hd 64; vj_xattn cases: 0.50)
    EMUL_MAX = 0.902, C = 2 EMUL_MAX = 1.804

To first order no ratio can exceed 1 (every rounding is at most u relative, and E adds them up without
cancellation), so C < 2 whatever the inputs. tests/test_attn_bounds.py asserts that the emulation stays
within EMUL_MAX, so the record cannot go stale.

Inputs: seeded standard normal q, k, v, dO (vj_xattn: k, v of standard deviation 2, as in
tests/test_gpu_pooler.py), rounded to bf16, with one change: the last key of every sequence is pulled
towards the sequence's last query, k_last += ln(L + 1) hd^-1/2 q_last (vj_xattn: (ln(N + 1) + 2) hd^-1/2),
which lifts that score by about ln(L + 1). Among L random keys the edge key would carry a weight of
1 / L, and a kernel that drops or misplaces exactly that key (M1, M6) would move the outputs by less than
the rounding bound; with the pull every mutant is visible in every group of every case, with a margin.

Mutants (float64, no rounding; each must exceed C E on the outputs MUTANT_OUTPUTS names):
    M1  the last key of a sequence is not attended (sequences of length >= 2)
    M2  the last query of a sequence is skipped by the dK / dV accumulation (length >= 2: a sequence of
        one token has dS = 0 and so dK = 0 whatever the kernel does)
    M3  at a frame boundary the last query of a frame also sees the first key of the next frame
    M4  within the last 64-key tile the dropout mask uses column j + 1 for key j
    M5  O and dV are scaled by 1 - 2^-5
    M6  (vj_xattn, N >= 2: dq = 0 for a single key) the last 64-key chunk is left out of the dq combine
    M7  (vj_xattn, nq > 16) the second query block (queries 16 ... 31) is left out of dK / dV
"""

import functools
import math
import zlib
from collections import namedtuple

import numpy as np
import torch

from test_dropout import vj_dropout_mask_ref

U = 2.0 ** -8
EMUL_MAX = 0.902
C = 2 * EMUL_MAX
LN2 = math.log(2.0)

MUTANT_OUTPUTS = {"M1": ("o", "dv", "dk"), "M2": ("dk", "dv"), "M3": ("o", "dv"), "M4": ("o", "dv"),
                  "M5": ("o", "dv"), "M6": ("dq",), "M7": ("dk", "dv")}

# vj_attn: groups = ((nseq, len), ...), fblk = 0: dense, p = 0: no dropout
AttnCase = namedtuple("AttnCase", "name hd H groups fblk p seed")
# vj_xattn: B batches of nq queries over N keys
XCase = namedtuple("XCase", "name hd H B nq N")

ATTN_HD = (32, 64, 80, 88)
XATTN_HD = (32, 64, 88, 128)
DENSE_TABLES = (((1, 1), (2, 33), (1, 64), (1, 129)),
                ((2, 32), (1, 63), (1, 65), (1, 257)),
                ((1, 127), (0, 40), (1, 128), (1, 256)))  # (0, 40): a group without sequences
FC_GROUPS = ((2, 129), (1, 65))
FC_FBLK = (1, 32, 64, 43, 129, 1000)
DROP_P, DROP_SEED = 0.2, 4242
XATTN_SHAPES = ((2, 1, 1), (2, 1, 63), (1, 3, 64), (2, 16, 65), (1, 17, 129), (1, 32, 64), (2, 33, 130))


def _heads(hd):
    return 3 if hd == 32 else 2


def _attn_cases():
    out = []
    for hd in ATTN_HD:
        H = _heads(hd)
        for i, g in enumerate(DENSE_TABLES):
            out.append(AttnCase(f"dense{i}-hd{hd}", hd, H, g, 0, 0.0, 0))
        if hd == 32:  # two 128-row tiles per wave: the backward's block boundary falls at 256
            out.append(AttnCase("dense255-hd32", hd, H, ((1, 255),), 0, 0.0, 0))
        for fblk in FC_FBLK:
            out.append(AttnCase(f"fc{fblk}-hd{hd}", hd, H, FC_GROUPS, fblk, 0.0, 0))
        out.append(AttnCase(f"drop-hd{hd}", hd, H, ((1, 65), (2, 33), (1, 129)), 0, DROP_P, DROP_SEED))
        out.append(AttnCase(f"dropfc43-hd{hd}", hd, H, ((1, 129),), 43, DROP_P, DROP_SEED + 1))
    return out


ATTN_CASES = _attn_cases()
XATTN_CASES = [XCase(f"x{B}-{nq}-{N}-hd{hd}", hd, 2, B, nq, N) for hd in XATTN_HD for B, nq, N in XATTN_SHAPES]


def _bf(x):
    return x.bfloat16().double()


def _core(q, k, v, do, s, vis=None, Z=None, emulate=None, dkv_rows=None, dq_keys=None, ov_scale=1.0, bounds=False):
    """One (sequence, head): q, do [Lq, hd], k, v [Lk, hd] float64. vis: bool [Lq, Lk] visibility, Z: dropout
    scale matrix. emulate: None (exact), "mfma" (every rounding point) or "out" (outputs and stored O).
    dkv_rows / dq_keys: the queries the dK / dV sums and the keys the dQ sum take (mutants). Returns a dict
    of o, dq, dk, dv, lse (natural log) and, with bounds, E_o, E_dq, E_dk, E_dv."""
    out_r = _bf if emulate else (lambda x: x)
    in_r = _bf if emulate == "mfma" else (lambda x: x)
    S = s * (q @ k.t())
    if vis is not None:
        S = S.masked_fill(~vis, float("-inf"))
    lse = torch.logsumexp(S, -1)
    P = torch.exp(S - lse[:, None])
    Zm = torch.ones_like(P) if Z is None else Z
    Pz = P * Zm
    O = out_r((in_r(P) * Zm) @ v)  # the forward rounds p, then drops and scales
    delta = (do * O).sum(-1)
    dS = in_r(P * (Zm * (do @ v.t()) - delta[:, None]))
    Pzr = in_r(Pz)
    rows = torch.ones(q.shape[0], dtype=torch.bool) if dkv_rows is None else dkv_rows
    keys = torch.ones(k.shape[0], dtype=torch.bool) if dq_keys is None else dq_keys
    r = dict(o=O * ov_scale, lse=lse,
             dq=out_r(s * ((dS * keys[None, :].double()) @ k)),
             dk=out_r(s * ((dS * rows[:, None].double()).t() @ q)),
             dv=out_r((Pzr * rows[:, None].double()).t() @ do) * ov_scale)
    if bounds:
        assert emulate is None and dkv_rows is None and dq_keys is None and ov_scale == 1.0
        E_o = U * (O.abs() + Pz @ v.abs())
        E_d = (do.abs() * (U * O.abs() + E_o)).sum(-1)
        E_dS = U * dS.abs() + P * E_d[:, None]
        r.update(E_o=E_o, E_dq=U * r["dq"].abs() + s * (E_dS @ k.abs()),
                 E_dk=U * r["dk"].abs() + s * (E_dS.t() @ q.abs()), E_dv=U * (r["dv"].abs() + Pz.t() @ do.abs()))
    return r


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


# ------------------------------------------------------------------------------------------------
# vj_attn
def attn_tokens(case):
    return sum(n * l for n, l in case.groups)


def attn_sequences(case):
    """[(group, first token, length)] of every sequence of the launch."""
    out, t0 = [], 0
    for g, (n, l) in enumerate(case.groups):
        for _ in range(n):
            out.append((g, t0, l))
            t0 += l
    return out


@functools.lru_cache(maxsize=None)
def attn_inputs(case):
    """Seeded bf16 operands of a case: qkv [T, 3 D] (q | k | v, head h at h * hd) and dO [T, D]. Shared,
    never modified."""
    g = _gen(case.name)
    T, D = attn_tokens(case), case.H * case.hd
    qkv, do = torch.randn(T, 3 * D, generator=g), torch.randn(T, D, generator=g)
    for _, t0, L in attn_sequences(case):  # the edge key carries weight (see the module docstring)
        qkv[t0 + L - 1, D:2 * D] += math.log(L + 1.0) * case.hd ** -0.5 * qkv[t0 + L - 1, :D]
    return qkv.bfloat16(), do.bfloat16()


def _visible(L, fblk, leak=False):
    if not fblk:
        return None
    f = torch.arange(L) // fblk
    vis = f[None, :] <= f[:, None]
    if leak:  # M3: query i, the last of its frame, also sees key i + 1
        i = torch.arange(L - 1)
        i = i[(i + 1) % fblk == 0]
        vis[i, i + 1] = True
    return vis


def _drop_z(case, t0, L, h, shift_last_tile=False):
    if not case.p:
        return None
    rows = (np.arange(t0, t0 + L) * case.H + h)
    keep = vj_dropout_mask_ref(case.seed, rows, np.arange(L + 1), case.p)
    if shift_last_tile:  # M4
        j0 = 64 * ((L - 1) // 64)
        keep[:, j0:L] = keep[:, j0 + 1:L + 1].copy()
    return torch.from_numpy(keep[:, :L]).double() / (1.0 - case.p)


def attn_mutants(case):
    """The mutants that change something in at least one sequence of the case."""
    lens = [l for n, l in case.groups if n]
    m = ["M5"]
    if any(l >= 2 for l in lens):
        m += ["M1", "M2"]
    if case.fblk and any(l > case.fblk for l in lens):
        m.append("M3")
    if case.p:
        m.append("M4")
    return sorted(m)


def mutant_applies(case, mutant, L):
    """Whether `mutant` changes a sequence of length L of the case."""
    return {"M1": L >= 2, "M2": L >= 2, "M3": bool(case.fblk) and L > case.fblk, "M4": case.p > 0, "M5": True}[mutant]


@functools.lru_cache(maxsize=None)
def attn_variant(case, variant="exact"):
    """Outputs of a whole launch: o, dq, dk, dv float64 [T, D], lse float64 [H, T] (natural log); variant
    "exact" adds the bounds E_o, E_dq, E_dk, E_dv. variant: "exact", "emul" or a mutant name."""
    qkv, do = attn_inputs(case)
    T, H, hd = attn_tokens(case), case.H, case.hd
    D = H * hd
    q, k, v = (qkv[:, i * D:(i + 1) * D].double().reshape(T, H, hd) for i in range(3))
    do = do.double().reshape(T, H, hd)
    names = ("o", "dq", "dk", "dv") + (("E_o", "E_dq", "E_dk", "E_dv") if variant == "exact" else ())
    res = {n: torch.zeros(T, H, hd, dtype=torch.float64) for n in names}
    lse = torch.zeros(H, T, dtype=torch.float64)
    for _, t0, L in attn_sequences(case):
        mut = variant if variant.startswith("M") and mutant_applies(case, variant, L) else None
        vis = _visible(L, case.fblk, leak=mut == "M3")
        kw = {}
        if mut == "M1":
            vis = torch.ones(L, L, dtype=torch.bool) if vis is None else vis
            vis[:, L - 1] = False
        elif mut == "M2":
            kw["dkv_rows"] = torch.arange(L) < L - 1
        elif mut == "M5":
            kw["ov_scale"] = 1.0 - 2.0 ** -5
        for h in range(H):
            sl = slice(t0, t0 + L)
            r = _core(q[sl, h], k[sl, h], v[sl, h], do[sl, h], hd ** -0.5, vis=vis,
                      Z=_drop_z(case, t0, L, h, shift_last_tile=mut == "M4"),
                      emulate="mfma" if variant == "emul" else None, bounds=variant == "exact", **kw)
            for n in names:
                res[n][sl, h] = r[n]
            lse[h, sl] = r["lse"]
    out = {n: x.reshape(T, D) for n, x in res.items()}
    out["lse"] = lse
    return out


# ------------------------------------------------------------------------------------------------
# vj_xattn
@functools.lru_cache(maxsize=None)
def xattn_inputs(case):
    """Seeded bf16 operands: q [B nq, D], kv [B N, 2 D] (k | v), dO [B nq, D]."""
    g = _gen(case.name)
    B, nq, N, D = case.B, case.nq, case.N, case.H * case.hd
    q, kv, do = torch.randn(B * nq, D, generator=g), 2 * torch.randn(B * N, 2 * D, generator=g), torch.randn(B * nq, D, generator=g)
    for b in range(B):  # the edge key carries weight
        kv[b * N + N - 1, :D] += (math.log(N + 1.0) + 2.0) * case.hd ** -0.5 * q[b * nq + nq - 1]
    return q.bfloat16(), kv.bfloat16(), do.bfloat16()


def xattn_mutants(case):
    return (["M6"] if case.N >= 2 else []) + (["M7"] if case.nq > 16 else [])


@functools.lru_cache(maxsize=None)
def xattn_variant(case, variant="exact"):
    """o, dq float64 [B nq, D], dk, dv [B N, D], lse [B H, nq] (natural log); "exact" adds the bounds."""
    q, kv, do = xattn_inputs(case)
    B, nq, N, H, hd = case.B, case.nq, case.N, case.H, case.hd
    D = H * hd
    q, do = (x.double().reshape(B, nq, H, hd) for x in (q, do))
    k, v = (kv[:, i * D:(i + 1) * D].double().reshape(B, N, H, hd) for i in range(2))
    ex = variant == "exact"
    shp = dict(o=(B, nq), dq=(B, nq), dk=(B, N), dv=(B, N))
    names = tuple(shp) + (tuple("E_" + n for n in shp) if ex else ())
    res = {n: torch.zeros(*shp[n.replace("E_", "")], H, hd, dtype=torch.float64) for n in names}
    lse = torch.zeros(B * H, nq, dtype=torch.float64)
    kw = {}
    if variant == "M6":
        kw["dq_keys"] = torch.arange(N) < 64 * ((N - 1) // 64)
    elif variant == "M7":
        i = torch.arange(nq)
        kw["dkv_rows"] = (i < 16) | (i >= 32)
    for b in range(B):
        for h in range(H):
            r = _core(q[b, :, h], k[b, :, h], v[b, :, h], do[b, :, h], hd ** -0.5,
                      emulate="out" if variant == "emul" else None, bounds=ex, **kw)
            for n in names:
                res[n][b, :, h] = r[n]
            lse[b * H + h] = r["lse"]
    out = {n: x.reshape(-1, D) for n, x in res.items()}
    out["lse"] = lse
    return out


# ------------------------------------------------------------------------------------------------
def ratio(got, exact, E):
    """Elementwise |got - exact| / E (0 where both vanish, inf where only E does or got is not finite)."""
    err = (got - exact).abs()
    r = torch.where(E > 0, err / E.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0).to(err.dtype))
    return torch.where(torch.isfinite(got), r, torch.full_like(r, math.inf))


def assert_within(got, exact, E, what, c=C):
    """|got - exact| <= c E on every element (NaN / inf in got fail); returns the largest ratio."""
    r = ratio(got, exact, E)
    bad = ~(r <= c)
    if bool(bad.any()):
        i = [int(x) for x in bad.nonzero()[0]]
        assert False, (f"{what}: {int(bad.sum())} of {bad.numel()} elements outside {c:.3g} E (largest ratio "
                       f"{float(r.max()):.3g}); first at {i}: got {float(got[tuple(i)])!r}, exact "
                       f"{float(exact[tuple(i)])!r}, E {float(E[tuple(i)]):.3g}")
    return float(r.max()) if r.numel() else 0.0
