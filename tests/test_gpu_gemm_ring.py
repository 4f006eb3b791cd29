"""GPU: the staggered GEMM main loops' ring bookkeeping, bitwise against the one-tile kernel.

The S64 loop (and the 32-deep form 1) keeps its LDS ring positions as running byte offsets that advance with
one add and one wrap per use, builds the two granule-half buffer descriptors once per DMA tile and issues the
granule halves in a fixed alternation. None of that may change a bit of any output: every case below runs
the same call under VJ_GEMM_STG=0 (the one-tile kernel, which has no ring) and under VJ_GEMM_STG=1, and
compares the whole output buffers, guard bands included, as integers.

Shapes. vj_gemm_bf16 hands a problem to the 256-row kernel from M = 1024 on, and a block only crosses tile
boundaries when it owns several tiles, so the row counts are 48 full tile rows plus the residues 129, 255,
257 and 513: the last tile row then has a one-row (129 = 128 + 1), a nearly full (255 = 128 + 127) or an
empty (257, 513: one row in all) second A granule, and with VJ_GEMM_PXCD=1 (8 blocks) every block walks 6
to 19 tiles (N = 256 / 512 / 768: one / two / three column tiles), so the offsets wrap across several tile
boundaries in one block. K = 64, 128, 192, 320 are 1, 2, 3, 5 steps of S64 (2, 4, 6, 10 units of form 1): the read and the DMA
offsets wrap at different phases of a tile, and at K = 64 the DMA stream is three tiles ahead. The operands
are windows of NaN-filled buffers with lda = 328, ldb = 336 (K = 320: 8 / 16 elements of padding, smaller K
more), the outputs windows of sentinel-filled buffers with ldc = N + 24, ldc2 = N + 40, ldaux = N + 32.
"""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import vjepa_oracle as orc  # noqa: E402
from test_gemm_variants import EPI_BF16, EPI_BF16_RESID, EPI_GELU, EPI_ROPE, plan, set_knobs  # noqa: E402
from test_gpu_gemm_strided import DEV, BF16, InFrame, OutFrame, _in_vec  # noqa: E402

FULL_ROWS = 48 * 256
RESIDUES = (129, 255, 257, 513)
KMAX = 320
ROPE_H, ROPE_HD = 4, 64  # N = 768: three 256-wide column tiles


@functools.lru_cache(maxsize=None)
def _problem(M, N):
    """Operand frames of one shape (K = KMAX columns; a case reads the first K), built once and never modified."""
    g = torch.Generator().manual_seed(7919 * M + N)
    A = torch.randn(M, KMAX, generator=g).bfloat16()
    B = (0.1 * torch.randn(N, KMAX, generator=g)).bfloat16()
    bias = torch.randn(N, generator=g)
    resid = torch.randn(M, N, generator=g).bfloat16()
    ids = torch.randint(0, 8 * 16, (M,), generator=g).int()
    return dict(a=InFrame(A, KMAX + 8), b=InFrame(B, KMAX + 16), bias=_in_vec(bias), resid=InFrame(resid, N + 32),
                ids=ids.to(DEV))


@functools.lru_cache(maxsize=None)
def _rope_tables():
    return tuple(t.to(DEV) for t in orc.rope_tables(ROPE_HD, 16))


def _launch(M, N, K, epi):
    """One call into fresh sentinel-filled frames; returns them after the guard-band check (on the device)."""
    from vjepa2_amd import ops

    p = _problem(M, N)
    a, b = p["a"].win[:, :K], p["b"].win[:, :K]
    outs = [OutFrame(M, N, N + 24, BF16)]
    if epi == EPI_ROPE:
        cos_t, sin_t = _rope_tables()
        ops._call("vj_qkv_rope_gemm", M, K, a.data_ptr(), p["a"].ld, b.data_ptr(), p["b"].ld, p["bias"].data_ptr(),
                  outs[0].win.data_ptr(), outs[0].ld, ROPE_H, ROPE_HD, p["ids"].data_ptr(), 0, 16, 4, cos_t.data_ptr(),
                  sin_t.data_ptr(), cos_t.shape[0], torch.cuda.current_stream().cuda_stream)
    else:
        if epi == EPI_GELU:  # both outputs: the saved derivative (C) and the activation (C2)
            outs.append(OutFrame(M, N, N + 40, BF16))
        aux = p["resid"] if epi == EPI_BF16_RESID else None
        ops.gemm(M, N, K, a, p["a"].ld, True, b, p["b"].ld, True, epi, out=outs[0].win, ldc=outs[0].ld,
                 out2=outs[1].win if len(outs) > 1 else None, ldc2=outs[1].ld if len(outs) > 1 else 0, bias=p["bias"],
                 aux=aux.win if aux else None, ldaux=aux.ld if aux else 0)
    torch.cuda.synchronize()
    for i, f in enumerate(outs):
        band = f.bits.clone()
        band.as_strided((f.rows, f.cols), (f.ld, 1), f.off).fill_(f.sent)
        touched = int((band != f.sent).sum())
        assert touched == 0, f"M={M} N={N} K={K} epi={epi} output {i}: {touched} guard elements written"
        inside = f.bits.as_strided((f.rows, f.cols), (f.ld, 1), f.off)
        assert not bool((inside == f.sent).any()), f"M={M} N={N} K={K} epi={epi} output {i}: elements not written"
    return outs


def _compare(M, N, K, epi, form, knobs, monkeypatch):
    set_knobs(monkeypatch, dict(knobs, VJ_GEMM_STG="0"))
    assert plan(M, N, K, "KK", epi, 0) == (256, 256, 8, 0)
    one = _launch(M, N, K, epi)
    set_knobs(monkeypatch, dict(knobs, VJ_GEMM_STG="1"))
    assert plan(M, N, K, "KK", epi, 0) == (256, 256, 8, form), "the case must run the main loop it names"
    stg = _launch(M, N, K, epi)
    for i, (x, y) in enumerate(zip(stg, one)):
        diff = x.bits != y.bits
        assert not bool(diff.any()), (f"form {form} M={M} N={N} K={K} epi={epi} {knobs} output {i}: "
                                      f"{int(diff.sum())} elements differ from the one-tile kernel's; first at "
                                      f"flat index {int(diff.nonzero()[0])} (window offset {x.off}, ld {x.ld})")


@pytest.mark.parametrize("K", [64, 128, 192, 320])
@pytest.mark.parametrize("group", [None, "0"], ids=["group_default", "group0"])
@pytest.mark.parametrize("form", [2, 1], ids=["s64", "form1"])
def test_gemm_ring_offsets_match_one_tile(form, group, K, monkeypatch):
    """EPI_BF16, EPI_GELU (both outputs), EPI_BF16_RESID and the fused QKV + RoPE epilogue on every (residue,
    N) of the module docstring, S64 (default) and form 1 (VJ_GEMM_STG64=0), grouped (default) and row-major
    (VJ_GEMM_GROUP=0) tile order, VJ_GEMM_PXCD=1: whole output buffers bitwise equal to the one-tile kernel's."""
    knobs = {"VJ_GEMM_PXCD": "1", "VJ_GEMM_BM192": "0"}
    if form == 1:
        knobs["VJ_GEMM_STG64"] = "0"
    if group is not None:
        knobs["VJ_GEMM_GROUP"] = group
    for r in RESIDUES:
        M = FULL_ROWS + r
        for N in (256, 512):
            for epi in (EPI_BF16, EPI_GELU, EPI_BF16_RESID):
                _compare(M, N, K, epi, form, knobs, monkeypatch)
        _compare(M, 3 * ROPE_H * ROPE_HD, K, EPI_ROPE, form, knobs, monkeypatch)
