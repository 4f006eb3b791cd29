"""GPU: the memory-bound kernels of csrc/vj_ops.hip at every dispatch branch, with padded leading dimensions
inside poisoned frames, against float64 references.

Operands are windows (row 2, column 8, two slack rows behind; tests/test_gpu_gemm_strided.py's InFrame /
OutFrame) of NaN-filled buffers, outputs windows of buffers pre-filled with a NaN sentinel bit pattern, vectors
(gamma, mean, dgamma, row_loss, ...) slices of longer NaN / sentinel vectors, leading dimensions pairwise
different multiples of 8 (bytes kernels: of 16 bytes). A wrong offset shows as a wrong value or a touched
guard, never as a fault. Where an ops.* wrapper fixes an output stride the C entry point is called directly
(vjepa2_amd._lib.call). One framed call is checked four ways:
 (1) guard band: every element of each output buffer outside its window still holds the sentinel bits;
 (2) reference: the window against float64 math on the CPU over exactly the values the kernel reads;
 (3) bitwise equal to the same call on contiguous copies (a leading dimension only enters addresses);
 (4) determinism (LayerNorm backward, colsum): a second identical call gives bitwise the same column sums.

Instantiations launched, per kernel template of vj_ops.hip:
  k_ln_fwd<XBF, YF32, NV>      XBF, YF32 in {0, 1}^2, NV in {1, 2, 4, 6, 8} each (test_layernorm_fwd: f32 rows by
                               default, bf16 rows under VJ_LN_FWD=1 or D % 8 = 4; LN_FWD_CASES names the NV per
                               D); bf16 rows with ldx % 8 = 4 or ldy % 8 = 4 (test_layernorm_fwd_strides_mod4)
  k_ln_fwd<XBF, false, 4, YF8> XBF in {0, 1} (test_fp8_rows_framed, D = 520)
  k_ln_fwd3<XBF, YF32, NV, 4>  XBF = 1: NV in {1, 2, 3, 4} by default; XBF = 0 (VJ_LN_FWD=3): NV in {1, 2, 3, 4},
                               D <= 1024; both YF32
  k_quant_rows_fp8<XBF>        XBF in {0, 1}, K = 520: three trips of the row loop (test_fp8_rows_framed)
  k_ln_bwd<ACC, NV>            ACC in {0, 1}, NV in {1, 2, 4, 6, 8}: by D % 8 = 4 (D = 4, 68, 252, 260, 516, 1028,
                               1540, 2044) and by lddy % 8 = 4 at every D % 8 = 0 of the table; M = 4101 at D = 68
                               takes the second trip of the 1024-block grid (test_layernorm_bwd)
  k_ln_bwd2<ACC, NV, SUMS, BFR> ACC, SUMS, BFR in {0, 1}^3, NV in {1, 2, 3, 4}; M = 3077 at D = 64 takes the
                               second trip of the 768-block grid, f32 and bf16 residual stream
  k_colsum2_multi              S = 1 .. 1024 partial rows, nsum in {2, 4}, with null outputs (sum_in absent)
  k_colsum1<BF>, k_colsum2     BF in {0, 1}; M = 1 .. 16389 (S = 256, uneven last slice), N = 8 .. 1032 (three
                               column blocks), accumulate on / off (test_colsum_exact)
  k_jepa_loss<ZBF, TBF>        {0, 1}^2, D = 4 .. 2048, p = 1 and p = 2, 1 - 4 groups; k_sum1 with R = 311 > 256
  k_rope<F32>                  F32 in {0, 1}; forward and (bf16) inverse, ids and ids_mod
  k_adamw, k_ema, k_check_finite, k_cast_bf16 (+ k_cast_bf16_tail): n = 4, 4100 and 4 (4096 * 256 + 257): the
                               second grid-stride trip; fused EMA, skipped step, p_bf16 absent
  k_gather_rows (gather and scatter; 1 to 256 uint4 per row under 64 threads), k_fill_rows, k_add_rows (idx
  and idx_mod), k_ids64to32, k_transpose_bf16, k_transpose_bf16_batch
"""

import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import vjepa_oracle as orc  # noqa: E402
from test_gpu_gemm_strided import (BF16, DEV, F32, ROW0, SENTINEL, SLACK, InFrame, OutFrame, _col0,  # noqa: E402
                                   _in_vec)

U24 = 2.0 ** -24  # f32 unit roundoff
LN_EPS = 1e-6
TOL_F32 = (1e-4, 1e-4)   # the suite's LayerNorm bounds (test_gpu_kernels.py::test_layernorm)
TOL_BF16 = (1e-3, 8e-3)


def _call(name, *args):
    from vjepa2_amd import _lib

    return _lib.call(name, *args)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _p(f):
    """Device pointer of a frame's window (None: a null argument)."""
    return None if f is None else f.win.data_ptr()


def _r8(n):
    return (n + 7) // 8 * 8


class InFrame4(InFrame):
    """InFrame whose leading dimension is a multiple of 4 elements only (8-B bf16 / 16-B f32 rows): the
    strides that take the kernels' narrower-vector fallbacks."""

    def __init__(self, t, ld):
        rows, cols = t.shape
        assert ld % 4 == 0 and ld > cols
        self.ld = ld
        c0 = _col0(ld, t.element_size())
        buf = torch.full(((ROW0 + rows + SLACK) * ld + c0,), float("nan"), dtype=t.dtype)
        buf.as_strided((rows, cols), (ld, 1), ROW0 * ld + c0).copy_(t)
        self.buf = buf.to(DEV)
        self.win = self.buf.as_strided((rows, cols), (ld, 1), ROW0 * ld + c0)
        assert self.win.data_ptr() % 16 == 0


def _frame(t, ld):
    return InFrame(t, ld) if ld == t.shape[1] or ld % 8 == 0 else InFrame4(t, ld)


def _ovec(n, dtype=F32, init=None, shift_bytes=0):
    """An [n] output vector: n contiguous elements inside a sentinel buffer (an [n, 1] OutFrame, ld = 1)."""
    f = OutFrame(n, 1, 1, dtype, shift_bytes)
    if init is not None:
        f.fill(init.reshape(n, 1))
    return f


def _oflat(n, dtype=F32, init=None):
    """As _ovec for n % 4 == 0: an [n / 4, 4] OutFrame with ld = 4 (the window is one contiguous run)."""
    assert n % 4 == 0
    f = OutFrame(n // 4, 4, 4, dtype)
    if init is not None:
        f.fill(init.reshape(n // 4, 4))
    return f


def _vals(bits, dtype):
    return bits.view(dtype).double()


def _close(got, exp, tol, what, extra=None):
    """(2) |got - exp| <= atol + rtol |exp| (+ extra) elementwise, float64; NaN / inf in got fail."""
    atol, rtol = tol
    bound = atol + rtol * exp.abs()
    if extra is not None:
        bound = bound + extra
    err = (got - exp).abs()
    ok = err <= bound
    if not bool(ok.all()):
        i = tuple(int(v) for v in (~ok).nonzero()[0])
        assert False, (f"{what}: {int((~ok).sum())} of {ok.numel()} outside atol {atol:.3g} rtol {rtol:.3g}; first at "
                       f"{i}: got {float(got[i])!r}, expected {float(exp[i])!r}, max err {float(err[ok.logical_not()].max()):.3e}")


def _same(a, b, what):
    """(3) / (4) bitwise equal."""
    diff = a != b
    assert not bool(diff.any()), (f"{what}: {int(diff.sum())} of {diff.numel()} elements differ bitwise; first at "
                                  f"{[int(v) for v in diff.nonzero()[0]]}")


def _same_all(res, ref, what):
    assert res.keys() == ref.keys()
    for k in res:
        _same(res[k], ref[k], f"{what} output {k}")


# ------------------------------------------------------------------------------------------------
# LayerNorm forward
def _ln_nv(D):
    v = (D + 255) // 256
    return 1 if v <= 1 else 2 if v <= 2 else 4 if v <= 4 else 6 if v <= 6 else 8


def _fwd_kernel(D, xbf, mode, ldx, ldy, yf32):
    """(kernel, NV) of vj_layernorm_fwd's dispatch for 16-B aligned pointers (mode: VJ_LN_FWD or None)."""
    E = 8 if xbf else 4
    nv3 = (D + 64 * E - 1) // (64 * E)
    if (mode != "1" and (xbf or mode == "3") and D % E == 0 and ldx % E == 0 and ldy % (4 if yf32 else E) == 0
            and nv3 <= 4):
        return "fwd3", nv3
    return "fwd", _ln_nv(D)


# (D, rows, then the (kernel, NV) expected for: f32 rows by default and under VJ_LN_FWD=1 | f32 rows under
# VJ_LN_FWD=3 | bf16 rows by default and under VJ_LN_FWD=3 | bf16 rows under VJ_LN_FWD=1); fwd = k_ln_fwd,
# fwd3 = k_ln_fwd3. D = 260, 516, 1028, 1540 (bf16: 520, 1032, 1544) sit one lane-vector past a lane-span
# boundary, D % 8 = 4 keeps bf16 rows on k_ln_fwd, f32 rows wider than 1024 do not fit k_ln_fwd3.
LN_FWD_CASES = [
    (4, (1, 3, 5, 17), ("fwd", 1), ("fwd3", 1), ("fwd", 1), ("fwd", 1)),
    (8, (5, 17), ("fwd", 1), ("fwd3", 1), ("fwd3", 1), ("fwd", 1)),
    (64, (5, 17), ("fwd", 1), ("fwd3", 1), ("fwd3", 1), ("fwd", 1)),
    (252, (5, 17), ("fwd", 1), ("fwd3", 1), ("fwd", 1), ("fwd", 1)),
    (256, (5, 17), ("fwd", 1), ("fwd3", 1), ("fwd3", 1), ("fwd", 1)),
    (260, (5, 17, 301), ("fwd", 2), ("fwd3", 2), ("fwd", 2), ("fwd", 2)),
    (512, (5, 17), ("fwd", 2), ("fwd3", 2), ("fwd3", 1), ("fwd", 2)),
    (516, (5, 17), ("fwd", 4), ("fwd3", 3), ("fwd", 4), ("fwd", 4)),
    (520, (1, 3, 5, 17), ("fwd", 4), ("fwd3", 3), ("fwd3", 2), ("fwd", 4)),
    (1024, (5, 17), ("fwd", 4), ("fwd3", 4), ("fwd3", 2), ("fwd", 4)),
    (1028, (5, 17), ("fwd", 6), ("fwd", 6), ("fwd", 6), ("fwd", 6)),
    (1032, (5, 17), ("fwd", 6), ("fwd", 6), ("fwd3", 3), ("fwd", 6)),
    (1536, (5, 17), ("fwd", 6), ("fwd", 6), ("fwd3", 3), ("fwd", 6)),
    (1540, (5, 17), ("fwd", 8), ("fwd", 8), ("fwd", 8), ("fwd", 8)),
    (1544, (5, 17, 301), ("fwd", 8), ("fwd", 8), ("fwd3", 4), ("fwd", 8)),
    (2040, (5, 17), ("fwd", 8), ("fwd", 8), ("fwd3", 4), ("fwd", 8)),
    (2048, (1, 3, 5, 17), ("fwd", 8), ("fwd", 8), ("fwd3", 4), ("fwd", 8)),
]
LN_FWD_BY_D = {c[0]: c for c in LN_FWD_CASES}


def _fwd_lds(D):
    return _r8(D) + 8, _r8(D) + 24  # ldx, ldy


def test_layernorm_fwd_case_table_covers_every_nv():
    """The table above agrees with the dispatch (mirrored in _fwd_kernel) for the padded and the contiguous
    strides, and hits every NV of k_ln_fwd {1, 2, 4, 6, 8} and of k_ln_fwd3 {1, 2, 3, 4} for both input types."""
    hit = set()
    for D, rows, f32_def, f32_3, bf_def, bf_1 in LN_FWD_CASES:
        assert {5, 17} <= set(rows)
        for ldx, ldy in (_fwd_lds(D), (D, D)):
            for yf32 in (True, False):
                assert _fwd_kernel(D, False, None, ldx, ldy, yf32) == f32_def == _fwd_kernel(D, False, "1", ldx, ldy, yf32)
                assert _fwd_kernel(D, False, "3", ldx, ldy, yf32) == f32_3
                assert _fwd_kernel(D, True, None, ldx, ldy, yf32) == bf_def == _fwd_kernel(D, True, "3", ldx, ldy, yf32)
                assert _fwd_kernel(D, True, "1", ldx, ldy, yf32) == bf_1
        hit |= {("f32",) + f32_def, ("f32",) + f32_3, ("bf16",) + bf_def, ("bf16",) + bf_1}
    for xt in ("f32", "bf16"):
        assert {nv for t, k, nv in hit if t == xt and k == "fwd"} == {1, 2, 4, 6, 8}
        assert {nv for t, k, nv in hit if t == xt and k == "fwd3"} == {1, 2, 3, 4}
    assert max(D for D, _, _, f3, _, _ in LN_FWD_CASES if f3[0] == "fwd3") == 1024


@functools.lru_cache(maxsize=None)
def _ln_data(M, D, offset):
    """Rows of one shape: offset 1 -> 3 randn + 1 (the suite's inputs), offset 100 -> randn + 100 (a large
    mean: a one-pass E[x^2] - mean^2 variance loses 60x the bound there). Shared, never modified."""
    g = torch.Generator().manual_seed(7919 * D + 31 * M + offset)
    x = (3.0 if offset == 1 else 1.0) * torch.randn(M, D, generator=g) + offset
    return dict(x=x, xb=x.bfloat16(), w=torch.randn(D, generator=g), b=torch.randn(D, generator=g),
                dy=torch.randn(M, D, generator=g).bfloat16(), ri=torch.randn(M, D, generator=g),
                init=1.0 + torch.rand(4, D, generator=g))


def _ln64(x, w, b):
    """float64 LayerNorm of the rows the kernel reads -> (y, mean, rstd)."""
    x = x.double()
    mu = x.mean(1, keepdim=True)
    xc = x - mu
    rs = ((xc * xc).mean(1, keepdim=True) + LN_EPS).rsqrt()
    y = xc * rs
    if w is not None:
        y = y * w.double() + b.double()
    return y, mu[:, 0], rs[:, 0]


def _ln_fwd_launch(fx, M, D, w, b, ydt, ldy, stats, what):
    fy = OutFrame(M, D, ldy, ydt)
    fm, fr = (_ovec(M), _ovec(M)) if stats else (None, None)
    _call("vj_layernorm_fwd", M, D, _p(fx), int(fx.win.dtype == BF16), fx.ld, None if w is None else w.data_ptr(),
          None if b is None else b.data_ptr(), LN_EPS, _p(fy), int(ydt == F32), ldy, _p(fm), _p(fr), _st())
    torch.cuda.synchronize()
    res = {"y": fy.read(f"{what} y")}
    if stats:
        res["mean"], res["rstd"] = fm.read(f"{what} mean"), fr.read(f"{what} rstd")
    return res


def _check_ln_fwd(res, ref, ydt, what):
    y, mu, rs = ref
    _close(_vals(res["y"], ydt), y, TOL_F32 if ydt == F32 else TOL_BF16, f"{what} y")
    if "mean" in res:
        _close(_vals(res["mean"], F32)[:, 0], mu, (0.0, 0.0), f"{what} mean", extra=1e-5 * mu.abs().clamp(min=1.0))
        _close(_vals(res["rstd"], F32)[:, 0], rs, (0.0, 1e-4), f"{what} rstd")


def _set_mode(monkeypatch, mode):
    if mode is None:
        monkeypatch.delenv("VJ_LN_FWD", raising=False)
    else:
        monkeypatch.setenv("VJ_LN_FWD", mode)


@pytest.mark.parametrize("D", [c[0] for c in LN_FWD_CASES])
def test_layernorm_fwd(D, monkeypatch):
    """vj_layernorm_fwd, x f32 / bf16 -> y f32 / bf16, default dispatch, VJ_LN_FWD=1 and =3 (the kernels and NV
    per D: LN_FWD_CASES), both input sets, x and y in frames with ldx != ldy, gamma / beta / mean / rstd slices
    of NaN / sentinel vectors; at M = 5 under the default dispatch also without affine and without the stats
    pointers. Checks (1)-(3)."""
    rows = LN_FWD_BY_D[D][1]
    ldx, ldy = _fwd_lds(D)
    for M in rows:
        for offset in (1, 100):
            d = _ln_data(M, D, offset)
            w, b = _in_vec(d["w"]), _in_vec(d["b"])
            for xbf in (False, True):
                x = d["xb"] if xbf else d["x"]
                fpad, fcon = InFrame(x, ldx), InFrame(x, D)
                refs = {True: _ln64(x, d["w"], d["b"]), False: _ln64(x, None, None)}
                for mode in (None, "1", "3"):
                    _set_mode(monkeypatch, mode)
                    for ydt in (F32, BF16):
                        variants = [(True, True)]
                        if M == 5 and mode is None:
                            variants += [(False, True), (True, False), (False, False)]
                        for affine, stats in variants:
                            what = (f"ln fwd M={M} D={D} offset={offset} x={'bf16' if xbf else 'f32'} "
                                    f"y={'f32' if ydt == F32 else 'bf16'} VJ_LN_FWD={mode} affine={affine} stats={stats}")
                            ww, bb = (w, b) if affine else (None, None)
                            res = _ln_fwd_launch(fpad, M, D, ww, bb, ydt, ldy, stats, what)
                            _check_ln_fwd(res, refs[affine], ydt, what)
                            _same_all(res, _ln_fwd_launch(fcon, M, D, ww, bb, ydt, D, stats, what + " contiguous"), what)


@pytest.mark.parametrize("case", ["ldx", "ldy"])
def test_layernorm_fwd_strides_mod4(case, monkeypatch):
    """bf16 rows whose strides forbid 16-B vectors: ldx = 532 = 4 (mod 8) (f32 output), or bf16 output with ldy =
    540 = 4 (mod 8). k_ln_fwd3 does not apply, vj_layernorm_fwd must fall back to k_ln_fwd<.., 4> (D = 520) and
    still be right: checks (1), (2), and (3) against the contiguous call under VJ_LN_FWD=1 (the same kernel)."""
    D = 520
    ldx, ldy, ydt = (532, 544, F32) if case == "ldx" else (528, 540, BF16)
    assert _fwd_kernel(D, True, None, ldx, ldy, ydt == F32) == ("fwd", 4) != _fwd_kernel(D, True, None, D, D, ydt == F32)
    for M in (5, 17):
        for offset in (1, 100):
            d = _ln_data(M, D, offset)
            w, b = _in_vec(d["w"]), _in_vec(d["b"])
            what = f"ln fwd mod-4 stride M={M} offset={offset} ldx={ldx} ldy={ldy}"
            _set_mode(monkeypatch, None)
            res = _ln_fwd_launch(_frame(d["xb"], ldx), M, D, w, b, ydt, ldy, True, what)
            _check_ln_fwd(res, _ln64(d["xb"], d["w"], d["b"]), ydt, what)
            _set_mode(monkeypatch, "1")
            _same_all(res, _ln_fwd_launch(InFrame(d["xb"], D), M, D, w, b, ydt, D, True, what + " contiguous"), what)


@pytest.mark.parametrize("xbf", [False, True])
def test_fp8_rows_framed(xbf):
    """vj_layernorm_fwd_fp8 and vj_quant_rows_fp8 with padded ldx / ldy, D = K = 520 (k_quant_rows_fp8's row
    loop takes three trips), M = 5: the e4m3 bytes (a bf16 sentinel frame of D / 2 columns) and the exponents
    keep their guard bands and equal, bitwise, the call on a contiguous x with the narrowest legal ldy (528:
    fp8 rows are 16-B aligned). The values are test_gpu_fp8.py's subject."""
    M, D = 5, 520
    d = _ln_data(M, D, 1)
    x = d["xb"] if xbf else d["x"]
    w, b = _in_vec(d["w"]), _in_vec(d["b"])
    out = {}
    for ldx, ldy in ((536, 560), (D, 528)):
        fx = InFrame(x, ldx)
        y1, e1, m1, r1 = OutFrame(M, D // 2, ldy // 2, BF16), _ovec(M), _ovec(M), _ovec(M)
        _call("vj_layernorm_fwd_fp8", M, D, _p(fx), int(xbf), ldx, w.data_ptr(), b.data_ptr(), LN_EPS, _p(y1), ldy,
              _p(e1), _p(m1), _p(r1), _st())
        y2, e2 = OutFrame(M, D // 2, ldy // 2, BF16), _ovec(M)
        _call("vj_quant_rows_fp8", M, D, _p(fx), int(xbf), ldx, _p(y2), ldy, _p(e2), _st())
        torch.cuda.synchronize()
        out[ldx] = {k: f.read(f"fp8 rows ldx={ldx} {k}") for k, f in
                    dict(ln_y=y1, ln_exp=e1, ln_mean=m1, ln_rstd=r1, q_y=y2, q_exp=e2).items()}
    _same_all(out[536], out[D], "fp8 rows")
    _, mu, rs = _ln64(x, None, None)
    _close(_vals(out[536]["ln_mean"], F32)[:, 0], mu, (0.0, 0.0), "fp8 ln mean", extra=1e-5 * mu.abs().clamp(min=1.0))
    _close(_vals(out[536]["ln_rstd"], F32)[:, 0], rs, (0.0, 1e-4), "fp8 ln rstd")
    amax = x.double().abs().amax(1)  # the least e with amax 2^-e <= 448
    assert torch.equal(out[536]["q_exp"][:, 0].long(), torch.ceil(torch.log2(amax / 448.0)).long())


# ------------------------------------------------------------------------------------------------
# LayerNorm backward
# (D, rows, entry forms): v2 = vj_layernorm_bwd on k_ln_bwd2 (16-B accesses), fb = vj_layernorm_bwd on the
# float4 kernel k_ln_bwd (reached by D % 8 = 4, or at D % 8 = 0 by lddy % 8 = 4), bf = vj_layernorm_bwd_bf16
# (k_ln_bwd2<.., BFR>). NV: k_ln_bwd2 = ceil(D / 512), k_ln_bwd = _ln_nv(D).
LN_BWD_CASES = [
    (4, (1, 3, 5, 17), ("fb",)),            # k_ln_bwd NV 1
    (8, (1, 3, 5, 17), ("v2", "fb", "bf")),  # k_ln_bwd2 NV 1, k_ln_bwd NV 1
    (64, (5, 17, 3077), ("v2", "fb", "bf")),  # NV 1 / 1; M = 3077: 770 > 768 blocks of 4 rows
    (68, (5, 17, 4101), ("fb",)),           # k_ln_bwd NV 1; M = 4101: 1026 > 1024 blocks
    (252, (5, 17), ("fb",)),                # NV 1
    (256, (5, 17), ("v2", "fb", "bf")),     # NV 1 / 1
    (260, (5, 17), ("fb",)),                # NV 2
    (512, (5, 17), ("v2", "fb", "bf")),     # NV 1 / 2
    (516, (5, 17, 301), ("fb",)),           # NV 4
    (520, (5, 17), ("v2", "fb", "bf")),     # NV 2 / 4
    (1024, (5, 17), ("v2", "fb", "bf")),    # NV 2 / 4
    (1028, (5, 17), ("fb",)),               # NV 6
    (1032, (5, 17, 301), ("v2", "fb", "bf")),  # NV 3 / 6
    (1536, (5, 17), ("v2", "fb", "bf")),    # NV 3 / 6
    (1540, (5, 17), ("fb",)),               # NV 8
    (1544, (5, 17), ("v2", "fb", "bf")),    # NV 4 / 8
    (2040, (5, 17), ("v2", "fb", "bf")),    # NV 4 / 8
    (2044, (5, 17), ("fb",)),               # NV 8
    (2048, (1, 3, 5, 17), ("v2", "fb", "bf")),  # NV 4 / 8
]
LN_BWD_BY_D = {c[0]: c for c in LN_BWD_CASES}
# dres_in present / absent, nsum 0 / 2 / 4 (4 without dres_in: sum_out only), bf16 copy on / off, gamma null
LN_BWD_OPTS = [dict(ri=True, nsum=4, bf=True, gamma=True), dict(ri=False, nsum=2, bf=False, gamma=True),
               dict(ri=True, nsum=0, bf=True, gamma=True), dict(ri=False, nsum=4, bf=False, gamma=False)]
COLS = ("dgamma", "dbeta", "sum_in", "sum_out")


def test_layernorm_bwd_case_table_covers_every_nv():
    nv_fb = {_ln_nv(D) for D, _, forms in LN_BWD_CASES if D % 8 == 4}
    nv_fbs = {_ln_nv(D) for D, _, forms in LN_BWD_CASES if D % 8 == 0 and "fb" in forms}
    nv_v2 = {(D + 511) // 512 for D, _, forms in LN_BWD_CASES if "v2" in forms}
    assert nv_fb == nv_fbs == {1, 2, 4, 6, 8} and nv_v2 == {1, 2, 3, 4}
    assert {4, 68, 260, 516, 1028, 1540, 2044} <= {D for D, _, _ in LN_BWD_CASES if D % 8 == 4}
    assert all((("v2" in f) == ("bf" in f) == (D % 8 == 0)) and "fb" in f for D, _, f in LN_BWD_CASES)


def _col_chain(M, cap):
    """The longest chain of sequential f32 additions one column sum of the LayerNorm backward goes through."""
    nbl = min((M + 3) // 4, cap)                 # blocks launched, 4 waves each, a wave owns every (4 nbl)-th row
    rpw = (M + 4 * nbl - 1) // (4 * nbl)         # rows one wave adds up in sequence (acc += term)
    s4 = ((nbl + 31) // 32 + 3) // 4             # partials one of a thread's 4 running sums takes (k_colsum2_multi)
    return rpw + 3 + s4 + 2 + 32 + 1


def _ln_bwd_lds(D, form, alt=False):
    """Pairwise different leading dimensions of dy, x, dres_in, dres, dres_bf16; the strided fallback (fb at
    D % 8 = 0) has lddy = 4 (mod 8); alt: its second layout (lddy = D + 12, everything else contiguous)."""
    if alt:
        return dict(dy=D + 12, x=D, ri=D, r=D, rb=D)
    b = _r8(D)
    lds = dict(dy=b + 8, x=b + 16, ri=b + 24, r=b + 32, rb=b + 40)
    if form == "fb" and D % 8 == 0:
        lds["dy"] = D + 4
    assert len(set(lds.values())) == 5
    return lds


def _ln_bwd_launch(form, M, D, d, stats, lds, opt, what):
    """One vj_layernorm_bwd / vj_layernorm_bwd_bf16 call into fresh frames; returns {name: bits} after (1)."""
    from vjepa2_amd import _lib

    bfr = form == "bf"
    x = d["xb"] if bfr else d["x"]
    ri = (d["ri"].bfloat16() if bfr else d["ri"]) if opt["ri"] else None
    fdy, fx = _frame(d["dy"], lds["dy"]), _frame(x, lds["x"])
    fri = _frame(ri, lds["ri"]) if ri is not None else None
    mean, rstd = _in_vec(stats[0]), _in_vec(stats[1])
    gamma = _in_vec(d["w"]) if opt["gamma"] else None
    outs = {"dres": OutFrame(M, D, lds["r"], BF16 if bfr else F32)}
    if opt["bf"] and not bfr:
        outs["dres_bf"] = OutFrame(M, D, lds["rb"], BF16)
    nsum = opt["nsum"]
    names = [] if nsum == 0 else ["dgamma", "dbeta"] if nsum == 2 else (
        ["dgamma", "dbeta", "sum_in", "sum_out"] if opt["ri"] else ["dgamma", "dbeta", "sum_out"])
    for k in names:  # accumulated into: pre-set to a non-zero vector
        outs[k] = _ovec(D, F32, d["init"][COLS.index(k)])
    nws = _lib.load().vj_layernorm_bwd_blocks(M) * nsum * D
    if nsum:
        outs["ws"] = _ovec(nws)
    pc = [_p(outs.get(k)) for k in COLS]
    gp = None if gamma is None else gamma.data_ptr()
    if bfr:
        _call("vj_layernorm_bwd_bf16", M, D, _p(fdy), fdy.ld, _p(fx), fx.ld, mean.data_ptr(), rstd.data_ptr(), gp,
              _p(fri), fri.ld if fri else 0, _p(outs["dres"]), lds["r"], *pc, _p(outs.get("ws")), nws, _st())
    else:
        _call("vj_layernorm_bwd", M, D, _p(fdy), fdy.ld, _p(fx), fx.ld, mean.data_ptr(), rstd.data_ptr(), gp, _p(fri),
              fri.ld if fri else 0, _p(outs["dres"]), lds["r"], _p(outs.get("dres_bf")), lds["rb"], *pc,
              _p(outs.get("ws")), nws, _st())
    torch.cuda.synchronize()
    res = {k: f.read(f"{what} {k}") for k, f in outs.items()}
    res.pop("ws", None)  # scratch: only its guard band is checked
    return res


def _ln_bwd_ref(d, bfr, opt):
    """float64 autograd of layer_norm on the rows the kernel reads, and per column vector (expected sum, sum
    of |terms|), each including the vector's initial value."""
    x = (d["xb"] if bfr else d["x"]).double().requires_grad_(True)
    D = x.shape[1]
    w = d["w"].double() if opt["gamma"] else None
    dy = d["dy"].double()
    torch.nn.functional.layer_norm(x, (D,), w, None if w is None else d["b"].double(), LN_EPS).backward(dy)
    dres = x.grad
    ri = None
    if opt["ri"]:
        ri = (d["ri"].bfloat16() if bfr else d["ri"]).double()
        dres = dres + ri
    _, mu, rs = _ln64(x.detach(), None, None)
    xh = (x.detach() - mu[:, None]) * rs[:, None]
    terms = dict(dgamma=dy * xh, dbeta=dy, sum_in=ri, sum_out=dres)
    cols = {}
    for i, k in enumerate(COLS):
        if terms[k] is not None:
            i0 = d["init"][i].double()
            cols[k] = (i0 + terms[k].sum(0), i0.abs() + terms[k].abs().sum(0))
    return dres, cols


def _check_ln_bwd(res, ref, bfr, M, cap, what):
    dres, cols = ref
    if bfr:  # one bf16 rounding of an f32 value within 1e-4 relative of the exact sum: at most 1 ulp off
        _close(_vals(res["dres"], BF16), dres, (1e-5, 0.0), f"{what} dres (bf16 stream)", extra=dres.abs() * 2.0 ** -7)
    else:
        _close(_vals(res["dres"], F32), dres, TOL_F32, f"{what} dres")
    if "dres_bf" in res:
        _close(_vals(res["dres_bf"], BF16), dres, TOL_BF16, f"{what} dres_bf16")
    c = _col_chain(M, cap) + 5
    for k in COLS:
        if k in res:
            exp, mag = cols[k]
            bound = c * U24 * mag
            if M <= 301:  # never looser than the suite's 1e-3 / 1e-4 at its M = 301
                bound = torch.minimum(bound, 1e-3 + 1e-4 * exp.abs())
            _close(_vals(res[k], F32)[:, 0], exp, (0.0, 0.0), f"{what} {k} (c = {c})", extra=bound)


@pytest.mark.parametrize("D", [c[0] for c in LN_BWD_CASES])
def test_layernorm_bwd(D):
    """vj_layernorm_bwd on k_ln_bwd2 and on the float4 fallback k_ln_bwd, and vj_layernorm_bwd_bf16 (kernels
    and NV per D: LN_BWD_CASES), with dy, x, dres_in, dres, dres_bf16 in frames of pairwise different strides,
    mean / rstd (the forward kernel's) and gamma slices of NaN vectors, dgamma / dbeta / sum_in / sum_out slices
    of sentinel vectors pre-set to a non-zero vector, the workspace followed by sentinels; options
    LN_BWD_OPTS. Checks (1)-(4); (3) for the strided fallback compares two different paddings (the
    contiguous call runs the other kernel), (4) repeats the first option set.

    Column vectors: |err| <= c 2^-24 sum_m |term_m| per column, terms in float64 (the initial value counts as
    a term). c = the longest chain of sequential f32 additions plus 5 roundings of one term (x - mean, times
    rstd, times dy, and the f32 mean and rstd it uses). The chain (_col_chain), for nbl = min(ceil(M / 4), cap)
    blocks (cap 768 for k_ln_bwd2, 1024 for k_ln_bwd): a wave adds its rpw = ceil(M / (4 nbl)) rows in sequence;
    the block adds its 4 waves in sequence (3); k_colsum2_multi's thread (one of 32 row groups) spreads its
    ceil(nbl / 32) partials over 4 running sums (ceil(ceil(nbl / 32) / 4)), combines them pairwise (2), then 32
    row groups are added in sequence (32) and the total to the output (1). M = 5: c = 45; M = 301: 45; M = 3077:
    2 + 3 + 6 + 35 + 5 = 51; M = 4101: 2 + 3 + 8 + 35 + 5 = 53. For M <= 301 the bound is capped by the suite's
    1e-3 + 1e-4 |expected| (test_layernorm at M = 301), so it is never looser."""
    from vjepa2_amd import ops

    _, rows, forms = LN_BWD_BY_D[D]
    for M in rows:
        d = _ln_data(M, D, 1)
        stats = {}
        for bfr in (False, True):  # mean / rstd as the forward kernel writes them
            if bfr and "bf" not in forms:
                continue
            _, m, r = ops.layernorm_fwd((d["xb"] if bfr else d["x"]).to(DEV), d["w"].to(DEV), d["b"].to(DEV), LN_EPS,
                                        out_dtype=F32)
            stats[bfr] = (m.cpu(), r.cpu())
        for form in forms:
            bfr = form == "bf"
            cap = 1024 if form == "fb" else 768
            strided_fb = form == "fb" and D % 8 == 0
            for io, opt in enumerate(LN_BWD_OPTS):
                if bfr and io == 2:
                    continue  # without column sums the bf16 form has one output: covered by option 0's dres
                what = f"ln bwd {form} M={M} D={D} opt={io}"
                lds = _ln_bwd_lds(D, form)
                res = _ln_bwd_launch(form, M, D, d, stats[bfr], lds, opt, what)
                _check_ln_bwd(res, _ln_bwd_ref(d, bfr, opt), bfr, M, cap, what)
                other = _ln_bwd_lds(D, form, alt=True) if strided_fb else dict.fromkeys(lds, D)
                _same_all(res, _ln_bwd_launch(form, M, D, d, stats[bfr], other, opt, what + " contiguous"), what)
                if io == 0:
                    _same_all(res, _ln_bwd_launch(form, M, D, d, stats[bfr], lds, opt, what + " repeat"), what + " repeat")


# ------------------------------------------------------------------------------------------------
# Column sums
COLSUM_N = (8, 96, 512, 520, 1032)


def _colsum_launch(fx, M, N, out0, accumulate, what):
    S = min(256, max(1, (M + 63) // 64))
    fo, fws = _ovec(N, F32, out0 if accumulate else None), _ovec(S * N)
    _call("vj_colsum_f32", M, N, _p(fx), int(fx.win.dtype == BF16), fx.ld, _p(fo), int(accumulate), _p(fws), S * N, _st())
    torch.cuda.synchronize()
    fws.read(f"{what} workspace")
    return fo.read(f"{what} out")[:, 0]


@pytest.mark.parametrize("M", [1, 3, 63, 64, 65, 1000, 16389])
def test_colsum_exact(M):
    """vj_colsum_f32 over small integers (randint(-8, 9), bf16 and f32): every partial sum is exactly
    representable whatever the order, so the result must equal the int64 column sums bitwise; one dropped,
    doubled or misaddressed row fails. N = 8 ... 1032 (512 columns per block: N = 520 and 1032 end in an
    8-column block), accumulate on (onto integers) and off (onto the sentinel), x in a frame with padded ld
    and contiguous. M = 16389 reaches the S = 256 cap: slices of 65 rows (a tail row after the 16-row unrolled
    steps), the last non-empty one of 9 rows, three empty. Checks (1)-(4)."""
    g = torch.Generator().manual_seed(M)
    xi = torch.randint(-8, 9, (M, max(COLSUM_N)), generator=g)
    o0 = torch.randint(-100, 101, (max(COLSUM_N),), generator=g)
    for N in COLSUM_N:
        exp = xi[:, :N].sum(0)
        for dt in (BF16, F32):
            x = xi[:, :N].to(dt)
            frames = (InFrame(x, N + 8 + (8 if dt == F32 else 0)), InFrame(x, N))
            for acc in (True, False):
                what = f"colsum M={M} N={N} {'bf16' if dt == BF16 else 'f32'} accumulate={acc}"
                want = (exp + o0[:N] if acc else exp).float().view(torch.int32)
                got = [_colsum_launch(f, M, N, o0[:N].float(), acc, what) for f in frames]
                _same(got[0], want, what)
                _same(got[1], want, what + " contiguous")
                if N == 520:
                    _same(_colsum_launch(frames[0], M, N, o0[:N].float(), acc, what), got[0], what + " repeat")


@pytest.mark.parametrize("N", [10, 1001])
def test_colsum_column_padding_path(N):
    """ops.colsum with N % 8 != 0 (zero-padded columns, a temporary sum, then add / copy), exact integers."""
    from vjepa2_amd import ops

    g = torch.Generator().manual_seed(N)
    for M in (65, 1000):
        xi = torch.randint(-8, 9, (M, N), generator=g)
        o0 = torch.randint(-100, 101, (N,), generator=g)
        for dt in (BF16, F32):
            for acc in (True, False):
                fo = _ovec(N, F32, o0.float())
                ops.colsum(xi.to(dt).to(DEV), fo.win[:, 0], accumulate=acc)
                torch.cuda.synchronize()
                want = (xi.sum(0) + o0 if acc else xi.sum(0)).float().view(torch.int32)
                _same(fo.read(f"ops.colsum N={N}")[:, 0], want, f"ops.colsum M={M} N={N} {dt} accumulate={acc}")


def test_colsum_randn():
    """The suite's randn case (70000 x 96 bf16, accumulate, 5e-3 / 1e-4) in a padded frame, against float64,
    bitwise equal to the contiguous call and to a repeat."""
    M, N = 70000, 96
    g = torch.Generator().manual_seed(5)
    x = torch.randn(M, N, generator=g).bfloat16()
    o0 = torch.ones(N)
    fp, fc = InFrame(x, N + 8), InFrame(x, N)
    got = _colsum_launch(fp, M, N, o0, True, "colsum randn")
    _close(_vals(got, F32), 1.0 + x.double().sum(0), (5e-3, 1e-4), "colsum randn")
    _same(got, _colsum_launch(fc, M, N, o0, True, "colsum randn contiguous"), "colsum randn contiguous")
    _same(got, _colsum_launch(fp, M, N, o0, True, "colsum randn repeat"), "colsum randn repeat")


# ------------------------------------------------------------------------------------------------
# Fused target LayerNorms + JEPA loss
LOSS_GROUPS = {1: [5], 2: [7, 11], 3: [3, 9, 2], 4: [1, 6, 4, 300]}  # R = 5, 18, 14, 311 (> 256, R % 4 = 3)
LOSS_NPAIRS = {1: 1, 2: 4, 3: 3, 4: 2}                               # != len(groups) for 2 and 4 groups
LOSS_TROWS = 50


@functools.lru_cache(maxsize=None)
def _loss_data(D, ng):
    groups = LOSS_GROUPS[ng]
    R = sum(groups)
    g = torch.Generator().manual_seed(104729 * D + ng)
    rows = torch.randint(0, LOSS_TROWS, (R,), generator=g)
    rows[0], rows[-1] = 0, LOSS_TROWS - 1  # the target's first and last row
    if R > 2:
        rows[1] = 0                        # a repeat
    return dict(groups=groups, R=R, rows=rows, z=torch.randn(R, D, generator=g),
                tgt=torch.randn(LOSS_TROWS, D, generator=g), gamma=1 + 0.1 * torch.randn(D, generator=g),
                beta=0.1 * torch.randn(D, generator=g))


def _loss_ref(d, z, tgt, p, npairs):
    """float64: h = LN(LN(tgt[rows]; gamma, beta, 1e-6); 1e-5), then orc.jepa_loss's formula per mask group,
    mean(|z - h|^p) / p, averaged over npairs -> (loss, row_loss, d = z - h, w per row (f32, as the kernel))."""
    D = z.shape[1]
    h = torch.nn.functional.layer_norm(tgt.double()[d["rows"]], (D,), d["gamma"].double(), d["beta"].double(), 1e-6)
    h = torch.nn.functional.layer_norm(h, (D,), None, None, 1e-5)
    diff = z.double() - h
    w32 = torch.cat([(torch.tensor(1.0 / npairs, dtype=F32) / (torch.tensor(float(n), dtype=F32) * float(D))).expand(n)
                     for n in d["groups"]])
    row_loss = w32.double() * (diff.abs() ** p).sum(1) / p
    loss, r0 = 0.0, 0
    for n in d["groups"]:
        loss = loss + torch.mean(diff[r0:r0 + n].abs() ** p) / p
        r0 += n
    return loss / npairs, row_loss, diff, w32


def _loss_launch(d, z, tgt, D, p, npairs, lds, what):
    from vjepa2_amd import _lib

    R = d["R"]
    fz, ft = InFrame(z, lds[0]), InFrame(tgt, lds[1])
    fdz, frl, fl = OutFrame(R, D, lds[2], BF16), _ovec(R), _ovec(1)
    rows = d["rows"].int().to(DEV)
    gamma, beta = _in_vec(d["gamma"]), _in_vec(d["beta"])
    _call("vj_jepa_loss", R, D, _p(fz), int(z.dtype == BF16), fz.ld, _p(ft), int(tgt.dtype == BF16), ft.ld,
          rows.data_ptr(), gamma.data_ptr(), beta.data_ptr(), 1e-6, 1e-5, float(p), len(d["groups"]),
          _lib.int_array(d["groups"]), 1.0 / npairs, _p(fdz), lds[2], _p(frl), _p(fl), _st())
    torch.cuda.synchronize()
    return {"dz": fdz.read(f"{what} dz"), "row_loss": frl.read(f"{what} row_loss"), "loss": fl.read(f"{what} loss")}


@pytest.mark.parametrize("p", [1, 2])
@pytest.mark.parametrize("D", [4, 128, 260, 1024, 1408, 2048])
def test_jepa_loss(D, p):
    """vj_jepa_loss, (z, target) f32 / bf16 in every combination, 1 - 4 mask groups of unequal sizes, npairs !=
    len(groups), loss_rows with repeats and the target's first and last row, z / target / dz in frames with
    padded ldz != ldt != lddz, row_loss and the loss slices of sentinel vectors. Checks (1)-(3).
    Loss and each row_loss: relative 1e-5. p = 1: dz is bitwise bf16(w_g) sign(d) wherever the float64 |d| >
    1e-4 (the excluded share, asserted on the reference alone, is at most 0.1 %: for unit-variance randn z and
    normalised targets d ~ N(0, 2), P(|d| < 1e-4) = 5.6e-5), and one of 0, +-bf16(w_g) elsewhere. p = 2: dz = w_g d
    within one bf16 rounding (rtol 2^-8) plus 1e-3 w_g."""
    b = _r8(D)
    for ng in (1, 2, 3, 4):
        d = _loss_data(D, ng)
        npairs = LOSS_NPAIRS[ng]
        for zbf in (False, True):
            for tbf in (False, True):
                z = d["z"].bfloat16() if zbf else d["z"]
                tgt = d["tgt"].bfloat16() if tbf else d["tgt"]
                what = f"jepa loss D={D} p={p} groups={d['groups']} z_bf16={zbf} tgt_bf16={tbf}"
                res = _loss_launch(d, z, tgt, D, p, npairs, (b + 8, b + 16, b + 24), what)
                loss, row_loss, diff, w32 = _loss_ref(d, z, tgt, p, npairs)
                _close(_vals(res["loss"], F32)[0, 0], loss, (0.0, 1e-5), f"{what} loss")
                _close(_vals(res["row_loss"], F32)[:, 0], row_loss, (0.0, 1e-5), f"{what} row_loss")
                dz = _vals(res["dz"], BF16)
                wb = w32.bfloat16().double()[:, None]
                if p == 1:
                    sure = diff.abs() > 1e-4
                    assert int((~sure).sum()) <= 1e-3 * sure.numel(), f"{what}: {int((~sure).sum())} elements excluded"
                    exp = wb * torch.sign(diff)
                    assert torch.equal(dz[sure], exp.expand_as(dz)[sure]), f"{what}: dz != bf16(w_g) sign(d)"
                    assert bool(((dz == 0) | (dz.abs() == wb))[~sure].all()), f"{what}: dz near d = 0"
                else:
                    wd = w32.double()[:, None]
                    _close(dz, wd * diff, (0.0, 2.0 ** -8), f"{what} dz", extra=(1e-3 * wd).expand_as(dz))
                _same_all(res, _loss_launch(d, z, tgt, D, p, npairs, (D, D, D), what + " contiguous"), what)


# ------------------------------------------------------------------------------------------------
# RoPE
TPR, TPF, NFR = 6, 18, 4  # 6 tokens per row, 3 rows, 18 tokens per frame, 4 frames: frame / height / width
MAXPOS = 6                # positions range over 4 / 3 / 6 values, so a swapped axis changes the angles


def _rope64(q, k, ids, H, hd, inverse):
    """The oracle's apply_rope_qk in float64 on q, k [T, H hd]; inverse: its transpose (autograd)."""
    T = q.shape[0]

    def heads(a):
        return a.reshape(T, H, hd).transpose(0, 1)[None]

    def flat(a):
        return a[0].transpose(0, 1).reshape(T, H * hd)

    if not inverse:
        qr, kr = orc.apply_rope_qk(heads(q), heads(k), ids[None], TPF, TPR)
        return flat(qr), flat(kr)
    zq, zk = torch.zeros_like(q).requires_grad_(True), torch.zeros_like(k).requires_grad_(True)
    qr, kr = orc.apply_rope_qk(heads(zq), heads(zk), ids[None], TPF, TPR)
    ((flat(qr) * q).sum() + (flat(kr) * k).sum()).backward()
    return zq.grad, zk.grad


def _rope_launch(data, T, H, hd, dt, padded, ids, ids_mod, inverse, tabs, what):
    """In place on a [T, W] window of a sentinel frame. padded: a row is [8 gap | q | 16 gap | k | 8 gap | v | 8
    gap] (q_off = 8, k_off = 8 + D + 16, ld = 3 D + 56), the gaps hold the sentinel; else [q | k | v], ld = 3 D.
    Returns the window's bits before and after, and (q_off, k_off, v_off)."""
    D = H * hd
    offs = (8, 24 + D, 32 + 2 * D) if padded else (0, D, 2 * D)
    W = 3 * D + 40 if padded else 3 * D
    f = OutFrame(T, W, W + 16 if padded else W, dt)
    idt, sent = SENTINEL[dt]
    before = torch.full((T, W), sent, dtype=idt)
    for o, part in zip(offs, data):
        before[:, o:o + D] = part.view(idt)
    f.win.copy_(before.view(dt).to(DEV))
    half = (hd // 3) // 2
    args = [T, H, hd, _p(f), f.ld, offs[0], offs[1], None if ids is None else ids.data_ptr(), ids_mod, TPF, TPR,
            tabs[0].data_ptr(), tabs[1].data_ptr(), half]
    if dt == F32:
        _call("vj_rope_f32", *args, _st())
    else:
        _call("vj_rope", *args, int(inverse), _st())
    torch.cuda.synchronize()
    return before, f.read(what), offs


@pytest.mark.parametrize("hd", [8, 24, 32, 64, 80, 88, 128])
def test_rope(hd):
    """vj_rope (bf16, forward and inverse) and vj_rope_f32 on a non-square token grid (6 per row, 3 rows, 18 per
    frame), H = 1 and 3, T = 1, 33, 200, ids given and ids = None with ids_mod = 54; q, k, v at q_off = 8, k_off =
    8 + D + 16, v behind, ld = 3 D + 56 in a sentinel frame with the cos / sin tables slices of NaN vectors.
    Every element outside the rotated part of the q and k windows (v, the gaps, each head's tail beyond 3 sw)
    keeps its bits. hd = 24 has no tail; hd = 80, 88, 128 end the rotated part inside an 8-chunk. Reference:
    the oracle in float64; bf16 1e-5 / 8e-3 (the suite's), f32 atol 1e-6, rtol 1e-5. Checks (1)-(3)."""
    cos_t, sin_t = orc.rope_tables(hd, MAXPOS)
    tabs = (_in_vec(cos_t.reshape(-1)), _in_vec(sin_t.reshape(-1)))
    sw = 2 * ((hd // 3) // 2)
    for H in (1, 3):
        D = H * hd
        rotated = (torch.arange(D) % hd) < 3 * sw
        for T in (1, 33, 200):
            g = torch.Generator().manual_seed(1000 * hd + 10 * T + H)
            ids_cpu = torch.randint(0, NFR * TPF, (T,), generator=g)
            raw = [torch.randn(T, D, generator=g) for _ in range(3)]
            for dt, inverse in ((BF16, False), (BF16, True), (F32, False)):
                data = [r.to(dt) for r in raw]
                for use_ids in (True, False):
                    ids = ids_cpu if use_ids else torch.arange(T) % (3 * TPF)
                    ids_d = ids.int().to(DEV) if use_ids else None
                    what = f"rope hd={hd} H={H} T={T} {dt} inverse={inverse} ids={'given' if use_ids else 'mod 54'}"
                    before, after, offs = _rope_launch(data, T, H, hd, dt, True, ids_d, 0 if use_ids else 3 * TPF,
                                                       inverse, tabs, what)
                    keep = torch.ones(before.shape[1], dtype=torch.bool)
                    for o in offs[:2]:
                        keep[o:o + D] = ~rotated
                    _same(after[:, keep], before[:, keep], f"{what}: outside the rotated q / k elements")
                    eq, ek = _rope64(data[0].double(), data[1].double(), ids, H, hd, inverse)
                    tol = (1e-5, 8e-3) if dt == BF16 else (1e-6, 1e-5)
                    _close(_vals(after[:, offs[0]:offs[0] + D], dt), eq, tol, f"{what} q")
                    _close(_vals(after[:, offs[1]:offs[1] + D], dt), ek, tol, f"{what} k")
                    _, cont, coffs = _rope_launch(data, T, H, hd, dt, False, ids_d, 0 if use_ids else 3 * TPF, inverse,
                                                  tabs, what + " contiguous")
                    for o, co, name in zip(offs, coffs, "qkv"):
                        _same(after[:, o:o + D], cont[:, co:co + D], f"{what} {name} vs contiguous")


# ------------------------------------------------------------------------------------------------
# AdamW, EMA, check-finite, cast
N_BIG = 4 * (4096 * 256 + 257)  # one grid-stride trip of 4096 blocks x 256 threads x 4 floats, plus a partial wave
MOM = 0.99925
ADAM = dict(lr=5e-4, b1=0.9, b2=0.999, eps=1e-8)


@functools.lru_cache(maxsize=None)
def _adam_data(n):
    g = torch.Generator().manual_seed(n)
    d = dict(p=torch.randn(n, generator=g), g=torch.randn(n, generator=g), m=0.1 * torch.randn(n, generator=g),
             v=torch.rand(n, generator=g), t=torch.randn(n, generator=g))
    d["g"][0] = d["m"][0] = d["v"][0] = 0.0  # degenerate: denominator eps, update 0 / eps = 0
    return d


def _adam64(d, wd, step, gs):
    """float64 AdamW with decoupled weight decay (torch.optim.AdamW's math)."""
    p, g, m, v = (d[k].double() for k in "pgmv")
    g = g * gs
    p = p * (1.0 - ADAM["lr"] * wd)
    m = m + (1.0 - ADAM["b1"]) * (g - m)
    v = v * ADAM["b2"] + (1.0 - ADAM["b2"]) * g * g
    den = v.sqrt() / math.sqrt(1.0 - ADAM["b2"] ** step) + ADAM["eps"]
    return p - ADAM["lr"] / (1.0 - ADAM["b1"] ** step) * (m / den), m, v


def _adam_launch(d, n, wd, step, gs, pbf=True, flag=None, ema=None, what="adamw"):
    """vj_adamw (ema None), vj_adamw_ema (ema 'fused') or vj_adamw then vj_ema (ema 'separate') on p, m, v, t
    (+ bf16 copies) inside sentinel buffers; returns {name: bits} after (1)."""
    fr = {k: _oflat(n, F32, d[k]) for k in ("p", "m", "v")}
    if pbf:
        fr["pbf"] = _oflat(n, BF16)
    if ema:
        fr["t"], fr["tbf"] = _oflat(n, F32, d["t"]), _oflat(n, BF16)
    g = _in_vec(d["g"])
    fp = None if flag is None else flag.data_ptr()
    hp = [ADAM["lr"], ADAM["b1"], ADAM["b2"], ADAM["eps"], wd, step, gs, fp]
    base = [n, _p(fr["p"]), g.data_ptr(), _p(fr["m"]), _p(fr["v"]), _p(fr.get("pbf"))]
    if ema == "fused":
        _call("vj_adamw_ema", *base, *hp, _p(fr["t"]), _p(fr["tbf"]), MOM, _st())
    else:
        _call("vj_adamw", *base, *hp, _st())
        if ema:
            _call("vj_ema", n, _p(fr["t"]), _p(fr["p"]), MOM, _p(fr["tbf"]), _st())
    torch.cuda.synchronize()
    return {k: f.read(f"{what} {k}").reshape(-1) for k, f in fr.items()}


def _check_adam(res, d, wd, step, gs, what):
    p, m, v = _adam64(d, wd, step, gs)
    _close(_vals(res["p"], F32), p, (1e-7, 2e-6), f"{what} p")
    _close(_vals(res["m"], F32), m, (1e-7, 2e-6), f"{what} m")
    _close(_vals(res["v"], F32), v, (1e-7, 4e-6), f"{what} v")
    if "pbf" in res:
        _same(res["pbf"], res["p"].view(F32).bfloat16().view(torch.int16), f"{what} p_bf16")
    assert float(_vals(res["p"], F32)[0]) == float(d["p"][0] * torch.tensor(1.0 - ADAM["lr"] * wd, dtype=F32))


@pytest.mark.parametrize("n", [4, 4100])
def test_adamw_variants(n):
    """vj_adamw against float64 (relative 2e-6, v 4e-6, atol 1e-7; the suite's bounds): grad_scale 1 / 0.5,
    weight_decay 0.04 / 0, step 1 / 1000, with and without p_bf16; element 0 has g = m = v = 0 and must come out
    as p (1 - lr wd) exactly (finite: 0 / eps). p, m, v, p_bf16 end in sentinels."""
    d = _adam_data(n)
    for gs in (1.0, 0.5):
        for wd in (0.04, 0.0):
            for step in (1, 1000):
                for pbf in (True, False):
                    what = f"adamw n={n} grad_scale={gs} wd={wd} step={step} p_bf16={pbf}"
                    _check_adam(_adam_launch(d, n, wd, step, gs, pbf=pbf, what=what), d, wd, step, gs, what)


def _ema64(t, p):
    momf = float(torch.tensor(MOM, dtype=F32))
    return t.double() * momf + (1.0 - momf) * p


def test_adamw_ema_past_the_grid_cap():
    """n = 4 (4096 x 256 + 257): k_adamw / k_ema take a second grid-stride trip that ends in a partial wave.
    AdamW against float64; fused vj_adamw_ema bitwise equal to vj_adamw + vj_ema; a step skipped by found_inf
    leaves p, m, v bitwise untouched while the EMA is still applied (to the old parameters)."""
    n = N_BIG
    d = _adam_data(n)
    sep = _adam_launch(d, n, 0.04, 3, 0.5, ema="separate", what="adamw + ema")
    _check_adam(sep, d, 0.04, 3, 0.5, "adamw n=N_BIG")
    _close(_vals(sep["t"], F32), _ema64(d["t"], _vals(sep["p"], F32)), (1e-7, 1e-6), "ema n=N_BIG")
    _same(sep["tbf"], sep["t"].view(F32).bfloat16().view(torch.int16), "ema target_bf16")
    _same_all(_adam_launch(d, n, 0.04, 3, 0.5, ema="fused", what="adamw_ema"), sep, "fused vs separate")
    flag = torch.ones(1, dtype=torch.int32, device=DEV)
    skipped = _adam_launch(d, n, 0.04, 3, 0.5, pbf=False, flag=flag, ema="fused", what="adamw_ema skipped")
    for k in "pmv":
        _same(skipped[k], d[k].view(torch.int32), f"skipped step {k}")
    _close(_vals(skipped["t"], F32), _ema64(d["t"], d["p"].double()), (1e-7, 1e-6), "ema of a skipped step")
    _same(skipped["t"], _adam_launch(d, n, 0.04, 3, 0.5, pbf=False, flag=flag, ema="separate", what="skipped separate")["t"],
          "skipped step: fused vs separate EMA")


def test_check_finite():
    """k_check_finite at n = 4 (4096 x 256 + 257): a single NaN (or inf) in the last float4, and one in the
    second grid-stride trip, raise the flag; +-3e38 and denormals do not; a flag that is already 1 stays 1."""
    n = N_BIG
    base = torch.randn(n, generator=torch.Generator().manual_seed(11))
    base[:4] = torch.tensor([3e38, -3e38, 1e-40, -1e-42])
    base[-4:] = torch.tensor([1e-45, -3e38, 3e38, 0.0])

    def run(x, flag0):
        buf = _in_vec(x)
        flag = _ovec(1)
        flag.win.view(torch.int32).fill_(flag0)
        _call("vj_check_finite", x.numel(), buf.data_ptr(), _p(flag), _st())
        torch.cuda.synchronize()
        return int(flag.read("check_finite flag")[0, 0])

    assert run(base, 0) == 0
    assert run(base, 1) == 1
    for idx, bad in ((n - 1, float("nan")), (n - 3, float("-inf")), (4 * 4096 * 256 + 5, float("nan")), (0, float("inf"))):
        x = base.clone()
        x[idx] = bad
        assert run(x, 0) == 1, f"{bad} at {idx} of {n} not found"
    small = base[:8].clone()
    assert run(small, 0) == 0
    small[7] = float("nan")
    assert run(small, 0) == 1


@pytest.mark.parametrize("in_off,out_off", [(0, 0), (1, 1), (0, 1), (1, 0), (0, 4)])
def test_cast_bf16(in_off, out_off):
    """vj_cast_bf16 bitwise against tensor.bfloat16() for n = 1, 3, 4, 7, 4101 and N_BIG + 1 (a second
    grid-stride trip and a scalar tail), over ties-to-even pairs, +-0, +-inf, NaN, denormals and values that
    round to inf. in / out start in_off / out_off elements off 16-B alignment: (0, 0) and (0, 4) (out 8-B
    aligned) take the vector kernel, an odd offset on either side makes the scalar kernel do it all. A
    sentinel behind out[n]. A NaN must come out as a NaN: its payload is not compared, tensor.bfloat16() itself
    gives 0x7FC0 from its scalar and 0xFFFF from its vectorised CPU path."""
    sp = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), 1.0 + 2.0 ** -8 + 2.0 ** -20, 0.0, -0.0,
                       float("inf"), float("-inf"), float("nan"), 1e-40, -1e-40, 9.2e-41, 3.3961775e38, -3.4e38, 3.38e38,
                       2.0 ** -126, 1.0 - 2.0 ** -9, 1.0 - 2.0 ** -10])
    g = torch.Generator().manual_seed(12)
    for n in (1, 3, 4, 7, 4101, N_BIG + 1):
        x = torch.randn(n, generator=g) * 50
        k = min(n, sp.numel())
        x[n - k:] = sp[:k]
        if n > 2 * k:
            x[:k] = sp[:k]
        what = f"cast_bf16 n={n} in_off={in_off} out_off={out_off}"
        src = _in_vec(torch.cat([torch.full((in_off,), float("nan")), x]))[in_off:]
        out = _ovec(n, BF16, shift_bytes=2 * out_off)
        assert src.data_ptr() % 16 == 4 * in_off and out.win.data_ptr() % 16 == 2 * out_off
        _call("vj_cast_bf16", n, src.data_ptr(), _p(out), _st())
        torch.cuda.synchronize()
        got, want = out.read(what)[:, 0], x.bfloat16().view(torch.int16)
        nan = x.isnan()
        assert bool(got.view(BF16)[nan].isnan().all()), f"{what}: NaN not kept"
        _same(got[~nan], want[~nan], what)


# ------------------------------------------------------------------------------------------------
# Row copies
@pytest.mark.parametrize("dt,C", [(F32, 4), (F32, 1408), (BF16, 8), (BF16, 2048)])
def test_gather_scatter_rows(dt, C):
    """vj_gather_rows (gather with duplicate indices, and scatter), rows of 1 to 352 uint4 under 64 threads
    (f32 x 1408: 352, bf16 x 2048: 256: the per-row loop iterates), padded strides on both sides, bitwise,
    guard bands; scatter leaves the rows it does not name untouched."""
    es = 4 if dt == F32 else 2
    idt = SENTINEL[dt][0]
    g = torch.Generator().manual_seed(C)
    S, R = 40, 23
    src = torch.randn(S, C, generator=g).to(dt)
    idx = torch.randint(0, S, (R,), generator=g)
    idx[:4] = torch.tensor([0, S - 1, 7, 7])
    perm = torch.randperm(S, generator=g)[:R]
    small = torch.randn(R, C, generator=g).to(dt)
    dst0 = torch.randn(S, C, generator=g).to(dt)
    out = {}
    for lds, ldd in ((C + 8, C + 16), (C, C)):
        fs, fd = _frame(src, lds), OutFrame(R, C, ldd, dt)
        idx_d, perm_d = idx.int().to(DEV), perm.int().to(DEV)
        _call("vj_gather_rows", R, C * es, _p(fs), lds * es, idx_d.data_ptr(), _p(fd), ldd * es, 0, _st())
        fr, fo = _frame(small, lds), OutFrame(S, C, ldd, dt)
        fo.fill(dst0)
        _call("vj_gather_rows", R, C * es, _p(fr), lds * es, perm_d.data_ptr(), _p(fo), ldd * es, 1, _st())
        torch.cuda.synchronize()
        out[lds] = (fd.read(f"gather C={C}"), fo.read(f"scatter C={C}"))
    exp = dst0.clone()
    exp[perm] = small
    for lds, (ga, sc) in out.items():
        _same(ga, src[idx].view(idt), f"gather {dt} C={C} lds={lds}")
        _same(sc, exp.view(idt), f"scatter {dt} C={C} lds={lds}")


@pytest.mark.parametrize("D", [1, 96, 130, 1408])
def test_fill_rows(D):
    """vj_fill_rows: the named rows get the vector (under 128 threads: D = 130 and 1408 iterate, D = 1 uses one
    lane), every other row and the guard band keep their bits."""
    g = torch.Generator().manual_seed(D)
    S = 20
    dst0, vec = torch.randn(S, D, generator=g), torch.randn(D, generator=g)
    idx = torch.tensor([0, S - 1, 5, 11])
    out = []
    for ldd in (D + 8, D):
        fo, idx_d, vec_d = OutFrame(S, D, ldd, F32), idx.int().to(DEV), _in_vec(vec)
        fo.fill(dst0)
        _call("vj_fill_rows", idx.numel(), D, _p(fo), ldd, idx_d.data_ptr(), vec_d.data_ptr(), _st())
        torch.cuda.synchronize()
        out.append(fo.read(f"fill_rows D={D} ldd={ldd}"))
    exp = dst0.clone()
    exp[idx] = vec
    _same(out[0], exp.view(torch.int32), f"fill_rows D={D}")
    _same(out[1], exp.view(torch.int32), f"fill_rows D={D} contiguous")


@pytest.mark.parametrize("D", [4, 130, 1408])
def test_add_rows(D):
    """vj_add_rows with idx (one id = -1 and one = trows: those rows are left untouched, as the kernel
    documents) and with idx_mod, padded ldd / ldt, bitwise against the f32 add, guard bands."""
    g = torch.Generator().manual_seed(D)
    R, trows = 19, 9
    dst0, table = torch.randn(R, D, generator=g), torch.randn(trows, D, generator=g)
    idx = torch.randint(0, trows, (R,), generator=g)
    idx[0], idx[1], idx[2], idx[3] = 0, trows - 1, -1, trows
    valid = (idx >= 0) & (idx < trows)
    exp_idx = dst0.clone()
    exp_idx[valid] = dst0[valid] + table[idx[valid]]
    exp_mod = dst0 + table[torch.arange(R) % 7]
    for ldd, ldt in ((_r8(D) + 16, _r8(D) + 8), (D, D)):
        for use_idx, exp in ((True, exp_idx), (False, exp_mod)):
            fo, ft = OutFrame(R, D, ldd, F32), InFrame(table, ldt)
            fo.fill(dst0)
            ip = idx.int().to(DEV)
            _call("vj_add_rows", R, D, _p(fo), ldd, _p(ft), ldt, trows, ip.data_ptr() if use_idx else None,
                  0 if use_idx else 7, _st())
            torch.cuda.synchronize()
            _same(fo.read(f"add_rows D={D}"), exp.view(torch.int32), f"add_rows D={D} ldd={ldd} idx={use_idx}")


@pytest.mark.parametrize("n", [1, 257])
def test_ids64to32(n):
    ids = torch.randint(0, 2 ** 31 - 1, (n,), generator=torch.Generator().manual_seed(n))
    ids[0] = 2 ** 31 - 1
    out, ids_d = _ovec(n), ids.to(DEV)
    _call("vj_ids64to32", n, ids_d.data_ptr(), _p(out), _st())
    torch.cuda.synchronize()
    _same(out.read(f"ids64to32 n={n}")[:, 0], ids.int(), f"ids64to32 n={n}")


# ------------------------------------------------------------------------------------------------
# Transposes
TRANSPOSE_SHAPES = [(8, 8), (8, 264), (264, 8), (72, 200), (136, 64)]


def test_transpose_bf16_strided():
    """vj_transpose_bf16 and one vj_transpose_bf16_batch launch mixing all the shapes, ld_src = cols + 8 and
    ld_dst = rows + 16 (and contiguous), bitwise, guard bands."""
    from vjepa2_amd import ops

    g = torch.Generator().manual_seed(13)
    mats = [torch.randn(r, c, generator=g).bfloat16() for r, c in TRANSPOSE_SHAPES]
    for padded in (True, False):
        srcs = [InFrame(m, m.shape[1] + (8 if padded else 0)) for m in mats]
        single = [OutFrame(m.shape[1], m.shape[0], m.shape[0] + (16 if padded else 0), BF16) for m in mats]
        batch = [OutFrame(m.shape[1], m.shape[0], m.shape[0] + (16 if padded else 0), BF16) for m in mats]
        for m, s, o in zip(mats, srcs, single):
            _call("vj_transpose_bf16", m.shape[0], m.shape[1], _p(s), s.ld, _p(o), o.ld, _st())
        desc, tiles = ops.transpose_batch_desc([(s.win, o.win) for s, o in zip(srcs, batch)])
        ops.transpose_bf16_batch(desc, len(mats), tiles)
        torch.cuda.synchronize()
        for m, o, ob in zip(mats, single, batch):
            want = m.t().contiguous().view(torch.int16)
            _same(o.read(f"transpose {tuple(m.shape)}"), want, f"transpose {tuple(m.shape)} padded={padded}")
            _same(ob.read(f"batched transpose {tuple(m.shape)}"), want, f"batched transpose {tuple(m.shape)} padded={padded}")


# ------------------------------------------------------------------------------------------------
# Argument checks: refused on the host, nothing launched, the output untouched
def test_argument_checks():
    g = torch.Generator().manual_seed(14)
    M, W = 4, 2064
    x = InFrame(torch.randn(M, W, generator=g), W + 8)
    xb = InFrame(torch.randn(M, W, generator=g).bfloat16(), W + 8)
    vec = _in_vec(torch.randn(W, generator=g))
    stat = _in_vec(torch.ones(M))
    rows = torch.zeros(M, dtype=torch.int32, device=DEV)
    tab = _in_vec(torch.ones(64))
    from vjepa2_amd import _lib

    def refused(outs, name, *args):
        with pytest.raises(RuntimeError, match=name):
            _call(name, *args, _st())
        torch.cuda.synchronize()
        for k, f in enumerate(outs):
            w = f.read(f"{name} output {k}")
            assert bool((w == f.sent).all()), f"{name}: a refused call wrote output {k}"

    for D in (6, 2052):
        y, m, r = OutFrame(M, W, W + 8, F32), _ovec(M), _ovec(M)
        refused([y, m, r], "vj_layernorm_fwd", M, D, _p(x), 0, x.ld, vec.data_ptr(), vec.data_ptr(), LN_EPS, _p(y), 1,
                y.ld, _p(m), _p(r))
        dres, dgm, dbt, ws = OutFrame(M, W, W + 8, F32), _ovec(W), _ovec(W), _ovec(2 * W)
        refused([dres, dgm, dbt, ws], "vj_layernorm_bwd", M, D, _p(xb), xb.ld, _p(x), x.ld, stat.data_ptr(),
                stat.data_ptr(), vec.data_ptr(), None, 0, _p(dres), dres.ld, None, 0, _p(dgm), _p(dbt), None, None,
                _p(ws), 2 * W)
        dz, rl, ls = OutFrame(M, W, W + 8, BF16), _ovec(M), _ovec(1)
        refused([dz, rl, ls], "vj_jepa_loss", M, D, _p(x), 0, x.ld, _p(x), 0, x.ld, rows.data_ptr(), vec.data_ptr(),
                vec.data_ptr(), 1e-6, 1e-5, 1.0, 1, _lib.int_array([M]), 1.0, _p(dz), dz.ld, _p(rl), _p(ls))
    out, ws = _ovec(16), _ovec(16)
    refused([out, ws], "vj_colsum_f32", M, 12, _p(x), 0, x.ld, _p(out), 0, _p(ws), 16)
    qkv = OutFrame(M, 192, 200, BF16)
    refused([qkv], "vj_rope", M, 1, 64, _p(qkv), qkv.ld, 0, 64, rows.data_ptr(), 0, TPF, TPR, tab.data_ptr(),
            tab.data_ptr(), 8, 0)  # hd = 64: half must be 10
    qkv32 = OutFrame(M, 192, 200, F32)
    refused([qkv32], "vj_rope_f32", M, 1, 64, _p(qkv32), qkv32.ld, 0, 64, rows.data_ptr(), 0, TPF, TPR, tab.data_ptr(),
            tab.data_ptr(), 11)
    p, m, v, pbf = _ovec(8), _ovec(8), _ovec(8), _ovec(8, BF16)
    refused([p, m, v, pbf], "vj_adamw", 6, _p(p), vec.data_ptr(), _p(m), _p(v), _p(pbf), 5e-4, 0.9, 0.999, 1e-8, 0.04, 1,
            1.0, None)
