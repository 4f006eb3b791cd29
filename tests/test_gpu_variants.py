"""GPU: the block-variant kernels of csrc/vj_variants.hip (SwiGLU gate, stochastic-depth row scale, dropout) with
padded, pairwise different leading dimensions inside poisoned frames, against CPU references, through both trips
of their grid-stride loops.

Every call is made twice: on operands that are windows (tests/test_gpu_gemm_strided.py's InFrame, tests/
test_gpu_rowops.py's InFrame4) of NaN-filled buffers with outputs in sentinel-filled OutFrames, scale a slice of a
NaN-padded vector, and on contiguous copies. Checks: (1) the guard band keeps its sentinel; (2) the window
matches the reference of tests/kernel_refs.py (SwiGLU: float64 with the derived bounds and the share of bitwise
matches; row scale and dropout: the same bf16-rounded arithmetic on the CPU, bitwise, NaN as NaN); (3) the framed
and the contiguous results are bitwise equal. stream_blocks caps the grid at 8192 blocks of 256 threads, so
the loops take a second trip from 2,097,153 chunks on: M = 8200 rows of 257 chunks (2,107,400) get there.

Instantiations and trips launched:
  k_swiglu_fwd, k_swiglu_bwd   (M, h) = (1, 8), (37, 344), (3, 2056), one trip, and (8200, 2056), two; leading
                               dimensions 2h + 8, h + 16, h + 24, 2h + 32; the edge values of
                               kernel_refs.SWIGLU_EDGES in row 0 (zeros, tiny values, the zero of silu', +-20,
                               +-88, +-100, +-3e38, NaN)
  k_rowscale_add<RB>           RB in {0, 1}; (M, N) = (1, 4), (777, 136), (8200, 1028) (two trips); leading
  k_rowscale_bf16              dimensions N + 4, N + 8, N + 12 (one of them = 4 mod 8); scale 0 and bf16(1 / keep);
                               +-inf and NaN in y on a row whose scale is 0 (-> NaN, as in torch)
  k_dropout<XF32, MODE>        all eight at (300, 520), p in {0, 0.1, 0.5, 0.999}, seeds 0, 987654321, 0xFFFFFFFF;
                               <true, 1> and <false, 0> at (8200, 1028) (two trips); (70000, 8): row id x
                               0x9e3779b1 wraps uint32 many times; the backward identity (the same call on a
                               gradient with the same seed). The reference threshold is round(float32(p) 2^32):
                               the entry point receives p as a float; at the four seeds of
                               kernel_refs.DROPOUT_GAP_CASES one element's hash lies between that and the
                               double's threshold, so either side thresholding the double fails there.
  argument checks              h % 8 != 0, ld < 2h, N % 4 != 0, p = 1, aux and resid together, a misaligned
                               pointer: an error code and a message, and no launch (the output keeps its sentinel)
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

import kernel_refs as kr  # noqa: E402
from test_gpu_gemm_strided import BF16, DEV, F32, InFrame, OutFrame, _in_vec  # noqa: E402
from test_gpu_rowops import InFrame4, _same  # noqa: E402

I16, I32 = torch.int16, torch.int32


def _call(name, *args):
    from vjepa2_amd import _lib

    return _lib.call(name, *args)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _frame(t, ld):
    return InFrame(t, ld) if ld == t.shape[1] or ld % 8 == 0 else InFrame4(t, ld)


def _p(f):
    return None if f is None else f.win.data_ptr()


def _eq_nan(got_bits, exp, what):
    """Bitwise equal to exp (a bf16 / f32 tensor), NaN as NaN."""
    got = got_bits.view(exp.dtype)
    ok = kr.same_bits_or_nan(got, exp)
    assert bool(ok.all()), (f"{what}: {int((~ok).sum())} of {ok.numel()} elements differ; first at "
                            f"{[int(v) for v in (~ok).nonzero()[0]]}")


# ------------------------------------------------------------------------------------------------
# SwiGLU
def _swiglu_run(x12, dh, framed, what):
    M, h = dh.shape
    ld, ldo, lddh, lddx = (2 * h + 8, h + 16, h + 24, 2 * h + 32) if framed else (2 * h, h, h, 2 * h)
    fx, fg = InFrame(x12, ld), InFrame(dh, lddh)
    fo, fd = OutFrame(M, h, ldo, BF16), OutFrame(M, 2 * h, lddx, BF16)
    _call("vj_swiglu_fwd", M, h, _p(fx), ld, _p(fo), ldo, _st())
    _call("vj_swiglu_bwd", M, h, _p(fg), lddh, _p(fx), ld, _p(fd), lddx, _st())
    torch.cuda.synchronize()
    return fo.read(f"{what} out"), fd.read(f"{what} dx12")


@pytest.mark.parametrize("shape", kr.SWIGLU_SMALL + [kr.SWIGLU_LARGE], ids=lambda s: f"{s[0]}x{s[1]}")
def test_swiglu_fwd_bwd(shape):
    M, h = shape
    x12, dh = kr.swiglu_inputs(M, h)
    what = f"swiglu M={M} h={h}"
    out, dx = _swiglu_run(x12, dh, True, what)
    out_c, dx_c = _swiglu_run(x12, dh, False, what + " contiguous")
    _same(out, out_c, what + " out framed vs contiguous")
    _same(dx, dx_c, what + " dx12 framed vs contiguous")
    ref = kr.swiglu_ref64(x12, dh)
    dxv = dx.view(BF16)
    r = (kr.check_swiglu(out.view(BF16), ref["v"], ref["bound"], ref["m"], what + " fwd"),
         kr.check_swiglu(dxv[:, :h], ref["v1"], ref["bound1"], ref["m1"], what + " dx1"),
         kr.check_swiglu(dxv[:, h:], ref["v2"], ref["bound2"], ref["m2"], what + " dx2"))
    print(f"{what}: largest error / bound fwd {r[0]:.4f} dx1 {r[1]:.4f} dx2 {r[2]:.4f}")


# ------------------------------------------------------------------------------------------------
# row scale
@pytest.mark.parametrize("shape", [(1, 4), (777, 136), (8200, 1028)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_rowscale(shape):
    M, N = shape
    g = torch.Generator().manual_seed(M + N)
    y = 3 * torch.randn(M, N, generator=g)
    resid = torch.randn(M, N, generator=g)
    inv = float(torch.tensor(1 / 0.9).bfloat16())
    scale = torch.where(torch.rand(M, generator=g) < 0.3, 0.0, inv)
    if M > 1:
        scale[1] = 0.0
        y[1, 0], y[1, 1], y[1, N - 1] = float("inf"), float("-inf"), float("nan")
        scale[0] = inv
    sv = _in_vec(scale)
    for kind in ("add_f32", "add_bf16", "bf16"):
        r = None if kind == "bf16" else (resid if kind == "add_f32" else resid.bfloat16())
        exp = kr.rowscale_ref(y, scale, r)
        assert M == 1 or bool(exp[1, [0, 1, N - 1]].isnan().all())
        res = []
        for framed in (True, False):
            what = f"rowscale {kind} M={M} N={N} framed={framed}"
            ldy, ldr, ldo = (N + 4, N + 8, N + 12) if framed else (N, N, N)
            fy = _frame(y, ldy)
            fo = OutFrame(M, N, ldo, exp.dtype)
            if r is None:
                _call("vj_rowscale_bf16", M, N, _p(fy), ldy, sv.data_ptr(), _p(fo), ldo, _st())
            else:
                fr = _frame(r, ldr)
                _call("vj_rowscale_add", M, N, _p(fy), ldy, sv.data_ptr(), _p(fr), ldr, _p(fo), ldo,
                      int(r.dtype == BF16), _st())
            torch.cuda.synchronize()
            res.append(fo.read(what))
            _eq_nan(res[-1], exp, what)
        _same(res[0], res[1], f"rowscale {kind} M={M} N={N} framed vs contiguous")


# ------------------------------------------------------------------------------------------------
# dropout
MODES = ("plain", "resid_f32", "resid_bf16", "aux")


def _drop_data(M, N):
    g = torch.Generator().manual_seed(3 * M + N)
    x = 3 * torch.randn(M, N, generator=g)
    return dict(x=x, xb=x.bfloat16(), resid=torch.randn(M, N, generator=g), aux=torch.randn(M, N, generator=g).bfloat16())


def _drop_case(d, x_f32, mode, p, seed, what):
    """One (XF32, MODE) instantiation, framed and contiguous, against dropout_ref; returns the expected tensor."""
    x = d["x"] if x_f32 else d["xb"]
    M, N = x.shape
    resid = {"resid_f32": d["resid"], "resid_bf16": d["resid"].bfloat16()}.get(mode)
    aux = d["aux"] if mode == "aux" else None
    exp = kr.dropout_ref(x, p, seed, resid=resid, aux=aux)
    res = []
    for framed in (True, False):
        ldx, lda, ldr, ldo = (N + 4, N + 8, N + 12, N + 16) if framed else (N, N, N, N)
        fx = _frame(x, ldx)
        fa = None if aux is None else _frame(aux, lda)
        fr = None if resid is None else _frame(resid, ldr)
        fo = OutFrame(M, N, ldo, exp.dtype)
        _call("vj_dropout", M, N, _p(fx), ldx, int(x_f32), _p(fa), lda if fa else 0, _p(fr), ldr if fr else 0,
              int(mode == "resid_f32"), _p(fo), ldo, p, seed, _st())
        torch.cuda.synchronize()
        res.append(fo.read(f"{what} framed={framed}"))
        _eq_nan(res[-1], exp, f"{what} framed={framed}")
    _same(res[0], res[1], f"{what} framed vs contiguous")
    return exp


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("x_f32", [True, False], ids=["xf32", "xbf16"])
def test_dropout_every_instantiation(x_f32, mode):
    M, N = 300, 520
    d = _drop_data(M, N)
    for p in (0.0, 0.1, 0.5, 0.999):
        for seed in (0, 987654321, 0xFFFFFFFF):
            exp = _drop_case(d, x_f32, mode, p, seed, f"dropout x_f32={x_f32} {mode} p={p} seed={seed}")
            if p == 0.0 and mode == "plain":  # everything kept, scale 1
                assert torch.equal(exp, d["x"].bfloat16())


@pytest.mark.parametrize("x_f32,mode,shape", [(True, "resid_f32", (8200, 1028)), (False, "plain", (8200, 1028)),
                                              (False, "plain", (70000, 8))],
                         ids=["xf32-resid_f32-second-trip", "xbf16-plain-second-trip", "row-hash-wraps"])
def test_dropout_large(x_f32, mode, shape):
    """(8200, 1028): 2,107,400 chunks, the second grid-stride trip; (70000, 8): row * 0x9e3779b1 exceeds 2^32 from
    row 2 on and wraps 43,000 times."""
    _drop_case(_drop_data(*shape), x_f32, mode, 0.3, 987654321, f"dropout x_f32={x_f32} {mode} {shape}")


@pytest.mark.parametrize("p,seed,at", kr.DROPOUT_GAP_CASES)
def test_dropout_threshold_is_the_f32_value_of_p(p, seed, at):
    """Seeds (found by search) at which one element's hash lies between round(p 2^32) of the double p and of
    float32(p): a reference that thresholds the double keeps that element, the library drops it."""
    M, N = 300, 520
    r, c = at
    assert not bool(kr.dropout_keep(seed, M, N, p)[r, c])
    _drop_case(_drop_data(M, N), True, "plain", p, seed, f"dropout p={p} seed={seed}")


def test_dropout_backward_is_the_same_call_on_the_gradient():
    M, N, p, seed = 300, 520, 0.3, 4242
    d = _drop_data(M, N)
    keep = kr.dropout_keep(seed, M, N, p)
    fwd = _drop_case(d, False, "plain", p, seed, "dropout forward")
    gy = d["aux"]  # a bf16 gradient
    bwd = _drop_case(dict(d, xb=gy), False, "plain", p, seed, "dropout backward")
    sc = float(torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(p)))
    assert torch.equal(bwd, (keep.float() * gy.float() * sc).bfloat16())
    assert bool((fwd[~keep] == 0).all()) and bool((bwd[~keep] == 0).all())
    assert bool((bwd[keep] != 0).float().mean() > 0.99)


# ------------------------------------------------------------------------------------------------
# argument checks
def test_argument_checks_return_errors_and_launch_nothing():
    from vjepa2_amd import _lib

    lib = _lib.load()
    M, h = 4, 16
    x = InFrame(torch.randn(M, 2 * h).bfloat16(), 2 * h + 8)
    xf = InFrame(torch.randn(M, 2 * h), 2 * h + 8)
    sv = _in_vec(torch.ones(M))
    ob, of = OutFrame(M, 2 * h, 2 * h + 8, BF16), OutFrame(M, 2 * h, 2 * h + 8, F32)
    st = _st()
    ld = 2 * h + 8
    cases = [
        ("swiglu_fwd h % 8", lambda: lib.vj_swiglu_fwd(M, 12, _p(x), ld, _p(ob), ld, st), "multiples of 8"),
        ("swiglu_fwd ld < 2h", lambda: lib.vj_swiglu_fwd(M, h, _p(x), 2 * h - 8, _p(ob), ld, st), "ld >= 2h"),
        ("swiglu_bwd ld < 2h", lambda: lib.vj_swiglu_bwd(M, h, _p(x), ld, _p(x), 2 * h - 8, _p(ob), ld, st), "ld, lddx >= 2h"),
        ("swiglu_bwd lddx < 2h", lambda: lib.vj_swiglu_bwd(M, h, _p(x), ld, _p(x), ld, _p(ob), h, st), "ld, lddx >= 2h"),
        ("swiglu_fwd misaligned", lambda: lib.vj_swiglu_fwd(M, h, _p(x) + 2, ld, _p(ob), ld, st), "16-B aligned"),
        ("rowscale_add N % 4", lambda: lib.vj_rowscale_add(M, 30, _p(xf), ld, sv.data_ptr(), _p(xf), ld, _p(of), ld, 0, st),
         "multiples of 4"),
        ("rowscale_bf16 N % 4", lambda: lib.vj_rowscale_bf16(M, 30, _p(xf), ld, sv.data_ptr(), _p(ob), ld, st), "multiples of 4"),
        ("rowscale_bf16 misaligned", lambda: lib.vj_rowscale_bf16(M, 32, _p(xf) + 4, ld, sv.data_ptr(), _p(ob), ld, st),
         "aligned"),
        ("dropout N % 4", lambda: lib.vj_dropout(M, 30, _p(x), ld, 0, None, 0, None, 0, 0, _p(ob), ld, 0.1, 1, st),
         "multiples of 4"),
        ("dropout p = 1", lambda: lib.vj_dropout(M, 32, _p(x), ld, 0, None, 0, None, 0, 0, _p(ob), ld, 1.0, 1, st),
         "p must be in [0, 1)"),
        ("dropout aux and resid", lambda: lib.vj_dropout(M, 32, _p(x), ld, 0, _p(x), ld, _p(x), ld, 0, _p(ob), ld, 0.1, 1, st),
         "bad arguments"),
        ("dropout misaligned", lambda: lib.vj_dropout(M, 32, _p(xf) + 4, ld, 1, None, 0, None, 0, 0, _p(ob), ld, 0.1, 1, st),
         "aligned"),
    ]
    for name, fn, msg in cases:
        rc = fn()
        assert rc != 0 and msg in _lib.last_error(), (name, rc, _lib.last_error())
    torch.cuda.synchronize()
    for o in (ob, of):
        bits = o.read("argument checks")
        assert bool((bits == o.sent).all()), "a rejected call wrote its output"
