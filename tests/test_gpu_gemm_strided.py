"""GPU: every GEMM variant with padded, pairwise different leading dimensions inside poisoned frames.

The product passes real strides (the SwiGLU MLP's x12[:, :h] / x12[:, h:] windows, ld = 2h), but every other
kernel-level GEMM test calls with lda == K, ldb == K, ldc == ldc2 == ldaux == N into a bare torch.empty(M, N):
a swapped leading dimension, a store outside the [M, N] window or an operand read past K inside a row would
pass them all. Here each operand is a window at (row 2, column 8) of a longer NaN-filled buffer (fp8: 0x7F
bytes, column 16) with at least two slack rows behind it, each output a window of the same kind in a
buffer pre-filled with a NaN sentinel bit pattern, the bias an [N] slice of a longer NaN vector, and lda,
ldb, ldc, ldc2, ldaux are pairwise different multiples of 8 (fp8 operands: of 16). The windows never touch
an allocation edge, so a wrong offset shows up as a wrong value or a touched guard, never as a fault.

One call is checked four ways:
 (a) guard band: every element of an output's buffer outside its window still holds the sentinel bits;
 (b) reference: the window against float64 math on the CPU over the same bf16-rounded (fp8: dequantised)
     operands, with the tolerances the suite already states (test_gpu_kernels.py, test_gpu_fp8.py):
       f32 outputs   atol 4e-4 sqrt(K), rtol 1e-4
       bf16 outputs  atol 1e-3, rtol 8e-3 (one bf16 rounding is 2^-9 = 1.95e-3 relative)
       GELU, GELU', GELU_BWD  atol 2e-3, rtol 1.5e-2 (test_gemm_256_tiles_vs_fp32). GELU is evaluated on the
         bf16-rounded pre-activation x and rounded again: |err| <= 2^-9 (|x gelu'(x)| + |gelu(x)|) <= 4.5e-3
         |gelu(x)| for x > 0 and < 7e-4 for x < 0; GELU' likewise <= 2^-9 (|x gelu''(x)| + |gelu'(x)|) with
         |x gelu''(x)| <= 0.35: inside the bound with a factor of three to spare
       fp8           2^-14 sum_k |a_k w_k| (test_fp8_gemm_matches_dequantized) for the accumulation, plus the
                     output format's tolerance above where the output is bf16
 (c) bitwise against contiguous: the same call on contiguous, unpadded copies under the same knobs gives
     bitwise the same outputs (a leading dimension only enters addresses, never the MFMA or summation order);
 (d) plan: before a 256-row case launches, vj_gemm256_plan (cus = 0: this device) under the case's knobs
     returns the tile rows, columns, waves and main-loop form the case table (tests/test_gemm_variants.py)
     declares, so each case runs the variant it names.
"""

import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import vjepa_oracle as orc  # noqa: E402
from test_gemm_variants import (EPI_BF16, EPI_BF16_RESID, EPI_F32, EPI_F32_RESID, EPI_GELU, EPI_GELU_BWD,  # noqa: E402
                                EPI_ROPE, LAYOUTS, STRIDED_CASES, expected_plan, plan, set_knobs)

DEV = "cuda"
BF16, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
ROW0, COL0 = 2, 8  # the window's first row and column in its backing buffer
SLACK = 2          # whole rows behind the window
# output sentinels: NaN payloads no kernel produces, compared as integers
SENTINEL = {BF16: (torch.int16, 0x7FC1), F32: (torch.int32, 0x7FC12345)}
TOL_BF16 = (1e-3, 8e-3)
TOL_GELU = (2e-3, 1.5e-2)


def TOL_F32(K):
    return 4e-4 * math.sqrt(K), 1e-4


def _col0(ld, itemsize, shift_bytes=0):
    """First window column: COL0 (fp8 bytes: 16), moved right until the window pointer is 16-B aligned (it
    already is for a leading dimension that is a multiple of 8 elements), then by shift_bytes."""
    c = 16 if itemsize == 1 else COL0
    while ((ROW0 * ld + c) * itemsize) % 16:
        c += 1
    return c + shift_bytes // itemsize


class InFrame:
    """A [rows, cols] operand as a window (leading dimension ld) of a longer buffer that is NaN (uint8:
    0x7F, the e4m3 NaN) everywhere else. ld == cols gives the contiguous, unpadded copy."""

    def __init__(self, t, ld):
        rows, cols = t.shape
        assert ld >= cols
        self.ld = ld
        if ld == cols:
            self.win = t.contiguous().to(DEV)
            return
        assert ld % 8 == 0 and ld > cols
        c0 = _col0(ld, t.element_size())
        buf = torch.full(((ROW0 + rows + SLACK) * ld + c0,), 0x7F if t.dtype == U8 else float("nan"), dtype=t.dtype)
        buf.as_strided((rows, cols), (ld, 1), ROW0 * ld + c0).copy_(t)
        self.buf = buf.to(DEV)
        self.win = self.buf.as_strided((rows, cols), (ld, 1), ROW0 * ld + c0)
        assert self.win.data_ptr() % 16 == 0


def _in_vec(v, pad=True):
    """An [n] vector as a 16-B aligned slice of a longer NaN-filled one."""
    if not pad:
        return v.to(DEV)
    buf = torch.full((v.numel() + 24,), float("nan"), dtype=v.dtype)
    buf[8:8 + v.numel()] = v
    out = buf.to(DEV)[8:8 + v.numel()]
    assert out.data_ptr() % 16 == 0
    return out


class OutFrame:
    """A [rows, cols] output window (leading dimension ld) of a buffer pre-filled with the sentinel bits;
    always framed (also for ld == cols: rows of sentinel before and behind a contiguous output)."""

    def __init__(self, rows, cols, ld, dtype, shift_bytes=0):
        assert ld >= cols
        self.rows, self.cols, self.ld, self.dtype = rows, cols, ld, dtype
        self.idt, self.sent = SENTINEL[dtype]
        self.off = ROW0 * ld + _col0(ld, self.idt.itemsize, shift_bytes)
        self.bits = torch.full(((ROW0 + rows + SLACK) * ld + self.off,), self.sent, dtype=self.idt, device=DEV)
        self.win = self.bits.view(dtype).as_strided((rows, cols), (ld, 1), self.off)
        assert self.win.data_ptr() % 16 == shift_bytes % 16

    def fill(self, t):
        """Initial window contents (an output that is also read: accumulate)."""
        self.win.copy_(t.to(DEV))

    def read(self, what):
        """(a) the guard band is untouched; returns the window's bits (CPU, integer view)."""
        raw = self.bits.cpu()
        win = raw.as_strided((self.rows, self.cols), (self.ld, 1), self.off).clone()
        raw.as_strided((self.rows, self.cols), (self.ld, 1), self.off).fill_(self.sent)
        bad = (raw != self.sent).nonzero()
        if bad.numel():
            rel = int(bad[0]) - self.off
            r = rel // self.ld
            assert False, (f"{what}: {bad.numel()} guard elements written; first at (row {r}, column "
                           f"{rel - r * self.ld}) relative to the [{self.rows}, {self.cols}] window, ld {self.ld}")
        return win

    def values(self, bits):
        return bits.view(self.dtype).double()


def _close64(got, exp, tol, what, extra=None):
    """(b) |got - exp| <= atol + rtol |exp| (+ extra) elementwise; NaN / inf in got fail."""
    atol, rtol = tol
    bound = atol + rtol * exp.abs()
    if extra is not None:
        bound = bound + extra
    err = (got - exp).abs()
    ok = err <= bound
    if not bool(ok.all()):
        r, c = [int(x) for x in (~ok).nonzero()[0]]
        assert False, (f"{what}: {int((~ok).sum())} of {ok.numel()} outside atol {atol:.3g} rtol {rtol:.3g}; first "
                       f"at ({r}, {c}): got {float(got[r, c])!r}, expected {float(exp[r, c])!r}")


def _gelu64(x):
    """GELU (erf form) and its derivative in float64."""
    cdf = 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))
    pdf = torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    return x * cdf, cdf + x * pdf


@functools.lru_cache(maxsize=None)
def _problem(M, N, K):
    """bf16 operands and the float64 product of one shape, built once and shared (never modified)."""
    g = torch.Generator().manual_seed(1000003 * M + 1009 * N + K)
    A = torch.randn(M, K, generator=g).bfloat16()
    B = (0.1 * torch.randn(N, K, generator=g)).bfloat16()
    bias = torch.randn(N, generator=g)
    resid = torch.randn(M, N, generator=g)
    dg = torch.randn(M, N, generator=g).bfloat16()  # stands in for a saved GELU derivative
    acc = A.double() @ B.double().t()
    return dict(A=A, B=B, bias=bias, resid=resid, resid_bf=resid.bfloat16(), dg=dg, acc=acc,
                pre=acc + bias.double())


def _operands(M, N, K, lay, padded):
    """A and B of _problem in the layout's storage, padded (lda = width + 8, ldb = width + 16) or contiguous."""
    p = _problem(M, N, K)
    ak, bk = LAYOUTS[lay]
    a = p["A"] if ak else p["A"].t().contiguous()
    b = p["B"] if bk else p["B"].t().contiguous()
    return InFrame(a, a.shape[1] + (8 if padded else 0)), InFrame(b, b.shape[1] + (16 if padded else 0))


# (name, epilogue, saves the GELU derivative)
EPILOGUES = [("bf16", EPI_BF16, False), ("f32", EPI_F32, False), ("f32_resid", EPI_F32_RESID, False),
             ("gelu_save", EPI_GELU, True), ("gelu", EPI_GELU, False), ("gelu_bwd", EPI_GELU_BWD, False),
             ("bf16_resid", EPI_BF16_RESID, False)]


def _launch(M, N, K, lay, epi, save, fa, fb, padded, splitk=1, ldc=None, shift_bytes=0):
    """One vj_gemm_bf16 (/ _splitk) call into fresh output frames. Returns {output name: (frame, bits)}
    after the guard check. padded: ldc = N + 24, ldc2 = N + 40, ldaux = N + 32 (else N)."""
    from vjepa2_amd import ops

    p = _problem(M, N, K)
    ak, bk = LAYOUTS[lay]
    ldc = ldc if ldc is not None else N + (24 if padded else 0)
    ldc2, ldaux = N + (40 if padded else 0), N + (32 if padded else 0)
    if padded:
        lds = [fa.ld, fb.ld, ldc, ldc2, ldaux]
        assert len(set(lds)) == 5, f"leading dimensions must be pairwise different: {lds}"
    bias = None if epi == EPI_GELU_BWD else _in_vec(p["bias"], padded)
    aux = {EPI_F32_RESID: p["resid"], EPI_BF16_RESID: p["resid_bf"], EPI_GELU_BWD: p["dg"]}.get(epi)
    faux = InFrame(aux, ldaux) if aux is not None else None
    outs = {}
    if epi != EPI_GELU or save:
        outs["C"] = OutFrame(M, N, ldc, F32 if epi in (EPI_F32, EPI_F32_RESID) else BF16, shift_bytes)
    if epi == EPI_GELU:
        outs["C2"] = OutFrame(M, N, ldc2, BF16)
    c, c2 = outs.get("C"), outs.get("C2")
    ops.gemm(M, N, K, fa.win, fa.ld, ak, fb.win, fb.ld, bk, epi, out=c.win if c else None, ldc=c.ld if c else 0,
             out2=c2.win if c2 else None, ldc2=c2.ld if c2 else 0, bias=bias, aux=faux.win if faux else None,
             ldaux=faux.ld if faux else 0, splitk=splitk)
    torch.cuda.synchronize()
    what = f"M={M} N={N} K={K} {lay} epi={epi} save={save} splitk={splitk} ldc={ldc}"
    return {k: (f, f.read(f"{what} output {k}")) for k, f in outs.items()}


def _check_reference(M, N, K, epi, res, what):
    """(b) for the outputs of one vj_gemm_bf16 call."""
    p = _problem(M, N, K)
    val = {k: f.values(bits) for k, (f, bits) in res.items()}
    if epi == EPI_BF16:
        _close64(val["C"], p["pre"], TOL_BF16, what)
    elif epi == EPI_F32:
        _close64(val["C"], p["pre"], TOL_F32(K), what)
    elif epi == EPI_F32_RESID:
        _close64(val["C"], p["pre"] + p["resid"].double(), TOL_F32(K), what)
    elif epi == EPI_BF16_RESID:
        _close64(val["C"], p["pre"] + p["resid_bf"].double(), TOL_BF16, what)
    elif epi == EPI_GELU_BWD:
        _close64(val["C"], p["acc"] * p["dg"].double(), TOL_GELU, what)
    else:
        act, der = _gelu64(p["pre"])
        _close64(val["C2"], act, TOL_GELU, what + " GELU")
        if "C" in val:
            _close64(val["C"], der, TOL_GELU, what + " GELU'")


def _assert_same_bits(res, ref, what):
    """(c) bitwise equal outputs."""
    for k, (_, bits) in res.items():
        diff = bits != ref[k][1]
        assert not bool(diff.any()), (f"{what} output {k}: {int(diff.sum())} elements differ bitwise from the "
                                      f"contiguous call; first at {[int(x) for x in diff.nonzero()[0]]}")


def _assert_plan(case, lay, epi, N=None):
    """(d) the 256-row kernel the launch will run is the one the case declares (this device's CU count)."""
    want = expected_plan(case, epi)
    if want is None:
        assert case.M < 1024, "a 128 x 128-kernel case must stay below the 256-row kernel's M threshold"
        return
    assert case.M >= 1024 and case.N >= 128
    got = plan(case.M, N or case.N, case.K, lay, epi, 0)
    assert got == want, f"{case.name} {lay} epi {epi}: plan {got}, the case declares {want}"


def _rope_setup(M, N):
    """QKV widths of the table: N = 480 = 3 x 2 heads x 80, N = 264 = 3 x 1 x 88."""
    H, hd = {480: (2, 80), 264: (1, 88)}[N]
    g = torch.Generator().manual_seed(N)
    ids = torch.randint(0, 8 * 16, (M,), generator=g)
    cos_t, sin_t = orc.rope_tables(hd, 16)
    return H, hd, ids, cos_t, sin_t


def _rope_expected(y, M, H, hd, ids, tpf, tpr):
    """The oracle's RoPE of the q and k columns of y [M, 3 H hd] (float64)."""
    D = H * hd
    q = y[:, :D].reshape(M, H, hd).transpose(0, 1)[None]
    k = y[:, D:2 * D].reshape(M, H, hd).transpose(0, 1)[None]
    qr, kr = orc.apply_rope_qk(q, k, ids[None], tpf, tpr)
    return torch.cat([qr[0].transpose(0, 1).reshape(M, D), kr[0].transpose(0, 1).reshape(M, D), y[:, 2 * D:]], 1)


def _launch_rope(M, N, K, fa, fb, padded):
    from vjepa2_amd import ops

    p = _problem(M, N, K)
    H, hd, ids, cos_t, sin_t = _rope_setup(M, N)
    out = OutFrame(M, N, N + (24 if padded else 0), BF16)
    bias, ids_d, cd, sd = _in_vec(p["bias"], padded), ids.int().to(DEV), cos_t.to(DEV), sin_t.to(DEV)
    ops._call("vj_qkv_rope_gemm", M, K, fa.win.data_ptr(), fa.ld, fb.win.data_ptr(), fb.ld, bias.data_ptr(),
              out.win.data_ptr(), out.ld, H, hd, ids_d.data_ptr(), 0, 16, 4, cd.data_ptr(), sd.data_ptr(),
              cos_t.shape[0], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return {"C": (out, out.read(f"qkv_rope M={M} N={N} K={K} ldc={out.ld}"))}


CASE_LAYOUTS = [(c, lay) for c in STRIDED_CASES for lay in c.knobs]


@pytest.mark.parametrize("case,lay", CASE_LAYOUTS, ids=[f"{c.name}-{lay}" for c, lay in CASE_LAYOUTS])
def test_gemm_variant_strided(case, lay, monkeypatch):
    """Every epilogue of one (kernel variant, operand layout) of the case table, checks (a)-(d). All cases
    run with VJ_GEMM_PXCD=1: 8 blocks, so some blocks walk two tiles and the next-tile hand-over runs with
    padded leading dimensions too. M = 1032 leaves a last row tile of 8 (192-row tiles: 72) rows, N = 480 =
    256 + 224, N = 264 = 128 + 128 + 8, K = 72 / 40 an 8-deep tail chunk, K = 96 three form-1 units, K =
    192 three S64 steps; M = 264, N = 136 the 128 x 128 kernel with ragged last tiles."""
    M, N, K = case.M, case.N, case.K
    set_knobs(monkeypatch, dict(case.knobs[lay], VJ_GEMM_PXCD="1"))
    pa, pb = _operands(M, N, K, lay, True)
    ca, cb = _operands(M, N, K, lay, False)
    for name, epi, save in EPILOGUES:
        if epi == EPI_BF16_RESID and lay != "KK":
            continue
        _assert_plan(case, lay, epi)
        what = f"{case.name} {lay} {name}"
        res = _launch(M, N, K, lay, epi, save, pa, pb, True)
        _check_reference(M, N, K, epi, res, what)
        _assert_same_bits(res, _launch(M, N, K, lay, epi, save, ca, cb, False), what)
    if lay == "KK" and N in (480, 264):  # the fused QKV + RoPE epilogue (N = 136 is no QKV width)
        _assert_plan(case, lay, EPI_ROPE)
        H, hd, ids, _, _ = _rope_setup(M, N)
        res = _launch_rope(M, N, K, pa, pb, True)
        exp = _rope_expected(_problem(M, N, K)["pre"], M, H, hd, ids, 16, 4)
        _close64(res["C"][0].values(res["C"][1]), exp, TOL_BF16, f"{case.name} qkv_rope")
        _assert_same_bits(res, _launch_rope(M, N, K, ca, cb, False), f"{case.name} qkv_rope")


def _rows_128_kernel(M, N, K, lay, epi):
    """The 128 x 128 kernel's output bits for a K-major-A problem: the contiguous call in two row chunks
    below the 256-row kernel's M threshold (an output element's K order does not depend on the chunking)."""
    from vjepa2_amd import ops

    assert LAYOUTS[lay][0] == 1
    p = _problem(M, N, K)
    ak, bk = LAYOUTS[lay]
    b = (p["B"] if bk else p["B"].t().contiguous()).to(DEV)
    bias = p["bias"].to(DEV)
    out = torch.empty(M, N, dtype=BF16, device=DEV)
    for r0, r1 in ((0, 512), (512, M)):
        assert r1 - r0 < 1024
        a = p["A"][r0:r1].contiguous().to(DEV)
        aux = p["resid_bf"][r0:r1].contiguous().to(DEV) if epi == EPI_BF16_RESID else None
        ops.gemm(r1 - r0, N, K, a, K, ak, b, b.stride(0), bk, epi, out=out[r0:r1], ldc=N, bias=bias, aux=aux,
                 ldaux=N)
    torch.cuda.synchronize()
    return out.cpu().view(torch.int16)


@pytest.mark.parametrize("ldc,shift", [(490, 0), (490, 8), (504, 8)])
def test_gemm_256_declines_unaligned_output(ldc, shift, monkeypatch):
    """M = 1032, N = 480, K-major operands, bf16 output: with ldc = 2 (mod 4), or with the output pointer 8
    bytes off 16-B alignment, the 256-row kernel declines (its stores are 8 / 16 bytes wide) and the 128 x
    128 kernel must produce the result: guard band, float64 reference, and bitwise the 128 x 128 kernel's
    own output."""
    M, N, K = 1032, 480, 72
    set_knobs(monkeypatch, {"VJ_GEMM_PXCD": "1"})
    assert plan(M, N, K, "KK", EPI_BF16, 0) is not None  # the plan alone would take it: ldc / alignment decline
    assert ldc % 4 or shift % 16
    pa, pb = _operands(M, N, K, "KK", True)
    res = _launch(M, N, K, "KK", EPI_BF16, False, pa, pb, True, ldc=ldc, shift_bytes=shift)
    assert res["C"][0].win.data_ptr() % 16 == shift
    _check_reference(M, N, K, EPI_BF16, res, f"ldc={ldc} shift={shift}")
    diff = res["C"][1] != _rows_128_kernel(M, N, K, "KK", EPI_BF16)
    assert not bool(diff.any()), f"{int(diff.sum())} elements differ from the 128 x 128 kernel's output"


@pytest.mark.parametrize("lay", ["KM", "MM"])
def test_gemm_bf16_resid_mn_major_b_falls_through(lay, monkeypatch):
    """EPI_BF16_RESID with an MN-major B at M = 1032: the 256-row kernel has no such instantiation
    (Cfg256::supported), so the call falls through to the 128 x 128 kernel and must still be right."""
    M, N, K = 1032, 480, 72
    set_knobs(monkeypatch, {"VJ_GEMM_PXCD": "1"})
    pa, pb = _operands(M, N, K, lay, True)
    ca, cb = _operands(M, N, K, lay, False)
    res = _launch(M, N, K, lay, EPI_BF16_RESID, False, pa, pb, True)
    _check_reference(M, N, K, EPI_BF16_RESID, res, f"bf16_resid {lay}")
    _assert_same_bits(res, _launch(M, N, K, lay, EPI_BF16_RESID, False, ca, cb, False), f"bf16_resid {lay}")
    if lay == "KM":
        diff = res["C"][1] != _rows_128_kernel(M, N, K, lay, EPI_BF16_RESID)
        assert not bool(diff.any()), f"{int(diff.sum())} elements differ from the 128 x 128 kernel's output"


SPLITK_SHAPES = [(264, 136, "MM"), (264, 480, "MM"), (136, 136, "KK"), (136, 136, "KM"), (136, 136, "MK"),
                 (136, 136, "MM")]


@pytest.mark.parametrize("M,N,lay", SPLITK_SHAPES, ids=[f"{m}x{n}-{lay}" for m, n, lay in SPLITK_SHAPES])
def test_gemm_splitk_strided(M, N, lay, monkeypatch):
    """Split-K (splitk = 2 over K = 200: slices of 128 and 72) with padded operands, ldc != ldaux: the 256-row
    partial kernel with 128-wide (M = 264, N = 136) and 256-wide (N = 480) tiles, the 128 x 128 partial
    kernel (M = 136) in all four layouts, then k_splitk_reduce4 (ldc = N + 24) or, with ldc = 2 (mod 4), the
    scalar k_splitk_reduce."""
    K = 200
    set_knobs(monkeypatch, {"VJ_GEMM_PXCD": "1"})
    pa, pb = _operands(M, N, K, lay, True)
    ca, cb = _operands(M, N, K, lay, False)
    for name, epi, _ in EPILOGUES[:3]:
        ref = _launch(M, N, K, lay, epi, False, ca, cb, False, splitk=2)
        for ldc in (N + 24, N + 26):
            what = f"splitk {M}x{N} {lay} {name} ldc={ldc}"
            res = _launch(M, N, K, lay, epi, False, pa, pb, True, splitk=2, ldc=ldc)
            _check_reference(M, N, K, epi, res, what)
            _assert_same_bits(res, ref, what)


@pytest.mark.parametrize("N", [136, 480])
@pytest.mark.parametrize("accumulate", [0, 1])
def test_wgrad_splitk_strided(N, accumulate):
    """vj_gemm_bf16_wgrad called directly with splitk = 2 (ops.wgrad_splitk never splits at these sizes) and
    ws = splitk (M N + M) floats, so the fused row-sum kernel (EPI_PARTIAL_RS) runs: padded lddy, ldx, lddw,
    dw in a guard band (accumulate = 1: dw is also the residual the reduce reads), db an [M] slice of a
    sentinel vector, the workspace followed by sentinels; against float64 and bitwise against the
    contiguous call."""
    from vjepa2_amd import ops

    M, K = 264, 200  # dw [M, N] (+)= dY^T X, dY [K, M], X [K, N]; K = tokens
    g = torch.Generator().manual_seed(N + accumulate)
    dY = torch.randn(K, M, generator=g).bfloat16()
    X = torch.randn(K, N, generator=g).bfloat16()
    dw0, db0 = torch.randn(M, N, generator=g), torch.randn(M, generator=g)
    exp_w = dY.double().t() @ X.double() + (dw0.double() if accumulate else 0.0)
    exp_b = dY.double().sum(0) + (db0.double() if accumulate else 0.0)
    idt, sent = SENTINEL[F32]
    nws = 2 * (M * N + M)
    results = []
    for padded in (True, False):
        fy, fx = InFrame(dY, M + (8 if padded else 0)), InFrame(X, N + (16 if padded else 0))
        dw = OutFrame(M, N, N + (24 if padded else 0), F32)
        dw.fill(dw0)
        dbits = torch.full((M + 24,), sent, dtype=idt, device=DEV)
        db = dbits.view(F32)[8:8 + M]
        db.copy_(db0.to(DEV))
        wbits = torch.full((nws + 64,), sent, dtype=idt, device=DEV)
        ops._call("vj_gemm_bf16_wgrad", M, N, K, fy.win.data_ptr(), fy.ld, fx.win.data_ptr(), fx.ld,
                  dw.win.data_ptr(), dw.ld, accumulate, db.data_ptr(), accumulate, 2, wbits.data_ptr(), nws,
                  torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        wbits_dw = dw.read(f"wgrad dw N={N} accumulate={accumulate} padded={padded}")
        dcpu = dbits.cpu()
        assert bool((dcpu[:8] == sent).all()) and bool((dcpu[8 + M:] == sent).all()), "wgrad wrote around db"
        assert bool((wbits.cpu()[nws:] == sent).all()), "wgrad wrote past its workspace"
        results.append((wbits_dw, dcpu[8:8 + M].clone()))
        _close64(dw.values(wbits_dw), exp_w, TOL_F32(K), f"wgrad dw N={N} accumulate={accumulate} padded={padded}")
        _close64(dcpu[8:8 + M].view(F32).double()[None], exp_b[None], TOL_F32(K),
                 f"wgrad db N={N} accumulate={accumulate} padded={padded}")
    assert torch.equal(results[0][0], results[1][0]), "wgrad dw: padded call differs bitwise from the contiguous one"
    assert torch.equal(results[0][1], results[1][1]), "wgrad db: padded call differs bitwise from the contiguous one"


# ------------------------------------------------------------------------------------------------
# fp8
@functools.lru_cache(maxsize=None)
def _fp8_problem(M, N, K):
    """Per-row scaled e4m3 operands (quantised by the library, exact: test_quant_rows_fp8_exact) and the
    float64 product of their dequantised values."""
    from vjepa2_amd import ops

    g = torch.Generator().manual_seed(M + N + K)
    a = torch.randn(M, K, generator=g) * torch.exp(torch.randn(M, 1, generator=g))  # per-row magnitudes
    w = 0.05 * torch.randn(N, K, generator=g)
    bias = torch.randn(N, generator=g)
    resid = torch.randn(M, N, generator=g)
    a8, ea = ops.quant_rows_fp8(a.to(DEV))
    w8, ew = ops.quant_rows_fp8(w.to(DEV))
    torch.cuda.synchronize()
    a8, ea, w8, ew = a8.cpu(), ea.cpu(), w8.cpu(), ew.cpu()
    ad = torch.ldexp(a8.view(torch.float8_e4m3fn).float(), ea[:, None].float()).double()
    wd = torch.ldexp(w8.view(torch.float8_e4m3fn).float(), ew[:, None].float()).double()
    return dict(a8=a8, ea=ea, w8=w8, ew=ew, bias=bias, resid=resid, pre=ad @ wd.t() + bias.double(),
                bound=2.0 ** -14 * (ad.abs() @ wd.abs().t() + bias.double().abs()))


def _launch_fp8(M, N, K, epi, save, padded, rope=False):
    from vjepa2_amd import ops

    p = _fp8_problem(M, N, K)
    fa, fb = InFrame(p["a8"], K + (16 if padded else 0)), InFrame(p["w8"], K + (32 if padded else 0))
    ldc, ldc2, ldaux = (N + (x if padded else 0) for x in (24, 40, 32))
    if padded:
        assert fa.ld % 16 == 0 and fb.ld % 16 == 0 and len({fa.ld, fb.ld, ldc, ldc2, ldaux}) == 5
    ea, ew, bias = p["ea"].to(DEV), p["ew"].to(DEV), _in_vec(p["bias"], padded)
    outs = {}
    if rope:
        H, hd, ids, cos_t, sin_t = _rope_setup(M, N)
        c = outs["C"] = OutFrame(M, N, ldc, BF16)
        ids_d, cd, sd = ids.int().to(DEV), cos_t.to(DEV), sin_t.to(DEV)
        ops._call("vj_qkv_rope_gemm_fp8", M, K, fa.win.data_ptr(), fa.ld, ea.data_ptr(), fb.win.data_ptr(), fb.ld,
                  ew.data_ptr(), bias.data_ptr(), c.win.data_ptr(), c.ld, H, hd, ids_d.data_ptr(), 0, 16, 4,
                  cd.data_ptr(), sd.data_ptr(), cos_t.shape[0], torch.cuda.current_stream().cuda_stream)
    else:
        faux = InFrame(p["resid"], ldaux) if epi == EPI_F32_RESID else None
        if epi != EPI_GELU or save:
            outs["C"] = OutFrame(M, N, ldc, F32 if epi in (EPI_F32, EPI_F32_RESID) else BF16)
        if epi == EPI_GELU:
            outs["C2"] = OutFrame(M, N, ldc2, BF16)
        c, c2 = outs.get("C"), outs.get("C2")
        ops.linear_fwd_fp8(fa.win, ea, fb.win, ew, bias, epi, out=c.win if c else None, out2=c2.win if c2 else None,
                           resid=faux.win if faux else None)
    torch.cuda.synchronize()
    what = f"fp8 M={M} N={N} K={K} epi={epi} save={save} rope={rope} padded={padded}"
    return {k: (f, f.read(f"{what} output {k}")) for k, f in outs.items()}


def test_fp8_gemm_strided():
    """The fp8 GEMM (256 x 128 tiles, 128-deep MFMA steps over e4m3 bytes) with padded lda / ldb (multiples
    of 16), ldc, ldc2, ldaux: M = N = 264 leaves 8-row / 8-column last tiles, K = 208 a 80-byte tail.
    Epilogues BF16, F32, F32_RESID, GELU (with and without the saved derivative) and the fused QKV + RoPE
    (N = 264 = 3 x 88), checks (a)-(c); the fp8 GEMM has one kernel shape, so there is no plan to assert."""
    M, N, K = 264, 264, 208
    p = _fp8_problem(M, N, K)
    pre, bound = p["pre"], p["bound"]
    for name, epi, save in EPILOGUES[:5]:
        res = _launch_fp8(M, N, K, epi, save, True)
        val = {k: f.values(bits) for k, (f, bits) in res.items()}
        if epi == EPI_F32:
            _close64(val["C"], pre, (0.0, 0.0), "fp8 f32", extra=bound)
        elif epi == EPI_F32_RESID:
            r64 = p["resid"].double()
            _close64(val["C"], pre + r64, (0.0, 0.0), "fp8 f32_resid", extra=bound + 2.0 ** -23 * (pre.abs() + r64.abs()))
        elif epi == EPI_BF16:
            _close64(val["C"], pre, TOL_BF16, "fp8 bf16", extra=bound)
        else:  # |gelu'| <= 1.13 carries the accumulation bound through the activation, |gelu''| <= 0.8
            act, der = _gelu64(pre)
            _close64(val["C2"], act, TOL_GELU, f"fp8 {name} GELU", extra=1.13 * bound)
            if save:
                _close64(val["C"], der, TOL_GELU, f"fp8 {name} GELU'", extra=0.8 * bound)
        _assert_same_bits(res, _launch_fp8(M, N, K, epi, save, False), f"fp8 {name}")
    H, hd, ids, _, _ = _rope_setup(M, N)
    res = _launch_fp8(M, N, K, EPI_ROPE, False, True, rope=True)
    exp = _rope_expected(pre, M, H, hd, ids, 16, 4)
    # a rotated pair mixes two columns: the larger of their accumulation bounds, times |cos| + |sin| <= sqrt(2)
    pair = torch.maximum(bound, bound.view(M, N // 2, 2).flip(-1).reshape(M, N)) * math.sqrt(2.0)
    _close64(res["C"][0].values(res["C"][1]), exp, TOL_BF16, "fp8 qkv_rope", extra=pair)
    _assert_same_bits(res, _launch_fp8(M, N, K, EPI_ROPE, False, False, rope=True), "fp8 qkv_rope")
