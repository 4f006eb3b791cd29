"""GPU: the attention kernels (vj_attn_fwd_ex / vj_attn_bwd_ex, vj_xattn_fwd / vj_xattn_bwd) at their tile-edge
lengths, through the C ABI with strides, offsets and output buffers of the test's own, against per-element
rounding bounds.

Every other attention test passes ld = 3 D, offsets 0, D, 2 D and ldo = D into bare torch.empty buffers and
compares whole-tensor norms: a swapped leading dimension, a store past row T or into the head-dim padding
(80 / 88 are padded to 96 in the kernel), a stats row written into stats[1] by the forward, one wrong row
or one frame boundary off by one would pass them all. Here (frames in the style of
tests/test_gpu_gemm_strided.py):
  * qkv is a window of a NaN-filled buffer, ld = 3 D + 56, q / k / v at columns 8, D + 24, 2 D + 40 (gaps
    of NaN between them); dO, the vj_xattn q and kv likewise;
  * o, dqkv (ldd = 3 D + 64, same offsets), stats and the vj_xattn o, dq, dkv, lse2 are windows of
    buffers pre-filled with a NaN sentinel bit pattern; all leading dimensions are pairwise different;
  * every window has GUARD rows of fill above and below and columns of fill left and right, so a wrong
    address shows up as a wrong value or a touched guard, never as a fault.
One call is checked four ways:
 (a) every guard element still holds the sentinel: around o's D columns, between and around the dq / dk /
     dv column ranges, stats[1] after a forward-only call, behind the vj_xattn workspace;
 (b) every output element is within C E of the float64 reference (tests/attn_bounds.py: E is the
     first-order bound of the documented rounding points, C = 2 x the CPU emulation's worst ratio; the
     CPU file tests/test_attn_bounds.py proves on the same inputs that a dropped edge key, a skipped
     query, a leaked frame boundary, a shifted dropout column, a 3 % scale error and a dropped
     cross-attention chunk or query block all exceed it); lse within the tolerances the suite states
     (vj_attn: atol 2e-3, rtol 1e-4 in natural-log units, vj_xattn: 1e-4 in log2 units);
 (c) the same call on contiguous packed copies through ops.attn_fwd / attn_bwd (ops.xattn_*) gives
     bitwise the same values (a stride or offset only enters addresses);
 (d) a second framed call is bitwise identical.
Each test prints its largest |err| / E per output (pytest -s shows them).
"""

import ctypes

import pytest
import torch

import attn_bounds as ab

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
SENTINEL = {BF16: (torch.int16, 0x7FC1), F32: (torch.int32, 0x7FC12345)}  # NaNs no kernel produces
GUARD = 136  # rows of fill above and below every window: more than one 128-row block
_ids = lambda c: c.name  # noqa: E731


class Frame:
    """[rows, ld] elements inside a [GUARD + rows + GUARD, ld] buffer filled with the dtype's sentinel (a NaN).
    cols: {name: (first column, width)}, the windows; they touch neither the first nor the last column.
    Inputs are put() into their windows, outputs read() back after the guard check."""

    def __init__(self, rows, ld, dtype, cols):
        self.rows, self.ld, self.dtype, self.cols = rows, ld, dtype, dict(cols)
        self.idt, self.sent = SENTINEL[dtype]
        spans = sorted(self.cols.values())
        assert spans[0][0] > 0 and spans[-1][0] + spans[-1][1] < ld
        assert all(a[0] + a[1] <= b[0] for a, b in zip(spans, spans[1:]))
        self.bits = torch.full((rows + 2 * GUARD, ld), self.sent, dtype=self.idt, device=DEV)

    def ptr(self, col=0):
        return self.bits[GUARD, col:].data_ptr()

    def put(self, name, t):
        c0, w = self.cols[name]
        assert t.shape == (self.rows, w) and t.dtype == self.dtype
        self.bits.view(self.dtype)[GUARD:GUARD + self.rows, c0:c0 + w].copy_(t.to(DEV))

    def read(self, what, untouched=()):
        """(a): everything outside the windows, and every window named in `untouched`, still holds the
        sentinel. Returns {name: the window's bits (CPU, integer view)}."""
        raw = self.bits.cpu()
        inside = torch.zeros_like(raw, dtype=torch.bool)
        out = {}
        for name, (c0, w) in self.cols.items():
            out[name] = raw[GUARD:GUARD + self.rows, c0:c0 + w].clone()
            if name not in untouched:
                inside[GUARD:GUARD + self.rows, c0:c0 + w] = True
        bad = ((raw != self.sent) & ~inside).nonzero()
        if bad.numel():
            r, c = int(bad[0, 0]) - GUARD, int(bad[0, 1])
            assert False, (f"{what}: {bad.shape[0]} guard elements written; first at (row {r}, column {c}) of the "
                           f"[{self.rows}, {self.ld}] frame, windows {self.cols}")
        return out


def _values(bits, dtype):
    return bits.view(dtype).double()


def _same_bits(a, b, what):
    for n in a:
        diff = a[n] != b[n]
        assert not bool(diff.any()), (f"{what}: {n} differs bitwise in {int(diff.sum())} elements; first at "
                                      f"{[int(x) for x in diff.nonzero()[0]]}")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _report(name, ratios):
    print(f"[attn-edges] {name}: " + " ".join(f"{n}={r:.3f}" for n, r in ratios.items()))


# ------------------------------------------------------------------------------------------------
# vj_attn_fwd_ex / vj_attn_bwd_ex
def _attn_dims(case):
    T, D = ab.attn_tokens(case), case.H * case.hd
    offs = (8, D + 24, 2 * D + 40)
    lds = dict(ld=3 * D + 56, ldd=3 * D + 64, ldo=D + 24, lddo=D + 40)
    assert len(set(lds.values())) == 4 and all(v % 8 == 0 for v in lds.values()) and all(o % 8 == 0 for o in offs)
    return T, D, offs, lds


def _attn_framed(case, fblk=None, fwd_only=False):
    """One forward (+ backward) through the C ABI on framed buffers: {output name: bits} after check (a)."""
    from vjepa2_amd._lib import call, int_array

    qkv, do = ab.attn_inputs(case)
    T, D, offs, lds = _attn_dims(case)
    H, hd = case.H, case.hd
    fblk = case.fblk if fblk is None else fblk
    ns, ln = int_array([n for n, _ in case.groups]), int_array([l for _, l in case.groups])
    names3 = ("q", "k", "v")
    fq = Frame(T, lds["ld"], BF16, {n: (c, D) for n, c in zip(names3, offs)})
    for i, n in enumerate(names3):
        fq.put(n, qkv[:, i * D:(i + 1) * D])
    fo = Frame(T, lds["ldo"], BF16, {"o": (8, D)})
    fs = Frame(1, 2 * H * T + 16, F32, {"lse": (8, H * T), "delta": (8 + H * T, H * T)})
    what = f"{case.name} fblk={fblk}"
    call("vj_attn_fwd_ex", T, H, hd, fq.ptr(), lds["ld"], *offs, fo.ptr(8), lds["ldo"], fs.ptr(8), hd ** -0.5,
         len(case.groups), ns, ln, fblk, case.p, case.seed, _stream())
    torch.cuda.synchronize()
    res = fo.read(f"{what} o")
    res["lse"] = fs.read(f"{what} stats after the forward", untouched=("delta",))["lse"]  # stats[1] is the backward's
    inputs = fq.read(f"{what} qkv")
    if fwd_only:
        return res
    fdo = Frame(T, lds["lddo"], BF16, {"do": (8, D)})
    fdo.put("do", do)
    fd = Frame(T, lds["ldd"], BF16, {"d" + n: (c, D) for n, c in zip(names3, offs)})
    call("vj_attn_bwd_ex", T, H, hd, fq.ptr(), lds["ld"], *offs, fo.ptr(8), lds["ldo"], fdo.ptr(8), lds["lddo"],
         fs.ptr(8), fd.ptr(), lds["ldd"], hd ** -0.5, len(case.groups), ns, ln, None, 0, 0, 0, None, None, fblk,
         case.p, case.seed, _stream())
    torch.cuda.synchronize()
    res.update(fd.read(f"{what} dqkv"))
    st = fs.read(f"{what} stats after the backward")
    res["delta"] = st["delta"]
    # the backward's inputs are unchanged
    _same_bits({"o": res["o"], "lse": res["lse"]}, {"o": fo.read(f"{what} o")["o"], "lse": st["lse"]}, what + " inputs")
    _same_bits(inputs, fq.read(f"{what} qkv"), what + " qkv")
    fdo.read(f"{what} dO")
    return res


def _attn_packed(case, fwd_only=False):
    """(c)'s other side: the same launch on packed contiguous tensors through vjepa2_amd.ops."""
    from vjepa2_amd import ops

    qkv, do = ab.attn_inputs(case)
    D = case.H * case.hd
    groups = [tuple(g) for g in case.groups]
    kw = dict(fblk=case.fblk, dropout_p=case.p, seed=case.seed)
    qkv_d = qkv.to(DEV)
    o, stats = ops.attn_fwd(qkv_d, case.H, case.hd, groups, case.hd ** -0.5, **kw)
    torch.cuda.synchronize()
    res = {"o": o.view(torch.int16).cpu(), "lse": stats[0].reshape(1, -1).view(torch.int32).cpu()}
    if fwd_only:
        return res
    dqkv = ops.attn_bwd(qkv_d, o, do.to(DEV), stats, case.H, case.hd, groups, case.hd ** -0.5, **kw)
    torch.cuda.synchronize()
    bits = dqkv.view(torch.int16).cpu()
    res.update(dq=bits[:, :D], dk=bits[:, D:2 * D], dv=bits[:, 2 * D:],
               delta=stats[1].reshape(1, -1).view(torch.int32).cpu())
    return res


def _attn_check_reference(case, res):
    """(b) for one launch's outputs; returns the largest ratio per output."""
    ex = ab.attn_variant(case)
    T, H = ab.attn_tokens(case), case.H
    ratios = {n: ab.assert_within(_values(res[n], BF16), ex[n], ex["E_" + n], f"{case.name} {n}")
              for n in ("o", "dq", "dk", "dv") if n in res}
    lse = _values(res["lse"], F32).reshape(H, T) * ab.LN2  # stats hold log2 units
    bad = ~((lse - ex["lse"]).abs() <= 2e-3 + 1e-4 * ex["lse"].abs())
    assert not bool(bad.any()), f"{case.name} lse: {int(bad.sum())} outside atol 2e-3 rtol 1e-4; first at {bad.nonzero()[0]}"
    if "delta" in res:
        # stats[1] = -rowsum(dO o O) over the O the forward stored: products of two bf16 are exact in f32,
        # and the sum takes fewer than 128 f32 roundings of 2^-24 each: |err| <= 2^-17 sum |dO o O|
        o64 = _values(res["o"], BF16).reshape(T, H, case.hd)
        do64 = ab.attn_inputs(case)[1].double().reshape(T, H, case.hd)
        exp = -(do64 * o64).sum(-1).t()
        mag = (do64 * o64).abs().sum(-1).t()
        got = _values(res["delta"], F32).reshape(H, T)
        bad = ~((got - exp).abs() <= 2.0 ** -17 * mag)
        assert not bool(bad.any()), f"{case.name} delta: {int(bad.sum())} rows off; first at {bad.nonzero()[0]}"
    return ratios


@pytest.mark.parametrize("case", ab.ATTN_CASES, ids=_ids)
def test_attn_edges(case):
    """Dense, frame-causal and dropout launches of the tables (tests/attn_bounds.py), checks (a)-(d). A frame
    block that covers every sequence must also equal the dense (fblk = 0) call bitwise."""
    res = _attn_framed(case)
    _report(case.name, _attn_check_reference(case, res))
    _same_bits(res, _attn_packed(case), f"{case.name} framed vs packed")
    _same_bits(res, _attn_framed(case), f"{case.name} second framed call")
    if case.fblk and all(case.fblk >= l for n, l in case.groups if n):
        _same_bits(res, _attn_framed(case, fblk=0), f"{case.name} vs fblk = 0")


@pytest.mark.parametrize("case", [c for c in ab.ATTN_CASES if c.name in ("dense0-hd88", "dense1-hd32", "fc43-hd64",
                                                                         "drop-hd80")], ids=_ids)
def test_attn_forward_only_leaves_stats1(case):
    """A forward without a backward (inference, the target encoder): stats[1] stays untouched, also by the
    last head's tail rows (checked inside _attn_framed), and O / lse equal the packed forward."""
    res = _attn_framed(case, fwd_only=True)
    _attn_check_reference(case, res)
    _same_bits(res, _attn_packed(case, fwd_only=True), f"{case.name} forward only")


@pytest.mark.parametrize("offs", [(4, 152, 296), (8, 156, 296), (8, 152, 297)])
def test_attn_misaligned_offset_is_an_error_without_a_launch(offs):
    """A q / k / v offset that is no multiple of 8 returns an error and writes nothing (valid, framed
    buffers: a launch would have left its mark)."""
    from vjepa2_amd import _lib

    case = next(c for c in ab.ATTN_CASES if c.name == "dense0-hd64")
    T, D, good, lds = _attn_dims(case)
    assert offs != good and any(o % 8 for o in offs)
    H, hd = case.H, case.hd
    ns, ln = _lib.int_array([n for n, _ in case.groups]), _lib.int_array([l for _, l in case.groups])
    fq = Frame(T, lds["ld"], BF16, {"qkv": (8, 3 * D + 40)})
    fq.put("qkv", torch.zeros(T, 3 * D + 40, dtype=BF16))
    fo = Frame(T, lds["ldo"], BF16, {"o": (8, D)})
    fs = Frame(1, 2 * H * T + 16, F32, {"stats": (8, 2 * H * T)})
    fd = Frame(T, lds["ldd"], BF16, {"dqkv": (8, 3 * D + 40)})
    lib = _lib.load()
    rc = lib.vj_attn_fwd_ex(T, H, hd, fq.ptr(), lds["ld"], *offs, fo.ptr(8), lds["ldo"], fs.ptr(8), hd ** -0.5,
                            len(case.groups), ns, ln, 0, 0.0, 0, _stream())
    assert rc != 0 and "column offsets" in _lib.last_error(), _lib.last_error()
    rc = lib.vj_attn_bwd_ex(T, H, hd, fq.ptr(), lds["ld"], *offs, fo.ptr(8), lds["ldo"], fo.ptr(8), lds["ldo"],
                            fs.ptr(8), fd.ptr(), lds["ldd"], hd ** -0.5, len(case.groups), ns, ln, None, 0, 0, 0, None,
                            None, 0, 0.0, 0, _stream())
    assert rc != 0 and "column offsets" in _lib.last_error(), _lib.last_error()
    torch.cuda.synchronize()
    fo.read("o", untouched=("o",))
    fs.read("stats", untouched=("stats",))
    fd.read("dqkv", untouched=("dqkv",))


# ------------------------------------------------------------------------------------------------
# vj_xattn_fwd / vj_xattn_bwd
def _xattn_framed(case):
    from vjepa2_amd._lib import call

    q, kv, do = ab.xattn_inputs(case)
    B, nq, N, H, hd = case.B, case.nq, case.N, case.H, case.hd
    D = H * hd
    ldq, ldkv, ldo, lddo, lddq, lddkv = D + 16, 2 * D + 24, D + 32, D + 40, D + 48, 2 * D + 56
    assert len({ldq, ldkv, ldo, lddo, lddq, lddkv}) == 6
    fq = Frame(B * nq, ldq, BF16, {"q": (8, D)})
    fq.put("q", q)
    fkv = Frame(B * N, ldkv, BF16, {"kv": (8, 2 * D)})
    fkv.put("kv", kv)
    fo = Frame(B * nq, ldo, BF16, {"o": (8, D)})
    fl = Frame(1, B * H * nq + 16, F32, {"lse2": (8, B * H * nq)})
    n = ctypes.c_long(0)
    call("vj_xattn_ws_floats", B, nq, N, H, hd, ctypes.byref(n))
    n = n.value
    wsent = SENTINEL[F32][1]
    ws = torch.full((n + 256,), wsent, dtype=torch.int32, device=DEV)  # the workspace, then guard
    what = case.name
    call("vj_xattn_fwd", B, nq, N, H, hd, fq.ptr(8), ldq, fkv.ptr(8), ldkv, fo.ptr(8), ldo, fl.ptr(8), hd ** -0.5,
         ws.data_ptr(), n, _stream())
    torch.cuda.synchronize()
    res = fo.read(f"{what} o")
    res.update(fl.read(f"{what} lse2"))
    assert bool((ws[n:] == wsent).all()), f"{what}: the forward wrote past its workspace"
    fdo = Frame(B * nq, lddo, BF16, {"do": (8, D)})
    fdo.put("do", do)
    fdq = Frame(B * nq, lddq, BF16, {"dq": (8, D)})
    fdkv = Frame(B * N, lddkv, BF16, {"dk": (8, D), "dv": (8 + D, D)})
    call("vj_xattn_bwd", B, nq, N, H, hd, fq.ptr(8), ldq, fkv.ptr(8), ldkv, fo.ptr(8), ldo, fdo.ptr(8), lddo,
         fl.ptr(8), hd ** -0.5, fdq.ptr(8), lddq, fdkv.ptr(8), lddkv, ws.data_ptr(), n, _stream())
    torch.cuda.synchronize()
    res.update(fdq.read(f"{what} dq"))
    res.update(fdkv.read(f"{what} dkv"))
    assert bool((ws[n:] == wsent).all()), f"{what}: the backward wrote past its workspace"
    _same_bits({"o": res["o"], "lse2": res["lse2"]}, {"o": fo.read(f"{what} o")["o"], "lse2": fl.read(what)["lse2"]},
               what + " inputs of the backward")
    for f in (fq, fkv, fdo):
        f.read(f"{what} operands")
    return res


def _xattn_packed(case):
    from vjepa2_amd import ops

    q, kv, do = (x.to(DEV) for x in ab.xattn_inputs(case))
    B, nq, N, H, hd = case.B, case.nq, case.N, case.H, case.hd
    D = H * hd
    o, lse2 = ops.xattn_fwd(q, kv, B, nq, N, H, hd, hd ** -0.5)
    dq, dkv = ops.xattn_bwd(q, kv, o, do, lse2, B, nq, N, H, hd, hd ** -0.5)
    torch.cuda.synchronize()
    bits = dkv.view(torch.int16).cpu()
    return dict(o=o.view(torch.int16).cpu(), lse2=lse2.reshape(1, -1).view(torch.int32).cpu(),
                dq=dq.view(torch.int16).cpu(), dk=bits[:, :D], dv=bits[:, D:])


@pytest.mark.parametrize("case", ab.XATTN_CASES, ids=_ids)
def test_xattn_edges(case):
    """Cross-attention at N = 1, 63, 64, 65 (one chunk, a full one, one key into the second), nq = 16, 17, 32,
    33 (one query pass, the dK / dV accumulation across two and three), checks (a)-(d)."""
    res = _xattn_framed(case)
    ex = ab.xattn_variant(case)
    ratios = {n: ab.assert_within(_values(res[n], BF16), ex[n], ex["E_" + n], f"{case.name} {n}")
              for n in ("o", "dq", "dk", "dv")}
    lse2 = _values(res["lse2"], F32).reshape(case.B * case.H, case.nq)
    err = (lse2 - ex["lse"] / ab.LN2).abs().max().item()
    assert err < 1e-4, f"{case.name} lse2: {err:.3g}"
    _report(case.name, ratios)
    _same_bits(res, _xattn_packed(case), f"{case.name} framed vs packed")
    _same_bits(res, _xattn_framed(case), f"{case.name} second framed call")
