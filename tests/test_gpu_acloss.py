"""GPU: the AC post-training loss kernels (vj_acloss.hip) through ops.ac_loss_fwd / ops.ac_loss_bwd against float64
torch autograd of the reference's op sequence (F.layer_norm without affine, mean(|zn - h| ** p) / p). Sources are
frame slices of longer sequences (sample stride > R * D), every output lives inside guard bands, inputs must come
back unchanged and two calls must agree bitwise.

Bounds. zn, the stats, the per-row sums and the loss have analytic bounds for the kernel's summation shape (below).
dz without normalisation is two or three roundings and has an analytic bound too. dz with normalisation is the
LayerNorm backward of a gradient that itself carries zn's error; there the yardstick is torch's own f32 evaluation
of the same sequence on the same device against float64, and the kernel is allowed 4 x its maximum error (the two
f32 summation orders are unrelated). The constant row (variance 0, rstd = 1 / sqrt(eps) = 316) amplifies every
rounding 316-fold, so it is measured against its own yardstick, not hidden under it nor allowed to widen the
other rows' one.

sign() is discontinuous at 0, so no per-element bound can hold where |zn - h| is below zn's own rounding error.
With normalisation the targets are therefore placed at least 0.05 away from the float64 zn; the exact-zero case
(sign(0) = 0) is tested where zn is exact: without normalisation, on elements with z == h bitwise."""

import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0**-24  # f32 unit roundoff
EPS = 1e-5
SENTINEL = -777.25
GL = 0.75  # the upstream gradient of the loss
SHAPES = [(1, 1, 96), (3, 5, 96), (2, 3, 1024), (2, 256, 1408), (1, 2, 2048), (65, 1, 96)]


def guarded(shape, pad=96):
    """(whole buffer, view of `shape` in its middle); check_guards(buf) after the call."""
    n = math.prod(shape)
    buf = torch.full((pad + n + pad,), SENTINEL, dtype=torch.float32, device=DEV)
    return buf, buf[pad:pad + n].view(*shape)


def check_guards(buf, pad=96):
    assert bool((buf[:pad] == SENTINEL).all()) and bool((buf[-pad:] == SENTINEL).all()), "guard band written"


def make_inputs(B, R, D, normalize, seed):
    """z: the last frame of a [B, T, R, D] sequence, h: frame 1 of a [B, T + 1, R, D] one, gzn dense."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g)  # noqa: E731
    T = 2 if R * D > 4096 else 3
    zseq = rn(B, T, R, D) * 1.7 + 0.3
    zseq[0, -1, 0] = 0.7  # a constant row: variance 0, no NaN
    hseq = rn(B, T + 1, R, D)
    if normalize:
        zn64 = F.layer_norm(zseq[:, -1].double(), (D,), eps=EPS)
        side = torch.where(torch.rand(B, R, D, device=DEV, generator=g) < 0.5, -1.0, 1.0)
        hseq[:, 1] = (zn64 + side * (0.05 + rn(B, R, D).abs())).float()
        assert float((zn64 - hseq[:, 1].double()).abs().min()) > 0.04
    else:
        zseq[:, -1, :, ::5] = hseq[:, 1, :, ::5]  # z == h bitwise on every fifth column
    z, h = zseq[:, -1], hseq[:, 1]
    assert B == 1 or (z.stride(0) == T * R * D and h.stride(0) == (T + 1) * R * D)
    return zseq, hseq, z, h, rn(B, R, D) * 0.01


def sequence(z, h, normalize, p, dtype):
    """The reference's op sequence in `dtype`: (zn, per-row sums, loss, dz without gzn); d(sum zn * gzn)/dz is
    added by the caller (autograd is linear in the upstream gradients)."""
    zz = z.to(dtype).detach().clone().requires_grad_()
    zn = F.layer_norm(zz, (zz.shape[-1],), eps=EPS) if normalize else zz
    t = torch.abs(zn - h.to(dtype)) ** p
    loss = torch.mean(t) / p
    return zz, zn, t.sum(-1), loss


def grads(z, h, normalize, p, gzn, dtype):
    zz, zn, _, loss = sequence(z, h, normalize, p, dtype)
    tot = loss * GL
    if gzn is not None:
        tot = tot + (zn * gzn.to(dtype)).sum()
    return torch.autograd.grad(tot, zz)[0]


def bounds(z, h, normalize, p):
    """float64 results and the bounds of an f32 evaluation in the kernel's summation shape (a lane adds
    4 * ceil(D / 256) <= 32 terms, then a 6-level tree: depth L = 4 ceil(D / 256) + 6; u = 2^-24):
      mean:    |dm| <= (L + 2) u mean|z|                       (the sum, 1 / D and the product)
      rstd:    relative (L + 4) / 2 u + 3 u                    (variance sum on rounded differences; add, sqrt, divide)
      zn:      |dzn| <= rstd |dm| + |zn| (2 u + rel(rstd))     (tests/test_gpu_plan_kernels.py frame_ref: same kernel body)
      d:       d^ = fl(zn^ - h): |d^ - d| <= |dzn| + u |d| =: e
      term:    p = 1: e;  p = 2: fl(d^ d^) - d^2 <= 2 |d| e + e^2 + u d^2
      rowsum:  sum of the term errors + (L + 1) u rowsum       (the D-term sum in the same shape, one store)
      loss:    the rowsum errors / (N p) + 2 u loss            (f64 accumulation, one scale, one rounding to f32)
    each doubled for the second-order terms dropped. Without normalisation zn = z exactly (dzn = 0)."""
    B, R, D = z.shape
    L = 4 * -(-D // 256) + 6
    z64, h64 = z.double(), h.double()
    out = {}
    if normalize:
        m = z64.mean(-1, keepdim=True)
        rstd = 1.0 / torch.sqrt(z64.var(-1, unbiased=False, keepdim=True) + EPS)
        zn = (z64 - m) * rstd
        bm = 2 * (L + 2) * U * z64.abs().mean(-1, keepdim=True)
        rel = ((L + 4) / 2 + 3) * U
        bzn = 2 * (rstd * (L + 2) * U * z64.abs().mean(-1, keepdim=True) + zn.abs() * (2 * U + rel))
        out.update(mean=m[..., 0], rstd=rstd[..., 0], bmean=bm[..., 0], brstd=2 * rel * rstd[..., 0])
    else:
        zn, bzn = z64, torch.zeros_like(z64)
    d = zn - h64
    e = bzn + U * d.abs()
    t = d.abs() ** p
    te = e if p == 1.0 else 2 * d.abs() * e + e * e + U * d * d
    rows = t.sum(-1)
    brows = 2 * (te.sum(-1) + (L + 1) * U * rows)
    loss = t.mean() / p
    out.update(zn=zn, bzn=bzn, rows=rows, brows=brows, loss=loss,
               bloss=brows.sum() / (B * R * D * p) + 2 * U * loss)
    return out


@pytest.mark.parametrize("p", [1.0, 2.0])
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("B,R,D", SHAPES)
def test_ac_loss_kernels_vs_float64(B, R, D, normalize, p):
    from vjepa2_amd import ops

    zseq, hseq, z, h, gzn = make_inputs(B, R, D, normalize, seed=B * 1000 + R * 10 + D + int(normalize))
    zseq0, hseq0, gzn0 = zseq.clone(), hseq.clone(), gzn.clone()
    ref = bounds(z, h, normalize, p)
    N = B * R * D

    # ---- forward: zn wanted and not wanted
    for want_zn in (True, False):
        zbuf, zn = guarded((B, R, D))
        sbuf, stats = guarded((B * R, 2))
        rbuf, rows = guarded((B * R,))
        lbuf, loss = guarded((1,))
        out = ops.ac_loss_fwd(z, h, normalize=normalize, loss_exp=p, eps=EPS, want_zn=want_zn,
                              zn=zn if want_zn else None, stats=stats, rowsum=rows, loss=loss)
        for b in (zbuf, sbuf, rbuf, lbuf):
            check_guards(b)
        if want_zn:
            assert out[1] is zn and torch.isfinite(zn).all()
            err = (zn.double() - ref["zn"]).abs()
            assert bool((err <= ref["bzn"]).all()), ("zn", (err - ref["bzn"]).max().item())
            if not normalize:
                assert torch.equal(zn, z)
        else:
            assert out[1] is None and bool((zn == SENTINEL).all())
        if normalize:
            assert torch.isfinite(stats).all()
            em = (stats[:, 0].double() - ref["mean"].reshape(-1)).abs()
            er = (stats[:, 1].double() - ref["rstd"].reshape(-1)).abs()
            assert bool((em <= ref["bmean"].reshape(-1)).all()), ("mean", em.max().item())
            assert bool((er <= ref["brstd"].reshape(-1)).all()), ("rstd", er.max().item())
        else:
            assert out[2] is None and bool((stats == SENTINEL).all())  # no stats without normalisation
        err = (rows.double() - ref["rows"].reshape(-1)).abs()
        print(f"rowsum err max {err.max().item():.3e} of bound min {ref['brows'].min().item():.3e}")
        assert bool((err <= ref["brows"].reshape(-1)).all()), ("rowsum", (err - ref["brows"].reshape(-1)).max().item())
        lerr = abs(float(loss.double()[0]) - float(ref["loss"]))
        print(f"loss {float(loss[0]):.8f} err {lerr:.3e} bound {float(ref['bloss']):.3e}")
        assert lerr <= float(ref["bloss"]), ("loss", lerr, float(ref["bloss"]))
        # two calls, bitwise
        l2, zn2, st2 = ops.ac_loss_fwd(z, h, normalize=normalize, loss_exp=p, eps=EPS, want_zn=want_zn)
        assert torch.equal(l2, loss) and (not want_zn or torch.equal(zn2, zn))
        assert not normalize or torch.equal(st2, stats)

    # ---- backward: gzn present and absent, on the stats of the last forward
    st = stats if normalize else None
    for use_g in (True, False):
        gz = gzn if use_g else None
        dz64 = grads(z, h, normalize, p, gz, torch.float64)
        dbuf, dz = guarded((B, R, D))
        got = ops.ac_loss_bwd(z, st, h, normalize=normalize, loss_exp=p, scale=GL / N, gzn=gz, dz=dz)
        check_guards(dbuf)
        assert got is dz and torch.isfinite(dz).all()
        err = (dz.double() - dz64).abs()
        if normalize:
            yard = (grads(z, h, normalize, p, gz, torch.float32).double() - dz64).abs()
            rest = torch.ones(B, R, dtype=torch.bool, device=DEV)
            rest[0, 0] = False  # the constant row against its own yardstick
            for name, sel in (("constant row", ~rest), ("other rows", rest)):
                if not bool(sel.any()):
                    continue
                e, y = err[sel].max().item(), yard[sel].max().item()
                print(f"dz {name}: kernel err {e:.3e}, torch f32 err {y:.3e}")
                assert e <= 4 * y, f"dz {name}: kernel max err {e:.3e} > 4 x torch f32's own {y:.3e} vs float64"
        else:
            # dz = fl(fl(s sign(d) |d| ** (p - 1)) + gzn): s rounded from f64 (u), d = fl(z - h) (u, p = 2 only),
            # the product (u), the sum (u |dz|); doubled
            gl64 = dz64 - (gz.double() if use_g else 0.0)
            bound = 2 * (3 * U * gl64.abs() + U * dz64.abs())
            assert bool((err <= bound).all()), ("dz", (err - bound).max().item())
            same = z == h
            assert bool(same[..., ::5].all())
            want = gz[same] if use_g else torch.zeros_like(dz[same])
            assert torch.equal(dz[same], want)  # sign(0) = 0: only gzn flows where z == h
        assert torch.equal(ops.ac_loss_bwd(z, st, h, normalize=normalize, loss_exp=p, scale=GL / N, gzn=gz), dz)

    # ---- the normalise-only call of the roll-out and its backward (no h: only gzn flows)
    _, zn3, st3 = ops.ac_loss_fwd(z, None, normalize=normalize, eps=EPS)
    err = (zn3.double() - ref["zn"]).abs()
    assert bool((err <= ref["bzn"]).all())
    dz3 = ops.ac_loss_bwd(z, st3, None, normalize=normalize, gzn=gzn)
    if normalize:
        zz = z.double().detach().clone().requires_grad_()
        want = torch.autograd.grad((F.layer_norm(zz, (D,), eps=EPS) * gzn.double()).sum(), zz)[0]
        zf = z.detach().clone().requires_grad_()
        yard = (torch.autograd.grad((F.layer_norm(zf, (D,), eps=EPS) * gzn).sum(), zf)[0].double() - want).abs()
        e = (dz3.double() - want).abs()
        rest = torch.ones(B, R, dtype=torch.bool, device=DEV)
        rest[0, 0] = False
        for sel in (~rest, rest):
            if bool(sel.any()):
                assert e[sel].max().item() <= 4 * yard[sel].max().item(), (e[sel].max().item(), yard[sel].max().item())
    else:
        assert torch.equal(dz3, gzn)

    assert torch.equal(zseq, zseq0) and torch.equal(hseq, hseq0) and torch.equal(gzn, gzn0)  # inputs are read only


def test_general_exponent_takes_the_powf_path():
    """loss_exp 1.5: neither special path. The device powf is accurate to a few ulp, not correctly rounded, so
    each term is given 8 u for the power in place of the product's single u of the p = 2 derivation."""
    from vjepa2_amd import ops

    B, R, D, p = 2, 3, 96, 1.5
    _, _, z, h, gzn = make_inputs(B, R, D, False, seed=11)
    z64, h64 = z.double(), h.double()
    t = (z64 - h64).abs() ** p
    loss, zn, _ = ops.ac_loss_fwd(z, h, normalize=False, loss_exp=p)
    L = 4 + 6
    bound = (2 * (8 + L + 2) * U * t.sum() / (B * R * D * p)).item()
    assert abs(float(loss[0]) - float(t.mean() / p)) <= bound
    dz = ops.ac_loss_bwd(z, None, h, normalize=False, loss_exp=p, scale=GL / (B * R * D), gzn=gzn)
    want = grads(z, h, False, p, gzn, torch.float64)
    gl64 = want - gzn.double()
    assert bool(((dz.double() - want).abs() <= 2 * (10 * U * gl64.abs() + U * want.abs())).all())
    same = z == h
    assert torch.equal(dz[same], gzn[same])  # 0 ** (p - 1) never reaches the sum
