"""GPU: the fused multi-view softmax cross-entropy (vj_xent, ops.xent) against float64
F.cross_entropy / F.softmax on the CPU.

Bounds. The reference is float64; the margin comes from torch's own float32 CPU result on the same
inputs: with d_loss / d_row / d_grad its max deviation from float64 (at most 7.2e-7 and 5.6e-8 for the loss
and the gradient over the seeded shapes below),
    |loss - ref|     <= max(4 d_loss, 4 * 2^-23 * max(1, |ref|))     (and the same for row_loss)
    |dlogits - ref|  <= max(4 d_grad, 2^-20)
i.e. a few float32 roundings at the loss's magnitude and a few ulp at the gradient's scale (<= 1).
pred and correct must equal the float64 reference for every row: the test first asserts on the reference
alone that every row's top-1 mean-softmax probability is at least 1.001 x its top-2 (minimum over the
seeded shapes 1.0024 at (3, 16, 400)), so no near-tie can excuse a wrong argmax.
Each case runs with ld = C and with ld = C + 5 inside NaN-filled guard bands (input and gradient
buffers): padding and bands must come back bit-unchanged.
"""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 64
# (V, B, C): the probe configs' class counts (27, 48, 174, 400, 1000: none a multiple of 64), one class, one
# and several lane sweeps per row, more rows than one workgroup's waves
SHAPES = [(1, 1, 1), (1, 7, 48), (3, 4, 174), (2, 5, 1000), (3, 2, 1025), (2, 3, 4099), (1, 64, 27), (3, 16, 400)]
# the kernel's other paths: several workgroups + the finishing launch (V*B*C > 65536 and B > 16), more
# than 64 views (statistics no longer in registers), the widest supported row in one workgroup
EXTRA = [(2, 40, 1025), (65, 2, 7), (1, 2, 32768)]


def _inputs(V, B, C):
    g = torch.Generator().manual_seed(1000 * V + 10 * B + C)
    logits = 3 * torch.randn(V * B, C, generator=g)
    labels = torch.randint(0, C, (B,), generator=g)
    if B >= 2:
        labels[0] = 0
        labels[-1] = C - 1
    return logits, labels


def _reference(logits, labels, V, dtype=torch.float64):
    """(loss [V], row_loss [V*B], dlogits [V*B, C], mean softmax [B, C]) in `dtype` on the CPU; an
    out-of-range label matches no class (loss = log-sum-exp, gradient = softmax / B)."""
    R, C = logits.shape
    B = R // V
    x = logits.to(dtype)
    lab = labels.long().repeat(V)
    ok = (lab >= 0) & (lab < C)
    if bool(ok.all()):
        row = F.cross_entropy(x, lab, reduction="none")
        loss = torch.stack([F.cross_entropy(x[v * B:(v + 1) * B], labels.long()) for v in range(V)])
    else:
        row = torch.logsumexp(x, 1) - torch.where(ok, x.gather(1, lab.clamp(0, C - 1)[:, None])[:, 0],
                                                  torch.zeros((), dtype=dtype))
        loss = row.view(V, B).mean(1)
    p = F.softmax(x, dim=1)
    onehot = torch.zeros_like(p)
    onehot[ok, lab[ok]] = 1
    return loss, row, (p - onehot) / B, p.view(V, B, C).mean(0)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _padded(R, C, ld, fill=None):
    """A [R, C] view with row stride ld inside a NaN-filled buffer with guard bands; returns (buffer, view)."""
    buf = torch.full((2 * GUARD + R * ld,), float("nan"), device=DEV)
    view = buf[GUARD:GUARD + R * ld].view(R, ld)[:, :C]
    if fill is not None:
        view.copy_(fill)
    return buf, view


def _untouched(buf_before, buf_after, R, C, ld):
    """Everything outside the [R, C] view is bit-identical."""
    keep = torch.ones(buf_before.numel(), dtype=torch.bool, device=buf_before.device)
    keep[GUARD:GUARD + R * ld].view(R, ld)[:, :C] = False
    return torch.equal(_bits(buf_before)[keep], _bits(buf_after)[keep])


def _run(logits, labels, V, pad, want_grad=True):
    from vjepa2_amd import ops

    R, C = logits.shape
    B = R // V
    if not pad:
        return ops.xent(logits.to(DEV), labels, views=V, want_grad=want_grad), True
    ld = C + 5
    xbuf, x = _padded(R, C, ld, logits.to(DEV))
    gbuf, gview = _padded(R, C, ld)
    x0, g0 = xbuf.clone(), gbuf.clone()
    out = (torch.empty(V, device=DEV), torch.empty(R, device=DEV), gview if want_grad else None,
           torch.empty(B, dtype=torch.int32, device=DEV), torch.empty(1, dtype=torch.int32, device=DEV))
    res = ops.xent(x, labels, views=V, want_grad=want_grad, out=out)
    torch.cuda.synchronize()
    clean = torch.equal(_bits(x0), _bits(xbuf)) and _untouched(g0, gbuf, R, C, ld)
    if not want_grad:
        clean = clean and torch.equal(_bits(g0), _bits(gbuf))
    return res, clean


def _check(logits, labels, V, pad, tag):
    ref_loss, ref_row, ref_grad, ref_prob = _reference(logits, labels.cpu(), V)
    f_loss, f_row, f_grad, _ = _reference(logits, labels.cpu(), V, torch.float32)
    d_loss = (f_loss.double() - ref_loss).abs().max().item()
    d_row = (f_row.double() - ref_row).abs().max().item()
    d_grad = (f_grad.double() - ref_grad).abs().max().item()
    (loss, row, grad, pred, correct), clean = _run(logits, labels, V, pad)
    loss, row, grad = loss.cpu().double(), row.cpu().double(), grad.cpu().double()
    tol = lambda d, ref: torch.clamp(4 * 2.0**-23 * ref.abs().clamp_min(1.0), min=4 * d)  # noqa: E731
    e_loss, e_row, e_grad = (loss - ref_loss).abs(), (row - ref_row).abs(), (grad - ref_grad).abs().max().item()
    print(f"{tag} pad={pad}: loss err {e_loss.max().item():.3e} (torch f32 {d_loss:.3e}), row err "
          f"{e_row.max().item():.3e} (torch f32 {d_row:.3e}), grad err {e_grad:.3e} (torch f32 {d_grad:.3e})")
    assert torch.isfinite(loss).all() and torch.isfinite(row).all() and torch.isfinite(grad).all()
    assert bool((e_loss <= tol(d_loss, ref_loss)).all()), (e_loss.max().item(), d_loss)
    assert bool((e_row <= tol(d_row, ref_row)).all()), (e_row.max().item(), d_row)
    assert e_grad <= max(4 * d_grad, 2.0**-20), (e_grad, d_grad)
    assert clean, "padding or guard bands were written"
    return pred.cpu(), int(correct.item()), ref_prob


@pytest.mark.parametrize("pad", [False, True])
@pytest.mark.parametrize("V,B,C", SHAPES + EXTRA)
def test_xent_vs_float64(V, B, C, pad):
    logits, labels = _inputs(V, B, C)
    _, _, _, ref_prob = _reference(logits, labels, V)
    if C > 1:  # on the reference alone: every row's argmax is decided by more than rounding
        top2 = ref_prob.topk(2, dim=1).values
        ratio = (top2[:, 0] / top2[:, 1]).min().item()
        print(f"({V}, {B}, {C}): min top-1 / top-2 of the mean softmax {ratio:.4f}")
        assert ratio >= 1.001, ratio
    pred, correct, _ = _check(logits, labels, V, pad, f"({V}, {B}, {C})")
    ref_pred = ref_prob.argmax(1)
    assert torch.equal(pred.long(), ref_pred), (pred, ref_pred)  # every row, nothing excluded
    assert correct == int((ref_pred == labels).sum())


def test_xent_extreme_rows():
    """Logits of +-1e4 and rows of equal values: finite, and the float64 losses (160.4741, 0, 1.3863)."""
    logits = torch.tensor([[80.0, -80.0, 0.0, 79.5], [-1e4, 0.0, 1e4, 5.0], [3e4] * 4])
    labels = torch.tensor([1, 2, 3])
    for pad in (False, True):
        pred, correct, _ = _check(logits, labels, 1, pad, "extreme")
        assert pred.tolist() == [0, 2, 0] and correct == 1  # equal values: the lowest index
    ref = _reference(logits, labels, 1)[1]
    assert torch.allclose(ref, torch.tensor([160.4741, 0.0, 1.3863], dtype=torch.float64), atol=1e-4)


def test_xent_exact_tie_takes_lower_index():
    from vjepa2_amd import ops

    g = torch.Generator().manual_seed(5)
    for V, B, C, a, b in ((1, 2, 174, 17, 130), (3, 2, 1025, 64, 1024), (2, 1, 400, 63, 64)):
        logits = torch.randn(V * B, C, generator=g)
        logits[:, a] = 9.0  # identical maximal columns in every view: identical probabilities
        logits[:, b] = 9.0
        labels = torch.full((B,), a)
        _, _, _, pred, correct = ops.xent(logits.to(DEV), labels, views=V)
        assert pred.tolist() == [a] * B and int(correct) == B


def test_xent_validation_mode_and_determinism():
    from vjepa2_amd import ops

    for V, B, C in ((3, 4, 174), (2, 40, 1025)):
        logits, labels = _inputs(V, B, C)
        x, lab = logits.to(DEV), labels.to(DEV)
        a = ops.xent(x, lab, views=V)
        b = ops.xent(x, lab, views=V)
        for s, t in zip(a, b):
            assert torch.equal(_bits(s), _bits(t))  # bitwise: fixed-order reductions
        (v, clean) = _run(logits, labels, V, pad=True, want_grad=False)  # dlogits = NULL
        assert clean and v[2] is None
        for i in (0, 1, 3, 4):
            assert torch.equal(_bits(a[i]), _bits(v[i]))


def test_xent_out_of_range_labels(monkeypatch):
    """Device labels are not read back (check off): -100 and C index nothing and match no class. CPU
    labels raise like F.cross_entropy's index check."""
    from vjepa2_amd import ops

    monkeypatch.delenv("VJ_CHECK_INDICES", raising=False)
    V, B, C = 2, 4, 48
    logits, labels = _inputs(V, B, C)
    labels[1], labels[2] = -100, C
    for dtype in (torch.int64, torch.int32):
        pred, correct, ref_prob = _check(logits, labels.to(dtype).to(DEV), V, True, f"labels {dtype}")
        ref_pred = ref_prob.argmax(1)
        assert torch.equal(pred.long(), ref_pred)
        assert correct == int((ref_pred == labels).sum())
    for bad in (-1, C):
        cpu = labels.clamp(0, C - 1)
        cpu[3] = bad
        with pytest.raises(IndexError):
            ops.xent(logits.to(DEV), cpu, views=V)
    monkeypatch.setenv("VJ_CHECK_INDICES", "1")
    with pytest.raises(IndexError):
        ops.xent(logits.to(DEV), labels.to(DEV), views=V)
