"""GPU: the fused sigmoid focal loss + gradient + top-k recall bookkeeping (vj_focal, ops.focal).

Loss and gradient. The reference is the formula of evals/action_anticipation_frozen/losses.py:9-49
(reduction="sum") restated with torch ops and differentiated by autograd, in float64 on the CPU. The bound
is measured: the same formula in torch float32 ops on the device has a max error E against float64, and
the kernel may be at most max(4 E, 8 float32 ulp of the largest reference magnitude) away (its softplus /
exp forms are a different but equally valid float32 evaluation, each a few ulp off). Each case prints
its ratios kernel error / that bound. The float64 reference is itself only good to about one float64 ulp of 1
per element: torch evaluates log(1 + e^-|x|) and 1 - p, which lose everything below 2^-53 (a non-target logit
of -44 has loss 7.5e-20; the float64 formula returns 0, and at +80 the target's gradient sigmoid(80) - 1 is 0
instead of -1.8e-35). Where every term of a tensor is that small the two bounds above collapse to ~1e-41, so
REF64_ABS = 2^-50 per element is added for the reference's own error: nine orders below one float32 ulp of any
loss or gradient of ordinary size, it decides only those degenerate cases.
Measured over all cases below: the largest ratio is 0.32 for a loss and 0.46 for a gradient.

Hits and counters must equal the reference's sigmoid -> zero the invalid classes -> topk -> membership on
rows that are tie-free by construction, x = (perm(C) - C/2) / 512. Where the reference itself would have to
break a tie (an invalid label with fewer than k valid classes: all invalid classes are 0 after the mask), and
in the two explicit tie tests, the kernel is held to its documented rank rule instead.

Logits are column slices of one wider NaN-filled buffer, gradients have a row stride > C inside a NaN-filled
buffer, loss / hit / counters sit between guard bands: everything outside the views must stay bit-unchanged.
"""

import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 32
K = 5
REF64_ABS = 2.0 ** -50
BS = (1, 3, 17)
CS = (1, 4, 5, 6, 63, 64, 65, 300, 4000)
# B * sum(C) <= 16384 runs as one workgroup, anything above as several + the finishing launch: the shapes
# next to the switch on both sides (16384 / 16385 / 16388 elements), one row too long for one workgroup (a
# single several-waves workgroup that finishes itself), and three-head mixes on both sides
EDGE = [(4, (4096,)), (5, (3277,)), (1, (16385,)), (2, (4097, 4097))]
MIXED = [(1, (7, 9, 13)), (3, (65, 1, 300)), (17, (97, 300, 4000)), (3, (4000, 64, 5))]
# (alpha, gamma, scale): scale None = logits stretched to reach +-80
COMBOS = [(0.25, 2.0, 3.0), (-1.0, 2.0, 3.0), (0.25, 1.5, 3.0), (0.25, 0.0, 3.0), (0.25, 2.0, None), (-1.0, 1.5, None),
          (-1.0, 0.0, None)]


def _formula(x, labels, alpha, gamma):
    """losses.py:9-49 with reduction="sum"; a label outside [0, C) has no target class."""
    B, C = x.shape
    lab = labels.long()
    ok = (lab >= 0) & (lab < C)
    t = torch.zeros_like(x)
    t[ok, lab[ok]] = 1
    p = torch.sigmoid(x)
    ce = F.binary_cross_entropy_with_logits(x, t, reduction="none")
    p_t = p * t + (1 - p) * (1 - t)
    loss = ce * ((1 - p_t) ** gamma)
    if alpha >= 0:
        loss = (alpha * t + (1 - alpha) * (1 - t)) * loss
    return loss.sum()


def _loss_grad(x, labels, alpha, gamma, dtype, device):
    xx = x.to(device=device, dtype=dtype).requires_grad_(True)
    loss = _formula(xx, labels.to(device), alpha, gamma)
    (g,) = torch.autograd.grad(loss, xx)
    return loss.detach().double().cpu(), g.double().cpu()


def _ulp32(v):
    return 2.0 ** (math.floor(math.log2(v)) - 23) if v > 0 else 2.0 ** -149


def _logits(B, Cs, scale, seed):
    g = torch.Generator().manual_seed(seed)
    xs = []
    for C in Cs:
        x = torch.randn(B, C, generator=g)
        x = x * scale if scale is not None else x / x.abs().max() * 80
        if scale is None and B * C >= 2:
            x.view(-1)[0], x.view(-1)[-1] = 80.0, -80.0
        xs.append(x)
    labels = [torch.randint(0, C, (B,), generator=g) for C in Cs]
    if scale is None:
        for x, lb in zip(xs, labels):
            lb[0] = 0  # the +80 element is a target
    return xs, labels


class _Bufs:
    """Inputs and outputs of one call inside guard bands: logits as column slices of one NaN-filled buffer,
    gradients with row stride C + 3, loss / row_loss / hit / tp / fn between bands."""

    def __init__(self, xs, B):
        Cs = [x.shape[1] for x in xs]
        nseg = len(xs)
        self.B, self.Cs, self.nseg = B, Cs, nseg
        W = sum(Cs) + 2 * (nseg + 1)
        self.xbuf = torch.full((B, W), float("nan"), device=DEV)
        self.x, o = [], 2
        for x in xs:
            self.x.append(self.xbuf[:, o:o + x.shape[1]])
            self.x[-1].copy_(x)
            o += x.shape[1] + 2
        self.f = torch.full((4 * GUARD + nseg + nseg * B,), float("nan"), device=DEV)
        self.loss = self.f[GUARD:GUARD + nseg]
        self.row_loss = self.f[2 * GUARD + nseg:2 * GUARD + nseg + nseg * B]
        self.dbuf = [torch.full((2 * GUARD + B * (C + 3),), float("nan"), device=DEV) for C in Cs]
        self.d = [b[GUARD:GUARD + B * (C + 3)].view(B, C + 3)[:, :C] for b, C in zip(self.dbuf, Cs)]
        self.i = torch.full((3 * GUARD + nseg * B + 2 * sum(Cs) + 2 * GUARD * nseg,), -777, dtype=torch.int32,
                            device=DEV)
        o = GUARD
        self.hit = self.i[o:o + nseg * B].view(nseg, B)
        o += nseg * B + GUARD
        self.tp, self.fn = [], []
        for C in Cs:
            self.tp.append(self.i[o:o + C])
            o += C + GUARD
            self.fn.append(self.i[o:o + C])
            o += C + GUARD
        for t in self.tp + self.fn:
            t.zero_()
        self.snap()

    def snap(self):
        self.before = [t.clone() for t in (self.xbuf, self.f, self.i, *self.dbuf)]

    def check_untouched(self):
        """Bit-identical outside the output views (inputs entirely)."""
        after = (self.xbuf, self.f, self.i, *self.dbuf)
        keep = [torch.ones_like(t, dtype=torch.bool) for t in after]
        n, B = self.nseg, self.B
        keep[1][GUARD:GUARD + n] = False
        keep[1][2 * GUARD + n:2 * GUARD + n + n * B] = False
        ki = keep[2]
        for v in (self.hit, *self.tp, *self.fn):
            off = v.storage_offset()
            ki[off:off + v.numel()] = False
        for kd, C in zip(keep[3:], self.Cs):
            kd[GUARD:GUARD + B * (C + 3)].view(B, C + 3)[:, :C] = False
        for b, a, k in zip(self.before, after, keep):
            bits = torch.int32
            assert torch.equal(b.view(bits)[k], a.view(bits)[k]), "a write outside the output views"

    def out(self):
        return (self.loss, self.row_loss, self.d, self.hit)


def _rank_hits(x, labels, valid, k):
    """The documented rank rule, in plain Python on the CPU (x float32 [B, C])."""
    B, C = x.shape
    hits = []
    for b in range(B):
        lb = int(labels[b])
        if not 0 <= lb < C:
            hits.append(None)
            continue
        v = [True] * C if valid is None else [bool(z) for z in valid]
        row = x[b].tolist()
        xl = row[lb]
        if v[lb]:
            rank = sum(1 for c in range(C) if v[c] and (row[c] > xl or (row[c] == xl and c < lb)))
        else:
            rank = sum(1 for c in range(C) if v[c] or c < lb)
        hits.append(rank < k)
    return hits


def _reference_hits(x, labels, valid, k):
    """metrics.py:26-42 on the CPU: sigmoid, zero the invalid classes, topk, membership."""
    s = torch.sigmoid(x)
    if valid is not None:
        m = torch.zeros_like(s)
        for c in torch.nonzero(valid).flatten().tolist():
            m[:, c] = s[:, c]
        s = m
    preds = s.topk(min(k, x.shape[1]), dim=1).indices
    return [bool(gt in p) for p, gt in zip(preds, labels)]


def _check_loss_case(B, Cs, i32):
    nseg = len(Cs)
    for ci, (alpha, gamma, scale) in enumerate(COMBOS):
        xs, labels = _logits(B, Cs, scale, seed=100 * B + 7 * sum(Cs) + ci)
        if i32:
            labels = [lb.int() for lb in labels]
        bufs = _Bufs(xs, B)
        lab_dev = [lb.to(DEV) for lb in labels]
        loss, dls, hit = ops_focal(bufs.x, lab_dev, bufs.tp, bufs.fn, alpha=alpha, gamma=gamma, k=K, out=bufs.out())
        torch.cuda.synchronize()
        bufs.check_untouched()
        first = (loss.clone(), [d.clone() for d in dls], hit.clone())
        tp1 = [t.clone() for t in bufs.tp]
        fn1 = [t.clone() for t in bufs.fn]
        for s in range(nseg):
            ref_l, ref_g = _loss_grad(xs[s], labels[s], alpha, gamma, torch.float64, "cpu")
            t32_l, t32_g = _loss_grad(xs[s], labels[s], alpha, gamma, torch.float32, DEV)
            assert torch.isfinite(ref_l) and torch.isfinite(ref_g).all()
            e_l = abs(float(t32_l - ref_l))
            e_g = float((t32_g - ref_g).abs().max())
            bound_l = max(4 * e_l, 8 * _ulp32(abs(float(ref_l)))) + B * Cs[s] * REF64_ABS
            bound_g = max(4 * e_g, 8 * _ulp32(float(ref_g.abs().max()))) + REF64_ABS
            k_l = abs(float(loss[s].double().cpu() - ref_l))
            k_g = float((dls[s].double().cpu() - ref_g).abs().max())
            print(f"focal B={B} C={Cs[s]} nseg={nseg} alpha={alpha} gamma={gamma} scale={scale}: "
                  f"loss err {k_l:.3e} (torch f32 E {e_l:.3e}, bound {bound_l:.3e}, ratio {k_l / bound_l:.3f}) "
                  f"grad err {k_g:.3e} (E {e_g:.3e}, bound {bound_g:.3e}, ratio {k_g / bound_g:.3f})")
            assert k_l <= bound_l, (B, Cs[s], alpha, gamma, scale, k_l, bound_l)
            assert k_g <= bound_g, (B, Cs[s], alpha, gamma, scale, k_g, bound_g)
            # every label was counted exactly once, as the hit flag says
            want_tp = torch.zeros(Cs[s], dtype=torch.int32)
            want_fn = torch.zeros(Cs[s], dtype=torch.int32)
            for b, h in enumerate(_rank_hits(xs[s], labels[s], None, K)):
                assert bool(hit[s, b]) == h
                (want_tp if h else want_fn)[int(labels[s][b])] += 1
            assert torch.equal(bufs.tp[s].cpu(), want_tp) and torch.equal(bufs.fn[s].cpu(), want_fn)
        # a second call: bitwise-equal floats, counters accumulated
        loss2, dls2, hit2 = ops_focal(bufs.x, lab_dev, bufs.tp, bufs.fn, alpha=alpha, gamma=gamma, k=K, out=bufs.out())
        torch.cuda.synchronize()
        assert torch.equal(loss2.view(torch.int32), first[0].view(torch.int32))
        assert torch.equal(hit2, first[2])
        for s in range(nseg):
            assert torch.equal(dls2[s].contiguous().view(torch.int32), first[1][s].contiguous().view(torch.int32))
            assert torch.equal(bufs.tp[s], 2 * tp1[s]) and torch.equal(bufs.fn[s], 2 * fn1[s])


def ops_focal(*a, **kw):
    from vjepa2_amd import ops

    return ops.focal(*a, **kw)


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("B", BS)
def test_focal_loss_and_gradient_one_head(B, C):
    _check_loss_case(B, (C,), i32=(B + C) % 2 == 1)


@pytest.mark.parametrize("B,Cs", EDGE + MIXED)
def test_focal_loss_and_gradient_switch_and_mixed_heads(B, Cs):
    _check_loss_case(B, Cs, i32=B % 2 == 0)


def _tie_free_rows(B, C, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.stack([(torch.randperm(C, generator=g).float() - C / 2) / 512 for _ in range(B)])
    return x, g


def _masks(C, g):
    """None, about half the classes, fewer than k classes, one class."""
    out = [None]
    if C >= 2:
        out.append(torch.rand(C, generator=g) < 0.5)
        few = torch.zeros(C, dtype=torch.bool)
        few[torch.randperm(C, generator=g)[:min(C - 1, K - 2)]] = True
        out.append(few)
        one = torch.zeros(C, dtype=torch.bool)
        one[C // 2] = True
        out.append(one)
    return out


@pytest.mark.parametrize("B,Cs", [(1, (1,)), (3, (4, 5, 6)), (17, (63, 64, 65)), (17, (97, 300, 4000)), (3, (300,)),
                                  (5, (3277,))])
def test_focal_hits_and_counters_equal_the_reference(B, Cs):
    g0 = torch.Generator().manual_seed(B + sum(Cs))
    for mi in range(4):
        xs, labels, valids = [], [], []
        for s, C in enumerate(Cs):
            x, g = _tie_free_rows(B, C, seed=31 * B + C + mi)
            ms = _masks(C, g)
            v = ms[mi % len(ms)]
            lb = torch.randint(0, C, (B,), generator=g0)
            if v is not None and B >= 2:  # labels inside and outside the valid set
                inside = torch.nonzero(v).flatten()
                outside = torch.nonzero(~v).flatten()
                if len(inside):
                    lb[0] = inside[0]
                if len(outside):
                    lb[1] = outside[-1]
            xs.append(x), labels.append(lb), valids.append(v)
        bufs = _Bufs(xs, B)
        lab_dev = [lb.to(DEV) for lb in labels]
        val_dev = [None if v is None else v.to(DEV) for v in valids]
        for kind in (1, 0):
            for t in bufs.tp + bufs.fn:
                t.zero_()
            bufs.hit.fill_(-777)
            bufs.snap()
            loss, dls, hit = ops_focal(bufs.x, lab_dev, bufs.tp, bufs.fn, valid=val_dev, k=K, loss_kind=kind,
                                       out=bufs.out())
            torch.cuda.synchronize()
            bufs.check_untouched()
            if kind == 0:  # metrics only: the loss and gradient buffers that were handed in stay as they were
                assert loss is None and dls is None
                for b4, now in zip(bufs.before[1:2] + bufs.before[3:], [bufs.f, *bufs.dbuf]):
                    assert torch.equal(b4.view(torch.int32), now.view(torch.int32))
            for s, C in enumerate(Cs):
                v, x, lb = valids[s], xs[s], labels[s]
                ref = _reference_hits(x, lb, v, K)
                rule = _rank_hits(x, lb, v, K)
                nvalid = C if v is None else int(v.sum())
                want_tp = torch.zeros(C, dtype=torch.int32)
                want_fn = torch.zeros(C, dtype=torch.int32)
                for b in range(B):
                    label_valid = v is None or bool(v[lb[b]])
                    if label_valid or nvalid >= min(K, C):  # the reference's own answer is tie-free
                        assert rule[b] == ref[b], (s, b)
                    assert bool(hit[s, b]) == rule[b], (s, b, int(lb[b]))
                    (want_tp if rule[b] else want_fn)[int(lb[b])] += 1
                assert torch.equal(bufs.tp[s].cpu(), want_tp), s
                assert torch.equal(bufs.fn[s].cpu(), want_fn), s


def test_focal_tie_rule():
    """Against the rule's definition, not torch: among equal logits the lower class index ranks first."""
    C = 8
    # an all-zero row: label l has l classes ahead of it
    x = torch.zeros(C, C)
    labels = torch.arange(C)
    # the label tied at the boundary: four classes are greater, one equals the label's logit
    lo = torch.tensor([[9., 9., 9., 9., 1., 0., 1., 0.]])  # label 6 ties with class 4 (lower index): rank 5, miss
    hi = torch.tensor([[9., 9., 9., 9., 1., 0., 1., 0.]])  # label 4 ties with class 6 (higher index): rank 4, hit
    nanrow = torch.tensor([[float("nan")] * 7 + [0.]])     # a NaN is not greater: label 7 has rank 0
    x = torch.cat([x, lo, hi, nanrow]).to(DEV)
    labels = torch.cat([labels, torch.tensor([6, 4, 7])]).to(DEV)
    tp = torch.zeros(C, dtype=torch.int32, device=DEV)
    fn = torch.zeros(C, dtype=torch.int32, device=DEV)
    _, _, hit = ops_focal([x], [labels], [tp], [fn], k=K, loss_kind=0)
    assert hit[0].tolist() == [1, 1, 1, 1, 1, 0, 0, 0] + [0, 1, 1]
    assert tp.tolist() == [1, 1, 1, 1, 2, 0, 0, 1] and fn.tolist() == [0, 0, 0, 0, 0, 1, 2, 1]
    # the label's own class invalid: valid classes count as greater, lower invalid indices as ties
    valid = torch.tensor([0, 1, 0, 1, 0, 1, 0, 0], dtype=torch.bool, device=DEV)  # 3 valid
    tp.zero_(), fn.zero_()
    _, _, hit = ops_focal([x[:C]], [labels[:C]], [tp], [fn], valid=[valid], k=K, loss_kind=0)
    # label 0: rank 3, label 2: 3 + 1, label 4: 3 + 2 = 5 (miss), 6 and 7: miss; valid labels 1, 3, 5: ranks 0, 1, 2
    assert hit[0].tolist() == [1, 1, 1, 1, 0, 1, 0, 0]


def test_focal_out_of_range_device_label_touches_no_counter():
    B, C = 4, 70
    xs, labels = _logits(B, (C,), 3.0, seed=5)
    labels[0][1], labels[0][2] = C, -1
    bufs = _Bufs(xs, B)
    loss, dls, hit = ops_focal(bufs.x, [labels[0].to(DEV)], bufs.tp, bufs.fn, k=K, out=bufs.out())
    torch.cuda.synchronize()
    bufs.check_untouched()
    assert hit[0, 1] == 0 and hit[0, 2] == 0
    assert int(bufs.tp[0].sum() + bufs.fn[0].sum()) == 2
    ref_l, ref_g = _loss_grad(xs[0], labels[0], 0.25, 2.0, torch.float64, "cpu")  # rows 1, 2: no target class
    assert abs(float(loss[0]) - float(ref_l)) <= 8 * _ulp32(float(ref_l))
    assert float((dls[0].double().cpu() - ref_g).abs().max()) <= 8 * _ulp32(float(ref_g.abs().max()))
    with pytest.raises(IndexError, match="out of range"):
        ops_focal(bufs.x, [labels[0]], bufs.tp, bufs.fn)  # CPU labels are checked on the host
