"""Time the loss / metric stage of the frozen action-anticipation probe at the EK100 shape two ways in one
process: the fused kernel (vj_focal: three heads, loss, gradient, top-5 recall counters, no read-back) and the
reference's op sequence on the device (sigmoid_focal_loss per head + backward to the logits, then
ClassMeanRecall: sigmoid, topk(5), the per-sample `gt in p` membership loop with its host syncs).

Shape (configs/eval/vitl/ek100.yaml): B = 16, verbs 97, nouns 300, actions ~3.8 k (3806 here), one classifier.

    python tools/focal_bench.py [--rounds 9] [--reps 20]

Method: every timed window ends in a device synchronise and is taken with the host clock; both variants are
warmed up; they alternate round by round and the median, minimum and maximum over rounds are printed.
Needs the GPU (no fallback).
"""

import argparse
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from vjepa2_amd import ops  # noqa: E402


def _sync_time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def focal_torch(x, labels, alpha=0.25, gamma=2.0):
    """losses.py:9-49, reduction="sum"."""
    t = F.one_hot(labels, x.shape[1]).float()
    p = torch.sigmoid(x)
    ce = F.binary_cross_entropy_with_logits(x, t, reduction="none")
    p_t = p * t + (1 - p) * (1 - t)
    loss = ce * ((1 - p_t) ** gamma)
    if alpha >= 0:
        loss = (alpha * t + (1 - alpha) * (1 - t)) * loss
    return loss.sum()


def recall_torch(x, labels, tp, fn, k=5):
    """metrics.py:26-42 (one rank: no all-reduce)."""
    preds = torch.sigmoid(x).topk(k, dim=1).indices
    for p, gt in zip(preds, labels):
        if gt in p:
            tp[gt] += 1
        else:
            fn[gt] += 1


def stage_reference(xs, labels, tps, fns, with_loop):
    xs = [x.detach().requires_grad_(True) for x in xs]
    loss = sum(focal_torch(x, lb) for x, lb in zip(xs, labels))
    loss.backward()
    if with_loop:
        with torch.no_grad():
            for x, lb, tp, fn in zip(xs, labels, tps, fns):
                recall_torch(x, lb, tp, fn)
    return loss.detach(), [x.grad for x in xs]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--classes", type=int, nargs=3, default=[97, 300, 3806])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("focal_bench needs an MI355X (no CPU path)")
    dev = torch.device("cuda", 0)
    B, Cs = a.batch, a.classes
    g = torch.Generator(device=dev).manual_seed(1)
    buf = 3 * torch.randn(B, sum(Cs), device=dev, generator=g)  # the three heads' logits side by side
    xs, o = [], 0
    for C in Cs:
        xs.append(buf[:, o:o + C])
        o += C
    labels = [torch.randint(0, C, (B,), device=dev, generator=g) for C in Cs]
    i32 = dict(dtype=torch.int32, device=dev)
    tp, fn = [torch.zeros(C, **i32) for C in Cs], [torch.zeros(C, **i32) for C in Cs]
    out = (torch.empty(3, device=dev), torch.empty(3 * B, device=dev), [torch.empty(B, C, device=dev) for C in Cs],
           torch.empty(3, B, **i32))
    tpf, fnf = [torch.zeros(C, device=dev) for C in Cs], [torch.zeros(C, device=dev) for C in Cs]
    variants = {
        "vj_focal (3 heads: loss, dlogits, top-5 counters; no read-back)":
            lambda: ops.focal(xs, labels, tp, fn, alpha=0.25, gamma=2.0, k=5, out=out),
        "torch ops: 3 focal losses + backward to the logits":
            lambda: stage_reference(xs, labels, tpf, fnf, False),
        "torch ops: the same + ClassMeanRecall's topk and membership loop":
            lambda: stage_reference(xs, labels, tpf, fnf, True)}
    for f in variants.values():
        for _ in range(3):
            f()
    # same numbers first: the fused stage against the torch sequence on the same logits
    for t in tp + fn + tpf + fnf:
        t.zero_()
    loss, dls, hit = ops.focal(xs, labels, tp, fn, alpha=0.25, gamma=2.0, k=5, out=out)
    rl, rg = stage_reference(xs, labels, tpf, fnf, True)
    assert abs(float(loss.sum()) - float(rl)) <= 1e-4 * float(rl), (float(loss.sum()), float(rl))
    assert all(float((d - r).abs().max()) <= 1e-5 for d, r in zip(dls, rg))
    assert all(torch.equal(t.float(), tf) for t, tf in zip(tp + fn, tpf + fnf)), "TP / FN of the two stages differ"
    times = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, f in variants.items():
            times[k].append(_sync_time(lambda: [f() for _ in range(a.reps)]) / a.reps)
    print(f"anticipation loss / metric stage, one classifier, B {B}, classes {Cs}, with the gradient; device "
          f"{torch.cuda.get_device_name(0)}")
    print(f"ms per call (median [min, max] of {a.rounds} rounds x {a.reps} repeats, variants alternating):")
    for k, t in times.items():
        print(f"  {k:66s} {statistics.median(t):8.4f}  [{min(t):.4f}, {max(t):.4f}]")
    ks = list(variants)
    fused = statistics.median(times[ks[0]])
    for k in ks[1:]:
        print(f"  fused / ({k}): {fused / statistics.median(times[k]):.4f}x the time")


if __name__ == "__main__":
    main()
