"""Time the frozen-encoder probe train step (vjepa2_amd/evals/video_classification_frozen.py) at the
reference's ViT-L SSv2 shape, on random tokens with no encoder, and its loss / accuracy stage alone two
ways in the same process: the fused kernel (vj_xent) and the reference's op sequence on the device.

Shape (configs/eval/vitl/ssv2.yaml): D = 1024, 16 heads, 4 probe blocks, 174 classes, B = 4,
2 segments x 2048 tokens per view, 3 views stacked, 20 classifier heads.

    python tools/probe_bench.py [--heads 20] [--steps 5] [--warmup 2] [--stage-rounds 9]

Method: every timed window ends in a device synchronise and is taken with the host clock; every shape
is warmed up first; the two loss-stage variants alternate round by round in one process and the
median, minimum and maximum over rounds are printed. Needs the GPU (no fallback).
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
from vjepa2_amd.attentive_pooler import AttentiveClassifier  # noqa: E402
from vjepa2_amd.evals.probe import init_opt  # noqa: E402
from vjepa2_amd.evals.video_classification_frozen import ProbeTrainer  # noqa: E402


def _sync_time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stage_fused(logits, labels, V, acc):
    """vj_xent per head + the meter's device-side bookkeeping; no host read-back."""
    B = labels.numel()
    correct = torch.empty(len(logits), dtype=torch.int32, device=labels.device)
    for h, lg in enumerate(logits):
        loss, row, dl, pred, _ = ops.xent(lg, labels, views=V, out=(acc["loss"][h], acc["row"], acc["dl"], acc["pred"],
                                                                  correct[h:h + 1]))
    return correct


def stage_reference(logits, labels, V, backward):
    """eval.py:325-331 per head: CrossEntropyLoss per view, view-averaged softmax, top-1, float();
    with `backward`, also the gradient of the view losses with respect to the logits (eval.py:339)."""
    B = labels.numel()
    crit = torch.nn.CrossEntropyLoss()
    accs = []
    for lg in logits:
        if backward:
            lg = lg.detach().requires_grad_(True)
        views = [lg[v * B:(v + 1) * B] for v in range(V)]
        losses = [crit(o, labels) for o in views]
        with torch.no_grad():
            probs = sum([F.softmax(o, dim=1) for o in views]) / len(views)
            accs.append(float(100.0 * probs.max(dim=1).indices.eq(labels).sum() / B))
        if backward:
            for lo in losses:
                lo.backward()
    return accs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--heads", type=int, default=20)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--stage-rounds", type=int, default=9)
    ap.add_argument("--stage-reps", type=int, default=20)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--tokens", type=int, default=2 * 2048)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--views", type=int, default=3)
    ap.add_argument("--classes", type=int, default=174)
    ap.add_argument("--depth", type=int, default=4)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_bench needs an MI355X (no CPU path)")
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    H, V, B, C = a.heads, a.views, a.batch, a.classes
    print(f"probe step: D {a.dim}, 16 heads, depth {a.depth}, {C} classes, B {B}, {a.tokens} tokens per view, "
          f"{V} views stacked, {H} classifier heads; device {torch.cuda.get_device_name(0)}")

    # ---- loss / accuracy stage alone
    g = torch.Generator(device=dev).manual_seed(1)
    logits = [3 * torch.randn(V * B, C, device=dev, generator=g) for _ in range(H)]
    labels = torch.randint(0, C, (B,), device=dev, generator=g)
    acc = dict(loss=torch.empty(H, V, device=dev), row=torch.empty(V * B, device=dev),
               dl=torch.empty(V * B, C, device=dev), pred=torch.empty(B, dtype=torch.int32, device=dev))
    variants = {"vj_xent (loss, dlogits, argmax, count; no read-back)": lambda: stage_fused(logits, labels, V, acc),
                "torch op sequence, forward + float() per head": lambda: stage_reference(logits, labels, V, False),
                "torch op sequence + backward to the logits": lambda: stage_reference(logits, labels, V, True)}
    for fn in variants.values():
        for _ in range(3):
            fn()
    times = {k: [] for k in variants}
    for _ in range(a.stage_rounds):
        for k, fn in variants.items():
            times[k].append(_sync_time(lambda: [fn() for _ in range(a.stage_reps)]) / a.stage_reps)
    # the fused stage's numbers against the torch sequence's, on the same logits
    ref_acc = stage_reference(logits, labels, V, False)
    got = stage_fused(logits, labels, V, acc).cpu()
    assert [float(100.0 * c / B) for c in got] == ref_acc, "top-1 of the two stages differ"
    print(f"loss / accuracy stage, {H} heads of [{V * B}, {C}] logits, ms per step "
          f"(median [min, max] of {a.stage_rounds} rounds x {a.stage_reps} repeats, variants alternating):")
    for k, t in times.items():
        print(f"  {k:58s} {statistics.median(t):8.3f}  [{min(t):.3f}, {max(t):.3f}]")
    base, fused = statistics.median(times[list(variants)[1]]), statistics.median(times[list(variants)[0]])
    print(f"  fused / torch forward-only sequence: {fused / base:.3f}x the time"
          + ("" if fused < base else "  (the fused stage is NOT faster)"))

    # ---- the whole probe train step on random tokens
    clfs = [AttentiveClassifier(embed_dim=a.dim, num_heads=16, depth=a.depth, num_classes=C).to(dev) for _ in range(H)]
    kw = [dict(ref_wd=0.01, final_wd=0.01, start_lr=1e-4, ref_lr=1e-3, final_lr=0.0, warmup=0.0) for _ in range(H)]
    opts, scalers, scheds, wds = init_opt(clfs, 1000, kw, 10, use_bfloat16=True)
    tr = ProbeTrainer(lambda clips, idx: clips, clfs, opts, scalers, scheds, wds, use_bfloat16=True)
    views = [torch.randn(B, a.tokens, a.dim, device=dev, generator=g) for _ in range(V)]
    for _ in range(a.warmup):
        tr.train_step(views, None, labels)
    steps = [_sync_time(lambda: tr.train_step(views, None, labels)) for _ in range(a.steps)]
    print(f"probe train step ({H} heads: forward, vj_xent, backward, inf check, AdamW; encoder excluded), ms per step "
          f"over {a.steps} steps after {a.warmup} warm-up: median {statistics.median(steps):.1f}  "
          f"[{min(steps):.1f}, {max(steps):.1f}]  = {statistics.median(steps) / H:.1f} ms per head")
    print(f"running top-1 per head, %, read back once at the end: {tr.train_meter.avg().round(2).tolist()}")
    print(f"peak device memory {torch.cuda.max_memory_allocated() / 2**30:.1f} GiB")


if __name__ == "__main__":
    main()
