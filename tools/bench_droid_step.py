"""Time one V-JEPA 2-AC post-training step (vjepa2_amd.droid.ACTrainer.train_step) at the DROID config's shape:
ViT-g/16 encoder (frozen), B 8, 8 frames, 256 x 256, predictor 24 x 1024, auto_steps 2, loss_exp 1, bf16.

Two arms on the same trainer and the same HIP predictor, alternating in one process:
  fused   the loss side on the vj_acloss.hip kernels (functions.ACLossFn), as shipped
  torch   the loss side as the reference's separate torch ops (F.layer_norm, the slice of h, mean(|z - h| ** p) / p,
          their autograd)
Both arms are warmed up, then timed with HIP events for --rounds rounds, one step per arm per round; the median
is reported with the spread (min .. max) and the peak allocated memory of a timed step.

    python tools/bench_droid_step.py [--out profiles/droid_step.txt] [--rounds 3] [--warmup 2]
"""

import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "droid_step.txt"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--model", default="vit_giant_xformers")
    a = ap.parse_args()

    from vjepa2_amd import droid

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    crop, patch, tub = 256, 16, 2
    enc, pred = droid.init_video_model(device=dev, patch_size=patch, max_num_frames=tub * a.frames, tubelet_size=tub,
                                       model_name=a.model, crop_size=crop, pred_depth=24, pred_num_heads=16,
                                       pred_embed_dim=1024, uniform_power=True, use_sdpa=True, use_rope=True,
                                       wide_silu=True, use_activation_checkpointing=True)
    opt, _, sched, wds = droid.init_opt(encoder=enc, predictor=pred, iterations_per_epoch=300, start_lr=7.5e-5,
                                        ref_lr=4.25e-4, warmup=15, anneal=15, num_epochs=315, wd=0.04, final_wd=0.04,
                                        final_lr=0.0, mixed_precision=True)
    tr = droid.ACTrainer(pred, enc, opt, (crop // patch) ** 2, auto_steps=2, loss_exp=1.0, normalize_reps=True,
                         mixed_precision=True)
    ds = droid.SyntheticDroidDataset(a.batch, a.frames, crop)
    items = [ds[i] for i in range(a.batch)]
    clips, actions, states, extr = (torch.stack([it[j] for it in items]).to(dev) for j in range(4))
    print("models and inputs on the device", flush=True)

    def step(side):
        tr.loss_side = side
        sched.step(), wds.step()
        return tr.train_step(clips, actions, states, extr)

    arms = (("fused", "hip"), ("torch", "torch"))
    for _ in range(a.warmup):
        for n, side in arms:
            print(f"warm-up {n}: (loss, jloss, sloss) {step(side).tolist()}", flush=True)
    torch.cuda.synchronize()
    ms = {n: [] for n, _ in arms}
    peak = {n: 0 for n, _ in arms}
    last = {}
    for _ in range(a.rounds):
        for n, side in arms:
            torch.cuda.reset_peak_memory_stats()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            out = step(side)
            e.record()
            torch.cuda.synchronize()
            ms[n].append(s.elapsed_time(e))
            peak[n] = max(peak[n], torch.cuda.max_memory_allocated())
            last[n] = out.tolist()
            print(f"{n}: {ms[n][-1]:.2f} ms", flush=True)
    lines = [f"V-JEPA 2-AC post-training step: {a.model}, B {a.batch}, {a.frames} frames, {crop}^2, predictor 24 x 1024, "
             f"auto_steps 2, loss_exp 1.0, bf16; {torch.cuda.get_device_name(0)}",
             f"HIP events, {a.warmup} warm-up steps per arm, arms alternating in one process, median of {a.rounds} rounds"]
    for n, _ in arms:
        v = ms[n]
        lines.append(f"{n:6s} loss side: {statistics.median(v):9.2f} ms/step  (min {min(v):.2f} .. max {max(v):.2f}; "
                     f"all {', '.join(f'{x:.2f}' for x in v)})  peak memory {peak[n] / 2**30:.2f} GiB  "
                     f"last (loss, jloss, sloss) {', '.join(f'{x:.4f}' for x in last[n])}")
    f, t = statistics.median(ms["fused"]), statistics.median(ms["torch"])
    lines.append(f"fused / torch = {f / t:.4f}  ({t - f:+.2f} ms per step, {a.batch * 1000.0 / f:.2f} clips/s fused)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
