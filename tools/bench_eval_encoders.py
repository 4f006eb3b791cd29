"""Time the multilevel eval encoder wrapper's forward at the reference's Diving48 ViT-L shape two ways in one
process: ClipAggregationMultilevel.forward_stacked (every tapped layer's LayerNorm written once, by
vj_layernorm_taps, into the buffer the classifiers read) and the unfused sequence on the same encoder
(forward()'s list of LayerNorm outputs, cat over levels, per-view reshape / cat, cat over views: what the
pieces before forward_taps would do).

Shape (configs/eval/vitl/diving48.yaml): vit_large RoPE, B = 2, 4 segments x 3 views, 32 x 256^2 frames,
out_layers [17, 19, 21, 23], random weights.

    python tools/bench_eval_encoders.py [--rounds 7] [--warmup 2] [--out profiles/eval_multilevel_bench.txt]

Method: HIP events around each forward on the current stream; both variants are warmed up first, then
alternate round by round; the median, minimum and maximum over rounds are reported, and for each variant
torch.cuda.max_memory_allocated of one forward (peak statistics reset before it, the other variant's
result freed). The two results are asserted bit-identical before anything is timed. Reads nothing outside
the tree. Needs the GPU (no fallback).
"""

import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from vjepa2_amd import vision_transformer as vit  # noqa: E402
from vjepa2_amd.multiclip import ClipAggregationMultilevel  # noqa: E402


def unfused(agg, x):
    """vit_encoder_multiclip_multilevel.py:112-141 around forward()'s list, then ProbeTrainer's cat over views."""
    clips, V = len(x), len(x[0])
    B, _, Fr, _, _ = x[0][0].size()
    outputs = torch.cat(agg.model(torch.cat([torch.cat(xi, dim=0) for xi in x], dim=0)), dim=1)
    _, N, D = outputs.size()
    T = Fr // agg.tubelet_size
    S = N // T
    eff_B = B * V
    views = []
    for j in range(V):
        o = [outputs[i * eff_B:(i + 1) * eff_B][j * B:(j + 1) * B].reshape(B, T, S, D) for i in range(clips)]
        views.append(torch.cat(o, dim=1).flatten(1, 2))
    return torch.cat(views, dim=0)


def fused(agg, x):
    return agg.forward_stacked(x, None)[0]


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    y = fn()
    e.record()
    e.synchronize()
    del y
    return s.elapsed_time(e)


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    y = fn()
    torch.cuda.synchronize()
    p = torch.cuda.max_memory_allocated()
    del y
    return base, p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--segments", type=int, default=4)
    ap.add_argument("--views", type=int, default=3)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                   "profiles", "eval_multilevel_bench.txt"))
    a = ap.parse_args()
    if a.rounds < 5:
        raise SystemExit("at least 5 rounds")
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval_encoders needs an MI355X (no CPU path)")
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    layers = [17, 19, 21, 23]
    enc = vit.vit_large_rope(img_size=a.size, num_frames=a.frames, tubelet_size=2, out_layers=layers)
    agg = ClipAggregationMultilevel(enc, tubelet_size=2, out_layers=layers).to(dev).eval()
    for p in agg.parameters():
        p.requires_grad = False
    g = torch.Generator(device=dev).manual_seed(1)
    x = [[torch.randn(a.batch, 3, a.frames, a.size, a.size, device=dev, generator=g) for _ in range(a.views)]
         for _ in range(a.segments)]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    with torch.no_grad():
        y0, y1 = fused(agg, x), unfused(agg, x)
        assert y0.shape == y1.shape and torch.equal(y0, y1), "the fused and the unfused wrapper outputs differ"
        assert torch.isfinite(y0).all()
        shape, gb = tuple(y0.shape), y0.numel() * 4 / 1e9
        del y0, y1
        say(f"multilevel wrapper forward: vit_large RoPE, B {a.batch}, {a.segments} segments x {a.views} views, "
            f"{a.frames} x {a.size}^2, taps {layers}; output {shape} f32 = {gb:.2f} GB; "
            f"device {torch.cuda.get_device_name(0)}")
        say("the two variants' outputs are bit-identical (asserted before timing)")
        variants = {"forward_stacked (vj_layernorm_taps into one buffer)": lambda: fused(agg, x),
                    "unfused (forward() list, cat, per-view reshape, cat)": lambda: unfused(agg, x)}
        for fn in variants.values():
            for _ in range(a.warmup):
                timed(fn)
        times = {k: [] for k in variants}
        for _ in range(a.rounds):
            for k, fn in variants.items():
                times[k].append(timed(fn))
        say(f"ms per forward, HIP events (median [min, max] of {a.rounds} rounds after {a.warmup} warm-up, "
            "variants alternating):")
        for k, t in times.items():
            say(f"  {k:55s} {statistics.median(t):9.2f}  [{min(t):.2f}, {max(t):.2f}]")
        (kf, tf), (ku, tu) = times.items()
        mf, mu = statistics.median(tf), statistics.median(tu)
        spread = max(max(tf) - min(tf), max(tu) - min(tu))
        say(f"  fused / unfused: {mf / mu:.4f}x the time; difference {mu - mf:.2f} ms, largest spread of a variant "
            f"{spread:.2f} ms" + ("" if mu - mf > spread else "  (NOT faster beyond the spread)"))
        say("torch.cuda.max_memory_allocated of one forward (model and input resident before it):")
        peaks = {}
        for k, fn in variants.items():
            base, p = peak(fn)
            peaks[k] = p
            say(f"  {k:55s} peak {p / 2**30:7.2f} GiB  (resident before {base / 2**30:.2f} GiB, "
                f"forward adds {(p - base) / 2**30:.2f} GiB)")
        d = (peaks[ku] - peaks[kf]) / 2**30
        say(f"  peak, fused / unfused: {peaks[kf] / peaks[ku]:.3f}; the fused forward's peak is "
            + (f"{d:.2f} GiB lower" if d > 0 else f"{-d:.2f} GiB HIGHER (no saving by this figure: its output buffer is "
               "live during the encoder pass, the unfused copies are made after the blocks' transients are freed)"))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
