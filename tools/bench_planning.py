"""Time one goal-image planning call (vjepa2_amd.planning.WorldModel.infer_next_action) at the DROID shape three
ways in one process, on the same HIP predictor:

  fused      vjepa2_amd.planning as shipped: vj_cem_sample / vj_plan_frame / vj_pose_step / vj_cem_update between
             the predictor forwards, nothing read back; rollout step h runs the predictor over all h + 1 frames;
  cached     the same with WorldModel.set_kv_cache(True): step h feeds frame h alone through
             predictor.forward_cached, the earlier frames' keys and values come from the per-block K/V cache
             (vj_kv_append + vj_attn_fwd_kv); R frame blocks per iteration instead of R (R + 1) / 2;
  reference  the same loop with the non-predictor stages written the way the reference's notebooks/utils
             (mpc_utils.py, world_model_wrapper.py) write them: torch ops for sampling, F.layer_norm, the four
             torch.cat per step, topk / index / mean / std, and compute_new_pose on the host (poses to the CPU,
             one rotation per sample in a Python loop with scipy if it is installed, else numpy, and back).

Shape: ViT-g/16 256^2 representations (embed 1408, 256 tokens per frame), AC predictor depth 24 / width 1024 /
16 heads, mpc_args S = 400, rollout 2, topk 10, 10 iterations. The encoder is not part of infer_next_action and
is not built: the context and goal representations are seeded layer-normed noise.

    python tools/bench_planning.py [--rounds 3] [--out profiles/planning_cem_droid.txt]
    python tools/bench_planning.py --variants fused cached --rollout 2 --kernels \\
        --out profiles/planning_kv_cache_droid.txt
    python tools/bench_planning.py --variants fused cached --rollout 4 --samples 200 --kernels \\
        --out profiles/planning_kv_cache_droid.txt --append

(Without the cache, S 400 at rollout 3 or 4 does not run: the fc2 GEMM's A operand of 400 * 4 * 258 rows of 4096
bf16 passes the 2 GB a GEMM operand may span. With it every GEMM sees 400 * 258 rows whatever the rollout.)

Method: every variant is warmed up with a whole call; they alternate round by round; a call is timed with HIP
events around it (and ends in a synchronise); the stages are the intervals between events recorded on the same
stream before and after every stage, so host-induced idle time (the reference's .cpu() round trip) falls into the
stage that causes it. Median, minimum and maximum over rounds. --kernels adds one more call per HIP variant, not
part of the medians, under ops.KernelEvents (HIP events around every launch of the library) and lists the kernels' totals.
Needs the GPU (no fallback).
"""

import argparse
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from vjepa2_amd import ops, planning  # noqa: E402
from vjepa2_amd.ac_predictor import vit_ac_predictor  # noqa: E402

STAGES = ["sample", "predictor", "frame", "pose", "update", "glue"]


class Stages:
    """Event marks on the current stream; the interval that ends at mark(name) belongs to stage `name`."""

    def __init__(self):
        self.marks = []

    def mark(self, name):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        self.marks.append((name, e))

    def totals(self):
        torch.cuda.synchronize()
        out = {s: 0.0 for s in STAGES}
        for (_, a), (name, b) in zip(self.marks, self.marks[1:]):
            out[name] += a.elapsed_time(b)
        return out, self.marks[0][1].elapsed_time(self.marks[-1][1])


def staged(fn, st, name):
    def f(*a, **k):
        st.mark("glue")
        r = fn(*a, **k)
        st.mark(name)
        return r
    return f


def run_fused(wm, rep, pose, goal, kv_cache=False):
    st = Stages()
    real = {n: getattr(ops, n) for n in ("cem_sample", "plan_frame", "pose_step", "cem_update")}
    fwd, fwd_c = wm.predictor.forward, wm.predictor.forward_cached
    wm.set_kv_cache(kv_cache)
    try:
        for n, stage in (("cem_sample", "sample"), ("plan_frame", "frame"), ("pose_step", "pose"),
                         ("cem_update", "update")):
            setattr(ops, n, staged(real[n], st, stage))
        wm.predictor.forward = staged(fwd, st, "predictor")
        wm.predictor.forward_cached = staged(fwd_c, st, "predictor")
        st.mark("glue")
        out = wm.infer_next_action(rep, pose, goal)
        st.mark("glue")
    finally:
        for n, f in real.items():
            setattr(ops, n, f)
        del wm.predictor.forward, wm.predictor.forward_cached  # the instance attributes that shadowed the methods
        wm.kv_cache = False  # the flag alone: the cache stays allocated for the next cached round
    return out, st.totals()


def run_cached(wm, rep, pose, goal):
    return run_fused(wm, rep, pose, goal, kv_cache=True)


def _rot(t):
    (sa, sb, sc), (ca, cb, cc) = np.sin(t), np.cos(t)
    return np.array([[cc * cb, cc * sb * sa - sc * ca, cc * sb * ca + sc * sa],
                     [sc * cb, sc * sb * sa + cc * ca, sc * sb * ca - cc * sa], [-sb, cb * sa, cb * ca]])


def host_pose(pose, action):
    """compute_new_pose the reference's way: to the host, one rotation product per sample, back."""
    dev, dt = pose.device, pose.dtype
    p, a = pose[:, 0].cpu().numpy(), action[:, 0].cpu().numpy()
    try:
        from scipy.spatial.transform import Rotation

        ms = [Rotation.from_euler("xyz", t).as_matrix() for t in p[:, 3:6]]
        ds = [Rotation.from_euler("xyz", t).as_matrix() for t in a[:, 3:6]]
        ang = [Rotation.from_matrix(d @ m).as_euler("xyz") for d, m in zip(ds, ms)]
    except ImportError:
        ms = [_rot(t.astype(np.float64)) for t in p[:, 3:6]]
        ds = [_rot(t.astype(np.float64)) for t in a[:, 3:6]]
        ang = [planning._matrix_euler_xyz(d @ m) for d, m in zip(ds, ms)]
    new = np.concatenate([p[:, :3] + a[:, :3], np.stack(ang), np.clip(p[:, -1:] + a[:, -1:], 0, 1)], axis=-1)
    return torch.from_numpy(new).to(dev).to(dt)[:, None]


def run_reference(wm, rep, pose, goal):
    """mpc_utils.cem / step_predictor's op sequence (torch ops + host pose step) around the HIP predictor."""
    st = Stages()
    a = wm.mpc_args
    S, rollout, k, maxnorm = a["samples"], a["rollout"], a["topk"], a["maxnorm"]
    mm, ms = a["momentum_mean"], a["momentum_std"]
    mg, sg = 0.15, 0.15
    dev = rep.device
    st.mark("glue")
    ctx, goal_s, pose_s = rep.repeat(S, 1, 1, 1), goal.repeat(S, 1, 1, 1), pose.repeat(S, 1, 1)
    mean = torch.cat([torch.zeros(rollout, 3, device=dev), torch.zeros(rollout, 1, device=dev)], dim=-1)
    std = torch.cat([torch.ones(rollout, 3, device=dev) * maxnorm, torch.ones(rollout, 1, device=dev)], dim=-1)
    for _ in range(a["cem_steps"]):
        acts, frames, poses = None, ctx, pose_s
        for h in range(rollout):
            st.mark("glue")
            x = torch.randn(S, 4, device=dev) * std[h] + mean[h]
            x[:, :3] = torch.clip(x[:, :3], min=-maxnorm, max=maxnorm)
            x[:, -1:] = torch.clip(x[:, -1:], min=-0.75, max=0.75)
            x = torch.cat([x[:, :3], torch.zeros(S, 3, device=dev), x[:, -1:]], dim=-1)[:, None]
            acts = torch.cat([acts, x], dim=1) if acts is not None else x
            st.mark("sample")
            with torch.no_grad():
                nxt = wm.predictor(frames.flatten(1, 2), acts, poses)[:, -wm.tokens_per_frame:]
            st.mark("predictor")
            nxt = F.layer_norm(nxt, (nxt.size(-1),)).view(S, 1, -1, nxt.size(-1))
            frames = torch.cat([frames, nxt], dim=1)
            st.mark("frame")
            poses = torch.cat([poses, host_pose(poses[:, -1:], acts[:, -1:])], dim=1)
            st.mark("pose")
        sims = planning.l1(frames[:, -1].flatten(1), goal_s[:, -1].flatten(1))
        st.mark("frame")
        sel = acts[sims.topk(k, largest=False).indices]
        m, s = sel.mean(dim=0), sel.std(dim=0)
        mean = torch.cat([m[..., :3] * (1.0 - mm) + mean[..., :3] * mm, m[..., -1:] * (1.0 - mg) + mean[..., -1:] * mg], -1)
        std = torch.cat([s[..., :3] * (1.0 - ms) + std[..., :3] * ms, s[..., -1:] * (1.0 - sg) + std[..., -1:] * sg], -1)
        st.mark("update")
    out = torch.cat([mean[..., :3], torch.zeros(rollout, 3, device=dev),
                     planning.round_small_elements(mean[..., -1:], 0.25)], dim=-1)
    st.mark("glue")
    return out, st.totals()


def bench(a, wm, rollout, rep, pose, goal, lines):
    wm.mpc_args = dict(wm.mpc_args, rollout=rollout)
    table = {"fused": run_fused, "cached": run_cached, "reference": run_reference}
    variants = {k: table[k] for k in a.variants}
    for f in variants.values():  # warm-up: every shape of the timed window
        f(wm, rep, pose, goal)
    res = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, f in variants.items():
            res[k].append(f(wm, rep, pose, goal)[1])
    lines += [f"goal-image planning, one infer_next_action: S {a.samples}, rollout {rollout}, topk 10, {a.cem_steps} CEM "
              f"iterations; AC predictor depth {a.depth} width 1024, 16 heads, embed 1408, 256 tokens per frame; "
              f"device {torch.cuda.get_device_name(0)}",
              f"ms per call, HIP events (median [min, max] of {a.rounds} rounds, variants alternating, all warmed up)"]
    med = {}
    for k, rs in res.items():
        tot = [t for _, t in rs]
        med[k] = statistics.median(tot)
        lines.append(f"  {k:10s} total {med[k]:10.2f}  [{min(tot):.2f}, {max(tot):.2f}]")
        for s in STAGES:
            v = [st[s] for st, _ in rs]
            lines.append(f"    {s:10s} {statistics.median(v):10.2f}  [{min(v):.2f}, {max(v):.2f}]  "
                         f"{100 * statistics.median(v) / med[k]:5.1f} % of the call")
    if "fused" in med and "reference" in med:
        lines.append(f"  fused / reference: {med['fused'] / med['reference']:.4f}x the time; the predictor forwards are "
                     f"{100 * statistics.median([st['predictor'] for st, _ in res['fused']]) / med['fused']:.1f} % of "
                     f"the fused call")
    if "fused" in med and "cached" in med:
        pf, pc = (statistics.median([st["predictor"] for st, _ in res[k]]) for k in ("fused", "cached"))
        lines.append(f"  cached / fused: {med['cached'] / med['fused']:.4f}x the time of the call, {pc / pf:.4f}x the time "
                     f"of the predictor forwards; frame blocks through the GEMMs per iteration {rollout} against "
                     f"{rollout * (rollout + 1) // 2}: row-count prediction {2 / (rollout + 1):.4f}x")
        cache = wm._rollout_cache(a.samples, rollout)
        lines.append(f"  K/V cache: {len(cache.kv)} x bf16 {list(cache.kv[0].shape)} = {cache.nbytes() / 2**30:.2f} GiB")
    if a.kernels:
        for k, f in variants.items():
            if k == "reference":
                continue
            ev = ops.KernelEvents()
            ev.start()
            try:
                f(wm, rep, pose, goal)
            finally:
                ev.stop()
            summ = sorted(ev.summary().items(), key=lambda kv: -kv[1]["total_ms"])
            lines.append(f"  {k}: kernels of one call, HIP events around every launch (ms, launches)")
            for name, d in summ[:12]:
                lines.append(f"    {name:34s} {d['total_ms']:10.2f}  {d['count']:6d}")
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--samples", type=int, default=400)
    ap.add_argument("--cem-steps", type=int, default=10)
    ap.add_argument("--depth", type=int, default=24)
    ap.add_argument("--rollout", type=int, nargs="+", default=[2], help="rollout horizons, one table each (at most 4)")
    ap.add_argument("--variants", nargs="+", default=["fused", "reference"], choices=["fused", "cached", "reference"])
    ap.add_argument("--kernels", action="store_true", help="per-kernel totals of one extra call per HIP variant")
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true", help="append to --out (tables of several invocations in one file)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_planning needs an MI355X (no CPU path)")
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    pred = vit_ac_predictor(img_size=256, patch_size=16, num_frames=8, tubelet_size=2, embed_dim=1408,
                            predictor_embed_dim=1024, depth=a.depth, num_heads=16, action_embed_dim=7).to(dev).eval()
    mpc = dict(rollout=2, samples=a.samples, topk=10, cem_steps=a.cem_steps, momentum_mean=0.15, momentum_std=0.15,
               maxnorm=0.05, verbose=False)
    wm = planning.WorldModel(encoder=None, predictor=pred, tokens_per_frame=256, transform=None, mpc_args=mpc,
                             device=dev)
    g = torch.Generator(device=dev).manual_seed(1)
    rep = F.layer_norm(torch.randn(1, 1, 256, 1408, device=dev, generator=g), (1408,))
    goal = F.layer_norm(torch.randn(1, 1, 256, 1408, device=dev, generator=g), (1408,))
    pose = torch.tensor([[[0.3, -0.1, 0.4, 0.5, -0.4, 0.3, 0.4]]], device=dev)
    lines = []
    for rollout in a.rollout:
        bench(a, wm, rollout, rep, pose, goal, lines)
    text = "\n".join(lines).rstrip("\n")
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a" if a.append else "w") as f:
            f.write(text + "\n" + ("\n" if a.append else ""))


if __name__ == "__main__":
    main()
