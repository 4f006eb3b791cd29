"""Generate tests/golden/planning.pt by running the REFERENCE's planner (notebooks/utils/mpc_utils.py and
notebooks/utils/world_model_wrapper.py) on CPU.

Like make_golden_anticipation.py this runs in the build container only, executes the reference read-only mounted
at /root/reference (``notebooks.utils`` resolves as a namespace package; scipy and tqdm are installed here) and
copies none of its text: the fixture holds inputs, recorded results and settings. Stub: ``timm.models.layers.
drop_path`` (inert). Weights are not stored: they are a function of a seed, and per-tensor (sum, sum of squares)
let a loader tell that it rebuilt the same ones.

(a) pose: 64 (pose, action) rows through ``compute_new_pose`` (f32 in, f32 out) and 64 (start, end) rows through
    ``poses_to_diff`` (f64): zero and small deltas, deltas on all three angles, pitch beyond +-pi/2 (the result is
    canonicalised, roll and yaw shifted by pi), roll near +-pi, gripper sums below 0 and above 1. Every recorded
    angle keeps roll and yaw >= 1e-3 from +-pi and pitch >= 0.05 from +-pi/2 (asserted), so that a last-bit
    difference cannot flip a sign or enter gimbal lock.
(b) cem: ``WorldModel.infer_next_action`` on the micro AC predictor of ac_predictor.pt's config (4 tokens per
    frame, 3 frames: rollout <= 2), S = 16, topk = 4, four runs (rollout 1; rollout 2; rollout 2 with
    axis={1: 0.01}; rollout 2 with close_gripper=1). Recorded per iteration: the noise of every torch.randn draw
    with ``mean`` / ``std`` at the time of the draw (a stand-in for torch.randn reads them from the calling
    frame), the action trajectories (a wrapper around the world model), the energies (a wrapper around the
    objective) and the elite set; and the returned action. Everything runs twice, in fp32 and with the predictor
    under ``torch.autocast("cpu", bfloat16)``; G = |bf16 - fp32| (mean, max) of the energies and of the final
    action. A seed is kept per run for which, in every iteration, both precisions choose the same elite set and
    the fp32 gap between the k-th and (k+1)-th smallest energy exceeds 4 G_energy(max).
(c) surface: parameter names and defaults of the reference's ``cem`` and ``WorldModel.__init__``.
(d) encode: ``WorldModel.encode`` of a micro RoPE encoder on two 32 x 32 frames.

Usage:  python tests/golden/make_golden_planning.py     (writes tests/golden/planning.pt)
"""

import functools
import inspect
import logging
import math
import os
import sys
import types

sys.dont_write_bytecode = True  # never write __pycache__ into the reference tree
REF = os.environ.get("VJEPA_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

timm = types.ModuleType("timm")
timm_models = types.ModuleType("timm.models")
timm_layers = types.ModuleType("timm.models.layers")
timm_layers.drop_path = lambda x, drop_prob=0.0, training=False, scale_by_keep=True: x
timm.models = timm_models
timm_models.layers = timm_layers
sys.modules.update({"timm": timm, "timm.models": timm_models, "timm.models.layers": timm_layers})
sys.path.insert(0, REF)

import notebooks.utils.mpc_utils as ref_mpc  # noqa: E402
import notebooks.utils.world_model_wrapper as ref_wm  # noqa: E402
import src.models.ac_predictor as ref_ac  # noqa: E402
import src.models.vision_transformer as ref_vit  # noqa: E402

torch.set_num_threads(8)
logging.disable(logging.INFO)  # the reference logs mean / std after every CEM iteration

PCFG = dict(img_size=32, patch_size=16, num_frames=6, tubelet_size=2, embed_dim=96, predictor_embed_dim=64, depth=2,
            num_heads=2, action_embed_dim=7, use_extrinsics=False, is_frame_causal=True)
ECFG = dict(img_size=32, patch_size=16, num_frames=2, tubelet_size=2, embed_dim=96, depth=2, num_heads=3,
            mlp_ratio=2.0, qkv_bias=True, use_rope=True, uniform_power=True)
WSEED = 71
# The seeded predictor barely reacts to a 0.05-sized action: its action embedding is scaled up (and the sampling
# kept wide: a large maxnorm, slow std momenta) so that the samples' energies spread far beyond the bf16 gap.
PERTURB = float(os.environ.get("PLAN_PERTURB", 0.15))
ACTION_GAIN = float(os.environ.get("PLAN_ACTION_GAIN", 30.0))
MPC = dict(samples=16, topk=4, momentum_mean=0.15, momentum_std=float(os.environ.get("PLAN_MSTD", 0.8)),
           momentum_mean_gripper=0.1, momentum_std_gripper=0.7, maxnorm=float(os.environ.get("PLAN_MAXNORM", 0.5)),
           verbose=False)
GOAL_ACTION = [0.2, -0.15, 0.25, 0.0, 0.0, 0.0, 0.5]
RUNS = [dict(name="rollout1", rollout=1, cem_steps=4, axis={}, close_gripper=None),
        dict(name="rollout2", rollout=2, cem_steps=3, axis={}, close_gripper=None),
        dict(name="axis", rollout=2, cem_steps=3, axis={1: 0.01}, close_gripper=None),
        dict(name="close", rollout=2, cem_steps=3, axis={}, close_gripper=1)]
MAX_SEEDS = 2000


def _sums(sd):
    return {k: (v.double().sum().item(), v.double().pow(2).sum().item()) for k, v in sd.items()}


def _perturb(m, scale=0.05):
    with torch.no_grad():
        for p in m.parameters():
            p.add_(scale * torch.randn_like(p))


# ------------------------------------------------------------------------------------------------ (a)
def _pose_rows():
    g = torch.Generator().manual_seed(11)
    rows = []  # (pose, action)

    def add(pose, action):
        rows.append((list(pose), list(action)))

    base = [0.3, -0.2, 0.5, 0.4, -0.3, 0.2, 0.5]
    add(base, [0.0] * 7)                                        # zero delta
    add([0.0] * 7, [0.0] * 7)
    for i in range(10):                                         # small xyz / gripper deltas, no rotation
        d = (0.05 * (2 * torch.rand(7, generator=g) - 1)).tolist()
        d[3:6] = [0.0, 0.0, 0.0]
        p = (torch.rand(7, generator=g) - 0.5).tolist()
        p[6] = 0.5
        add(p, d)
    for i in range(20):                                         # deltas on all three angles
        p = (2.0 * (torch.rand(7, generator=g) - 0.5)).tolist()
        p[4] = 1.2 * (p[4] / 1.0)
        p[6] = float(torch.rand(1, generator=g))
        d = (0.4 * (2 * torch.rand(7, generator=g) - 1)).tolist()
        add(p, d)
    add([0, 0, 0, 0.1, 2.0, 0.3, 0.2], [0.0] * 7)               # pitch beyond pi/2: canonicalised
    add([0, 0, 0, 0.1, -2.0, 0.3, 0.2], [0.0] * 7)
    add([0, 0, 0, -0.4, 2.4, 1.0, 0.2], [0, 0, 0, 0.1, 0.1, -0.2, 0])
    add([0, 0, 0, 0.7, -2.7, -1.3, 0.2], [0, 0, 0, -0.2, 0.05, 0.3, 0])
    add([0, 0, 0, 0.2, 1.2, 0.1, 0.2], [0, 0, 0, 0.0, 0.9, 0.0, 0])   # the sum passes pi/2
    add([0, 0, 0, 0.2, -1.1, 0.1, 0.2], [0, 0, 0, 0.1, -1.0, 0.0, 0])
    for r in (3.1, -3.1, 3.0, -3.05):                           # roll near +-pi
        add([0.1, 0.2, 0.3, r, 0.2, -0.4, 0.5], [0, 0, 0, 0.01, 0.0, 0.0, 0])
        add([0.1, 0.2, 0.3, r, -0.3, 0.6, 0.5], [0, 0, 0, 0.02 if r < 0 else -0.02, 0.1, 0.05, 0])
    for pg, ag in ((0.1, -0.4), (0.0, -0.75), (0.9, 0.3), (1.0, 0.75), (0.5, 1.0), (0.3, -0.3), (0.6, 0.4),
                   (0.25, -0.25)):                              # gripper sums below 0, above 1 and at the edges
        add([0.0, 0.1, 0.2, 0.3, 0.1, -0.2, pg], [0.01, -0.02, 0.03, 0.0, 0.0, 0.0, ag])
    while len(rows) < 64:                                       # larger rotations everywhere
        p = (6.0 * (torch.rand(7, generator=g) - 0.5)).tolist()
        p[4] = p[4] / 2.2
        p[6] = float(torch.rand(1, generator=g))
        d = (1.5 * (2 * torch.rand(7, generator=g) - 1)).tolist()
        d[6] = d[6] / 2
        add(p, d)
    return rows


def _angles_safe(a):
    a = np.asarray(a, dtype=np.float64)
    return (np.all(np.pi - np.abs(a[..., 0]) >= 1e-3) and np.all(np.pi - np.abs(a[..., 2]) >= 1e-3)
            and np.all(np.pi / 2 - np.abs(a[..., 1]) >= 0.05))


def gen_pose():
    rows = _pose_rows()
    pose = torch.tensor([r[0] for r in rows], dtype=torch.float32)
    action = torch.tensor([r[1] for r in rows], dtype=torch.float32)
    keep = []
    for i in range(len(rows)):
        new = ref_mpc.compute_new_pose(pose[i:i + 1, None], action[i:i + 1, None])
        s, e = pose[i].double(), (pose[i].double() + action[i].double())
        diff = ref_mpc.poses_to_diff(s, e)
        if _angles_safe(new[0, 0, 3:6].numpy()) and _angles_safe(diff[3:6].numpy()):
            keep.append(i)
    print(f"pose: {len(keep)} of {len(rows)} rows keep the margins")
    pose, action = pose[keep], action[keep]
    new_pose = ref_mpc.compute_new_pose(pose[:, None], action[:, None])
    assert new_pose.dtype == torch.float32 and tuple(new_pose.shape) == (len(keep), 1, 7)
    start, end = pose.double(), pose.double() + action.double()
    diff = torch.stack([ref_mpc.poses_to_diff(start[i], end[i]) for i in range(len(keep))])
    assert diff.dtype == torch.float64
    assert _angles_safe(new_pose[:, 0, 3:6].numpy()) and _angles_safe(diff[:, 3:6].numpy())
    assert len(keep) >= 56
    canon = int((np.abs(pose[:, 4].numpy()) > np.pi / 2).sum())
    grip_lo = int(((pose[:, 6] + action[:, 6]) < 0).sum())
    grip_hi = int(((pose[:, 6] + action[:, 6]) > 1).sum())
    print(f"pose: {canon} rows with |pitch| > pi/2 in, gripper sums < 0: {grip_lo}, > 1: {grip_hi}")
    assert canon >= 3 and grip_lo >= 1 and grip_hi >= 1
    print("pose: [0.1, 2.0, 0.3] ->", ref_mpc.compute_new_pose(torch.tensor([[[0, 0, 0, 0.1, 2.0, 0.3, 0.2]]]),
                                                             torch.zeros(1, 1, 7))[0, 0, 3:6].tolist())
    return dict(pose=pose, action=action, new_pose=new_pose[:, 0].contiguous(), start=start, end=end, diff=diff)


# ------------------------------------------------------------------------------------------------ (b)
class _Autocast(torch.nn.Module):
    def __init__(self, m):
        super().__init__()
        self.m = m

    def forward(self, *a):
        with torch.autocast("cpu", dtype=torch.bfloat16):
            return self.m(*a).float()


def _predictor():
    torch.manual_seed(WSEED)
    m = ref_ac.vit_ac_predictor(**PCFG)
    _perturb(m, PERTURB)
    with torch.no_grad():
        m.action_encoder.weight.mul_(ACTION_GAIN)
    return m.eval()


def _goal(pred, rep, pose):
    """A reachable goal: the fp32 prediction one GOAL_ACTION away from the context (a goal image is a state the
    arm can get to; against an unrelated goal every sample's energy is the same to within the bf16 gap)."""
    with torch.no_grad():
        y = pred(rep.flatten(1, 2), torch.tensor([[GOAL_ACTION]], dtype=torch.float32), pose)[:, -4:]
        return F.layer_norm(y, (y.size(-1),)).view(1, 1, 4, -1).contiguous()


def _run(pred, run, seed, rep, pose, goal, bf16):
    """One reference infer_next_action with every draw, action trajectory and energy recorded."""
    rec = dict(noise=[], mean=[], std=[], actions=[], energy=[], elites=[])
    real_randn, real_cem = torch.randn, ref_wm.cem
    calls = dict(n=0)

    def randn(*a, **k):
        out = real_randn(*a, **k)
        loc = sys._getframe(1).f_locals
        if calls["n"] % run["rollout"] == 0:
            rec["noise"].append([])
            rec["mean"].append(loc["mean"].detach().clone())
            rec["std"].append(loc["std"].detach().clone())
        rec["noise"][-1].append(out.detach().clone())
        calls["n"] += 1
        return out

    def cem(world_model, objective=ref_mpc.l1, **k):
        def wm(frames, actions, poses):
            if actions.shape[1] == run["rollout"]:
                rec["actions"].append(actions.detach().clone())
            return world_model(frames, actions, poses)

        def obj(a, b):
            sims = objective(a, b)
            rec["energy"].append(sims.detach().clone())
            rec["elites"].append(sorted(sims.topk(MPC["topk"], largest=False).indices.tolist()))
            return sims

        return real_cem(world_model=wm, objective=obj, **k)

    args = dict(MPC, rollout=run["rollout"], cem_steps=run["cem_steps"], axis=run["axis"])
    wm = ref_wm.WorldModel(encoder=None, predictor=_Autocast(pred) if bf16 else pred, tokens_per_frame=4,
                           transform=None, mpc_args=args, normalize_reps=True, device="cpu")
    torch.manual_seed(seed)
    torch.randn = randn
    ref_wm.cem = cem
    try:
        with torch.no_grad():
            out = wm.infer_next_action(rep, pose, goal, close_gripper=run["close_gripper"])
    finally:
        torch.randn = real_randn
        ref_wm.cem = real_cem
    n = run["cem_steps"]
    assert len(rec["noise"]) == n and len(rec["actions"]) == n and len(rec["energy"]) == n
    return dict(noise=torch.stack([torch.stack(x) for x in rec["noise"]]),  # [iters, rollout, S, 4]
                mean=torch.stack(rec["mean"]), std=torch.stack(rec["std"]),  # at the time of each iteration's draws
                actions=torch.stack(rec["actions"]), energy=torch.stack(rec["energy"]),
                elites=torch.tensor(rec["elites"], dtype=torch.int32), action=out.detach().clone())


def gen_cem():
    pred = _predictor()
    g = torch.Generator().manual_seed(WSEED + 1)
    rep = F.layer_norm(torch.randn(1, 1, 4, PCFG["embed_dim"], generator=g), (PCFG["embed_dim"],))
    pose = torch.tensor([[[0.3, -0.1, 0.4, 0.5, -0.4, 0.3, 0.4]]], dtype=torch.float32)
    goal = _goal(pred, rep, pose)
    out = dict(pred_cfg=dict(PCFG), weight_seed=WSEED, action_gain=ACTION_GAIN, pred_sums=_sums(pred.state_dict()), mpc=dict(MPC), rep=rep,
               goal=goal, goal_action=list(GOAL_ACTION), perturb=PERTURB, pose=pose, runs={})
    k = MPC["topk"]
    for run in RUNS:
        for tried, seed in enumerate(range(100, 100 + MAX_SEEDS), 1):
            f32 = _run(pred, run, seed, rep, pose, goal, bf16=False)
            b16 = _run(pred, run, seed, rep, pose, goal, bf16=True)
            same = bool(torch.equal(f32["elites"], b16["elites"]))
            de = (b16["energy"] - f32["energy"]).abs()
            srt = f32["energy"].sort(dim=1).values
            margin = (srt[:, k] - srt[:, k - 1]).min().item()
            if same and margin > 4 * de.max().item():
                break
        else:
            raise SystemExit(f"{run['name']}: no seed found")
        assert torch.equal(f32["noise"], b16["noise"])
        da = (b16["action"] - f32["action"]).abs()
        gaps = dict(energy=dict(mean=de.mean().item(), max=de.max().item()),
                    action=dict(mean=da.mean().item(), max=da.max().item()))
        print(f"cem {run['name']}: seed {seed} after {tried} tried; elite margin {margin:.3e}, G {gaps}; "
              f"energies {f32['energy'].min():.4f}..{f32['energy'].max():.4f}; action {f32['action'].tolist()}")
        # the reference's mean over the elites against a plain f32 sum in top-k order / in index order
        out["runs"][run["name"]] = dict(rollout=run["rollout"], cem_steps=run["cem_steps"],
                                        axis=[[a, v] for a, v in run["axis"].items()],
                                        close_gripper=run["close_gripper"], seed=seed, tried=tried, margin=margin,
                                        gaps=gaps, f32=f32,
                                        bf16=dict(energy=b16["energy"], action=b16["action"], elites=b16["elites"]))
    return out


# ------------------------------------------------------------------------------------------------ (c)
def _signature(f):
    out = []
    for n, p in inspect.signature(f).parameters.items():
        d = p.default
        if d is inspect.Parameter.empty:
            out.append([n, False, None])
        elif callable(d):
            out.append([n, True, "callable:" + d.__name__])
        elif isinstance(d, dict):
            out.append([n, True, [[k, v] for k, v in d.items()]])
        else:
            out.append([n, True, d])
    return out


def gen_surface():
    return dict(cem=_signature(ref_mpc.cem), world_model_init=_signature(ref_wm.WorldModel.__init__),
                names=["l1", "round_small_elements", "cem", "compute_new_pose", "poses_to_diff", "WorldModel"])


# ------------------------------------------------------------------------------------------------ (d)
def frames_transform(clip):
    """[1, T, H, W, C] array -> [C, T, H, W] tensor (an identity-like transform)."""
    return torch.from_numpy(np.ascontiguousarray(clip[0])).permute(3, 0, 1, 2).float()


def gen_encode():
    torch.manual_seed(WSEED + 2)
    enc = ref_vit.VisionTransformer(norm_layer=functools.partial(torch.nn.LayerNorm, eps=1e-6), **ECFG)
    _perturb(enc)
    enc.eval()
    g = torch.Generator().manual_seed(WSEED + 3)
    image = torch.randn(2, 32, 32, 3, generator=g).bfloat16().float()
    wm = ref_wm.WorldModel(encoder=enc, predictor=None, tokens_per_frame=4, transform=frames_transform, device="cpu")
    with torch.no_grad():
        h = wm.encode(image.numpy())
    print(f"encode: output {tuple(h.shape)}, mean |h| {h.abs().mean():.3e}")
    return dict(cfg=dict(ECFG), seed=WSEED + 2, enc_sums=_sums(enc.state_dict()), image=image, out=h)


def main():
    out = dict(pose=gen_pose(), cem=gen_cem(), surface=gen_surface(), encode=gen_encode())
    path = os.path.join(OUT, "planning.pt")
    torch.save(out, path)
    print(f"wrote {path} ({os.path.getsize(path) / 1e3:.1f} kB)")
    torch.load(path, weights_only=True)  # tensors, scalars and settings only
    assert os.path.getsize(path) < 1_000_000
    assert math.isfinite(out["cem"]["runs"]["rollout1"]["margin"])


if __name__ == "__main__":
    main()
