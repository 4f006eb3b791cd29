"""Goal-image planning with the V-JEPA 2-AC predictor: the cross-entropy method of the reference's
notebooks/utils/mpc_utils.py (l1, round_small_elements, cem, compute_new_pose, poses_to_diff) and
notebooks/utils/world_model_wrapper.py (WorldModel.encode / infer_next_action), same names, arguments and
defaults, with everything between two predictor forwards on the device (vj_plan.hip):

 * the actions of one CEM iteration come from one vj_cem_sample launch over a [rollout, S, 4] noise buffer
   (drawn by torch.randn(samples, 4) once per rollout step, in the reference's order);
 * the world model's step writes the normalised next frame straight into its slot of a pre-allocated
   [S, rollout + 1, HW, D] frame trajectory (vj_plan_frame, which also gives the L1 energy to the goal on the
   last step) and the next pose into a [S, rollout + 1, 7] pose trajectory (vj_pose_step): no torch.cat, no
   .cpu() / scipy round trip per step;
 * elite selection and the momentum update are one launch (vj_cem_update) on mean / std [rollout, 4] that
   never leave the device;
 * opt-in (WorldModel.set_kv_cache(True), not in the reference): rollout step h feeds the predictor frame h
   alone, the earlier frames' keys and values coming from a per-layer K/V cache (predictor.forward_cached), so
   a rollout of R steps pushes R frame blocks through the predictor's GEMMs instead of R (R + 1) / 2.

Deliberate difference from the reference: topk < 2 raises ValueError (the reference's unbiased std of a single
elite is NaN and silently poisons every later sample).
"""

import numpy as np
import torch

from . import ops


def l1(a, b):
    return torch.mean(torch.abs(a - b), dim=-1)


def round_small_elements(tensor, threshold):
    return tensor.masked_fill(torch.abs(tensor) < threshold, 0)


class _Trajectories:
    """The pre-allocated buffers of one cem() call. Slot 0 of frames / poses is the context; step h reads
    slots 0..h and fills slot h + 1."""

    def __init__(self, context_frame, context_pose, samples, rollout):
        hw, d = context_frame.shape[-2:]  # [1, 1, HW, D], or the notebook's [1, HW, D]
        dev = context_frame.device
        self.frames = torch.empty(samples, rollout + 1, hw, d, dtype=context_frame.dtype, device=dev)
        self.frames[:, :1] = context_frame
        self.poses = torch.empty(samples, rollout + 1, 7, dtype=torch.float32, device=dev)
        self.poses[:, :1] = context_pose
        self.actions = torch.empty(samples, rollout, 7, dtype=torch.float32, device=dev)
        self.noise = torch.empty(rollout, samples, 4, dtype=torch.float32, device=dev)
        self.energy = torch.empty(samples, dtype=torch.float32, device=dev)


def cem(
    context_frame,
    context_pose,
    goal_frame,
    world_model,
    rollout=1,
    cem_steps=100,
    momentum_mean=0.25,
    momentum_std=0.95,
    momentum_mean_gripper=0.15,
    momentum_std_gripper=0.15,
    samples=100,
    topk=10,
    verbose=False,
    maxnorm=0.05,
    axis={},
    objective=l1,
    close_gripper=None,
):
    """
    :param context_frame: [B=1, T=1, HW, D]
    :param goal_frame: [B=1, T=1, HW, D]
    :param world_model: f(frame_traj [S, t, HW, D], action_traj [S, t, 7], pose_traj [S, t, 7])
        -> (next_frame [S, 1, HW, D], next_pose [S, 1, 7])
    :return: [B=1, rollout, 7] an action trajectory over the rollout horizon (on the device)

    mpc_utils.py:28-163. ``world_model`` and ``objective`` are arbitrary callables. A world model that has a
    ``step_into(traj, h, goal)`` method (WorldModel's) fills the trajectory buffers in place and, given a
    goal, writes the L1 energy of the new frame and returns True; any other callable's results are copied
    into their slots. With ``objective is l1`` on f32 frames (width a multiple of 4, at most 2048) the energy
    is vj_plan_frame's, otherwise the callable's.
    """
    if topk < 2:
        raise ValueError(f"cem: topk must be >= 2 (got {topk}): the unbiased std of a single elite is NaN")
    if topk > samples:
        raise ValueError(f"cem: topk {topk} > samples {samples}")
    dev = context_frame.device
    if dev.type != "cuda":
        raise RuntimeError("vjepa2_amd.planning.cem runs on a HIP device; there is no CPU path")
    traj = _Trajectories(context_frame, context_pose, samples, rollout)
    goal = goal_frame.reshape(goal_frame.shape[-2], goal_frame.shape[-1]).contiguous()
    # current estimate of the mean / std of the distribution over action trajectories (columns x, y, z, gripper)
    mean = torch.zeros(rollout, 4, dtype=torch.float32, device=dev)
    std = torch.ones(rollout, 4, dtype=torch.float32, device=dev)
    std[:, :3] = maxnorm
    for ax in axis.keys():
        mean[:, ax] = axis[ax]
    step_into = getattr(world_model, "step_into", None)
    hw, d = goal.shape
    fused_l1 = objective is l1 and traj.frames.dtype == torch.float32 and d % 4 == 0 and d <= 2048

    for _ in range(cem_steps):
        for h in range(rollout):  # the reference draws one [S, 4] normal per rollout step, in this order
            traj.noise[h].copy_(torch.randn(samples, mean.size(1), device=mean.device))
        ops.cem_sample(traj.noise, mean, std, maxnorm, axis=axis, close_from=close_gripper, out=traj.actions)
        have_energy = False
        for h in range(rollout):
            last = h == rollout - 1
            if step_into is not None:
                have_energy = step_into(traj, h, goal if (last and fused_l1) else None) and last
            else:
                next_frame, next_pose = world_model(traj.frames[:, :h + 1], traj.actions[:, :h + 1],
                                                    traj.poses[:, :h + 1])
                traj.frames[:, h + 1:h + 2] = next_frame
                traj.poses[:, h + 1:h + 2] = next_pose
        final = traj.frames[:, -1]
        if have_energy:
            energy = traj.energy
        elif fused_l1:
            _, energy = ops.plan_frame(final, goal=goal, normalize=False, energy=traj.energy)
        else:
            energy = objective(final.flatten(1), goal.reshape(1, -1).expand(samples, -1))
            energy = energy.to(torch.float32).contiguous()
        ops.cem_update(energy, traj.actions, topk, mean, std, momentum_mean, momentum_std, momentum_mean_gripper,
                       momentum_std_gripper)

    new_action = torch.cat(
        [
            mean[..., :3],
            torch.zeros((rollout, 3), device=mean.device),
            round_small_elements(mean[..., -1:], 0.25),
        ],
        dim=-1,
    )[None, :]
    return new_action


def compute_new_pose(pose, action):
    """
    :param pose: [B, T=1, 7]
    :param action: [B, T=1, 7]
    :returns: [B, T=1, 7]

    mpc_utils.py:166-190 on the device (vj_pose_step): the rotation composition runs in f64 inside the kernel.
    """
    out = ops.pose_step(pose[:, 0].to(torch.float32), action[:, 0].to(torch.float32))
    return out.to(pose.dtype)[:, None]


def _euler_xyz_matrix(t):
    """scipy's Rotation.from_euler("xyz", t).as_matrix(): extrinsic x, y, z = Rz(t2) Ry(t1) Rx(t0)."""
    (sa, sb, sc), (ca, cb, cc) = np.sin(t), np.cos(t)
    return np.array([[cc * cb, cc * sb * sa - sc * ca, cc * sb * ca + sc * sa],
                     [sc * cb, sc * sb * sa + cc * ca, sc * sb * ca - cc * sa],
                     [-sb, cb * sa, cb * ca]], dtype=np.float64)


def _matrix_euler_xyz(m):
    """Rotation.from_matrix(m).as_euler("xyz"): pitch in [-pi/2, pi/2]; at gimbal lock the third angle is 0."""
    cp = np.hypot(m[0, 0], m[1, 0])
    pitch = np.arctan2(-m[2, 0], cp)
    if cp > 1e-7:
        return np.array([np.arctan2(m[2, 1], m[2, 2]), pitch, np.arctan2(m[1, 0], m[0, 0])])
    roll = np.arctan2(m[0, 1], m[1, 1]) if m[2, 0] < 0 else np.arctan2(-m[0, 1], m[1, 1])
    return np.array([roll, pitch, 0.0])


def poses_to_diff(start, end):
    """
    :param start: [7]
    :param end: [7]

    mpc_utils.py:193-226 in numpy float64 on the host, without scipy.
    """
    try:
        start = start.numpy()
        end = end.numpy()
    except Exception:
        pass
    xyz_diff = end[:3] - start[:3]
    s_rotation = _euler_xyz_matrix(np.asarray(start[3:6], dtype=np.float64))
    e_rotation = _euler_xyz_matrix(np.asarray(end[3:6], dtype=np.float64))
    theta_diff = _matrix_euler_xyz(e_rotation @ s_rotation.T)
    gripper_diff = end[-1:] - start[-1:]
    action = np.concatenate([xyz_diff, theta_diff, gripper_diff], axis=0)
    return torch.from_numpy(action)


class _PredictorStep:
    """WorldModel's step: a callable with the reference's step_predictor semantics, and step_into for cem()'s
    pre-allocated trajectories."""

    def __init__(self, wm):
        self.wm = wm

    def _predict(self, reps, actions, poses):
        """[S, T, HW, D] -> the predictor output as a [S, T, HW, D] view (no slice copy of the last frame)."""
        S, T, n_t, D = reps.shape
        if n_t != self.wm.tokens_per_frame:
            raise ValueError(f"{n_t} tokens per frame, WorldModel was built for {self.wm.tokens_per_frame}")
        with torch.no_grad():
            out = self.wm.predictor(reps.flatten(1, 2), actions, poses)
        return out.view(S, T, n_t, D)

    def __call__(self, reps, actions, poses):
        out = self._predict(reps, actions, poses)
        S, _, n_t, D = out.shape
        nxt = torch.empty(S, 1, n_t, D, dtype=torch.float32, device=out.device)
        ops.plan_frame(out[:, -1], dst=nxt[:, 0], normalize=self.wm.normalize_reps)
        return nxt, compute_new_pose(poses[:, -1:], actions[:, -1:])

    def _predict_cached(self, traj, h):
        """The predictor output for frame h alone, [S, HW, D]: frames 0 .. h-1 of this CEM iteration are in the
        K/V cache (step 0 resets it: its action is resampled every iteration, so nothing carries over)."""
        S, slots, n_t, D = traj.frames.shape
        if n_t != self.wm.tokens_per_frame:
            raise ValueError(f"{n_t} tokens per frame, WorldModel was built for {self.wm.tokens_per_frame}")
        cache = self.wm._rollout_cache(S, slots - 1)
        if h == 0:
            cache.reset()
        with torch.no_grad():
            return self.wm.predictor.forward_cached(traj.frames[:, h], traj.actions[:, h:h + 1],
                                                    traj.poses[:, h:h + 1], cache=cache)

    def step_into(self, traj, h, goal):
        if self.wm.kv_cache:
            last = self._predict_cached(traj, h)
        else:
            last = self._predict(traj.frames[:, :h + 1], traj.actions[:, :h + 1], traj.poses[:, :h + 1])[:, -1]
        ops.plan_frame(last, goal=goal, dst=traj.frames[:, h + 1], normalize=self.wm.normalize_reps,
                       energy=traj.energy if goal is not None else None)
        ops.pose_step(traj.poses[:, h], traj.actions[:, h], out=traj.poses[:, h + 1])
        return goal is not None


class WorldModel(object):
    """world_model_wrapper.py:12-75 on the HIP encoder / AC predictor."""

    def __init__(
        self,
        encoder,
        predictor,
        tokens_per_frame,
        transform,
        mpc_args={
            "rollout": 2,
            "samples": 400,
            "topk": 10,
            "cem_steps": 10,
            "momentum_mean": 0.15,
            "momentum_std": 0.15,
            "maxnorm": 0.05,
            "verbose": True,
        },
        normalize_reps=True,
        device="cuda:0",
    ):
        super().__init__()
        self.encoder = encoder
        self.predictor = predictor
        self.normalize_reps = normalize_reps
        self.transform = transform
        self.tokens_per_frame = tokens_per_frame
        self.device = device
        self.mpc_args = mpc_args
        self.kv_cache = False  # set_kv_cache(): the constructor keeps the reference's signature
        self._cache = None

    def set_kv_cache(self, on=True):
        """Opt in to (or out of) the K/V cache across rollout steps: infer_next_action's rollout then feeds the
        predictor one frame per step and keeps the earlier frames' keys and values (predictor.forward_cached)
        instead of re-running every earlier frame, which is the reference's structure and the default. The
        generic __call__ path and cem() with a plain callable never cache. Returns self."""
        self.kv_cache = bool(on)
        if not self.kv_cache:
            self._cache = None
        return self

    def _rollout_cache(self, samples, rollout):
        """The K/V cache of the planning rollout, allocated once and again only when samples or rollout change."""
        c = self._cache
        if c is None or (c.batch, c.max_frames) != (samples, rollout):
            self._cache = None  # free the old buffers before the new ones are allocated
            c = self._cache = self.predictor.new_cache(samples, rollout)
        return c

    def encode(self, image):
        clip = np.expand_dims(image, axis=0)
        clip = self.transform(clip)[None, :]
        B, C, T, H, W = clip.size()
        clip = clip.permute(0, 2, 1, 3, 4).flatten(0, 1).unsqueeze(2).repeat(1, 1, 2, 1, 1)
        clip = clip.to(self.device, non_blocking=True)
        with torch.no_grad():
            h = self.encoder(clip)
        h = h.view(B, T, -1, h.size(-1)).flatten(1, 2)
        if self.normalize_reps:
            h = h.to(torch.float32).contiguous()
            out = torch.empty_like(h)
            ops.plan_frame(h, dst=out, normalize=True)
            h = out
        return h

    def infer_next_action(self, rep, pose, goal_rep, close_gripper=None):
        mpc_action = cem(
            context_frame=rep,
            context_pose=pose,
            goal_frame=goal_rep,
            world_model=_PredictorStep(self),
            close_gripper=close_gripper,
            **self.mpc_args,
        )[0]

        return mpc_action
