"""GPU: vjepa2_amd.planning end to end against the reference planner's recordings (tests/golden/planning.pt,
make_golden_planning.py): WorldModel.infer_next_action on the fixture's micro AC predictor fed the recorded
noise, inside the envelope G = |reference under bf16 autocast - reference fp32| the fixture carries (never
measured on the code under test; the factor 1.5 is the margin the anticipation tests use for such envelopes),
the absence of host synchronisation in the loop, encode, compute_new_pose and the generic-callable path."""

import pytest
import torch

import planning_fixture as fx

pytestmark = pytest.mark.gpu

DEV = "cuda"
RUNS = ["rollout1", "rollout2", "axis", "close"]


def world_model(run=None, **kw):
    from vjepa2_amd.planning import WorldModel

    args = fx.run_args(run) if run is not None else None
    extra = dict(mpc_args=args) if args is not None else {}
    return WorldModel(encoder=None, predictor=fx.predictor(DEV), tokens_per_frame=4, transform=None, device=DEV,
                      **extra, **kw)


def replay(monkeypatch, run, cem_steps=None):
    """infer_next_action of one recorded run fed its recorded noise; returns (action, per-iteration records of
    what reached vj_cem_update: energy, actions, elite indices)."""
    from vjepa2_amd import ops, planning

    c = fx.load()["cem"]
    wm = world_model(run)
    if cem_steps is not None:
        wm.mpc_args = dict(wm.mpc_args, cem_steps=cem_steps)
    rec = []
    real = ops.cem_update

    def update(energy, actions, k, mean, std, *a, **kw):
        idx = real(energy, actions, k, mean, std, *a, want_idx=True, **kw)
        rec.append(dict(energy=energy.clone(), actions=actions.clone(), elites=idx.clone(), mean=mean.clone(),
                        std=std.clone()))
        return idx

    monkeypatch.setattr(planning.ops, "cem_update", update)
    monkeypatch.setattr(torch, "randn", fx.ReplayRandn(run["f32"]["noise"]))
    out = wm.infer_next_action(c["rep"].to(DEV), c["pose"].to(DEV), c["goal"].to(DEV),
                               close_gripper=run["close_gripper"])
    monkeypatch.undo()
    return out, rec


@pytest.mark.parametrize("name", RUNS)
def test_iteration0_energies_inside_the_bf16_envelope(monkeypatch, name):
    """Iteration 0 (mean and std are the initial ones, the actions the recorded ones bit for bit): the HIP
    energies against the reference's fp32 energies, mean |diff| <= 1.5 G_mean and max |diff| <= 1.5 G_max."""
    run = fx.load()["cem"]["runs"][name]
    _, rec = replay(monkeypatch, run, cem_steps=1)
    assert len(rec) == 1
    assert torch.equal(rec[0]["actions"].cpu(), run["f32"]["actions"][0])
    d = (rec[0]["energy"].cpu() - run["f32"]["energy"][0]).abs()
    G = run["gaps"]["energy"]
    print(f"{name}: |HIP - fp32| energies mean {d.mean():.3e} max {d.max():.3e}; G mean {G['mean']:.3e} max {G['max']:.3e}")
    assert d.mean().item() <= 1.5 * G["mean"], (d.mean().item(), G["mean"])
    assert d.max().item() <= 1.5 * G["max"], (d.max().item(), G["max"])


@pytest.mark.parametrize("name", RUNS)
def test_full_loop_elites_and_action(monkeypatch, name):
    """Every iteration selects the reference's elite set (its k-th / (k+1)-th energy gap exceeds 4 G_max in the
    fixture), and the returned action is within 1.5 G_action of the fp32 reference's. G_action is 0 in the
    fixture (both of the reference's precisions pick the same elites, so their actions are the same bits):
    the HIP loop has to return the reference's bits, which it does because vj_cem_sample and vj_cem_update
    evaluate the reference's f32 expressions in its order."""
    run = fx.load()["cem"]["runs"][name]
    out, rec = replay(monkeypatch, run)
    f = run["f32"]
    assert len(rec) == run["cem_steps"]
    for it, r in enumerate(rec):
        assert torch.equal(r["elites"].cpu(), f["elites"][it]), (name, it, r["elites"].tolist(), f["elites"][it].tolist())
    assert out.is_cuda and tuple(out.shape) == (run["rollout"], 7)
    want = f["action"]
    d = (out.cpu() - want).abs()
    G = run["gaps"]["action"]
    print(f"{name}: |HIP - fp32| action mean {d.mean():.3e} max {d.max():.3e}; G mean {G['mean']:.3e} max {G['max']:.3e}")
    assert d.max().item() <= 1.5 * G["max"], (d.max().item(), G["max"])
    assert d.mean().item() <= 1.5 * G["mean"], (d.mean().item(), G["mean"])
    assert not out[:, 3:6].any()


def test_infer_next_action_never_synchronises(monkeypatch):
    """With .cpu / .item / .tolist / .numpy, torch.cuda.synchronize and the synchronize methods of streams and
    events raising, a whole infer_next_action (rollout 2, 3 iterations) completes. One call runs first without
    the patches: the library's one-time set-up (RoPE tables uploaded and cached per geometry, index caches) is
    not part of the loop."""
    c = fx.load()["cem"]
    run = c["runs"]["close"]
    wm = world_model(run)
    rep, pose, goal = c["rep"].to(DEV), c["pose"].to(DEV), c["goal"].to(DEV)
    wm.infer_next_action(rep, pose, goal, close_gripper=1)

    def trip(name):
        def f(*a, **k):
            raise AssertionError(f"host synchronisation inside the planning loop: {name}")
        return f

    with monkeypatch.context() as m:
        for meth in ("cpu", "item", "tolist", "numpy"):
            m.setattr(torch.Tensor, meth, trip("Tensor." + meth))
        m.setattr(torch.cuda, "synchronize", trip("torch.cuda.synchronize"))
        m.setattr(torch.cuda.Stream, "synchronize", trip("Stream.synchronize"))
        m.setattr(torch.cuda.Event, "synchronize", trip("Event.synchronize"))
        out = wm.infer_next_action(rep, pose, goal, close_gripper=1)
    assert out.is_cuda and torch.isfinite(out.cpu()).all()
    assert out[1, 6].item() == pytest.approx(1.0, abs=0.3)  # the gripper mean moves towards the closed 1.0


def test_encode_matches_reference():
    """The encoder tests' tolerance (rel L1 < 1e-2 against the reference's fp32 output)."""
    from vjepa2_amd.planning import WorldModel

    e = fx.load()["encode"]
    wm = WorldModel(encoder=fx.encoder(DEV), predictor=None, tokens_per_frame=4, transform=fx.frames_transform,
                    device=DEV)
    h = wm.encode(e["image"].numpy())
    assert tuple(h.shape) == tuple(e["out"].shape) and h.is_cuda
    rel = ((h.float().cpu() - e["out"]).abs().mean() / e["out"].abs().mean()).item()
    assert rel < 1e-2, rel
    raw = WorldModel(encoder=wm.encoder, predictor=None, tokens_per_frame=4, transform=fx.frames_transform,
                     normalize_reps=False, device=DEV).encode(e["image"].numpy())
    assert tuple(raw.shape) == tuple(h.shape) and not torch.allclose(raw.float(), h.float())


def test_compute_new_pose_public_call():
    from vjepa2_amd.planning import compute_new_pose

    p = fx.load()["pose"]
    got = compute_new_pose(p["pose"][:, None].to(DEV), p["action"][:, None].to(DEV))
    assert got.is_cuda and tuple(got.shape) == (p["pose"].shape[0], 1, 7) and got.dtype == torch.float32
    got, want = got[:, 0].cpu(), p["new_pose"]
    assert torch.equal(got[:, :3], want[:, :3]) and torch.equal(got[:, 6], want[:, 6])
    assert (got[:, 3:6].double() - want[:, 3:6].double()).abs().max().item() <= 2.0**-22


def test_generic_callables_give_the_torch_loop(monkeypatch):
    """A trivial Python world model and a custom (L2) objective: the same elites, iteration by iteration, and the
    same action as a torch implementation of mpc_utils.py's loop on the same noise. The toy's energies are
    spread far wider than f32 rounding, so both sides rank them alike."""
    from vjepa2_amd import ops, planning

    S, k, rollout, steps, hw, D = 48, 6, 2, 4, 3, 20  # D % 4 == 0 is not needed on this path
    g = torch.Generator().manual_seed(21)
    W = torch.randn(7, hw * D, generator=g).to(DEV)
    ctx = torch.randn(1, 1, hw, D, generator=g).to(DEV)
    goal = (ctx + 0.05 * torch.randn(1, 1, hw, D, generator=g).to(DEV))
    pose = torch.tensor([[[0.1, 0.2, 0.3, 0.0, 0.1, -0.1, 0.5]]], device=DEV)
    noise = torch.randn(steps, rollout, S, 4, generator=g)
    mpc = dict(rollout=rollout, cem_steps=steps, samples=S, topk=k, maxnorm=0.05, momentum_mean=0.15,
               momentum_std=0.25, momentum_mean_gripper=0.1, momentum_std_gripper=0.3, axis={2: 0.02})

    def toy(frames, actions, poses):
        nxt = frames[:, -1:] + (actions[:, -1] @ W).view(-1, 1, hw, D)
        return nxt, poses[:, -1:] + actions[:, -1:]

    def l2(a, b):
        return ((a - b) ** 2).sum(dim=-1).sqrt()

    elites = []
    real = ops.cem_update

    def update(energy, actions, kk, mean, std, *a, **kw):
        idx = real(energy, actions, kk, mean, std, *a, want_idx=True, **kw)
        elites.append(idx.clone())
        return idx

    monkeypatch.setattr(planning.ops, "cem_update", update)
    monkeypatch.setattr(torch, "randn", fx.ReplayRandn(noise))
    got = planning.cem(ctx, pose, goal, toy, objective=l2, **mpc)
    monkeypatch.undo()

    # the same loop in torch (mpc_utils.py:62-161), elites in index order
    mean = torch.zeros(rollout, 4, device=DEV)
    std = torch.ones(rollout, 4, device=DEV)
    std[:, :3] = mpc["maxnorm"]
    mean[:, 2] = 0.02
    want_elites = []
    for it in range(steps):
        frames, poses, acts = ctx.repeat(S, 1, 1, 1), pose.repeat(S, 1, 1), None
        for h in range(rollout):
            a = noise[it, h].to(DEV) * std[h] + mean[h]
            a[:, :3] = torch.clip(a[:, :3], min=-0.05, max=0.05)
            a[:, -1:] = torch.clip(a[:, -1:], min=-0.75, max=0.75)
            a[:, 2] = 0.02
            a = torch.cat([a[:, :3], torch.zeros(S, 3, device=DEV), a[:, -1:]], dim=-1)[:, None]
            acts = a if acts is None else torch.cat([acts, a], dim=1)
            nf, npose = toy(frames, acts, poses)
            frames, poses = torch.cat([frames, nf], dim=1), torch.cat([poses, npose], dim=1)
        sims = l2(frames[:, -1].flatten(1), goal.repeat(S, 1, 1, 1)[:, -1].flatten(1))
        idx = sims.topk(k, largest=False).indices
        want_elites.append(idx.sort().values.to(torch.int32))
        sel = acts[idx]
        m, s = sel.mean(dim=0), sel.std(dim=0)
        mean = torch.cat([m[..., :3] * (1.0 - 0.15) + mean[..., :3] * 0.15, m[..., -1:] * (1.0 - 0.1) + mean[..., -1:] * 0.1], -1)
        std = torch.cat([s[..., :3] * (1.0 - 0.25) + std[..., :3] * 0.25, s[..., -1:] * (1.0 - 0.3) + std[..., -1:] * 0.3], -1)
    assert len(elites) == steps
    for it in range(steps):
        assert torch.equal(elites[it], want_elites[it]), (it, elites[it].tolist(), want_elites[it].tolist())
    want = torch.cat([mean[..., :3], torch.zeros(rollout, 3, device=DEV),
                      planning.round_small_elements(mean[..., -1:], 0.25)], dim=-1)[None]
    assert tuple(got.shape) == (1, rollout, 7)
    assert torch.allclose(got, want, rtol=0, atol=1e-6), (got - want).abs().max().item()
