"""GPU: the planner with the K/V cache across rollout steps (WorldModel.set_kv_cache(True)) against the reference
planner's recordings (tests/golden/planning.pt), mirroring tests/test_gpu_planning.py: the same envelopes
G = |reference under bf16 autocast - reference fp32| (never measured on the code under test), the reference's
elite sets and action bits, the absence of host synchronisation, and what the cache is for: the rows fed to the
QKV GEMMs. The switch is a setter, not a constructor keyword: WorldModel.__init__ keeps the reference's signature
(tests/test_planning_host.py)."""

import pytest
import torch

import planning_fixture as fx

pytestmark = pytest.mark.gpu

DEV = "cuda"
RUNS = ["rollout1", "rollout2", "axis", "close"]  # rollout1: the degenerate single-step cache


def world_model(run=None, kv_cache=True):
    from vjepa2_amd.planning import WorldModel

    extra = dict(mpc_args=fx.run_args(run)) if run is not None else {}
    wm = WorldModel(encoder=None, predictor=fx.predictor(DEV), tokens_per_frame=4, transform=None, device=DEV, **extra)
    return wm.set_kv_cache(True) if kv_cache else wm


def replay(monkeypatch, run, cem_steps=None, wm=None):
    """test_gpu_planning.replay with the cache on: (action, what reached vj_cem_update per iteration, the model)."""
    from vjepa2_amd import ops, planning

    c = fx.load()["cem"]
    wm = wm if wm is not None else world_model(run)
    wm.mpc_args = fx.run_args(run)
    if cem_steps is not None:
        wm.mpc_args = dict(wm.mpc_args, cem_steps=cem_steps)
    rec = []
    real = ops.cem_update

    def update(energy, actions, k, mean, std, *a, **kw):
        idx = real(energy, actions, k, mean, std, *a, want_idx=True, **kw)
        rec.append(dict(energy=energy.clone(), actions=actions.clone(), elites=idx.clone()))
        return idx

    with monkeypatch.context() as m:
        m.setattr(planning.ops, "cem_update", update)
        m.setattr(torch, "randn", fx.ReplayRandn(run["f32"]["noise"]))
        out = wm.infer_next_action(c["rep"].to(DEV), c["pose"].to(DEV), c["goal"].to(DEV),
                                   close_gripper=run["close_gripper"])
    return out, rec, wm


def _check_against_recording(name, run, out, rec):
    f = run["f32"]
    assert len(rec) == run["cem_steps"]
    for it, r in enumerate(rec):
        assert torch.equal(r["elites"].cpu(), f["elites"][it]), (name, it, r["elites"].tolist(), f["elites"][it].tolist())
    assert out.is_cuda and tuple(out.shape) == (run["rollout"], 7)
    assert torch.equal(out.cpu(), f["action"]), (name, (out.cpu() - f["action"]).abs().max().item())


@pytest.mark.parametrize("name", RUNS)
def test_iteration0_energies_inside_the_bf16_envelope(monkeypatch, name):
    run = fx.load()["cem"]["runs"][name]
    _, rec, wm = replay(monkeypatch, run, cem_steps=1)
    assert wm.kv_cache and wm._cache is not None and wm._cache.frames == run["rollout"]
    assert len(rec) == 1 and torch.equal(rec[0]["actions"].cpu(), run["f32"]["actions"][0])
    d = (rec[0]["energy"].cpu() - run["f32"]["energy"][0]).abs()
    G = run["gaps"]["energy"]
    print(f"{name} (cached): |HIP - fp32| energies mean {d.mean():.3e} max {d.max():.3e}; G mean {G['mean']:.3e} "
          f"max {G['max']:.3e}")
    assert d.mean().item() <= 1.5 * G["mean"], (d.mean().item(), G["mean"])
    assert d.max().item() <= 1.5 * G["max"], (d.max().item(), G["max"])


@pytest.mark.parametrize("name", RUNS)
def test_full_loop_elites_and_action(monkeypatch, name):
    """Every iteration selects the reference's elite set (its k-th / (k+1)-th energy gap exceeds 4 G_max in the
    fixture) and the returned action has the fp32 reference's bits (G_action is 0 in the fixture)."""
    run = fx.load()["cem"]["runs"][name]
    assert run["gaps"]["action"]["max"] == 0
    out, rec, _ = replay(monkeypatch, run)
    _check_against_recording(name, run, out, rec)
    assert not out[:, 3:6].any()


def test_rows_through_the_qkv_gemm(monkeypatch):
    """One rollout-2 iteration feeds 2 depth S n_t rows to the QKV GEMMs with the cache and 3 depth S n_t
    without (R against R (R + 1) / 2 frame blocks)."""
    from vjepa2_amd import functions, ops

    run = fx.load()["cem"]["runs"]["rollout2"]
    real = ops.qkv_rope
    rows = []

    def counted(x, *a, **kw):
        rows.append(x.shape[0])
        return real(x, *a, **kw)

    monkeypatch.setattr(functions.ops, "qkv_rope", counted)
    depth, S, n_t = 2, fx.load()["cem"]["mpc"]["samples"], 2 + 4
    for cached, blocks in ((True, 2), (False, 3)):
        del rows[:]
        replay(monkeypatch, run, cem_steps=1, wm=world_model(run, kv_cache=cached))
        assert sum(rows) == blocks * depth * S * n_t, (cached, rows)
        assert len(rows) == 2 * depth


def test_infer_next_action_never_synchronises(monkeypatch):
    """test_gpu_planning's never-synchronises test with the cache on (rollout 2, 3 iterations: the cache is
    reset at two iteration boundaries). The first, unpatched call does the one-time set-up: RoPE tables, index
    and layout caches, the cache's allocation."""
    c = fx.load()["cem"]
    run = c["runs"]["close"]
    wm = world_model(run)
    rep, pose, goal = c["rep"].to(DEV), c["pose"].to(DEV), c["goal"].to(DEV)
    wm.infer_next_action(rep, pose, goal, close_gripper=1)
    cache = wm._cache

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
    assert wm._cache is cache  # allocated once
    assert out.is_cuda and torch.isfinite(out.cpu()).all()
    assert out[1, 6].item() == pytest.approx(1.0, abs=0.3)


def test_shape_change_reallocates_and_still_matches(monkeypatch):
    """One WorldModel across calls whose rollout and samples change: rollout 2 -> 1 -> 2 replays the recordings
    (elites and action bits each time) on a reallocated cache; samples 16 -> 8 has no recording, so iteration 0's
    energies are compared with the uncached path's on the same seeded noise: both are held to 1.5 G_max of the
    reference on the recorded runs, so they may differ from each other by at most 3 G_max."""
    runs = fx.load()["cem"]["runs"]
    out, rec, wm = replay(monkeypatch, runs["rollout2"])
    _check_against_recording("rollout2", runs["rollout2"], out, rec)
    c2 = wm._cache
    assert (c2.batch, c2.max_frames) == (16, 2)
    out, rec, _ = replay(monkeypatch, runs["rollout1"], wm=wm)
    _check_against_recording("rollout1", runs["rollout1"], out, rec)
    c1 = wm._cache
    assert c1 is not c2 and (c1.batch, c1.max_frames) == (16, 1)
    out, rec, _ = replay(monkeypatch, runs["axis"], wm=wm)
    _check_against_recording("axis", runs["axis"], out, rec)
    assert wm._cache is not c1 and wm._cache.max_frames == 2

    from vjepa2_amd import ops, planning

    c = fx.load()["cem"]
    energies = {}
    for cached in (True, False):
        m8 = wm if cached else world_model(runs["rollout2"], kv_cache=False)
        m8.mpc_args = dict(fx.run_args(runs["rollout2"]), samples=8, cem_steps=1)
        real = ops.cem_update
        with monkeypatch.context() as m:
            m.setattr(planning.ops, "cem_update",
                      lambda e, *a, _c=cached, **kw: (energies.__setitem__(_c, e.clone()), real(e, *a, **kw))[1])
            torch.manual_seed(5)
            m8.infer_next_action(c["rep"].to(DEV), c["pose"].to(DEV), c["goal"].to(DEV))
    assert (wm._cache.batch, wm._cache.max_frames) == (8, 2)
    d = (energies[True] - energies[False]).abs().max().item()
    G = runs["rollout2"]["gaps"]["energy"]["max"]
    print(f"samples 8: |cached - uncached| energies max {d:.3e}; 3 G_max {3 * G:.3e}")
    assert energies[True].shape == (8,) and d <= 3 * G, (d, G)


def test_default_is_unchanged(monkeypatch):
    """Without set_kv_cache, and with set_kv_cache(False), the planner is the uncached one bit for bit and
    allocates no cache."""
    run = fx.load()["cem"]["runs"]["rollout2"]
    a, rec_a, wa = replay(monkeypatch, run, wm=world_model(run, kv_cache=False))
    b, rec_b, wb = replay(monkeypatch, run, wm=world_model(run, kv_cache=False).set_kv_cache(False))
    assert wa.kv_cache is False and wa._cache is None and wb._cache is None
    assert torch.equal(a, b)
    for ra, rb in zip(rec_a, rec_b):
        assert torch.equal(ra["energy"], rb["energy"])
