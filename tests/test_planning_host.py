"""CPU: the host side of vjepa2_amd.planning against the reference's recorded results (tests/golden/planning.pt):
poses_to_diff (numpy f64, no scipy), round_small_elements, the public surface and the topk < 2 refusal."""

import inspect

import numpy as np
import pytest
import torch

import planning_fixture as fx


def test_poses_to_diff_matches_reference():
    """float64 against float64: 1e-12 (the recorded angles keep >= 1e-3 from +-pi and >= 0.05 from +-pi/2, so the
    two formulations of the same rotation agree to a few ulps of f64)."""
    from vjepa2_amd.planning import poses_to_diff

    p = fx.load()["pose"]
    n = p["start"].shape[0]
    assert n >= 56
    for i in range(n):
        got = poses_to_diff(p["start"][i], p["end"][i])
        assert got.dtype == torch.float64 and tuple(got.shape) == (7,)
        err = (got - p["diff"][i]).abs().max().item()
        assert err <= 1e-12, (i, err, got.tolist(), p["diff"][i].tolist())
    # numpy rows work as well (the reference accepts both)
    got = poses_to_diff(p["start"][3].numpy(), p["end"][3].numpy())
    assert (got - p["diff"][3]).abs().max().item() <= 1e-12


def test_poses_to_diff_needs_no_scipy(monkeypatch):
    import sys

    from vjepa2_amd import planning

    monkeypatch.setitem(sys.modules, "scipy", None)  # import scipy -> ImportError
    p = fx.load()["pose"]
    got = planning.poses_to_diff(p["start"][0], p["end"][0])
    assert (got - p["diff"][0]).abs().max().item() <= 1e-12


def test_round_small_elements():
    from vjepa2_amd.planning import round_small_elements

    x = torch.tensor([[0.3, -0.2, 0.25, -0.25, 0.0, 0.2499, float("nan"), -1.0]])
    keep = x.clone()
    y = round_small_elements(x, 0.25)
    assert torch.equal(x[~x.isnan()], keep[~keep.isnan()])  # the input is not modified
    want = torch.tensor([[0.3, 0.0, 0.25, -0.25, 0.0, 0.0, float("nan"), -1.0]])
    assert torch.equal(y.isnan(), want.isnan()) and torch.equal(y[~y.isnan()], want[~want.isnan()])
    assert y.data_ptr() != x.data_ptr()


def test_l1_is_mean_abs_over_last_dim():
    from vjepa2_amd.planning import l1

    a, b = torch.randn(5, 12), torch.randn(5, 12)
    assert torch.equal(l1(a, b), (a - b).abs().mean(dim=-1))


def test_public_surface_matches_reference():
    from vjepa2_amd import planning

    s = fx.load()["surface"]
    for name in s["names"]:
        assert hasattr(planning, name), name
    assert fx.signature(planning.cem) == s["cem"]
    assert fx.signature(planning.WorldModel.__init__) == s["world_model_init"]
    for meth in ("encode", "infer_next_action"):
        assert callable(getattr(planning.WorldModel, meth))
    assert list(inspect.signature(planning.WorldModel.infer_next_action).parameters) == [
        "self", "rep", "pose", "goal_rep", "close_gripper"]
    assert list(inspect.signature(planning.compute_new_pose).parameters) == ["pose", "action"]
    assert list(inspect.signature(planning.poses_to_diff).parameters) == ["start", "end"]


def test_cem_refuses_topk_below_two():
    """The one deliberate difference from the reference (its std over one elite is NaN): refused before any
    device work, so this needs no GPU."""
    from vjepa2_amd.planning import cem

    z = torch.zeros(1, 1, 4, 96)
    with pytest.raises(ValueError, match="topk must be >= 2"):
        cem(z, torch.zeros(1, 1, 7), z, world_model=lambda *a: None, topk=1, samples=8)
    with pytest.raises(ValueError, match="topk must be >= 2"):
        cem(z, torch.zeros(1, 1, 7), z, world_model=lambda *a: None, topk=0, samples=8)


def test_fixture_margins():
    """What the generator asserts, re-checked on the stored values: the pose angles keep their distance from the
    branch cuts, and every CEM iteration's elite boundary is wider than 4 G_energy(max)."""
    f = fx.load()
    for ang in (f["pose"]["new_pose"][:, 3:6].double().numpy(), f["pose"]["diff"][:, 3:6].numpy()):
        assert np.all(np.pi - np.abs(ang[:, 0]) >= 1e-3) and np.all(np.pi - np.abs(ang[:, 2]) >= 1e-3)
        assert np.all(np.pi / 2 - np.abs(ang[:, 1]) >= 0.05)
    k = f["cem"]["mpc"]["topk"]
    for name, run in f["cem"]["runs"].items():
        e = run["f32"]["energy"].sort(dim=1).values
        assert (e[:, k] - e[:, k - 1]).min().item() > 4 * run["gaps"]["energy"]["max"], name
        assert torch.equal(run["f32"]["elites"], run["bf16"]["elites"]), name
