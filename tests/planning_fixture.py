"""Shared loader of tests/golden/planning.pt (written by tests/golden/make_golden_planning.py).

The fixture stores no weights: the micro AC predictor and the micro encoder are rebuilt here from the recorded
seeds with this project's classes, whose constructors draw in the reference's order, followed by the generator's
perturbation draws (and the action-embedding gain), and checked against the per-tensor (sum, sum of squares) the
reference's weights had."""

import functools
import inspect
import os

import numpy as np
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@functools.lru_cache(maxsize=None)
def load():
    return torch.load(os.path.join(GOLD, "planning.pt"), weights_only=True)


def check_sums(sd, sums, what):
    assert list(sd) == list(sums), f"{what}: state_dict keys differ from the reference's"
    for k, v in sd.items():
        s1, s2 = sums[k]
        assert abs(float(v.double().sum()) - s1) <= 1e-6 * (1 + abs(s1)), f"{what}: seeded init differs: {k}"
        assert abs(float(v.double().pow(2).sum()) - s2) <= 1e-6 * (1 + abs(s2)), f"{what}: seeded init differs: {k}"


def _perturb(m, scale):
    with torch.no_grad():
        for p in m.parameters():
            p.add_(scale * torch.randn_like(p))


@functools.lru_cache(maxsize=None)
def _predictor_state():
    from vjepa2_amd.ac_predictor import vit_ac_predictor

    c = load()["cem"]
    rng = torch.get_rng_state()
    torch.manual_seed(c["weight_seed"])
    m = vit_ac_predictor(**c["pred_cfg"])
    _perturb(m, c["perturb"])
    with torch.no_grad():
        m.action_encoder.weight.mul_(c["action_gain"])
    torch.set_rng_state(rng)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    check_sums(sd, c["pred_sums"], "AC predictor")
    return sd


def predictor(device):
    """The fixture's micro AC predictor (seeded, perturbed, checked) on `device`, in eval mode."""
    from vjepa2_amd.ac_predictor import vit_ac_predictor

    m = vit_ac_predictor(**load()["cem"]["pred_cfg"])
    m.load_state_dict(_predictor_state())
    return m.to(device).eval()


def encoder(device):
    """The fixture's micro RoPE encoder (seeded, perturbed, checked) on `device`, in eval mode."""
    from functools import partial

    from vjepa2_amd import vision_transformer as vit

    e = load()["encode"]
    rng = torch.get_rng_state()
    torch.manual_seed(e["seed"])
    enc = vit.VisionTransformer(norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), **e["cfg"])
    _perturb(enc, 0.05)
    torch.set_rng_state(rng)
    check_sums(enc.state_dict(), e["enc_sums"], "encoder")
    return enc.to(device).eval()


def frames_transform(clip):
    """[1, T, H, W, C] array -> [C, T, H, W] tensor (the fixture's identity-like transform)."""
    return torch.from_numpy(np.ascontiguousarray(clip[0])).permute(3, 0, 1, 2).float()


def signature(f):
    """Parameter names and defaults of f in the fixture's plain-list form."""
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


def run_args(run):
    """mpc_args of one recorded run (cem's keyword arguments besides close_gripper)."""
    c = load()["cem"]
    return dict(c["mpc"], rollout=run["rollout"], cem_steps=run["cem_steps"], axis={a: v for a, v in run["axis"]})


class ReplayRandn:
    """Stand-in for torch.randn that hands out a run's recorded [S, 4] draws in order (on the asked device)."""

    def __init__(self, noise):
        self.draws = [d for it in noise for d in it]  # [iters, rollout, S, 4] -> the reference's call order
        self.n = 0

    def __call__(self, *shape, device=None, **kw):
        d = self.draws[self.n]
        assert tuple(shape) == tuple(d.shape), (shape, d.shape)
        self.n += 1
        return d.to(device)
