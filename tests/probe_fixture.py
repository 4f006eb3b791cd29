"""Shared loader of tests/golden/probe_steps.pt (written by tests/golden/make_golden_probe.py).

The fixture does not store the three classifiers' initial weights (size: see the generator's
docstring); they are rebuilt here from cfg["init_seed"] with this project's AttentiveClassifier, whose
constructor draws in the reference's order, followed by the generator's perturbation draws, and
checked against the per-tensor (sum, sum of squares) the reference's weights had."""

import functools
import os

import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@functools.lru_cache(maxsize=None)
def load():
    return torch.load(os.path.join(GOLD, "probe_steps.pt"), weights_only=True)


def classifier(cfg):
    from vjepa2_amd.attentive_pooler import AttentiveClassifier

    return AttentiveClassifier(embed_dim=cfg["embed_dim"], num_heads=cfg["num_heads"], depth=cfg["depth"],
                               mlp_ratio=cfg["mlp_ratio"], num_classes=cfg["num_classes"],
                               use_activation_checkpointing=True)


@functools.lru_cache(maxsize=None)
def _init_states():
    d = load()
    cfg = d["cfg"]
    rng = torch.get_rng_state()
    torch.manual_seed(cfg["init_seed"])
    states = []
    for sums in d["init_sums"]:
        m = classifier(cfg)
        with torch.no_grad():
            for p in m.parameters():
                p.add_(0.05 * torch.randn_like(p))
        sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
        assert list(sd) == list(sums), "state_dict keys differ from the reference's"
        for k, v in sd.items():
            s1, s2 = sums[k]
            # equal up to float rounding of the init kernels on another host CPU
            assert abs(float(v.double().sum()) - s1) <= 1e-6 * (1 + abs(s1)), f"seeded init differs: {k}"
            assert abs(float(v.double().pow(2).sum()) - s2) <= 1e-6 * (1 + abs(s2)), f"seeded init differs: {k}"
        states.append(sd)
    torch.set_rng_state(rng)
    return states


def init_states():
    """Fresh copies of the three classifiers' initial state_dict()s."""
    return [{k: v.clone() for k, v in sd.items()} for sd in _init_states()]


def opt_kwargs(d):
    """eval.py:98-108: multihead_kwargs -> init_opt's opt_kwargs."""
    return [dict(ref_wd=k["weight_decay"], final_wd=k["final_weight_decay"], start_lr=k["start_lr"], ref_lr=k["lr"],
                 final_lr=k["final_lr"], warmup=k["warmup"]) for k in d["multihead_kwargs"]]
