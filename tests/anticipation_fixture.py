"""Shared loader of tests/golden/anticipation_steps.pt (written by tests/golden/make_golden_anticipation.py).

The fixture stores no weights (size: see the generator's docstring). The three classifiers, the action-only
classifier, and the wrapper's encoder and predictor are rebuilt here from the recorded seeds with this
project's classes, whose constructors draw in the reference's order, followed by the generator's perturbation
draws, and checked against the per-tensor (sum, sum of squares) the reference's weights had."""

import functools
import os

import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HEADS = ("verb", "noun", "action")


@functools.lru_cache(maxsize=None)
def load():
    return torch.load(os.path.join(GOLD, "anticipation_steps.pt"), weights_only=True)


def classifier(cfg, action_only=False):
    from vjepa2_amd.evals.action_anticipation_frozen import AttentiveClassifier

    rng = lambda n: {i: i for i in range(n)}  # noqa: E731
    return AttentiveClassifier(verb_classes={} if action_only else rng(cfg["verbs"]),
                               noun_classes={} if action_only else rng(cfg["nouns"]),
                               action_classes=rng(cfg["actions"]), embed_dim=cfg["embed_dim"],
                               num_heads=cfg["num_heads"], depth=cfg["depth"], use_activation_checkpointing=True,
                               mlp_ratio=cfg["mlp_ratio"])


def perturb(m):
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.05 * torch.randn_like(p))


def check_sums(sd, sums, what):
    assert list(sd) == list(sums), f"{what}: state_dict keys differ from the reference's"
    for k, v in sd.items():
        s1, s2 = sums[k]
        # equal up to float rounding of the init kernels on another host CPU
        assert abs(float(v.double().sum()) - s1) <= 1e-6 * (1 + abs(s1)), f"{what}: seeded init differs: {k}"
        assert abs(float(v.double().pow(2).sum()) - s2) <= 1e-6 * (1 + abs(s2)), f"{what}: seeded init differs: {k}"


@functools.lru_cache(maxsize=None)
def _init_states():
    p = load()["probe"]
    cfg = p["cfg"]
    rng = torch.get_rng_state()
    torch.manual_seed(cfg["init_seed"])
    states = []
    for i, sums in enumerate(p["init_sums"]):
        m = classifier(cfg)
        perturb(m)
        sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
        check_sums(sd, sums, f"classifier {i}")
        states.append(sd)
    torch.set_rng_state(rng)
    return states


def init_states():
    """Fresh copies of the three classifiers' initial state_dict()s."""
    return [{k: v.clone() for k, v in sd.items()} for sd in _init_states()]


def action_only_classifier():
    """The seeded action-only classifier (no perturbation), checked against the reference's sums."""
    p = load()["probe"]
    rng = torch.get_rng_state()
    torch.manual_seed(p["cfg"]["init_seed"] + 1)
    m = classifier(p["cfg"], action_only=True)
    torch.set_rng_state(rng)
    check_sums(m.state_dict(), p["action_only_sums"], "action-only classifier")
    return m


def opt_kwargs(p):
    """eval.py:116-126: multihead_kwargs -> init_opt's opt_kwargs."""
    return [dict(ref_wd=k["weight_decay"], final_wd=k["final_weight_decay"], start_lr=k["start_lr"], ref_lr=k["lr"],
                 final_lr=k["final_lr"], warmup=k["warmup"]) for k in p["multihead_kwargs"]]


def wrapper_models():
    """(encoder, predictor) of fixture (a) on the CPU: seeded, perturbed, checked."""
    from functools import partial

    from vjepa2_amd import predictor as vpred
    from vjepa2_amd import vision_transformer as vit

    w = load()["wrapper"]
    c = w["cfg"]
    rng = torch.get_rng_state()
    torch.manual_seed(c["seed"])
    enc = vit.VisionTransformer(img_size=c["img_size"], patch_size=c["patch_size"], num_frames=c["clip_frames"],
                                tubelet_size=c["tubelet_size"], embed_dim=c["embed_dim"], depth=c["enc_depth"],
                                num_heads=c["num_heads"], mlp_ratio=c["mlp_ratio"], qkv_bias=True, use_rope=True,
                                uniform_power=True, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6))
    pred = vpred.vit_predictor(img_size=c["img_size"], patch_size=c["patch_size"], num_frames=c["pred_frames"],
                               tubelet_size=c["tubelet_size"], embed_dim=c["embed_dim"],
                               predictor_embed_dim=c["pred_embed_dim"], depth=c["pred_depth"], num_heads=c["num_heads"],
                               uniform_power=True, use_mask_tokens=True, num_mask_tokens=c["num_mask_tokens"],
                               zero_init_mask_tokens=False, use_rope=True)
    perturb(enc)
    perturb(pred)
    torch.set_rng_state(rng)
    check_sums(enc.state_dict(), w["enc_sums"], "encoder")
    check_sums(pred.state_dict(), w["pred_sums"], "predictor")
    return enc.eval(), pred.eval()
