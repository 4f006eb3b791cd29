"""Shared loader of tests/golden/droid_steps.pt (written by tests/golden/make_golden_droid.py).

The fixture stores no initial weights and no clips: the micro encoder and AC predictor are rebuilt here from the
recorded seed with this project's classes (whose constructors draw in the reference's order), followed by the
generator's perturbation draws, and checked against the per-tensor (sum, sum of squares) the reference's weights
had; clips are redrawn from their item seeds by vjepa2_amd.droid.SyntheticDroidDataset and checked against the
recorded batch sums, actions, states and extrinsics."""

import functools
import os
from functools import partial

import torch

from planning_fixture import check_sums

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@functools.lru_cache(maxsize=None)
def load():
    return torch.load(os.path.join(GOLD, "droid_steps.pt"), weights_only=True)


def vit_micro(patch_size=16, **kw):
    """The fixture's encoder factory (registered as vision_transformer.vit_micro by the tests that go through
    init_video_model)."""
    from vjepa2_amd import vision_transformer as vt

    return vt.VisionTransformer(patch_size=patch_size, qkv_bias=True, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6),
                                **load()["micro"]["enc"], **kw)


def pred_kwargs(run):
    m = load()["micro"]
    return dict(img_size=m["crop"], patch_size=m["patch"], num_frames=2 * m["fpc"], tubelet_size=m["tubelet"],
                embed_dim=m["enc"]["embed_dim"], predictor_embed_dim=64, depth=2, num_heads=2, uniform_power=True,
                use_rope=True, is_frame_causal=True, use_extrinsics=run["cfg"]["use_extrinsics"])


@functools.lru_cache(maxsize=None)
def _states(name):
    """(encoder state_dict, predictor state_dict) of run `name`: the generator's temporary checkpoint."""
    from vjepa2_amd.ac_predictor import vit_ac_predictor

    f = load()
    m, run = f["micro"], f["runs"][name]
    rng = torch.get_rng_state()
    torch.manual_seed(m["weight_seed"])
    enc = vit_micro(img_size=m["crop"], num_frames=2 * m["fpc"], tubelet_size=m["tubelet"], uniform_power=True,
                    use_rope=True)
    pred = vit_ac_predictor(**pred_kwargs(run))
    with torch.no_grad():
        for mod in (enc, pred):
            for p in mod.parameters():
                p.add_(m["perturb"] * torch.randn_like(p))
    torch.set_rng_state(rng)
    esd = {k: v.detach().clone() for k, v in enc.state_dict().items()}
    psd = {k: v.detach().clone() for k, v in pred.state_dict().items()}
    check_sums(esd, run["enc_sums"], "encoder")
    check_sums(psd, run["pred_sums"], "AC predictor")
    return esd, psd


def checkpoint(name, path):
    """Write run `name`'s pre-trained micro checkpoint (what the reference's load_pretrained was fed) to `path`."""
    esd, psd = _states(name)
    pre = lambda sd: {"module.backbone." + k: v.clone() for k, v in sd.items()}  # noqa: E731
    torch.save({"epoch": 0, "target_encoder": pre(esd), "predictor": pre(psd)}, path)
    return path


def models(name, device):
    """(encoder, predictor) of run `name` with the fixture's weights, on `device`."""
    from vjepa2_amd.ac_predictor import vit_ac_predictor

    f = load()
    m, run = f["micro"], f["runs"][name]
    esd, psd = _states(name)
    enc = vit_micro(img_size=m["crop"], num_frames=2 * m["fpc"], tubelet_size=m["tubelet"], uniform_power=True,
                    use_rope=True)
    pred = vit_ac_predictor(**pred_kwargs(run))
    enc.load_state_dict(esd)
    pred.load_state_dict(psd)
    return enc.to(device), pred.to(device)


@functools.lru_cache(maxsize=None)
def batches(name):
    """The run's recorded batches as (clips, actions, states, extrinsics) CPU tensors: clips redrawn, the rest as
    recorded (the reference's scipy pose differences), after checking that the data set draws the same."""
    from vjepa2_amd.droid import SyntheticDroidDataset

    f = load()
    m = f["micro"]
    ds = SyntheticDroidDataset(1000, m["fpc"], m["crop"], seed=m["data_seed"])
    out = []
    for b in f["runs"][name]["batches"]:
        items = [ds[i] for i in b["items"]]
        clips = torch.stack([it[0] for it in items])
        s = float(clips.double().sum())
        assert abs(s - b["clip_sum"]) <= 1e-9 * (1 + abs(b["clip_sum"])), "the data set's clips differ"
        assert torch.equal(torch.stack([it[2] for it in items]), b["states"])
        assert torch.equal(torch.stack([it[3] for it in items]), b["extrinsics"])
        # numpy pose differences against scipy's: f64 results rounded to f32, angles below 1 in magnitude
        assert (torch.stack([it[1] for it in items]) - b["actions"]).abs().max().item() <= 2.0**-23
        out.append((clips, b["actions"], b["states"], b["extrinsics"]))
    return out
