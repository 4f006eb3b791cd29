"""Generate tests/golden/multilevel.pt and tests/golden/image_encoder.pt by running the REFERENCE's two
remaining eval encoder wrappers on the CPU:

  * evals/video_classification_frozen/modelcustom/vit_encoder_multiclip_multilevel.py ClipAggregation
    (the Diving48 / Jester configs) around a micro encoder with out_layers;
  * evals/image_classification_frozen/modelcustom/vit_encoder.py init_module (the IN1K configs), called
    with a temporary checkpoint file and a micro factory registered in the reference's
    src.models.vision_transformer namespace at run time.

Like make_golden.py / make_golden_probe.py this executes the reference read-only (VJEPA_REFERENCE names its
checkout) and copies none of its text: the fixtures hold inputs, weights, recorded outputs and settings,
and load with torch.load(..., weights_only=True). Only ``timm.models.layers.drop_path`` is stubbed (inert:
no stochastic depth in a frozen encoder).

Every output is recorded twice: in fp32, and under ``torch.autocast("cpu", dtype=torch.bfloat16)`` (the
reference's mixed-precision branch with the device's 16-bit type). The rel-L1 between the two is printed
and stored per tensor (``gaps``): the reference's own 16-bit error, i.e. the headroom under the 1e-2
bound the HIP path (bf16 GEMM operands) is held to in tests/test_gpu_multilevel.py and
tests/test_gpu_image_eval.py.

Usage:  VJEPA_REFERENCE=<checkout> python tests/golden/make_golden_eval_encoders.py
"""

import os
import sys
import tempfile
import types

sys.dont_write_bytecode = True  # never write __pycache__ into the reference tree
REF = os.environ.get("VJEPA_REFERENCE")
if not REF:
    raise SystemExit("set VJEPA_REFERENCE to a checkout of the reference implementation")
OUT = os.path.dirname(os.path.abspath(__file__))

import torch  # noqa: E402

timm = types.ModuleType("timm")
timm_models = types.ModuleType("timm.models")
timm_layers = types.ModuleType("timm.models.layers")
timm_layers.drop_path = lambda x, drop_prob=0.0, training=False, scale_by_keep=True: x
timm.models = timm_models
timm_models.layers = timm_layers
sys.modules.update({"timm": timm, "timm.models": timm_models, "timm.models.layers": timm_layers})
sys.path.insert(0, REF)

import src.models.vision_transformer as vit  # noqa: E402

torch.set_num_threads(8)


def rel_l1(a, b):
    return ((a.double() - b.double()).abs().sum() / b.double().abs().sum()).item()


def save(name, d):
    path = os.path.join(OUT, name)
    torch.save(d, path)
    size = os.path.getsize(path)
    print(f"wrote {path} ({size / 1e3:.1f} kB)")
    assert size < 1_000_000, size
    torch.load(path, weights_only=True)  # tensors and scalars only


def _micro(**kw):
    """gen_multiclip's micro encoder (make_golden.py) with the depth and extras a case asks for."""
    cfg = dict(patch_size=16, tubelet_size=2, embed_dim=64, depth=2, num_heads=1, mlp_ratio=4, qkv_bias=True,
               uniform_power=True, norm_layer=lambda d: torch.nn.LayerNorm(d, eps=1e-6))
    cfg.update(kw)
    return vit.VisionTransformer(**cfg)


def _perturb(m, seed):
    """Non-trivial LayerNorm / bias values (the constructor leaves them at 1 / 0): the taps share one norm.
    Then every weight is rounded to bf16, so that the fixture stores it exactly in half the bytes (the
    reference runs on the rounded values; loaders widen them back to fp32)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in m.parameters():
            if p.requires_grad:
                p.add_(0.05 * torch.randn(p.shape, generator=g))
                p.copy_(p.bfloat16().float())


def _state16(m):
    """Trained tensors of a _perturb()ed model as bf16 (exact); the sincos table is a function of the shapes."""
    sd = {k: v for k, v in m.state_dict().items() if k != "pos_embed"}
    assert all(torch.equal(v.bfloat16().float(), v) for v in sd.values())
    return {k: v.bfloat16() for k, v in sd.items()}


def gen_multilevel():
    sys.path.insert(0, os.path.join(REF, "evals", "video_classification_frozen", "modelcustom"))
    from vit_encoder_multiclip_multilevel import ClipAggregation

    g = torch.Generator().manual_seed(52)
    # clips x views of B=2, bf16 values (stored exactly)
    x = [[torch.randn(2, 3, 4, 32, 32, generator=g).bfloat16().float() for _ in range(2)] for _ in range(2)]
    clip_indices = [torch.randint(0, 8, (2, 4), generator=g) for _ in range(2)]
    torch.manual_seed(51)
    enc = _micro(img_size=32, num_frames=4, depth=3, use_rope=True)
    _perturb(enc, 53)
    out = dict(cfg=dict(img_size=32, patch_size=16, num_frames=4, tubelet_size=2, embed_dim=64, depth=3, num_heads=1,
                        mlp_ratio=4, max_frames=16), state=_state16(enc), x=[[v.bfloat16() for v in xi] for xi in x],
               clip_indices=clip_indices, cases={}, gaps={})
    for name, layers in (("taps_0_2", [0, 2]), ("taps_1", [1])):
        enc.out_layers = layers
        with torch.no_grad():  # the reference copies into a leaf Parameter in its constructor
            agg = ClipAggregation(enc, tubelet_size=2, max_frames=16, use_pos_embed=True, out_layers=layers)
        with torch.no_grad():
            outs = agg([list(v) for v in x], clip_indices=clip_indices)
            with torch.autocast("cpu", dtype=torch.bfloat16):
                outs16 = agg([list(v) for v in x], clip_indices=clip_indices)
            # without clip_indices no temporal embedding is added: what the S = (L*N) // T rule is read from
            nopos = [o.float().clone() for o in agg([list(v) for v in x], clip_indices=None)]
        outs = [o.float().clone() for o in outs]
        outs16 = [o.float().clone() for o in outs16]
        gaps = [rel_l1(a, b) for a, b in zip(outs16, outs)]
        print(f"multilevel {name}: out_layers {layers}, views {[tuple(o.shape) for o in outs]}, "
              f"reference bf16-autocast vs fp32 rel-L1 per view {gaps}")
        out["cases"][name] = dict(out_layers=list(layers), outs=outs, outs_nopos=nopos,
                                  outs_bf16=[o.bfloat16() for o in outs16])
        out["gaps"][name] = gaps
        out["pos_embed"] = agg.pos_embed.detach().clone()
    save("multilevel.pt", out)


def gen_image_encoder():
    import evals.image_classification_frozen.modelcustom.vit_encoder as mod

    g = torch.Generator().manual_seed(62)
    imgs = torch.randn(2, 3, 32, 32, generator=g)
    # one set of trained tensors for both variants (RoPE has no parameters; the sincos table is not trained)
    torch.manual_seed(61)
    src = _micro(num_frames=4, use_rope=True)  # img_size stays at the constructor's 224, as init_module's model
    _perturb(src, 63)
    state16 = _state16(src)
    state = {k: v.float() for k, v in state16.items()}
    # the factory init_module looks up by name in the reference's vision_transformer namespace
    mod.vit.vit_micro = lambda patch_size=16, **kw: _micro(patch_size=patch_size, **kw)
    out = dict(cfg=dict(resolution=32, img_as_video_nframes=4, patch_size=16, tubelet_size=2, embed_dim=64, depth=2,
                        num_heads=1, mlp_ratio=4), imgs=imgs, state=state16, variants={}, gaps={})
    for name, rope in (("rope", True), ("sincos", False)):
        enc_kw = dict(model_name="vit_micro", checkpoint_key="target_encoder", tubelet_size=2, use_rope=rope)
        with tempfile.TemporaryDirectory() as td:
            ckpt = os.path.join(td, "pretrained.pt")
            torch.save({"target_encoder": {"module.backbone." + k: v for k, v in state.items()}}, ckpt)
            model = mod.init_module(resolution=32, checkpoint=ckpt, model_kwargs=dict(encoder=dict(enc_kw)),
                                    wrapper_kwargs=dict(img_as_video_nframes=4))
        model.eval()
        assert model.img_height == 224, model.img_height  # input_size is swallowed: the quirk under test
        with torch.no_grad():
            y = model(imgs).float().clone()
            with torch.autocast("cpu", dtype=torch.bfloat16):
                y16 = model(imgs).float().clone()
        gap = rel_l1(y16, y)
        print(f"image encoder {name}: out {tuple(y.shape)}, reference bf16-autocast vs fp32 rel-L1 {gap}")
        out["variants"][name] = dict(use_rope=rope, out=y, out_bf16=y16.bfloat16())
        out["gaps"][name] = gap
    save("image_encoder.pt", out)


if __name__ == "__main__":
    gen_multilevel()
    gen_image_encoder()
