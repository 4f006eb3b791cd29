"""GPU: the multilevel eval encoder wrapper (ClipAggregationMultilevel over VisionTransformer.forward_taps
and vj_layernorm_taps): (a) bit for bit against forward()'s list put through the reference's op sequence in
torch, (b) against the reference's recorded outputs (tests/golden/multilevel.pt), (c) the video eval's
main() end to end on a multilevel config."""

import csv
import os
import shutil

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def rel_l1(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().sum() / b.abs().sum()).item()


def _micro(**kw):
    from vjepa2_amd import vision_transformer as vit

    cfg = dict(embed_dim=64, depth=2, num_heads=1, mlp_ratio=4, qkv_bias=True,
               norm_layer=lambda dim: nn.LayerNorm(dim, eps=1e-6))
    cfg.update(kw)
    return vit.VisionTransformer(**cfg)


def _unfused(enc, pos_embed, tubelet, x, clip_indices):
    """vit_encoder_multiclip_multilevel.py:112-155 in torch on the device around forward()'s list (what the
    code before forward_taps provides), then ProbeTrainer's cat over views."""
    clips, V = len(x), len(x[0])
    B, C, Fr, H, W = x[0][0].size()
    outputs = torch.cat(enc(torch.cat([torch.cat(xi, dim=0) for xi in x], dim=0)), dim=1)
    _, N, D = outputs.size()
    T = Fr // tubelet
    S = N // T
    eff_B = B * V
    views = []
    for j in range(V):
        o = [outputs[i * eff_B:(i + 1) * eff_B][j * B:(j + 1) * B].reshape(B, T, S, D) for i in range(clips)]
        o = torch.cat(o, dim=1).flatten(1, 2)
        if pos_embed is not None and clip_indices is not None:
            pe = pos_embed.repeat(B, 1, 1)
            pe = [torch.gather(pe, 1, c[:, ::tubelet].unsqueeze(-1).repeat(1, 1, D)) for c in clip_indices]
            pe = torch.cat(pe, dim=1).unsqueeze(2).repeat(1, 1, S, 1).flatten(1, 2)
            o += pe
        views.append(o)
    return torch.cat(views, dim=0)


@pytest.mark.parametrize("use_pos", [False, True], ids=["nopos", "pos"])
@pytest.mark.parametrize("clips,V,B,layers", [(1, 1, 1, [2]), (2, 2, 2, [0, 2]), (2, 1, 3, [0, 1, 2, 3])])
def test_stacked_equals_reference_sequence_bitwise(clips, V, B, layers, use_pos):
    from vjepa2_amd.multiclip import ClipAggregationMultilevel

    torch.manual_seed(7)
    enc = _micro(img_size=32, num_frames=4, patch_size=16, tubelet_size=2, depth=4, use_rope=True, uniform_power=True,
                 out_layers=layers)
    with torch.no_grad():
        for p in enc.parameters():  # the taps share the final norm: give it non-trivial weights
            p.add_(0.05 * torch.randn_like(p))
    agg = ClipAggregationMultilevel(enc, tubelet_size=2, max_frames=16, use_pos_embed=use_pos,
                                    out_layers=layers).to(DEV).eval()
    g = torch.Generator().manual_seed(8)
    x = [[torch.randn(B, 3, 4, 32, 32, generator=g).to(DEV) for _ in range(V)] for _ in range(clips)]
    ci = [torch.randint(0, 8, (B, 4), generator=g).to(DEV) for _ in range(clips)]
    with torch.no_grad():
        want = _unfused(agg.model, agg.pos_embed, 2, x, ci)
        got, nv = agg.forward_stacked(x, ci)
        views = agg(x, ci)
    L, N = len(layers), 2 * 2 * 2
    assert nv == V and got.shape == (V * B, clips * L * N, 64) and got.dtype == torch.float32
    assert torch.isfinite(want).all()
    assert torch.equal(got, want)
    # forward(): the reference's list over views, as row-slices of one buffer
    assert len(views) == V and all(v.shape == (B, clips * L * N, 64) for v in views)
    assert all(torch.equal(v, got[j * B:(j + 1) * B]) for j, v in enumerate(views))
    base = views[0].untyped_storage().data_ptr()
    for j, v in enumerate(views):
        assert v.untyped_storage().data_ptr() == base
        assert v.data_ptr() == views[0].data_ptr() + j * B * clips * L * N * 64 * 4


@pytest.mark.parametrize("case", ["taps_0_2", "taps_1"])
def test_multilevel_matches_reference(case):
    """Against the reference's fp32 outputs, rel-L1 < 1e-2 per view: the bound test_multiclip_matches_reference
    holds the same micro encoder and path to (the reference's own bf16-autocast error is 3.1e-3 to 3.2e-3 per
    view, fixture key 'gaps'). taps_1: the last tap comes before the last block, which is not run."""
    from vjepa2_amd.multiclip import ClipAggregationMultilevel

    g = torch.load(os.path.join(GOLD, "multilevel.pt"), weights_only=True)
    c, cfg = g["cases"][case], g["cfg"]
    enc = _micro(img_size=cfg["img_size"], num_frames=cfg["num_frames"], patch_size=cfg["patch_size"],
                 tubelet_size=cfg["tubelet_size"], depth=cfg["depth"], use_rope=True, uniform_power=True,
                 out_layers=c["out_layers"])
    enc.load_state_dict({k: v.float() for k, v in g["state"].items()})
    agg = ClipAggregationMultilevel(enc, tubelet_size=2, max_frames=cfg["max_frames"], use_pos_embed=True,
                                    out_layers=c["out_layers"]).to(DEV).eval()
    assert torch.equal(agg.pos_embed.cpu(), g["pos_embed"])
    x = [[v.float().to(DEV) for v in views] for views in g["x"]]
    outs = agg(x, clip_indices=[ci.to(DEV) for ci in g["clip_indices"]])
    assert len(outs) == len(c["outs"])
    errs = [rel_l1(o, e) for o, e in zip(outs, c["outs"])]
    print(f"multilevel {case}: rel-L1 per view {errs} (reference bf16 autocast: {g['gaps'][case]})")
    for o, e, err in zip(outs, c["outs"], errs):
        assert o.shape == e.shape
        assert err < 1e-2, errs


def test_video_eval_main_multilevel_end_to_end(tmp_path, monkeypatch):
    """video_classification_frozen.main on the tiny config of tests/test_gpu_probe.py's main test with the
    multilevel module name and out_layers: two epochs, resume after the first, val_only."""
    from vjepa2_amd import evals
    from vjepa2_amd import multiclip
    from vjepa2_amd import vision_transformer as vit
    from vjepa2_amd.evals import video_classification_frozen as app

    monkeypatch.setattr(vit, "vit_micro", lambda patch_size=16, **kw: _micro(patch_size=patch_size, **kw),
                        raising=False)
    for k in ("RANK", "WORLD_SIZE", "SLURM_NTASKS"):
        monkeypatch.delenv(k, raising=False)
    enc_kw = dict(model_name="vit_micro", checkpoint_key="target_encoder", tubelet_size=2, use_rope=True,
                  uniform_power=True)
    torch.manual_seed(3)
    enc = _micro(img_size=32, num_frames=4, patch_size=16, tubelet_size=2, use_rope=True, uniform_power=True)
    ckpt = tmp_path / "pretrained.pt"
    torch.save({"target_encoder": {"module.backbone." + k: v for k, v in enc.state_dict().items()}, "epoch": 7}, ckpt)

    def args(folder, **top):
        return dict(folder=str(folder), tag="micro", num_workers=0, **top,
                    model_kwargs=dict(checkpoint=str(ckpt), module_name=app.MULTILEVEL_MODULE,
                                      pretrain_kwargs=dict(encoder=dict(enc_kw)),
                                      wrapper_kwargs=dict(max_frames=16, use_pos_embed=False, out_layers=[0, 1])),
                    experiment=dict(classifier=dict(num_probe_blocks=2, num_heads=2),
                                    data=dict(dataset_type="VideoDataset", num_classes=5, resolution=32,
                                              frames_per_clip=4, num_segments=2, num_views_per_segment=2,
                                              num_samples=6, num_val_samples=4),
                                    optimization=dict(batch_size=2, num_epochs=2, use_bfloat16=True, multihead_kwargs=[
                                        dict(lr=1e-3, start_lr=1e-4, final_lr=1e-5, weight_decay=0.01,
                                             final_weight_decay=0.1, warmup=0.5),
                                        dict(lr=3e-3, start_lr=3e-3, final_lr=0.0, weight_decay=0.2,
                                             final_weight_decay=0.2, warmup=0.0)])))

    save = app.save_checkpoint

    def save_and_keep(path, classifiers, optimizers, scalers, epoch, batch_size, world_size):
        save(path, classifiers, optimizers, scalers, epoch, batch_size, world_size)
        shutil.copy(path, f"{path}.e{epoch}")

    monkeypatch.setattr(app, "save_checkpoint", save_and_keep)
    stacked_calls = []
    fs = multiclip.ClipAggregationMultilevel.forward_stacked

    def counted(self, x, clip_indices=None):
        stacked_calls.append(len(x[0]))
        return fs(self, x, clip_indices)

    monkeypatch.setattr(multiclip.ClipAggregationMultilevel, "forward_stacked", counted)
    run1 = tmp_path / "run1"
    acc = evals.main("video_classification_frozen", args(run1))
    out1 = run1 / "video_classification_frozen" / "micro"
    assert acc == acc and 0.0 <= acc <= 100.0  # finite
    # ProbeTrainer took the stacked path: 2 epochs x (3 training iterations of 1 view + 2 validation of 2)
    assert stacked_calls == ([1] * 3 + [2] * 2) * 2
    rows = list(csv.reader(open(out1 / "log_r0.csv")))
    assert [r[0] for r in rows] == ["1", "2"] and float(rows[1][2]) == pytest.approx(acc, abs=1e-5)
    full = torch.load(out1 / "latest.pt", weights_only=True)
    assert set(full) == {"classifiers", "opt", "scaler", "epoch", "batch_size", "world_size"} and full["epoch"] == 2
    e1 = torch.load(f"{out1 / 'latest.pt'}.e1", weights_only=True)
    for a, b in zip(e1["classifiers"], full["classifiers"]):  # every head's weights moved in epoch 2
        assert not torch.equal(a["module.linear.weight"], b["module.linear.weight"])
        assert all(torch.isfinite(v).all() for v in b.values())

    # resume after epoch 1 in a fresh folder: the same final weights, bit for bit
    out2 = tmp_path / "run2" / "video_classification_frozen" / "micro"
    os.makedirs(out2)
    shutil.copy(f"{out1 / 'latest.pt'}.e1", out2 / "latest.pt")
    acc2 = evals.main("video_classification_frozen", args(tmp_path / "run2", resume_checkpoint=True))
    resumed = torch.load(out2 / "latest.pt", weights_only=True)
    assert resumed["epoch"] == 2 and acc2 == acc
    for a, b in zip(full["classifiers"], resumed["classifiers"]):
        assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)

    acc3 = evals.main("video_classification_frozen", args(run1, val_only=True, resume_checkpoint=True))
    assert acc3 == acc
    rows = list(csv.reader(open(out1 / "log_r0.csv")))
    assert len(rows) == 3 and rows[2][1] == "-1.00000"
