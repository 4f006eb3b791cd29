"""GPU: the frozen image-classification eval (vjepa2_amd/evals/image_classification_frozen.py): its encoder
wrapper against the reference's recorded outputs (tests/golden/image_encoder.pt), the image repeat, and
main() end to end with resume."""

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


def _micro(patch_size=16, **kw):
    from vjepa2_amd import vision_transformer as vit

    cfg = dict(embed_dim=64, depth=2, num_heads=1, mlp_ratio=4, qkv_bias=True, uniform_power=True,
               norm_layer=lambda dim: nn.LayerNorm(dim, eps=1e-6))
    cfg.update(kw)
    return vit.VisionTransformer(patch_size=patch_size, **cfg)


def _encoder(tmp_path, monkeypatch, rope, state):
    from vjepa2_amd import vision_transformer as vit
    from vjepa2_amd.evals import image_classification_frozen as app

    monkeypatch.setattr(vit, "vit_micro", _micro, raising=False)
    ckpt = tmp_path / f"pretrained_{int(rope)}.pt"
    torch.save({"target_encoder": {"module.backbone." + k: v for k, v in state.items()}}, ckpt)
    enc_kw = dict(model_name="vit_micro", checkpoint_key="target_encoder", tubelet_size=2, use_rope=rope)
    return app.init_module(module_name=app.IMAGE_MODULE, resolution=32, checkpoint=str(ckpt),
                           model_kwargs=dict(encoder=enc_kw), wrapper_kwargs=dict(img_as_video_nframes=4), device=DEV)


@pytest.mark.parametrize("variant", ["rope", "sincos"])
def test_image_encoder_matches_reference(tmp_path, monkeypatch, variant):
    """rel-L1 < 1e-2 against the reference's fp32 output of its own init_module (resolution 32 on a model
    that keeps img_size 224; the sincos variant interpolates its 14x14 table to 2x2). The reference's own
    bf16-autocast error on these tensors is 3.9e-3 / 4.0e-3 (fixture key 'gaps'). And forward(imgs) is the
    encoder on the image repeated along time, bit for bit."""
    g = torch.load(os.path.join(GOLD, "image_encoder.pt"), weights_only=True)
    v = g["variants"][variant]
    m = _encoder(tmp_path, monkeypatch, v["use_rope"], {k: t.float() for k, t in g["state"].items()})
    assert m.model.img_height == 224 and m.embed_dim == 64
    imgs = g["imgs"].to(DEV)
    with torch.no_grad():
        y = m(imgs)
        rep = m.model(imgs.unsqueeze(2).repeat(1, 1, 4, 1, 1))
    assert y.shape == v["out"].shape and y.dtype == torch.float32
    assert torch.equal(y, rep)
    err = rel_l1(y, v["out"])
    print(f"image encoder {variant}: rel-L1 {err} (reference bf16 autocast: {g['gaps'][variant]})")
    assert err < 1e-2, err


def test_image_eval_main_end_to_end(tmp_path, monkeypatch):
    """main() on the synthetic images: CSV with the reference's header, latest.pt with its keys, the heads
    learn something, resume after epoch 1 continues the schedules where the uninterrupted run had them (per-
    head LR and WD of every resumed iteration, the first included) and ends at the same weights; val_only."""
    from vjepa2_amd import evals
    from vjepa2_amd import vision_transformer as vit
    from vjepa2_amd.evals import image_classification_frozen as app
    from vjepa2_amd.evals import video_classification_frozen as vcf

    for k in ("RANK", "WORLD_SIZE", "SLURM_NTASKS"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(vit, "vit_micro", _micro, raising=False)
    torch.manual_seed(3)
    enc = _micro(num_frames=4, use_rope=True)
    ckpt = tmp_path / "pretrained.pt"
    torch.save({"target_encoder": {"module.backbone." + k: v for k, v in enc.state_dict().items()}, "epoch": 7}, ckpt)
    enc_kw = dict(model_name="vit_micro", checkpoint_key="target_encoder", tubelet_size=2, use_rope=True)

    def args(folder, **top):
        return dict(folder=str(folder), tag="micro", num_workers=0, **top,
                    model_kwargs=dict(checkpoint=str(ckpt), module_name=app.IMAGE_MODULE,
                                      pretrain_kwargs=dict(encoder=dict(enc_kw)),
                                      wrapper_kwargs=dict(img_as_video_nframes=4)),
                    experiment=dict(classifier=dict(num_probe_blocks=2, num_heads=2),
                                    data=dict(dataset_name="ImageNet", num_classes=5, resolution=32, num_samples=6,
                                              num_val_samples=4),
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
    sched = []
    step = vcf.ProbeTrainer.train_step

    def recorded(self, clips, clip_indices, labels):
        r = step(self, clips, clip_indices, labels)
        sched.append((list(self.last_lr), list(self.last_wd)))
        return r

    monkeypatch.setattr(vcf.ProbeTrainer, "train_step", recorded)

    run1 = tmp_path / "run1"
    acc = evals.main("image_classification_frozen", args(run1))
    out1 = run1 / "image_classification_frozen" / "micro"
    assert acc == acc and 0.0 <= acc <= 100.0
    lines = open(out1 / "log_r0.csv").read().splitlines()
    assert lines[0] == "epoch,loss,acc" and len(lines) == 3 and [ln.split(",")[0] for ln in lines[1:]] == ["1", "2"]
    assert float(lines[2].split(",")[2]) == pytest.approx(acc, abs=1e-5)
    full = torch.load(out1 / "latest.pt", weights_only=True)
    assert set(full) == {"classifiers", "opt", "scaler", "epoch", "batch_size", "world_size"}
    assert full["epoch"] == 2 and full["batch_size"] == 2 and full["world_size"] == 1 and len(full["scaler"]) == 2
    assert all(float(s["step"]) == 6.0 for o in full["opt"] for s in o["state"].values())  # 2 epochs x ipe 3
    e1 = torch.load(f"{out1 / 'latest.pt'}.e1", weights_only=True)
    for a, b in zip(e1["classifiers"], full["classifiers"]):
        assert not torch.equal(a["module.linear.weight"], b["module.linear.weight"])
    uninterrupted = list(sched)
    assert len(uninterrupted) == 6
    assert uninterrupted[0][0][0] != uninterrupted[3][0][0]  # head 0: the schedule is not constant

    del sched[:]
    out2 = tmp_path / "run2" / "image_classification_frozen" / "micro"
    os.makedirs(out2)
    shutil.copy(f"{out1 / 'latest.pt'}.e1", out2 / "latest.pt")
    acc2 = evals.main("image_classification_frozen", args(tmp_path / "run2", resume_checkpoint=True))
    assert sched == uninterrupted[3:]  # LR and WD per head, from the first resumed iteration on
    resumed = torch.load(out2 / "latest.pt", weights_only=True)
    assert resumed["epoch"] == 2 and acc2 == acc
    for a, b in zip(full["classifiers"], resumed["classifiers"]):
        assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    assert open(out2 / "log_r0.csv").read().splitlines()[0] == "epoch,loss,acc"

    acc3 = evals.main("image_classification_frozen", args(run1, val_only=True, resume_checkpoint=True))
    assert acc3 == acc
    lines = open(out1 / "log_r0.csv").read().splitlines()
    assert lines[-1].split(",")[:2] == ["1", "-1.00000"]  # val_only starts at epoch 0 (eval.py:334-336)
