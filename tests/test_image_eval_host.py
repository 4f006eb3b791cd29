"""CPU: host logic of the frozen image-classification eval (vjepa2_amd/evals/image_classification_frozen.py):
the reference's config keys, folder and CSV format, the checkpoint's keys through the shared
save_checkpoint / load_checkpoint, the synthetic image loader's tuple, the single-GPU guard and the
reference's input_size quirk."""

import os

import pytest
import torch
import torch.nn as nn


def _args(folder, **top):
    return dict(folder=str(folder), tag="in1k-micro", **top,
                model_kwargs=dict(checkpoint="ckpt.pt",
                                  module_name="evals.image_classification_frozen.modelcustom.vit_encoder",
                                  pretrain_kwargs=dict(encoder=dict(model_name="vit_large", checkpoint_key="target_encoder")),
                                  wrapper_kwargs=dict(img_as_video_nframes=2)),
                experiment=dict(classifier=dict(num_probe_blocks=4, num_heads=16),
                                data=dict(dataset_name="ImageNet", num_classes=1000, root_path="/data",
                                          image_folder="imagenet", resolution=256, num_samples=6),
                                optimization=dict(batch_size=16, num_epochs=20, use_bfloat16=True, multihead_kwargs=[
                                    dict(lr=5e-3, start_lr=5e-3, final_lr=0.0, weight_decay=0.01,
                                         final_weight_decay=0.4, warmup=0.0),
                                    dict(lr=1e-3, start_lr=2e-4, final_lr=1e-5, weight_decay=0.1,
                                         final_weight_decay=0.1, warmup=0.5)])))


def test_config_keys(tmp_path):
    """eval.py:56-103: every key the reference reads, with its defaults."""
    from vjepa2_amd.evals import image_classification_frozen as app

    c = app.read_config(_args(tmp_path))
    assert c["val_only"] is False and c["resume_checkpoint"] is False and c["eval_tag"] == "in1k-micro"
    assert c["pretrain_folder"] == str(tmp_path) and c["checkpoint"] == "ckpt.pt" and c["module_name"] == app.IMAGE_MODULE
    assert c["args_wrapper"] == dict(img_as_video_nframes=2) and c["args_model"]["encoder"]["model_name"] == "vit_large"
    assert (c["num_probe_blocks"], c["num_heads"], c["num_classes"], c["resolution"]) == (4, 16, 1000, 256)
    assert (c["dataset_name"], c["root_path"], c["image_folder"], c["normalization"]) == ("ImageNet", "/data",
                                                                                         "imagenet", None)
    assert (c["batch_size"], c["num_epochs"], c["use_bfloat16"]) == (16, 20, True)
    assert (c["num_samples"], c["num_val_samples"]) == (6, None)
    assert c["opt_kwargs"][1] == dict(ref_wd=0.1, final_wd=0.1, start_lr=2e-4, ref_lr=1e-3, final_lr=1e-5, warmup=0.5)
    assert c["opt_kwargs"][0]["final_wd"] == 0.4 and len(c["opt_kwargs"]) == 2
    assert app.read_config(_args(tmp_path), resume_preempt=True)["resume_checkpoint"] is True
    a = _args(tmp_path, val_only=True)
    del a["experiment"]["classifier"]["num_probe_blocks"], a["experiment"]["data"]["resolution"]
    c = app.read_config(a)
    assert c["val_only"] is True and c["num_probe_blocks"] == 1 and c["resolution"] == 224


def test_folder_and_csv_format(tmp_path):
    """eval.py:121-131, 255 with src/utils/logging.py CSVLogger: image_classification_frozen/<tag>,
    log_r0.csv with the header 'epoch,loss,acc' then 'epoch,train_acc,val_acc' as %d,%.5f,%.5f."""
    from vjepa2_amd.evals import image_classification_frozen as app

    folder, log_file, latest = app.output_paths(str(tmp_path), "tag7")
    assert folder == os.path.join(str(tmp_path), "image_classification_frozen/", "tag7")
    assert log_file == os.path.join(folder, "log_r0.csv") and latest == os.path.join(folder, "latest.pt")
    assert app.output_paths(str(tmp_path), None)[0] == os.path.join(str(tmp_path), "image_classification_frozen/")
    assert not os.path.exists(folder)  # naming a path makes nothing
    os.makedirs(folder)
    log = app.CSVLog(log_file)
    log.log(1, 12.5, 50.0)
    log.log(2, -1.0, 100.0 / 3)
    assert open(log_file).read() == "epoch,loss,acc\n1,12.50000,50.00000\n2,-1.00000,33.33333\n"
    app.CSVLog(log_file)  # a restart appends a header line, as the reference's '+a' does
    assert open(log_file).read().endswith("33.33333\nepoch,loss,acc\n")


class _Opt(torch.optim.AdamW):
    arenas = ()  # what load_checkpoint touches of the arena optimizer besides the state dict


def test_checkpoint_keys_round_trip(tmp_path):
    """latest.pt through the shared save_checkpoint / load_checkpoint: the reference's keys
    (eval.py:209-216), 'module.'-prefixed classifier keys, optimizer state and mc_* group keys restored,
    val_only restoring the classifiers alone."""
    from vjepa2_amd.evals import action_anticipation_frozen as aaf
    from vjepa2_amd.evals import image_classification_frozen as app
    from vjepa2_amd.evals import probe
    from vjepa2_amd.evals import video_classification_frozen as vcf

    assert app.ProbeTrainer is vcf.ProbeTrainer  # shared, not copied
    for mod in (app, vcf, aaf):
        assert mod.init_opt is probe.init_opt and mod.save_checkpoint is probe.save_checkpoint
        assert mod.load_checkpoint is probe.load_checkpoint

    def heads(seed):
        torch.manual_seed(seed)
        cs = [nn.Linear(4, 3), nn.Linear(4, 3)]
        os_ = [_Opt(c.parameters(), lr=1e-3) for c in cs]
        for o in os_:
            o.param_groups[0].update(mc_warmup_steps=3, mc_start_lr=1e-4, mc_ref_lr=1e-3, mc_final_lr=0.0,
                                     mc_ref_wd=0.01, mc_final_wd=0.4)
        return cs, os_

    cs, os_ = heads(1)
    for c, o in zip(cs, os_):
        c(torch.randn(5, 4)).sum().backward()
        o.step()
    path = tmp_path / "latest.pt"
    probe.save_checkpoint(path, cs, os_, [None, None], 3, 16, 1)
    ck = torch.load(path, weights_only=True)
    assert set(ck) == {"classifiers", "opt", "scaler", "epoch", "batch_size", "world_size"}
    assert ck["epoch"] == 3 and ck["batch_size"] == 16 and ck["world_size"] == 1 and ck["scaler"] is None
    assert all(set(sd) == {"module.weight", "module.bias"} for sd in ck["classifiers"])
    cs2, os2 = heads(2)
    for o in os2:
        o.param_groups[0]["mc_ref_lr"] = 7.0
    *_, epoch = probe.load_checkpoint(path, cs2, os2, [None, None])
    assert epoch == 3
    assert all(torch.equal(a.weight, b.weight) for a, b in zip(cs, cs2))
    assert os2[0].param_groups[0]["mc_ref_lr"] == 1e-3 and os2[1].param_groups[0]["mc_final_wd"] == 0.4
    assert all(torch.equal(os_[0].state_dict()["state"][k]["exp_avg"], v["exp_avg"])
               for k, v in os2[0].state_dict()["state"].items())
    cs3, os3 = heads(3)
    *_, epoch = probe.load_checkpoint(path, cs3, os3, [None, None], val_only=True)
    assert epoch == 0 and torch.equal(cs3[1].bias, cs[1].bias) and os3[0].state_dict()["state"] == {}


def test_synthetic_image_dataset_tuple_and_determinism():
    """(img [3, S, S] f32, label) batched as eval.py:287 unpacks it; deterministic per index; the label
    offset of the video dataset."""
    import math

    from vjepa2_amd.evals.image_classification_frozen import SyntheticLabelledImageDataset, make_dataloader

    ds = SyntheticLabelledImageDataset(7, 16, 5)
    img, label = ds[3]
    assert img.shape == (3, 16, 16) and img.dtype == torch.float32 and isinstance(label, int) and 0 <= label < 5
    assert torch.equal(ds[3][0], img) and not torch.equal(ds[4][0], img)
    assert [ds[i][1] for i in range(7)] == [(7 * i + 3) % 5 for i in range(7)]
    g = torch.Generator().manual_seed(2003)
    assert torch.equal(img, torch.randn(3, 16, 16, generator=g) + 0.5 * math.sin(1.0 + label))
    assert not torch.equal(SyntheticLabelledImageDataset(7, 16, 5, seed_offset=1 << 20)[3][0], img)
    loader, sampler = make_dataloader(batch_size=3, num_samples=7, num_classes=5, img_size=16)
    assert len(loader) == 3  # drop_last=False
    batches = list(loader)
    imgs, labels = batches[0]
    assert imgs.shape == (3, 3, 16, 16) and labels.shape == (3,) and labels.dtype == torch.int64
    assert batches[-1][0].shape[0] == 1 and torch.equal(list(loader)[0][0], imgs)
    sampler.set_epoch(1)


def test_refuses_world_size_above_one_before_anything(monkeypatch, tmp_path):
    """The guard comes first: no config key is read (an empty config would raise otherwise), no checkpoint
    opened, no folder made. With world size 1 the eval is dispatched (and, without a device, stops at the
    device check, after the config was read)."""
    from vjepa2_amd import evals

    monkeypatch.setenv("RANK", "0")
    monkeypatch.setenv("WORLD_SIZE", "2")
    msg = (r"image_classification_frozen on the HIP path runs on one GPU \(world size 2 requested\): "
           "the multi-GPU run is not ported")
    with pytest.raises(NotImplementedError, match=msg):
        evals.main("image_classification_frozen", dict(folder=str(tmp_path)))
    with pytest.raises(NotImplementedError, match=msg):
        evals.main("evals.image_classification_frozen", _args(tmp_path))
    assert not any(tmp_path.iterdir())
    monkeypatch.setenv("WORLD_SIZE", "1")
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="needs an MI355X"):
            evals.main("image_classification_frozen", _args(tmp_path))
        assert not any(tmp_path.iterdir())


def test_input_size_quirk_and_wrapper(tmp_path, monkeypatch):
    """modelcustom/vit_encoder.py:55-59 passes input_size=resolution, which the constructor swallows: the
    built model keeps img_size 224 whatever the resolution. Non-strict load with the prefixes stripped;
    frozen, eval mode, embed_dim; any other module name refused."""
    from vjepa2_amd import vision_transformer as vit
    from vjepa2_amd.evals import image_classification_frozen as app

    def micro(patch_size=16, **kw):
        return vit.VisionTransformer(patch_size=patch_size, embed_dim=64, depth=2, num_heads=1, mlp_ratio=4,
                                     qkv_bias=True, norm_layer=lambda dim: nn.LayerNorm(dim, eps=1e-6), **kw)

    monkeypatch.setattr(vit, "vit_micro", micro, raising=False)
    torch.manual_seed(5)
    src = micro(num_frames=4, use_rope=False)
    sd = {"module.backbone." + k: v for k, v in src.state_dict().items() if k != "pos_embed"}
    ckpt = tmp_path / "pretrained.pt"
    torch.save({"target_encoder": sd}, ckpt)
    for rope in (True, False):
        enc_kw = dict(model_name="vit_micro", checkpoint_key="target_encoder", tubelet_size=2, use_rope=rope)
        m = app.init_module(module_name=app.IMAGE_MODULE, resolution=32, checkpoint=str(ckpt),
                            model_kwargs=dict(encoder=enc_kw), wrapper_kwargs=dict(img_as_video_nframes=4), device="cpu")
        assert m.model.img_height == 224 and m.model.img_width == 224 and m.model.num_frames == 4
        assert m.nframes == 4 and m.embed_dim == 64 and not m.training
        assert not any(p.requires_grad for p in m.parameters())
        assert torch.equal(m.model.blocks[1].attn.qkv.weight, src.blocks[1].attn.qkv.weight)
        assert (m.model.pos_embed is None) == rope
        if not rope:
            assert m.model.pos_embed.shape == (1, 2 * 14 * 14, 64)
        with pytest.raises(ValueError, match=r"image batch \[B, C, H, W\]"):
            m(torch.zeros(2, 3, 4, 32, 32))
    with pytest.raises(NotImplementedError, match="is ported"):
        app.init_module(module_name="evals.image_classification_frozen.modelcustom.other", resolution=32,
                        checkpoint=str(ckpt), model_kwargs=dict(encoder=enc_kw), wrapper_kwargs={}, device="cpu")
