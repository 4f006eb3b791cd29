"""CPU: the host side of V-JEPA 2-AC post-training (vjepa2_amd.droid, schedulers.WSDSchedule): schedules, the
optimizer's group layout, the app's refusals, the synthetic data set and the config parsing, against
tests/golden/droid_steps.pt (the reference's app on a micro model) where it has a recording."""

import os
import types

import pytest
import torch

import droid_fixture as fx

# the reference's configs/train/vitg16/droid-256px-8f.yaml, stored as it is (settings only)
REF_CFG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "droid-256px-8f.yaml")

# configs/train/vitg16/droid-256px-8f.yaml: the training keys, restated (not the SLURM sizing or the paths)
DROID_256_8F = dict(
    app="vjepa_droid",
    data=dict(batch_size=8, camera_views=["left_mp4_path"], crop_size=256, dataset_fpcs=[8], fps=4, patch_size=16,
              pin_mem=True, stereo_view=False, tubelet_size=2),
    data_aug=dict(auto_augment=False, horizontal_flip=False, motion_shift=False,
                  random_resize_aspect_ratio=[0.75, 1.35], random_resize_scale=[1.777, 1.777], reprob=0.0),
    loss=dict(auto_steps=2, loss_exp=1.0, normalize_reps=True, reg_coeff=0.0),
    meta=dict(dtype="bfloat16", eval_freq=100, resume_checkpoint=None, load_predictor=False,
              context_encoder_key="target_encoder", target_encoder_key="target_encoder", save_every_freq=25, seed=239,
              use_sdpa=True),
    model=dict(model_name="vit_giant_xformers", pred_depth=24, pred_embed_dim=1024, pred_is_frame_causal=True,
               pred_num_heads=16, uniform_power=True, use_activation_checkpointing=True, use_extrinsics=False,
               use_rope=True),
    optimization=dict(anneal=15, epochs=315, final_lr=0.0, final_weight_decay=0.04, ipe=300, lr=0.000425,
                      start_lr=0.000075, warmup=15, weight_decay=0.04),
)


def _groups(n=1, **extra):
    return types.SimpleNamespace(param_groups=[dict(extra) for _ in range(n)])


def test_wsd_schedule_crosses_both_phase_boundaries():
    """warmup 2, anneal 2, T_max 8 (4 stable steps), by hand: the warmup's last step is already the reference
    rate (step < warmup_steps is strict), the anneal's first step still is (progress 0)."""
    from vjepa2_amd.schedulers import WSDSchedule

    opt = _groups(2)
    opt.param_groups[1]["lr_scale"] = 0.5
    s = WSDSchedule(opt, warmup_steps=2, anneal_steps=2, T_max=8, start_lr=0.1, ref_lr=0.5, final_lr=0.1)
    want = [0.1 + 0.5 * 0.4, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5 + 0.5 * (0.1 - 0.5), 0.5 + 1.0 * (0.1 - 0.5)]
    for w in want:
        got = s.step()
        assert abs(got - w) <= 1e-12, (got, w)
        assert opt.param_groups[0]["lr"] == got and opt.param_groups[1]["lr"] == got * 0.5  # step() returns unscaled
    assert abs(want[0] - 0.3) < 1e-12 and abs(want[-2] - 0.3) < 1e-12 and abs(want[-1] - 0.1) < 1e-12


@pytest.mark.parametrize("name", ["a", "b"])
def test_schedules_reproduce_the_reference_recording(name):
    from vjepa2_amd.schedulers import CosineWDSchedule, WSDSchedule

    run = fx.load()["runs"][name]
    co = run["args"]["optimization"]
    ipe = co["ipe"]
    opt = _groups(1)
    s = WSDSchedule(opt, warmup_steps=int(co["warmup"] * ipe), anneal_steps=int(co["anneal"] * ipe),
                    T_max=int(co["epochs"] * ipe), start_lr=co["start_lr"], ref_lr=co["lr"], final_lr=co["final_lr"])
    w = CosineWDSchedule(opt, ref_wd=co["weight_decay"], final_wd=co["final_weight_decay"],
                         T_max=int(co["epochs"] * ipe))
    lrs = [st["lr"] for st in run["steps"]]
    assert len(set(lrs)) == 3  # the recording itself crosses warmup -> reference rate -> anneal
    for st in run["steps"]:
        assert abs(s.step() - st["lr"]) <= 1e-12
        assert abs(w.step() - st["wd"]) <= 1e-12


@pytest.mark.parametrize("name", ["a", "b"])
def test_init_opt_group_layout_equals_the_reference(name, monkeypatch):
    """The four groups of the reference's AdamW (encoder wd, predictor wd, encoder no-wd, predictor no-wd): sizes,
    keys and flags as recorded from its state_dict(); no state before a step. The arenas' bf16 shadow cast is
    the only device call of init_opt; it is replaced by torch's for this host-side check."""
    from vjepa2_amd import droid, ops

    monkeypatch.setattr(ops, "cast_bf16", lambda x, out=None: x.to(torch.bfloat16) if out is None else out.copy_(x))
    run = fx.load()["runs"][name]
    enc, pred = fx.models(name, "cpu")
    co = run["args"]["optimization"]
    opt, scaler, sched, wds = droid.init_opt(encoder=enc, predictor=pred, iterations_per_epoch=co["ipe"],
                                             start_lr=co["start_lr"], ref_lr=co["lr"], warmup=co["warmup"],
                                             anneal=co["anneal"], num_epochs=co["epochs"], wd=co["weight_decay"],
                                             final_wd=co["final_weight_decay"], final_lr=co["final_lr"])
    assert scaler is None and type(sched).__name__ == "WSDSchedule" and type(wds).__name__ == "CosineWDSchedule"
    sd = opt.state_dict()
    rec = run["opt"]
    assert [len(g["params"]) for g in sd["param_groups"]] == rec["group_sizes"]
    assert [sorted(k for k in g if k != "params") for g in sd["param_groups"]] == rec["group_keys"]
    assert [{k: g[k] for k in ("lr_scale", "WD_exclude") if k in g} for g in sd["param_groups"]] == rec["group_flags"]
    flat = [i for g in sd["param_groups"] for i in g["params"]]
    assert flat == list(range(sum(rec["group_sizes"]))) and sd["state"] == {}
    # the recorded state belongs to predictor groups only, never to the encoder's
    n0, n1, n2, n3 = rec["group_sizes"]
    pred_ids = set(range(n0, n0 + n1)) | set(range(n0 + n1 + n2, n0 + n1 + n2 + n3))
    assert set(rec["state_ids"]) <= pred_ids and len(rec["state_ids"]) > 0
    sched.step(), wds.step()
    assert [g["weight_decay"] for g in opt.param_groups[2:]] == [0.0, 0.0]  # the excluded groups stay undecayed
    assert [g["weight_decay"] for g in opt.param_groups[:2]] == [run["steps"][0]["wd"]] * 2


def _micro_args(tmp_path, **data_aug):
    run = fx.load()["runs"]["a"]
    args = {k: dict(v) if isinstance(v, dict) else v for k, v in run["args"].items()}
    args["folder"] = str(tmp_path / "out")
    args["data_aug"].update(data_aug)
    return args


def test_main_refuses_world_size_above_one(monkeypatch, tmp_path):
    from vjepa2_amd import droid

    monkeypatch.setenv("RANK", "0")
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError, match="one GPU"):
        droid.main(_micro_args(tmp_path))
    assert not any(tmp_path.iterdir())  # refused before anything is written
    with pytest.raises(NotImplementedError, match="one GPU"):
        droid.ACTrainer(None, None, None, 4, world_size=2)


@pytest.mark.parametrize("aug", [dict(auto_augment=True), dict(motion_shift=True), dict(reprob=0.25),
                                 dict(horizontal_flip=True)])
def test_main_refuses_unsupported_data_aug(aug, monkeypatch, tmp_path):
    from vjepa2_amd import droid

    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(NotImplementedError, match=next(iter(aug))):
        droid.main(_micro_args(tmp_path, **aug))
    assert not any(tmp_path.iterdir())


def test_main_and_init_video_model_refuse_a_predictor_without_rope(monkeypatch, tmp_path):
    from vjepa2_amd import droid

    monkeypatch.delenv("WORLD_SIZE", raising=False)
    args = _micro_args(tmp_path)
    args["model"]["use_rope"] = False
    with pytest.raises(NotImplementedError, match="use_rope"):
        droid.main(args)
    with pytest.raises(NotImplementedError, match="use_rope"):
        droid.init_video_model(device="cpu", model_name="vit_tiny", use_rope=False)


def test_synthetic_dataset_shapes_and_actions():
    from vjepa2_amd.droid import SyntheticDroidDataset
    from vjepa2_amd.planning import poses_to_diff

    T, S = 5, 32
    ds = SyntheticDroidDataset(7, T, S, seed=11)
    assert len(ds) == 7
    clip, actions, states, extrinsics = ds[3]
    assert (clip.shape, actions.shape, states.shape, extrinsics.shape) == ((3, T, S, S), (T - 1, 7), (T, 7), (T, 6))
    assert all(t.dtype == torch.float32 for t in (clip, actions, states, extrinsics))
    assert bool((states[:, 6] >= 0).all()) and bool((states[:, 6] <= 1).all())
    for t in range(T - 1):
        want = poses_to_diff(states[t].double(), states[t + 1].double()).float()
        assert torch.equal(actions[t], want)
    again = ds[3]
    assert all(torch.equal(x, y) for x, y in zip(again, (clip, actions, states, extrinsics)))  # seeded per index
    assert not torch.equal(ds[4][0], clip)
    fx.batches("a")  # and the draws are the ones the reference's recording was made on


def test_droid_config_parses_into_the_trainers_settings():
    from vjepa2_amd import droid, main as vmain

    ref = vmain.load_params(REF_CFG)  # pin every restated value against the file itself
    for k, v in DROID_256_8F.items():
        if isinstance(v, dict):
            for kk, vv in v.items():
                assert ref[k][kk] == vv, (k, kk, ref[k][kk], vv)
            extra = set(ref[k]) - set(v) - {"datasets", "num_workers", "pretrain_checkpoint"}
            assert not extra, (k, extra)
        else:
            assert ref[k] == v
    assert droid.settings(ref).model == droid.settings(dict(DROID_256_8F)).model  # the file itself parses the same
    args = {k: dict(v) if isinstance(v, dict) else v for k, v in DROID_256_8F.items()}
    args["folder"] = "/nowhere"
    args["meta"]["pretrain_checkpoint"] = "vitg.pt"
    c = droid.settings(args)
    assert (c.batch_size, c.max_num_frames, c.crop_size, c.patch_size, c.tubelet_size) == (8, 8, 256, 16, 2)
    assert c.tokens_per_frame == 256 and c.auto_steps == 2 and c.loss_exp == 1.0 and c.normalize_reps is True
    assert c.mixed_precision is True and c.shared_encoder is True and c.load_predictor is False and c.load_encoder
    assert (c.context_encoder_key, c.target_encoder_key, c.p_file, c.r_file) == ("target_encoder", "target_encoder",
                                                                                  "vitg.pt", None)
    assert (c.ipe, c.num_epochs, c.warmup, c.anneal) == (300, 315, 15, 15)
    assert (c.start_lr, c.lr, c.final_lr, c.wd, c.final_wd) == (0.000075, 0.000425, 0.0, 0.04, 0.04)
    assert c.enc_lr_scale == 1.0 and tuple(c.betas) == (0.9, 0.999) and c.eps == 1e-8 and c.seed == 239
    assert c.save_every_freq == 25
    m = c.model
    assert (m["model_name"], m["pred_depth"], m["pred_embed_dim"], m["pred_num_heads"]) == ("vit_giant_xformers", 24,
                                                                                            1024, 16)
    assert m["use_rope"] and m["uniform_power"] and m["use_sdpa"] and m["pred_is_frame_causal"]
    assert not m["use_extrinsics"] and m["use_activation_checkpointing"] is True  # accepted, and ignored
    assert m["max_num_frames"] == 16 and m["action_embed_dim"] == 7  # the mask's capacity: 8 doubled frames
    droid.check_data_aug(args["data_aug"])  # the config's own values pass
    # auto_steps is capped by the clip length, as in the reference
    args["loss"]["auto_steps"] = 99
    assert droid.settings(args).auto_steps == 8
