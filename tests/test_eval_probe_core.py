"""CPU: the core the three frozen-probe evals share (vjepa2_amd/evals/probe.py) and
distributed.env_world_size: the common config keys under each eval's own reader, the output paths, resume's
scheduler replay, the host-side label check and the launcher's world size."""

import os

import pytest
import torch
import torch.nn as nn

_MULTIHEAD = [dict(lr=5e-3, start_lr=5e-3, final_lr=0.0, weight_decay=0.01, final_weight_decay=0.4, warmup=0.0),
              dict(lr=1e-3, start_lr=2e-4, final_lr=1e-5, weight_decay=0.1, final_weight_decay=0.1, warmup=0.5)]
_OPT_KWARGS = [dict(ref_wd=0.01, final_wd=0.4, start_lr=5e-3, ref_lr=5e-3, final_lr=0.0, warmup=0.0),
               dict(ref_wd=0.1, final_wd=0.1, start_lr=2e-4, ref_lr=1e-3, final_lr=1e-5, warmup=0.5)]


def _minimal(data, **top):
    """The least an eval's reader accepts: every section present, no optional key. num_workers is given at
    both places a reader may look for it."""
    return dict(folder="/out", num_workers=3, **top,
                model_kwargs=dict(checkpoint="ckpt.pt", module_name="m", pretrain_kwargs=dict(encoder={}),
                                  wrapper_kwargs=dict(w=1)),
                experiment=dict(classifier={}, data=dict(num_workers=5, **data),
                                optimization=dict(batch_size=4, num_epochs=2, use_bfloat16=True,
                                                  multihead_kwargs=_MULTIHEAD)))


def test_common_config_keys_under_each_eval():
    from vjepa2_amd.evals import action_anticipation_frozen as aaf
    from vjepa2_amd.evals import image_classification_frozen as icf
    from vjepa2_amd.evals import probe
    from vjepa2_amd.evals import video_classification_frozen as vcf

    common = probe.read_config(_minimal({}))
    assert set(common) == {"val_only", "pretrain_folder", "resume_checkpoint", "eval_tag", "checkpoint", "module_name",
                           "args_model", "args_wrapper", "num_probe_blocks", "num_heads", "resolution", "batch_size",
                           "num_epochs", "use_bfloat16", "opt_kwargs"}
    for app, data in ((vcf, dict(num_classes=7)), (icf, dict(num_classes=7)), (aaf, dict(dataset="EK100"))):
        c = app.read_config(_minimal(data))
        assert {k: c[k] for k in common} == dict(common, num_heads=c["num_heads"]), app.__name__
        assert c["opt_kwargs"] == _OPT_KWARGS
        assert (c["val_only"], c["resume_checkpoint"], c["eval_tag"]) == (False, False, None)
        assert c["pretrain_folder"] == "/out"
        assert (c["checkpoint"], c["module_name"], c["args_model"], c["args_wrapper"]) == ("ckpt.pt", "m",
                                                                                         dict(encoder={}), dict(w=1))
        assert (c["num_probe_blocks"], c["resolution"]) == (1, 224)
        assert (c["batch_size"], c["num_epochs"], c["use_bfloat16"]) == (4, 2, True)
        assert app.read_config(_minimal(data), resume_preempt=True)["resume_checkpoint"] is True
        c = app.read_config(_minimal(data, val_only=True, resume_checkpoint=True, tag="t"))
        assert (c["val_only"], c["resume_checkpoint"], c["eval_tag"]) == (True, True, "t")
    # what the evals do not share: the default of classifier.num_heads, and where num_workers is read
    assert vcf.read_config(_minimal(dict(num_classes=7)))["num_heads"] == 16
    assert icf.read_config(_minimal(dict(num_classes=7)))["num_heads"] == 16
    assert aaf.read_config(_minimal(dict(dataset="EK100")))["num_heads"] is None
    assert vcf.read_config(_minimal(dict(num_classes=7)))["num_workers"] == 3
    assert icf.read_config(_minimal(dict(num_classes=7)))["num_workers"] == 3
    assert aaf.read_config(_minimal(dict(dataset="EK100")))["num_workers"] == 5
    for app, data in ((vcf, dict(num_classes=7)), (icf, dict(num_classes=7)), (aaf, dict(dataset="EK100"))):
        a = _minimal(data)
        a["experiment"]["classifier"] = dict(num_heads=2, num_probe_blocks=4)
        a["experiment"]["data"]["resolution"] = 384
        del a["num_workers"], a["experiment"]["data"]["num_workers"]
        c = app.read_config(a)
        assert (c["num_heads"], c["num_probe_blocks"], c["resolution"], c["num_workers"]) == (2, 4, 384, 0)


@pytest.mark.parametrize("eval_name", ["video_classification_frozen", "image_classification_frozen",
                                       "action_anticipation_frozen"])
def test_output_paths(eval_name, tmp_path):
    from vjepa2_amd.evals import image_classification_frozen as icf
    from vjepa2_amd.evals import probe

    root = str(tmp_path)
    folder, log_file, latest = probe.output_paths(root, eval_name, "tag7", 0)
    assert folder == os.path.join(root, eval_name + "/", "tag7") == f"{root}/{eval_name}/tag7"
    assert log_file == f"{folder}/log_r0.csv" and latest == f"{folder}/latest.pt"
    assert probe.output_paths(root, eval_name, None, 3) == (f"{root}/{eval_name}/", f"{root}/{eval_name}/log_r3.csv",
                                                            f"{root}/{eval_name}/latest.pt")
    assert not any(tmp_path.iterdir())  # naming a path makes nothing
    if eval_name == "image_classification_frozen":
        assert icf.output_paths(root, "tag7") == (folder, log_file, latest)


class _Opt(torch.optim.AdamW):
    arenas = ()  # what load_checkpoint touches of the arena optimizer besides the state dict


def _heads(seed):
    """Two nn.Linear heads with plain AdamW optimizers carrying the mc_* keys, and their schedulers."""
    from vjepa2_amd.evals.probe import CosineWDSchedule, WarmupCosineLRSchedule

    torch.manual_seed(seed)
    cs = [nn.Linear(4, 3), nn.Linear(4, 3)]
    os_ = [_Opt(c.parameters(), lr=1e-3) for c in cs]
    for o, (ref_lr, ref_wd) in zip(os_, ((1e-3, 0.01), (3e-3, 0.2))):
        o.param_groups[0].update(mc_warmup_steps=3, mc_start_lr=1e-4, mc_ref_lr=ref_lr, mc_final_lr=0.0,
                                 mc_ref_wd=ref_wd, mc_final_wd=0.4)
    T = 4 * 5  # num_epochs * ipe
    return cs, os_, [WarmupCosineLRSchedule(o, T_max=T) for o in os_], [CosineWDSchedule(o, T_max=T) for o in os_]


def _lr_wd(os_):
    return [(o.param_groups[0]["lr"], o.param_groups[0]["weight_decay"]) for o in os_]


def test_resume_replays_both_scheduler_lists(tmp_path):
    from vjepa2_amd.evals import probe

    ipe, epoch = 5, 2
    cs, os_, _, _ = _heads(1)
    for c, o in zip(cs, os_):
        c(torch.randn(5, 4)).sum().backward()
        o.step()
    path = tmp_path / "latest.pt"
    probe.save_checkpoint(path, cs, os_, [None, None], epoch, 16, 1)

    cs2, os2, lrs2, wds2 = _heads(2)
    assert probe.resume(path, cs2, os2, [None, None], lrs2, wds2, ipe) == epoch
    assert all(torch.equal(a.weight, b.weight) for a, b in zip(cs, cs2))
    assert [s._step for s in lrs2 + wds2] == [float(epoch * ipe)] * 4
    _, fresh, lrs, wds = _heads(3)
    for _ in range(epoch * ipe):
        [s.step() for s in lrs]
        [s.step() for s in wds]
    assert _lr_wd(os2) == _lr_wd(fresh) and _lr_wd(os2)[0] != _lr_wd(os2)[1]
    assert _lr_wd(os2) != _lr_wd(_heads(3)[1])  # the schedules have moved

    cs3, os3, lrs3, wds3 = _heads(4)
    before = _lr_wd(os3)
    assert probe.resume(path, cs3, os3, [None, None], lrs3, wds3, ipe, val_only=True) == 0
    assert [s._step for s in lrs3 + wds3] == [0.0] * 4 and _lr_wd(os3) == before
    assert torch.equal(cs3[1].bias, cs[1].bias) and os3[0].state_dict()["state"] == {}


def test_checked_labels_messages_and_range():
    from vjepa2_amd.evals.probe import checked_labels

    ok = torch.tensor([0, 4, 2])
    assert torch.equal(checked_labels(ok, 5, "cpu"), ok) and torch.equal(checked_labels(ok, 5, "cpu", what="verb"), ok)
    with pytest.raises(IndexError, match=r"^label 5 out of range for 5 classes$"):
        checked_labels(torch.tensor([0, 5, 2]), 5, "cpu")
    with pytest.raises(IndexError, match=r"^label -1 out of range for 5 classes$"):
        checked_labels(torch.tensor([3, -1]), 5, "cpu")
    with pytest.raises(IndexError, match=r"^noun label 7 out of range for 7 classes$"):
        checked_labels(torch.tensor([7]), 7, "cpu", what="noun")
    with pytest.raises(IndexError, match=r"^verb label -2 out of range for 3 classes$"):
        checked_labels(torch.tensor([-2, 1]), 3, "cpu", what="verb")
    with pytest.raises(IndexError, match=r"^label 9 out of range for 5 classes$"):  # both out: the high one is named
        checked_labels(torch.tensor([-1, 9]), 5, "cpu")


def test_env_world_size(monkeypatch):
    from vjepa2_amd.distributed import env_world_size

    for k in ("RANK", "WORLD_SIZE", "SLURM_NTASKS"):
        monkeypatch.delenv(k, raising=False)
    assert env_world_size() == 1
    monkeypatch.setenv("SLURM_NTASKS", "8")
    assert env_world_size() == 8
    monkeypatch.setenv("WORLD_SIZE", "4")  # without RANK the torchrun pair is incomplete: SLURM's count holds
    assert env_world_size() == 8
    monkeypatch.setenv("RANK", "1")
    assert env_world_size() == 4
    monkeypatch.delenv("SLURM_NTASKS")
    monkeypatch.setenv("WORLD_SIZE", "1")
    assert env_world_size() == 1
