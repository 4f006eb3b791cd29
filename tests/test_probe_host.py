"""CPU: host logic of the frozen-encoder probe eval (vjepa2_amd/evals/video_classification_frozen.py)
against the reference's recorded schedule (tests/golden/probe_steps.pt), the synthetic loader's tuple
layout, the eval_name dispatch and the single-GPU guard."""

import numpy as np
import pytest
import torch

import probe_fixture as pf


class _Opt:
    """What the schedulers touch of an optimizer."""

    def __init__(self, group):
        self.param_groups = [group]


def _group(kw, ipe):
    return dict(lr=1e-3, weight_decay=1e-2, mc_warmup_steps=int(kw["warmup"] * ipe), mc_start_lr=kw["start_lr"],
                mc_ref_lr=kw["ref_lr"], mc_final_lr=kw["final_lr"], mc_ref_wd=kw["ref_wd"], mc_final_wd=kw["final_wd"])


def test_schedulers_reproduce_reference_sequence():
    """WarmupCosineLRSchedule / CosineWDSchedule (eval.py:490-537) give the fixture's LR and WD of every
    iteration, float for float."""
    from vjepa2_amd.evals.probe import CosineWDSchedule, WarmupCosineLRSchedule

    d = pf.load()
    cfg = d["cfg"]
    opts = [_Opt(_group(kw, cfg["ipe"])) for kw in pf.opt_kwargs(d)]
    T = int(cfg["num_epochs"] * cfg["ipe"])
    lrs, wds = [WarmupCosineLRSchedule(o, T_max=T) for o in opts], [CosineWDSchedule(o, T_max=T) for o in opts]
    for it in range(cfg["iters"]):
        [s.step() for s in lrs]
        [s.step() for s in wds]
        assert [o.param_groups[0]["lr"] for o in opts] == d["f32"]["lr"][it], it
        assert [o.param_groups[0]["weight_decay"] for o in opts] == d["f32"]["wd"][it], it
    assert isinstance(lrs[0]._step, float)
    # the clamps: past T_max the LR stays at final_lr and the WD at final_wd, whichever side it came from
    for _ in range(2 * T):
        [s.step() for s in lrs]
        [s.step() for s in wds]
    for o, kw in zip(opts, pf.opt_kwargs(d)):
        assert o.param_groups[0]["lr"] >= kw["final_lr"]
        lo, hi = sorted((kw["ref_wd"], kw["final_wd"]))
        assert lo <= o.param_groups[0]["weight_decay"] <= hi


def test_fixture_initial_weights_rebuild():
    """The three initial state_dict()s the fixture does not store rebuild from its seed (checked against
    the reference's per-tensor sums inside the loader), and differ per head."""
    a = pf.init_states()
    assert len(a) == 3
    assert not torch.equal(a[0]["linear.weight"], a[1]["linear.weight"])
    d = pf.load()
    assert sum(d["agree"]) >= 3
    assert set(d["f32"]["grads0"][0]) == set(pf.classifier(d["cfg"]).state_dict())


def test_synthetic_dataset_tuple_layout():
    """The loader tuple is what eval.py:308-313 (and ProbeTrainer via run_one_epoch) unpacks: clips as a
    list over segments of lists over views of [B, 3, F, S, S], labels [B] int64, clip indices as a list
    over segments of [B, F]; deterministic per index."""
    from vjepa2_amd.evals.video_classification_frozen import make_dataloader

    loader, sampler = make_dataloader(batch_size=3, num_samples=7, num_classes=5, img_size=16, frames_per_clip=4,
                                      num_segments=2, num_views_per_segment=3)
    assert len(loader) == 3  # drop_last=False (eval.py:462)
    batches = list(loader)
    clips, labels, idx = batches[0]
    assert len(clips) == 2 and all(len(c) == 3 for c in clips)
    assert all(v.shape == (3, 3, 4, 16, 16) and v.dtype == torch.float32 for c in clips for v in c)
    assert labels.shape == (3,) and labels.dtype == torch.int64 and 0 <= int(labels.min()) and int(labels.max()) < 5
    assert len(idx) == 2 and all(i.shape == (3, 4) for i in idx)
    assert idx[1][0].tolist() == [4, 5, 6, 7]
    assert batches[-1][1].shape == (1,)
    again = list(loader)[0]
    assert torch.equal(again[0][1][2], clips[1][2]) and torch.equal(again[1], labels)
    assert not torch.equal(clips[0][0], clips[0][1])  # views differ


def test_top_one_meter_matches_average_meter():
    """TopOneMeter: the unweighted mean of per-iteration float32 percentages (eval.py:328-331)."""
    from vjepa2_amd.evals.probe import TopOneMeter

    m = TopOneMeter(2)
    m.update(torch.tensor([1, 3], dtype=torch.int32), 3)
    m.update(torch.tensor([2, 0], dtype=torch.int32), 2)
    want = [(float(100.0 * torch.tensor(1) / 3) + 100.0) / 2, (100.0 + 0.0) / 2]
    assert np.array_equal(m.avg(), np.array(want))
    m.reset()
    assert m.avg().tolist() == [0.0, 0.0]


def test_main_refuses_world_size_above_one(monkeypatch, tmp_path):
    from vjepa2_amd import evals

    monkeypatch.setenv("RANK", "0")
    monkeypatch.setenv("WORLD_SIZE", "2")
    args = dict(folder=str(tmp_path), model_kwargs=dict(checkpoint="none", module_name=None, pretrain_kwargs={},
                                                        wrapper_kwargs={}),
                experiment=dict(classifier={}, data=dict(num_classes=3),
                                optimization=dict(batch_size=2, num_epochs=1, use_bfloat16=True, multihead_kwargs=[])))
    with pytest.raises(NotImplementedError, match="one GPU"):
        evals.main("video_classification_frozen", args)
    assert not any(tmp_path.iterdir())  # refused before anything is written
    with pytest.raises(NotImplementedError, match="not ported"):
        evals.main("image_classification_frozen", args)
