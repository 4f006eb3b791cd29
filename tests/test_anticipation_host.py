"""CPU: the host-side pieces of the frozen action-anticipation eval (vjepa2_amd/evals/action_anticipation_frozen.py)
against tests/golden/anticipation_steps.pt: classifier keys and seeded init, label maps, metric arithmetic, the
wrapper's position arithmetic and range check, main's refusals."""

import pytest
import torch

import anticipation_fixture as af


def test_classifier_keys_and_seeded_init_equal_the_reference():
    """Three-query and action-only: state_dict() keys in order and the constructor's RNG order (the fixture
    loader asserts both against the reference's per-tensor sums)."""
    states = af.init_states()
    assert len(states) == 3
    keys = list(states[0])
    assert keys[0] == "pooler.query_tokens" and states[0]["pooler.query_tokens"].shape == (1, 3, 64)
    assert keys[-6:] == ["verb_classifier.weight", "verb_classifier.bias", "noun_classifier.weight",
                         "noun_classifier.bias", "action_classifier.weight", "action_classifier.bias"]
    m = af.action_only_classifier()
    assert m.action_only and m.heads == ("action",) and m.pooler.query_tokens.shape == (1, 1, 64)
    assert not hasattr(m, "verb_classifier") and list(m.state_dict())[-2:] == ["action_classifier.weight",
                                                                               "action_classifier.bias"]


def test_wrapper_models_seeded_init_equals_the_reference():
    """Fixture (a)'s encoder and predictor are rebuilt from the seed (the loader asserts the per-tensor sums)."""
    enc, pred = af.wrapper_models()
    c = af.load()["wrapper"]["cfg"]
    assert pred.num_patches == (c["pred_frames"] // c["tubelet_size"]) * (c["img_size"] // c["patch_size"]) ** 2
    assert pred.num_frames >= 2 * c["clip_frames"] and pred.num_mask_tokens >= 2
    assert c["embed_dim"] // c["num_heads"] == 32 and not enc.training and not pred.training


def test_init_classifier_signature():
    from vjepa2_amd.evals.action_anticipation_frozen import init_classifier

    cl = init_classifier(embed_dim=32, num_heads=2, num_blocks=1, device="cpu", num_classifiers=2,
                         action_classes={(0, 1): 0, (2, 1): 1}, verb_classes={0: 0, 2: 1}, noun_classes={1: 0})
    assert len(cl) == 2 and cl[0].action_classifier.out_features == 2 and cl[0].noun_classifier.out_features == 1


def test_unify_labels_equals_the_reference():
    from vjepa2_amd.evals.action_anticipation_frozen import unify_labels

    L = af.load()["labels"]
    got = unify_labels([tuple(p) for p in L["train"]], [tuple(p) for p in L["val"]])
    assert got["val_keep"] == L["keep"]
    assert [[k, i] for k, i in got["verbs"].items()] == L["verbs"]  # the set's own iteration order
    assert [[k, i] for k, i in got["nouns"].items()] == L["nouns"]
    assert [[k[0], k[1], i] for k, i in got["actions"].items()] == L["actions"]
    assert sorted(got["val_verbs"]) == L["val_verbs"] and sorted(got["val_nouns"]) == L["val_nouns"]
    assert sorted(got["val_actions"]) == L["val_actions"]
    assert not all(L["keep"]) and len(L["val_actions"]) < len(L["actions"])  # the case is not trivial


def test_read_annotation_pairs(tmp_path):
    from vjepa2_amd.evals.action_anticipation_frozen import read_annotation_pairs

    f = tmp_path / "ann.csv"
    f.write_text("narration_id,video_id,start_frame,verb_class,noun_class\na,P01_01,10,3,10\nb,P01_01,90,12,300\n")
    assert read_annotation_pairs(str(f)) == [(3, 10), (12, 300)]


def test_class_mean_recall_arithmetic_equals_the_reference():
    """result() from given TP / FN: the reference's float32 recall and accuracy, recorded per iteration."""
    from vjepa2_amd.evals.action_anticipation_frozen import ClassMeanRecall

    p = af.load()["probe"]
    n = 0
    for it in range(p["cfg"]["iters"] + 1):
        for i in range(3):
            for h in af.HEADS:
                tp, fn = p["f32"]["tp"][it][i][h], p["f32"]["fn"][it][i][h]
                m = ClassMeanRecall(tp.numel(), "cpu", k=5)
                assert m.TP.dtype == torch.int32 and m.TP.shape == tp.shape
                m.TP += tp
                m.FN += fn
                assert m.result() == p["f32"]["metrics"][it][i][h], (it, i, h)
                n += 1
    assert n == 45
    empty = ClassMeanRecall(4, "cpu").result()  # nothing counted yet: 0 / 0 as in the reference
    assert empty["recall"] != empty["recall"] and empty["accuracy"] != empty["accuracy"]


class _StubPredictor(torch.nn.Module):
    def __init__(self, num_patches, rope=True):
        super().__init__()
        self.num_patches, self.num_frames = num_patches, 0
        self.predictor_pos_embed = None if rope else torch.zeros(1)
        self.calls = 0

    def forward(self, x, masks_x, masks_y):
        self.calls += 1
        return torch.zeros(x.shape[0], masks_y.shape[1], x.shape[2])


def _wrapper(num_patches, **kw):
    from vjepa2_amd.evals.action_anticipation_frozen import AnticipativeWrapper

    enc = lambda x: torch.zeros(x.shape[0], 8, 16)  # noqa: E731  N = 8 tokens: 2 frames of a 2 x 2 grid
    pred = _StubPredictor(num_patches, rope=kw.pop("rope", True))
    return AnticipativeWrapper(enc, pred, frames_per_second=4, crop_size=32, patch_size=16, tubelet_size=2, **kw), pred


def test_wrapper_target_positions_and_range_check():
    w, pred = _wrapper(num_patches=32)
    times = torch.tensor([0.0, 0.5, 1.0, 1.49, 2.5])
    ctxt, tgt = w.target_positions(times, 8)
    assert ctxt.tolist() == [list(range(8))] * 5
    # ids = N + grid^2 * int(t * fps / tubelet) + arange(grid^2 * (num_output_frames // tubelet))
    assert tgt.tolist() == [[8 + 4 * s + j for j in range(4)] for s in (0, 1, 2, 2, 5)]
    assert tgt.dtype == torch.int64 and int(tgt.max()) == 31
    y = w(torch.zeros(5, 3, 4, 32, 32), times)
    assert y.shape == (5, 12, 16) and pred.calls == 1
    # num_steps: the oldest N_pred tokens go, the position ids stay
    w2, pred2 = _wrapper(num_patches=32, num_steps=2)
    assert w2(torch.zeros(5, 3, 4, 32, 32), times).shape == (5, 16, 16) and pred2.calls == 2
    w3, pred3 = _wrapper(num_patches=32, num_output_frames=4, no_encoder=True)
    assert w3(torch.zeros(2, 3, 4, 32, 32), torch.tensor([0.0, 2.0])).shape == (2, 8, 16)
    # one step further leaves the predictor's 32 positions: refused before the predictor is called
    for bad in (torch.tensor([0.0, 3.0]), torch.tensor([-0.5, 0.0])):
        w4, pred4 = _wrapper(num_patches=32)
        with pytest.raises(ValueError, match="leave the predictor's range"):
            w4(torch.zeros(2, 3, 4, 32, 32), bad)
        assert pred4.calls == 0
    w5, pred5 = _wrapper(num_patches=32, rope=False)
    with pytest.raises(NotImplementedError, match="RoPE predictor"):
        w5(torch.zeros(1, 3, 4, 32, 32), torch.tensor([0.0]))
    w6, pred6 = _wrapper(num_patches=32, no_predictor=True)
    assert w6(torch.zeros(1, 3, 4, 32, 32), torch.tensor([9.0])).shape == (1, 8, 16) and pred6.calls == 0


def test_synthetic_dataset_tuple_layout():
    from vjepa2_amd.evals.action_anticipation_frozen import SyntheticAnticipationDataset, make_dataloader

    pairs = SyntheticAnticipationDataset.make_pairs(7, 5, 4)
    loader = make_dataloader(pairs, batch_size=3, frames_per_clip=4, crop_size=16, anticipation_time_sec=[0.25, 1.75])
    assert len(loader) == 2  # num_batches = num_clips // batch_size (epickitchens.py:320)
    video, verb, noun, at = next(iter(loader))
    assert video.shape == (3, 3, 4, 16, 16) and video.dtype == torch.float32
    assert verb.tolist() == [p[0] for p in pairs[:3]] and noun.tolist() == [p[1] for p in pairs[:3]]
    assert at.shape == (3,) and not at.is_cuda and bool(((at >= 0.25) & (at <= 1.75)).all())
    fixed = make_dataloader(pairs, batch_size=3, frames_per_clip=4, crop_size=16, anticipation_time_sec=[1.0, 1.0])
    assert next(iter(fixed))[3].tolist() == [1.0, 1.0, 1.0]


def _args(tmp_path, module_name):
    return dict(folder=str(tmp_path), model_kwargs=dict(checkpoint="none", module_name=module_name, pretrain_kwargs={},
                                                        wrapper_kwargs={}),
                experiment=dict(classifier={}, data=dict(dataset="EK100"),
                                optimization=dict(batch_size=2, num_epochs=1, use_bfloat16=True, multihead_kwargs=[])))


def test_main_refuses_world_size_above_one_and_unknown_modules(monkeypatch, tmp_path):
    from vjepa2_amd import evals
    from vjepa2_amd.evals import action_anticipation_frozen as app

    for k in ("RANK", "WORLD_SIZE", "SLURM_NTASKS"):
        monkeypatch.delenv(k, raising=False)
    with pytest.raises(NotImplementedError, match="only evals.action_anticipation_frozen.modelcustom"):
        evals.main("action_anticipation_frozen", _args(tmp_path, "evals.some.other_module"))
    with pytest.raises(NotImplementedError, match="only evals.action_anticipation_frozen.modelcustom"):
        app.init_module("evals.some.other_module", "cpu", 4, 4, 32, "none", {}, {})
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError, match="one GPU"):
        evals.main("evals.action_anticipation_frozen", _args(tmp_path, app.ANTICIPATION_MODULE))
    assert not any(tmp_path.iterdir())  # refused before anything is written
