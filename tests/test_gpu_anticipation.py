"""GPU: AnticipativeWrapper, AnticipationTrainer and the action_anticipation_frozen app against the reference's
recorded runs (tests/golden/anticipation_steps.pt: the reference's wrapper on a tiny RoPE encoder + predictor,
and its classifiers, schedules, sigmoid_focal_loss and ClassMeanRecall over 4 training iterations and one
validation iteration, each in fp32 and again under bf16 autocast).

Bounds.
  * wrapper: mean |HIP - reference fp32| <= 1.5 x the reference's own mean |bf16 - fp32|, and the max <= 1.5 x
    its max gap (two independently rounded 16-bit evaluations of the same computation);
  * losses: G_loss is the reference's own mean |bf16 run - fp32 run| over all recorded losses; the mean distance
    to the fp32 run's losses and to the bf16 run's is within 1.5 G_loss, the max distance to the fp32 run's
    within 1.5 x the reference's max gap;
  * iteration-0 logits rel-L1 < 1e-2 and iteration-0 gradients rel-L1 < 4e-2 per tensor, the bounds
    test_gpu_probe.py uses for the same bf16-operand path against the fp32 reference;
  * weights after the 4 iterations: mean |w - reference fp32 w| per classifier <= G_w of that classifier
    (measured 0.960, 0.998 and 0.933 G_w: two independently rounded 16-bit runs sit at about the same distance
    from the fp32 one, so classifier 1 passes with no margin to speak of);
  * LR / WD of every iteration: equal to the reference's as Python floats;
  * on the qualifying iterations (the reference's two runs agree on every hit flag and every label's logit is
    more than 4 G_logits away from the top-k boundary; at least 3 of 5): hit flags, TP / FN, recall and accuracy
    equal the fp32 reference's exactly.
"""

import csv
import os
import shutil

import pytest
import torch

import anticipation_fixture as af

pytestmark = pytest.mark.gpu

DEV = "cuda"
HEADS = af.HEADS


def rel_l1(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).abs().mean() / b.abs().mean().clamp_min(1e-12)).item()


def _flat(sd):
    return torch.cat([v.detach().reshape(-1).double().cpu() for v in sd.values()])


# ------------------------------------------------------------------------------------------------ wrapper
@pytest.mark.parametrize("num_steps", [1, 2])
def test_wrapper_against_reference(num_steps):
    from vjepa2_amd.evals.action_anticipation_frozen import AnticipativeWrapper

    w = af.load()["wrapper"]
    c = w["cfg"]
    enc, pred = af.wrapper_models()
    model = AnticipativeWrapper(enc.to(DEV), pred.to(DEV), frames_per_second=c["fps"], crop_size=c["img_size"],
                                patch_size=c["patch_size"], tubelet_size=c["tubelet_size"],
                                num_output_frames=c["num_output_frames"], num_steps=num_steps).eval()
    with torch.no_grad():
        y = model(w["clips"].float().to(DEV), w["times"])
    ref, ref16, G = w["f32"][num_steps], w["bf16"][num_steps].float(), w["gaps"][num_steps]
    assert y.shape == ref.shape and torch.isfinite(y).all()
    d = (y.float().cpu() - ref).abs()
    print(f"num_steps {num_steps}: |HIP - fp32| mean {d.mean().item() / G['mean']:.3f} G_mean, max "
          f"{d.max().item() / G['max']:.3f} G_max (G mean {G['mean']:.3e}, max {G['max']:.3e}); vs reference bf16: mean "
          f"{(y.float().cpu() - ref16).abs().mean().item() / G['mean']:.3f} G_mean")
    N = 8
    dn = d[:, :N].mean().item(), d[:, N:].mean().item()
    print(f"  encoder tokens mean {dn[0]:.3e}, predicted tokens mean {dn[1]:.3e}")
    assert d.mean().item() <= 1.5 * G["mean"], d.mean().item() / G["mean"]
    assert d.max().item() <= 1.5 * G["max"], d.max().item() / G["max"]
    # a time whose positions would pass the predictor's range is refused before any predictor launch
    with pytest.raises(ValueError, match="leave the predictor's range"):
        model(w["clips"].float().to(DEV), torch.tensor([0.0, 0.5, 3.0]))


# ------------------------------------------------------------------------------------------------ trainer
def _trainer(use_bfloat16=True, use_focal_loss=True, classifiers=None, n=3):
    from vjepa2_amd.evals.action_anticipation_frozen import AnticipationTrainer
    from vjepa2_amd.evals.probe import init_opt

    p = af.load()["probe"]
    cfg = p["cfg"]
    if classifiers is None:
        classifiers = []
        for sd in af.init_states()[:n]:
            m = af.classifier(cfg)
            m.load_state_dict(sd)
            classifiers.append(m.to(DEV))
    opts, scalers, scheds, wd_scheds = init_opt(classifiers, cfg["ipe"], af.opt_kwargs(p)[:len(classifiers)],
                                                cfg["num_epochs"], use_bfloat16=use_bfloat16)
    model = lambda clips, times: clips  # noqa: E731  (the fixture's tokens are the wrapper's output)
    return AnticipationTrainer(model, classifiers, opts, scalers, scheds, wd_scheds, use_bfloat16=use_bfloat16,
                               use_focal_loss=use_focal_loss, alpha=cfg["alpha"], gamma=cfg["gamma"], k=cfg["k"])


def _valid_masks(p):
    cfg = p["cfg"]
    out = {}
    for h in HEADS:
        m = torch.zeros(cfg[h + "s"], dtype=torch.bool)
        m[p["valid"][h]] = True
        out[h] = m.to(DEV)
    return out


@pytest.fixture(scope="module")
def run():
    """The fixture's 4 training iterations and its validation iteration, once for every test below."""
    p = af.load()["probe"]
    cfg = p["cfg"]
    tr = _trainer()
    rec = dict(trainer=tr, logits0={}, grads0={}, losses=[], lr=[], wd=[], hits=[], tp=[], fn=[], metrics=[])
    state = dict(it=0)

    def on_logits(i, out):
        if state["it"] == 0:
            rec["logits0"][i] = {h: v.detach().clone() for h, v in out.items()}

    def on_grads(i):
        if state["it"] == 0:
            rec["grads0"][i] = {n: q.grad.detach().clone() for n, q in tr.classifiers[i].named_parameters()}

    tr.on_logits, tr.on_grads = on_logits, on_grads
    tr.reset_metrics(True)
    for it in range(cfg["iters"] + 1):
        state["it"] = it
        training = it < cfg["iters"]
        tokens = p["tokens"][it].float().to(DEV)
        if training:
            losses = tr.train_step(tokens, None, p["labels"][it])
            rec["lr"].append(list(tr.last_lr))
            rec["wd"].append(list(tr.last_wd))
        else:
            tr.reset_metrics(False)
            losses = tr.validate(tokens, None, p["labels"][it], valid=_valid_masks(p))
        rec["losses"].append(losses.double().cpu())
        rec["hits"].append(tr.last_hits.cpu())
        ms = tr.metrics[training]
        rec["tp"].append([{h: ms[h][i].TP.cpu().clone() for h in HEADS} for i in range(3)])
        rec["fn"].append([{h: ms[h][i].FN.cpu().clone() for h in HEADS} for i in range(3)])
        rec["metrics"].append([{h: ms[h][i].result() for h in HEADS} for i in range(3)])
    rec["losses"] = torch.stack(rec["losses"])
    return rec


def test_anticipation_logits_and_gradients_iteration0(run):
    p = af.load()["probe"]
    rep = []
    for i in range(3):
        for h in HEADS:
            e = rel_l1(run["logits0"][i][h], p["f32"]["logits0"][i][h])
            rep.append(f"classifier {i} {h} logits: rel-L1 {e:.2e} (reference bf16 vs fp32: "
                       f"{rel_l1(p['bf16']['logits0'][i][h], p['f32']['logits0'][i][h]):.2e})")
            assert e < 1e-2, "\n".join(rep)
    for i in range(3):
        ref = p["f32"]["grads0"][i]
        assert set(run["grads0"][i]) == set(ref)
        for n, g in run["grads0"][i].items():
            e = rel_l1(g, ref[n])
            rep.append(f"classifier {i} d{n}: {e:.2e}")
            assert e < 4e-2, "\n".join(rep)
    print("\n".join(rep))


def test_anticipation_losses_within_reference_envelope(run):
    p = af.load()["probe"]
    G, Gmax = p["gaps"]["loss"]["mean"], p["gaps"]["loss"]["max"]
    f32, b16 = p["f32"]["losses"], p["bf16"]["losses"]
    assert abs((b16 - f32).abs().mean().item() - G) < 1e-12  # G is the reference's own gap
    e32, e16 = (run["losses"] - f32).abs(), (run["losses"] - b16).abs()
    print(f"G_loss mean {G:.3e} max {Gmax:.3e}; vs reference fp32: mean {e32.mean().item() / G:.3f} G, max "
          f"{e32.max().item() / Gmax:.3f} G_max (per iteration {[round(x / G, 3) for x in e32.mean((1, 2)).tolist()]}); "
          f"vs reference bf16: mean {e16.mean().item() / G:.3f} G")
    assert run["losses"].shape == f32.shape and torch.isfinite(run["losses"]).all()
    assert e32.mean().item() <= 1.5 * G, e32.mean().item() / G
    assert e32.max().item() <= 1.5 * Gmax, e32.max().item() / Gmax
    assert e16.mean().item() <= 1.5 * G, e16.mean().item() / G


def test_anticipation_weights_after_four_iterations(run):
    p = af.load()["probe"]
    init = af.init_states()
    ratios = []
    for i, c in enumerate(run["trainer"].classifiers):
        ref = {k: init[i][k] + p["f32"]["wdelta"][i][k].float() for k in init[i]}
        sd = c.state_dict()
        assert list(sd) == list(ref)
        dist = (_flat(sd) - _flat(ref)).abs().mean().item()
        moved = (_flat(sd) - _flat(init[i])).abs().mean().item()
        ratios.append(dist / p["gaps"]["weights"][i])
        print(f"classifier {i}: mean |w - reference fp32 w| {dist:.3e} = {ratios[-1]:.3f} G_w "
              f"({p['gaps']['weights'][i]:.3e}); mean |w - initial w| {moved:.3e}")
    assert all(r <= 1.0 for r in ratios), ratios


def test_anticipation_schedule_hits_and_metrics(run):
    p = af.load()["probe"]
    cfg = p["cfg"]
    assert run["lr"] == p["f32"]["lr"] and run["wd"] == p["f32"]["wd"]
    q = p["qualify"]
    assert len(q) == cfg["iters"] + 1 and sum(q) >= 3  # at most 2 of the 5 iterations are skipped
    assert all((not a) or torch.equal(p["f32"]["hits"][i], p["bf16"]["hits"][i]) for i, a in enumerate(q))
    # TP / FN accumulate over the training iterations: exact only while every earlier iteration qualified too
    clean = True
    for it, a in enumerate(q):
        training = it < cfg["iters"]
        if not training:
            clean = True  # validation has counters of its own
        same = torch.equal(run["hits"][it], p["f32"]["hits"][it])
        print(f"iteration {it}: qualifies {a}; hit flags equal fp32's: {same}")
        if a:
            assert same, it
        clean = clean and a
        if a and clean:
            for i in range(3):
                for h in HEADS:
                    assert torch.equal(run["tp"][it][i][h], p["f32"]["tp"][it][i][h]), (it, i, h)
                    assert torch.equal(run["fn"][it][i][h], p["f32"]["fn"][it][i][h]), (it, i, h)
                    assert run["metrics"][it][i][h] == p["f32"]["metrics"][it][i][h], (it, i, h)
    # every sample was counted once per classifier and head
    for it in range(cfg["iters"] + 1):
        n = cfg["B"] * (it + 1 if it < cfg["iters"] else 1)
        assert all(int(run["tp"][it][i][h].sum() + run["fn"][it][i][h].sum()) == n for i in range(3) for h in HEADS)


def test_anticipation_cross_entropy_branch_and_action_only():
    """use_focal_loss false: the loss is CrossEntropyLoss per head (vj_xent), vj_focal only counts. And one
    step of an action-only classifier."""
    import torch.nn.functional as F

    p = af.load()["probe"]
    tr = _trainer(use_focal_loss=False, n=1)
    seen = {}
    tr.on_logits = lambda i, out: seen.update({h: v.detach().clone() for h, v in out.items()})
    before = _flat(tr.classifiers[0].state_dict())
    losses = tr.train_step(p["tokens"][0].float().to(DEV), None, p["labels"][0])
    for s, h in enumerate(HEADS):
        want = F.cross_entropy(seen[h].double().cpu(), p["labels"][0][h])
        assert abs(float(losses[0, s]) - float(want)) <= 1e-5 * float(want), (h, float(losses[0, s]), float(want))
        top5 = seen[h].cpu().topk(5, dim=1).indices
        assert tr.last_hits[0, s].tolist() == [int(lb in t) for t, lb in zip(top5, p["labels"][0][h])]
    assert tr.opts[0].steps == [1] and not torch.equal(before, _flat(tr.classifiers[0].state_dict()))
    assert int(tr.metrics[True]["action"][0].TP.sum() + tr.metrics[True]["action"][0].FN.sum()) == p["cfg"]["B"]

    m = af.action_only_classifier().to(DEV)
    tr = _trainer(classifiers=[m])
    assert tr.heads == ("action",)
    before = _flat(m.state_dict())
    losses = tr.train_step(p["tokens"][1].float().to(DEV), None, dict(action=p["labels"][1]["action"]))
    assert losses.shape == (1, 1) and torch.isfinite(losses).all() and tr.last_hits.shape == (1, 1, p["cfg"]["B"])
    assert tr.opts[0].steps == [1] and not torch.equal(before, _flat(m.state_dict()))
    assert set(tr.results(True)) == {"action"}


# ------------------------------------------------------------------------------------------------ main
def _ckpt(tmp_path):
    w = af.load()["wrapper"]
    enc, pred = af.wrapper_models()
    path = tmp_path / "pretrained.pt"
    torch.save({"target_encoder": {"module.backbone." + k: v for k, v in enc.state_dict().items()},
                "predictor": {"module.backbone." + k: v for k, v in pred.state_dict().items()}, "epoch": 3}, path)
    return path, w["cfg"]


def _micro_encoder(**kw):
    import torch.nn as nn

    from vjepa2_amd import vision_transformer as vit

    kw.pop("model_name", None), kw.pop("checkpoint_key", None)
    return vit.VisionTransformer(norm_layer=lambda dim: nn.LayerNorm(dim, eps=1e-6), **kw)


def test_anticipation_main_end_to_end(tmp_path, monkeypatch):
    """main() on the synthetic dataset with fixture (a)'s encoder and predictor: the 13-column CSV, latest.pt
    with the reference's key set, resume after epoch 1 continues the LR schedule and reaches the same weights,
    val_only returns the metrics dict; then a short run with use_focal_loss false."""
    from vjepa2_amd import evals
    from vjepa2_amd import vision_transformer as vit
    from vjepa2_amd.evals import action_anticipation_frozen as app

    monkeypatch.setattr(vit, "vit_micro", _micro_encoder, raising=False)
    for k in ("RANK", "WORLD_SIZE", "SLURM_NTASKS"):
        monkeypatch.delenv(k, raising=False)
    ckpt, c = _ckpt(tmp_path)
    enc_kw = dict(model_name="vit_micro", checkpoint_key="target_encoder", patch_size=c["patch_size"],
                  tubelet_size=c["tubelet_size"], embed_dim=c["embed_dim"], depth=c["enc_depth"],
                  num_heads=c["num_heads"], mlp_ratio=c["mlp_ratio"], qkv_bias=True, use_rope=True, uniform_power=True)
    prd_kw = dict(model_name="vit_predictor", checkpoint_key="predictor", num_frames=c["pred_frames"],
                  predictor_embed_dim=c["pred_embed_dim"], depth=c["pred_depth"], num_heads=c["num_heads"],
                  uniform_power=True, use_mask_tokens=True, num_mask_tokens=c["num_mask_tokens"],
                  zero_init_mask_tokens=False, use_rope=True)

    def args(folder, focal=True, epochs=2, **top):
        return dict(folder=str(folder), tag="micro", **top,
                    model_kwargs=dict(checkpoint=str(ckpt), module_name=app.ANTICIPATION_MODULE,
                                      pretrain_kwargs=dict(encoder=dict(enc_kw), predictor=dict(prd_kw)),
                                      wrapper_kwargs=dict(no_predictor=False, num_output_frames=2, num_steps=1)),
                    experiment=dict(classifier=dict(num_probe_blocks=2, num_heads=2),
                                    data=dict(dataset="EK100", num_workers=0, frames_per_clip=c["clip_frames"],
                                              frames_per_second=c["fps"], resolution=c["img_size"],
                                              train_anticipation_time_sec=[0.25, 1.75], anticipation_time_sec=[1.0, 1.0],
                                              num_samples=6, num_val_samples=5, num_verbs=4, num_nouns=3),
                                    optimization=dict(batch_size=2, num_epochs=epochs, use_bfloat16=True,
                                                      use_focal_loss=focal, multihead_kwargs=[
                                                          dict(lr=1e-3, start_lr=1e-4, final_lr=1e-5, weight_decay=0.01,
                                                               final_weight_decay=0.1, warmup=0.5),
                                                          dict(lr=3e-3, start_lr=3e-3, final_lr=0.0, weight_decay=0.2,
                                                               final_weight_decay=0.2, warmup=0.0)])))

    save = app.save_checkpoint

    def save_and_keep(path, classifiers, optimizers, scalers, epoch, batch_size, world_size):
        save(path, classifiers, optimizers, scalers, epoch, batch_size, world_size)
        shutil.copy(path, f"{path}.e{epoch}")

    monkeypatch.setattr(app, "save_checkpoint", save_and_keep)
    run1 = tmp_path / "run1"
    val = evals.main("action_anticipation_frozen", args(run1))
    assert set(val) == set(HEADS) and all(set(v) == {"accuracy", "recall"} for v in val.values())
    assert all(0.0 <= v[q] <= 100.0 for v in val.values() for q in v)
    out1 = run1 / "action_anticipation_frozen" / "micro"
    rows = list(csv.reader(open(out1 / "log_r0.csv")))
    assert rows[0] == list(app.CSV_COLUMNS) and len(rows[0]) == 13
    assert len(rows) == 3 and [r[0] for r in rows[1:]] == ["1", "2"] and all(len(r) == 13 for r in rows)
    assert float(rows[2][7]) == pytest.approx(val["action"]["accuracy"], abs=1e-5)
    assert float(rows[2][12]) == pytest.approx(val["noun"]["recall"], abs=1e-5)
    full = torch.load(out1 / "latest.pt", weights_only=True)
    assert set(full) == {"classifiers", "opt", "scaler", "epoch", "batch_size", "world_size"}
    assert full["epoch"] == 2 and full["batch_size"] == 2 and full["world_size"] == 1
    assert len(full["classifiers"]) == 2 and len(full["opt"]) == 2 and len(full["scaler"]) == 2
    assert all(k.startswith("module.") for sd in full["classifiers"] for k in sd)
    assert all(float(s["step"]) == 6.0 for o in full["opt"] for s in o["state"].values())  # 2 epochs x ipe 3

    # resume after epoch 1 in a fresh folder: the schedule continues, the same final weights and moments
    out2 = tmp_path / "run2" / "action_anticipation_frozen" / "micro"
    os.makedirs(out2)
    shutil.copy(f"{out1 / 'latest.pt'}.e1", out2 / "latest.pt")
    part = torch.load(out2 / "latest.pt", weights_only=True)
    assert part["epoch"] == 1
    part["classifiers"][0] = {k[len("module."):]: v for k, v in part["classifiers"][0].items()}  # both spellings load
    torch.save(part, out2 / "latest.pt")
    val2 = evals.main("action_anticipation_frozen", args(tmp_path / "run2", resume_checkpoint=True))
    resumed = torch.load(out2 / "latest.pt", weights_only=True)
    assert resumed["epoch"] == 2 and val2 == val
    for a, b in zip(full["opt"], resumed["opt"]):
        assert a["param_groups"][0]["lr"] == b["param_groups"][0]["lr"]  # the LR schedule went on from epoch 1
        assert a["param_groups"][0]["weight_decay"] == b["param_groups"][0]["weight_decay"]
        assert all(torch.equal(a["state"][k]["exp_avg_sq"], b["state"][k]["exp_avg_sq"]) for k in a["state"])
    for a, b in zip(full["classifiers"], resumed["classifiers"]):
        assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    assert [r[0] for r in csv.reader(open(out2 / "log_r0.csv"))] == ["epoch", "2"]

    # val_only on the trained classifiers: the training run's last validation metrics
    val3 = evals.main("action_anticipation_frozen", args(run1, val_only=True, resume_checkpoint=True))
    assert val3 == val

    # CrossEntropyLoss instead of the focal loss
    val4 = evals.main("action_anticipation_frozen", args(tmp_path / "run3", focal=False, epochs=1))
    assert set(val4) == set(HEADS) and all(v[q] == v[q] for v in val4.values() for q in v)
