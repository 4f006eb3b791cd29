"""GPU: ProbeTrainer and the video_classification_frozen app against the reference's recorded probe
training (tests/golden/probe_steps.pt: the reference's classifiers, init_opt, schedulers and the
arithmetic of run_one_epoch over 4 training iterations and one validation iteration, in fp32 and again
under bf16 autocast).

Bounds.
  * iteration-0 logits: rel-L1 < 1e-2; iteration-0 gradients: rel-L1 < 4e-2 per tensor (the bounds of
    test_gpu_pooler.py for the same bf16-operand path against the fp32 reference);
  * losses: G_loss is the reference's own mean |bf16 run - fp32 run| over all recorded losses. Every
    single loss (iteration, head, view) is within G_loss of the fp32 run's, and the mean distance to the
    bf16 run's losses is within 1.5 G_loss (two independently rounded 16-bit runs): the envelope rule of
    test_gpu_model.py::test_vitl_bf16_path_vs_reference_autocast, whose distance is the mean too. (A
    per-loss bound against the bf16 run would test the reference's own outliers: its largest single gap
    is 3.9 G_loss.)
  * weights after the 4 iterations: mean |w - reference fp32 w| per head <= G_w of that head, the
    reference's own bf16-vs-fp32 distance (both measured to the fp32 run's weights as the fixture stores
    them). Measured 0.9996, 0.942 and 0.815 G_w for the three heads: two independently rounded 16-bit
    runs sit at about the same distance from the fp32 one, so head 0 passes with no margin to speak of;
  * LR / WD of every iteration: equal to the reference's as Python floats;
  * top-1 on the iterations where the reference's two runs agree on every sample (at least 3 of 5).
"""

import csv
import os
import shutil

import pytest
import torch

import probe_fixture as pf

pytestmark = pytest.mark.gpu

DEV = "cuda"


def rel_l1(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).abs().mean() / b.abs().mean().clamp_min(1e-12)).item()


def _flat(sd):
    return torch.cat([v.detach().reshape(-1).double().cpu() for v in sd.values()])


def _trainer(use_bfloat16=True):
    from vjepa2_amd.evals.probe import init_opt
    from vjepa2_amd.evals.video_classification_frozen import ProbeTrainer

    d = pf.load()
    cfg = d["cfg"]
    clfs = []
    for sd in pf.init_states():
        m = pf.classifier(cfg)
        m.load_state_dict(sd)
        clfs.append(m.to(DEV))
    opts, scalers, scheds, wd_scheds = init_opt(clfs, cfg["ipe"], pf.opt_kwargs(d), cfg["num_epochs"],
                                                use_bfloat16=use_bfloat16)
    encoder = lambda clips, clip_indices: clips  # noqa: E731  (the fixture's tokens are the encoder's output)
    return ProbeTrainer(encoder, clfs, opts, scalers, scheds, wd_scheds, use_bfloat16=use_bfloat16)


@pytest.fixture(scope="module")
def run():
    """The fixture's 4 training iterations and its validation iteration, once for every test below."""
    d = pf.load()
    cfg = d["cfg"]
    tr = _trainer()
    rec = dict(trainer=tr, logits0={}, grads0={}, losses=[], lr=[], wd=[], pred=[])
    state = dict(it=0)

    def on_logits(h, logits):
        if state["it"] == 0:
            rec["logits0"][h] = logits.detach().clone()

    def on_grads(h):
        if state["it"] == 0:
            rec["grads0"][h] = {n: p.grad.detach().clone() for n, p in tr.classifiers[h].named_parameters()}

    tr.on_logits, tr.on_grads = on_logits, on_grads
    for it in range(cfg["iters"] + 1):
        state["it"] = it
        views = [t.float().to(DEV) for t in d["tokens"][it]]
        if it < cfg["iters"]:
            losses = tr.train_step(views, None, d["labels"][it])
            rec["lr"].append(list(tr.last_lr))
            rec["wd"].append(list(tr.last_wd))
        else:
            losses = tr.validate(views, None, d["labels"][it])
        rec["losses"].append(losses.double().cpu())
        rec["pred"].append(tr.last_pred.cpu())
    rec["losses"] = torch.stack(rec["losses"])
    return rec


def test_probe_logits_and_gradients_iteration0(run):
    d = pf.load()
    rep = []
    for h in range(3):
        e = rel_l1(run["logits0"][h], d["f32"]["logits0"][h])
        rep.append(f"head {h} logits: rel-L1 {e:.2e} (reference bf16 vs fp32: "
                   f"{rel_l1(d['bf16']['logits0'][h], d['f32']['logits0'][h]):.2e})")
        assert e < 1e-2, "\n".join(rep)
    for h in range(3):
        ref = d["f32"]["grads0"][h]
        assert set(run["grads0"][h]) == set(ref)
        for n, g in run["grads0"][h].items():
            e = rel_l1(g, ref[n])
            rep.append(f"head {h} d{n}: {e:.2e}")
            assert e < 4e-2, "\n".join(rep)
    print("\n".join(rep))


def test_probe_losses_within_reference_envelope(run):
    d = pf.load()
    G = d["gaps"]["loss"]
    f32, b16 = d["f32"]["losses"], d["bf16"]["losses"]
    assert abs((b16 - f32).abs().mean().item() - G) < 1e-12  # G is the reference's own gap
    e32, e16 = (run["losses"] - f32).abs(), (run["losses"] - b16).abs()
    print(f"G_loss {G:.3e}; vs reference fp32: max {e32.max().item() / G:.3f} G, mean {e32.mean().item() / G:.3f} G "
          f"(per iteration {[round(x / G, 3) for x in e32.mean((1, 2)).tolist()]}); vs reference bf16: mean "
          f"{e16.mean().item() / G:.3f} G (per iteration {[round(x / G, 3) for x in e16.mean((1, 2)).tolist()]})")
    assert run["losses"].shape == f32.shape and torch.isfinite(run["losses"]).all()
    assert e32.max().item() <= G, e32.max().item() / G
    assert e16.mean().item() <= 1.5 * G, e16.mean().item() / G


def test_probe_weights_after_four_iterations(run):
    d = pf.load()
    init = pf.init_states()
    ratios = []
    for h, c in enumerate(run["trainer"].classifiers):
        ref = {k: init[h][k] + d["f32"]["wdelta"][h][k].float() for k in init[h]}
        sd = c.state_dict()
        assert list(sd) == list(ref)
        dist = (_flat(sd) - _flat(ref)).abs().mean().item()
        moved = (_flat(sd) - _flat(init[h])).abs().mean().item()
        ratios.append(dist / d["gaps"]["weights"][h])
        print(f"head {h}: mean |w - reference fp32 w| {dist:.3e} = {ratios[-1]:.3f} G_w ({d['gaps']['weights'][h]:.3e}); "
              f"mean |w - initial w| {moved:.3e}")
    assert all(r <= 1.0 for r in ratios), ratios


def test_probe_schedule_and_top1(run):
    d = pf.load()
    cfg = d["cfg"]
    assert run["lr"] == d["f32"]["lr"] and run["wd"] == d["f32"]["wd"]
    agree = d["agree"]
    assert sum(agree) >= 3 and len(agree) == cfg["iters"] + 1
    assert all(torch.equal(d["f32"]["pred"][i], d["bf16"]["pred"][i]) == a for i, a in enumerate(agree))
    for it, a in enumerate(agree):
        ours = run["pred"][it].long()
        print(f"iteration {it}: reference runs agree: {a}; ours equals fp32's: {torch.equal(ours, d['f32']['pred'][it])}")
        if a:
            assert torch.equal(ours, d["f32"]["pred"][it]), it
            pct = [float(100.0 * p.eq(d["labels"][it]).sum() / cfg["B"]) for p in ours]
            assert pct == d["f32"]["top1"][it]
    # the device-side meters: unweighted mean of the per-iteration percentages (AverageMeter, eval.py:328-331)
    tr = run["trainer"]
    want = torch.tensor([[float(100.0 * p.eq(d["labels"][it]).sum() / cfg["B"]) for p in run["pred"][it].long()]
                         for it in range(cfg["iters"])], dtype=torch.float64).mean(0)
    assert torch.allclose(torch.from_numpy(tr.train_meter.avg()), want, rtol=0, atol=1e-9)
    val = [float(100.0 * p.eq(d["labels"][-1]).sum() / cfg["B"]) for p in run["pred"][-1].long()]
    assert tr.val_meter.avg().tolist() == val


def test_probe_optimizer_state_interchange(run):
    """Each head's state_dict() loads into a torch.optim.AdamW built as eval.py:471-483 builds it; the
    reference optimizer's recorded state loads into ours."""
    from vjepa2_amd.evals.probe import load_opt_state

    d = pf.load()
    tr = run["trainer"]
    for h, (c, opt) in enumerate(zip(tr.classifiers, tr.opts)):
        sd = opt.state_dict()
        g = sd["param_groups"][0]
        assert len(sd["param_groups"]) == 1 and g["params"] == list(range(len(list(c.parameters()))))
        ref_g = d["f32"]["opt_groups"][h][0]
        assert set(g) == set(ref_g), set(g) ^ set(ref_g)
        for k in ref_g:
            assert g[k] == ref_g[k], (h, k, g[k], ref_g[k])  # lr, weight_decay, mc_*: the same floats
        cpu = [torch.nn.Parameter(p.detach().cpu().clone()) for _, p in c.named_parameters()]
        kw = {k: v for k, v in ref_g.items() if k.startswith("mc_")}
        ref_opt = torch.optim.AdamW([dict(params=iter(cpu), **kw)])
        ref_opt.load_state_dict(sd)
        st = ref_opt.state_dict()["state"]
        assert len(st) == len(cpu) and all(float(s["step"]) == 4.0 for s in st.values())
        names = [n for n, _ in c.named_parameters()]
        i = names.index("linear.weight")
        a = opt.arenas[0]
        o, n = a.segment(c.linear.weight)
        assert torch.equal(st[i]["exp_avg"].reshape(-1), a.exp_avg[o:o + n].cpu())
    # the reference's state (head cfg["opt_state_head"]; moments stored as bf16) into a fresh trainer's optimizer
    h = d["cfg"]["opt_state_head"]
    fresh = _trainer()
    ref_sd = dict(state={k: dict(step=v["step"], exp_avg=v["exp_avg"].float(), exp_avg_sq=v["exp_avg_sq"].float())
                         for k, v in d["f32"]["opt_state"].items()}, param_groups=d["f32"]["opt_groups"][h])
    opt = fresh.opts[h]
    load_opt_state(opt, ref_sd)
    assert opt.steps == [4] and opt.param_groups[0]["lr"] == d["f32"]["lr"][-1][h]
    back = opt.state_dict()
    for k, v in ref_sd["state"].items():
        assert torch.equal(back["state"][k]["exp_avg"], v["exp_avg"])
        assert torch.equal(back["state"][k]["exp_avg_sq"], v["exp_avg_sq"])
    # and our moments after the same 4 iterations are the reference's, to the gradients' tolerance
    ours = tr.opts[h].state_dict()["state"]
    worst = max(rel_l1(ours[k]["exp_avg"], v["exp_avg"]) for k, v in ref_sd["state"].items())
    print(f"head {h}: exp_avg after 4 iterations vs the reference's, worst rel-L1 {worst:.2e}")
    assert worst < 4e-2


def test_probe_per_head_inf_skip():
    """A NaN in one head's gradients (its linear bias gradient buffer is poisoned before the step, so
    the step's own bias gradient adds onto NaN) skips that head's update only: GradScaler.step per head
    (eval.py:336), decided on the device."""
    d = pf.load()
    tr = _trainer(use_bfloat16=True)
    before = [{k: v.detach().clone() for k, v in c.state_dict().items()} for c in tr.classifiers]
    tr.classifiers[1].linear.bias.grad.fill_(float("nan"))
    views = [t.float().to(DEV) for t in d["tokens"][0]]
    losses = tr.train_step(views, None, d["labels"][0])
    assert torch.isfinite(losses).all()
    assert [o.steps for o in tr.opts] == [[1], [0], [1]]
    for h, c in enumerate(tr.classifiers):
        same = all(torch.equal(v, before[h][k]) for k, v in c.state_dict().items())
        assert same == (h == 1), h
    assert tr.opts[1].state_dict()["state"] == {}
    # the next step is clean again (zero_grad cleared the poison) and head 1 takes its first update
    tr.train_step([t.float().to(DEV) for t in d["tokens"][1]], None, d["labels"][1])
    assert [o.steps for o in tr.opts] == [[2], [1], [2]]
    assert all(torch.isfinite(p).all() for c in tr.classifiers for p in c.parameters())


def _micro(**kw):
    import torch.nn as nn

    from vjepa2_amd import vision_transformer as vit

    return vit.VisionTransformer(embed_dim=64, depth=2, num_heads=1, mlp_ratio=4, qkv_bias=True,
                                 norm_layer=lambda dim: nn.LayerNorm(dim, eps=1e-6), **kw)


def test_probe_main_end_to_end(tmp_path, monkeypatch):
    """main() on the synthetic dataset with the micro encoder of test_multiclip_matches_reference:
    CSV, latest.pt with the reference's key set, bitwise resume after epoch 1, val_only."""
    from vjepa2_amd import evals
    from vjepa2_amd import vision_transformer as vit
    from vjepa2_amd.evals import video_classification_frozen as app

    monkeypatch.setattr(vit, "vit_micro", _micro, raising=False)
    for k in ("RANK", "WORLD_SIZE", "SLURM_NTASKS"):
        monkeypatch.delenv(k, raising=False)
    enc_kw = dict(model_name="vit_micro", checkpoint_key="target_encoder", patch_size=16, tubelet_size=2,
                  use_rope=True, uniform_power=True)
    torch.manual_seed(3)
    enc = _micro(img_size=32, num_frames=4, patch_size=16, tubelet_size=2, use_rope=True, uniform_power=True)
    ckpt = tmp_path / "pretrained.pt"
    torch.save({"target_encoder": {"module.backbone." + k: v for k, v in enc.state_dict().items()}, "epoch": 7}, ckpt)

    def args(folder, **top):
        return dict(folder=str(folder), tag="micro", num_workers=0, **top,
                    model_kwargs=dict(checkpoint=str(ckpt), module_name=app.MULTICLIP_MODULE,
                                      pretrain_kwargs=dict(encoder=dict(enc_kw)),
                                      wrapper_kwargs=dict(max_frames=16, use_pos_embed=True)),
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
    run1 = tmp_path / "run1"
    acc = evals.main("video_classification_frozen", args(run1))
    out1 = run1 / "video_classification_frozen" / "micro"
    rows = list(csv.reader(open(out1 / "log_r0.csv")))
    assert len(rows) == 2 and [r[0] for r in rows] == ["1", "2"] and all(len(r) == 3 for r in rows)
    assert float(rows[1][2]) == pytest.approx(acc, abs=1e-5) and 0.0 <= acc <= 100.0
    full = torch.load(out1 / "latest.pt", weights_only=True)
    assert set(full) == {"classifiers", "opt", "scaler", "epoch", "batch_size", "world_size"}
    assert full["epoch"] == 2 and full["batch_size"] == 2 and full["world_size"] == 1
    assert len(full["classifiers"]) == 2 and len(full["opt"]) == 2 and len(full["scaler"]) == 2
    assert all(k.startswith("module.") for sd in full["classifiers"] for k in sd)
    assert all(float(s["step"]) == 6.0 for o in full["opt"] for s in o["state"].values())  # 2 epochs x ipe 3

    # resume after epoch 1 in a fresh folder: the same final weights and moments, bit for bit
    out2 = tmp_path / "run2" / "video_classification_frozen" / "micro"
    os.makedirs(out2)
    shutil.copy(f"{out1 / 'latest.pt'}.e1", out2 / "latest.pt")
    # ... with the classifier keys unprefixed in one head: both spellings load
    part = torch.load(out2 / "latest.pt", weights_only=True)
    assert part["epoch"] == 1
    part["classifiers"][0] = {k[len("module."):]: v for k, v in part["classifiers"][0].items()}
    torch.save(part, out2 / "latest.pt")
    acc2 = evals.main("video_classification_frozen", args(tmp_path / "run2", resume_checkpoint=True))
    resumed = torch.load(out2 / "latest.pt", weights_only=True)
    assert resumed["epoch"] == 2 and acc2 == acc
    for a, b in zip(full["classifiers"], resumed["classifiers"]):
        assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    for a, b in zip(full["opt"], resumed["opt"]):
        assert all(torch.equal(a["state"][k]["exp_avg_sq"], b["state"][k]["exp_avg_sq"]) for k in a["state"])
    assert [r[0] for r in csv.reader(open(out2 / "log_r0.csv"))] == ["2"]

    # val_only on the trained classifiers: the training run's last validation accuracy
    acc3 = evals.main("video_classification_frozen", args(run1, val_only=True, resume_checkpoint=True))
    assert acc3 == acc
    rows = list(csv.reader(open(out1 / "log_r0.csv")))
    assert len(rows) == 3 and rows[2][1] == "-1.00000"
