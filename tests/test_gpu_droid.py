"""GPU: V-JEPA 2-AC post-training (vjepa2_amd.droid) on the micro model of tests/golden/droid_steps.pt, the
reference's own app run for three iterations on CPU in fp32 and under bf16 autocast.

 * functions.ACLossFn under torch.autograd gives ops.ac_loss_bwd's bits.
 * One forward / backward of the step with the fused loss side against the same step with the reference's
   separate torch ops (F.layer_norm, the slice, mean(|z - h| ** p) / p, autograd) on the same HIP predictor: this
   isolates the new kernels from the bf16 blocks.
 * ACTrainer for three steps against the recording: lr / wd exact, the losses and the final predictor weights
   inside 1.5 x the reference's own |bf16 - fp32| envelope (tests/test_gpu_planning.py's margin), the frozen
   encoder untouched, two runs bitwise equal, the optimizer state laid out as the reference's.
 * main() end to end on a micro YAML: checkpoint keys, log, resume."""

import csv

import pytest
import torch
import torch.nn.functional as F
import yaml

import droid_fixture as fx
import test_gpu_acloss as kt

pytestmark = pytest.mark.gpu

DEV = "cuda"


# ------------------------------------------------------------------------------------------------ ACLossFn
@pytest.mark.parametrize("normalize,p", [(True, 1.0), (True, 2.0), (False, 1.0), (False, 2.0)])
def test_aclossfn_autograd_equals_the_direct_backward(normalize, p):
    from vjepa2_amd import ops
    from vjepa2_amd.functions import ACLossFn

    B, R, D = 3, 5, 96
    _, _, z0, h, gzn = kt.make_inputs(B, R, D, normalize, seed=77)
    N = B * R * D
    gl = torch.tensor(kt.GL, device=DEV)

    def run(use_loss, use_zn):
        full = torch.zeros(B, 2 * R, D, device=DEV)
        full[:, R:] = z0
        full.requires_grad_()
        z = full[:, R:]  # a frame slice of a longer sequence
        loss, zn = ACLossFn.apply(z, h if use_loss else None, normalize, p, kt.EPS)
        assert (loss is None) == (not use_loss)
        tot = 0.0
        if use_loss:
            assert loss.dim() == 0
            tot = tot + loss * gl
        if use_zn:
            tot = tot + (zn * gzn).sum()
        tot.backward()
        assert not full.grad[:, :R].any()
        return z.detach(), loss, full.grad[:, R:]

    z, loss, g = run(True, True)
    l_ref, _, stats = ops.ac_loss_fwd(z, h, normalize=normalize, loss_exp=p, eps=kt.EPS)
    assert torch.equal(loss.reshape(1), l_ref)
    assert torch.equal(g, ops.ac_loss_bwd(z, stats, h, normalize=normalize, loss_exp=p, scale=1.0 / N, gscale=gl,
                                          gzn=gzn))
    _, _, g = run(True, False)  # dzn None
    assert torch.equal(g, ops.ac_loss_bwd(z, stats, h, normalize=normalize, loss_exp=p, scale=1.0 / N, gscale=gl))
    _, _, g = run(False, True)  # the roll-out's normalise-only call: only dzn flows
    assert torch.equal(g, ops.ac_loss_bwd(z, stats, None, normalize=normalize, gzn=gzn))


# ------------------------------------------------------------------------------------------------ the step
def _trainer(name, mixed_precision=True, loss_side="hip"):
    from vjepa2_amd import droid

    run = fx.load()["runs"][name]
    m = fx.load()["micro"]
    enc, pred = fx.models(name, DEV)
    co, cl = run["args"]["optimization"], run["args"]["loss"]
    opt, scaler, sched, wds = droid.init_opt(
        encoder=enc, predictor=pred, iterations_per_epoch=co["ipe"], start_lr=co["start_lr"], ref_lr=co["lr"],
        warmup=co["warmup"], anneal=co["anneal"], num_epochs=co["epochs"], wd=co["weight_decay"],
        final_wd=co["final_weight_decay"], final_lr=co["final_lr"], mixed_precision=mixed_precision)
    tr = droid.ACTrainer(pred, enc, opt, (m["crop"] // m["patch"]) ** 2, auto_steps=min(cl["auto_steps"], m["fpc"]),
                         loss_exp=cl["loss_exp"], normalize_reps=cl["normalize_reps"],
                         mixed_precision=mixed_precision, loss_side=loss_side)
    return tr, enc, pred, opt, sched, wds


def _batch(name, i):
    return [t.to(DEV) for t in fx.batches(name)[i]]


def _loss_side_f64(tr):
    """The trainer's loss side as float64 torch ops (results handed back in f32): the yardstick's reference."""
    def loss(z, h, normalize, want_zn=True):
        zn = F.layer_norm(z.double(), (z.size(-1),)) if normalize else z.double()
        if h is None:
            return None, zn.float()
        return (torch.mean(torch.abs(zn - h.double()) ** tr.loss_exp) / tr.loss_exp).float(), zn.float()

    tr._loss = loss


@pytest.mark.parametrize("name", ["a", "b"])
def test_fused_loss_side_equals_the_torch_op_sequence(name):
    """One forward / backward with functions.ACLossFn against the same with torch's layer_norm and loss (fp32 torch
    autograd of the loss side) on the same HIP predictor, which isolates the new kernels from the bf16 blocks.

    Every ACLossFn call is checked on its own inputs against float64 with the kernel test's analytic bounds (zn,
    loss). The parameter gradients pass through the predictor's backward, whose GEMM operands are rounded to
    bf16: a last-bit difference in dz can move an operand by a bf16 ulp, so two correct f32 loss sides do not give
    the same gradients. The bound is the kernel test's for dz: a third arm runs the loss side in float64, torch's
    own f32 arm is measured against it per parameter (Frobenius norm: single elements of a small tensor cancel),
    and the fused arm is allowed 4 x that, plus one f32 ulp of the gradient's norm where the yardstick is zero.
    The losses likewise: the kernel's analytic bound on its own inputs, plus 4 x the torch arm's distance from
    the float64 arm for sloss, whose inputs went through the predictor again."""
    from vjepa2_amd.functions import ACLossFn, join_wgrad_stream

    tr_h, _, pred_h, _, _, _ = _trainer(name, loss_side="hip")
    tr_t, _, pred_t, _, _, _ = _trainer(name, loss_side="torch")
    tr_d, _, pred_d, _, _, _ = _trainer(name, loss_side="torch")
    _loss_side_f64(tr_d)
    clips, actions, states, extr = _batch(name, 0)
    ext = extr if pred_h.use_extrinsics else None

    calls = []
    real = ACLossFn.apply

    def spy(z, h, normalize, p, eps, want_zn=True):
        out = real(z, h, normalize, p, eps, want_zn)
        calls.append((z.detach(), None if h is None else h.detach(), normalize, p, out))
        return out

    ACLossFn.apply = spy
    try:
        jl_h, sl_h = tr_h.forward_losses(clips, actions, states, ext)
    finally:
        del ACLossFn.apply  # the class's own again
    steps = tr_h.auto_steps
    assert len(calls) == 1 + (steps - 1) + 1  # teacher forcing, the roll-out's normalisations, the rolled loss
    bl = []
    for z, h, normalize, p, (loss, zn) in calls:
        if h is None:
            ref = kt.bounds(z, torch.zeros_like(z), normalize, p)
        else:
            ref = kt.bounds(z, h, normalize, p)
            lerr = abs(float(loss.detach()) - float(ref["loss"]))
            print(f"loss {float(loss.detach()):.7f} err {lerr:.3e} bound {float(ref['bloss']):.3e}")
            assert lerr <= float(ref["bloss"])
            bl.append(float(ref["bloss"]))
        if zn is None:
            assert h is not None and not normalize  # only the rolled frames' loss-only call writes no zn
        else:
            assert bool(((zn.double() - ref["zn"]).abs() <= ref["bzn"]).all())
    assert [c[4][1] is None for c in calls] == [False] * steps + [True]
    (jl_h + sl_h).backward()
    jl_t, sl_t = tr_t.forward_losses(clips, actions, states, ext)
    (jl_t + sl_t).backward()
    jl_d, sl_d = tr_d.forward_losses(clips, actions, states, ext)
    (jl_d + sl_d).backward()
    jl_h, sl_h, jl_t, sl_t, jl_d, sl_d = (float(v.detach()) for v in (jl_h, sl_h, jl_t, sl_t, jl_d, sl_d))
    print(f"jloss fused {jl_h:.7f} torch {jl_t:.7f} f64 {jl_d:.7f}; sloss fused {sl_h:.7f} torch {sl_t:.7f} "
          f"f64 {sl_d:.7f}")
    # the f64 arm's loss was rounded to f32 once: one ulp of its value on top of the kernel's bound
    assert abs(jl_h - jl_d) <= bl[0] + 2.0**-23 * abs(jl_d)
    assert abs(sl_h - sl_d) <= bl[1] + 2.0**-23 * abs(sl_d) + 4 * abs(sl_t - sl_d)
    join_wgrad_stream()
    for tr in (tr_h, tr_t, tr_d):
        for a in tr.pred_arenas:
            a.finalize_grads()
    worst = 0.0
    for (k, ph), (_, pt), (_, pd) in zip(pred_h.named_parameters(), pred_t.named_parameters(),
                                         pred_d.named_parameters()):
        if k.startswith("extrinsics_encoder") and not pred_h.use_extrinsics:
            continue
        gh, gt, gd = ph.grad.double(), pt.grad.double(), pd.grad.double()
        norm = gd.norm().item()
        assert norm > 0, k
        e, y = (gh - gd).norm().item(), (gt - gd).norm().item()
        print(f"  {k}: fused - f64 {e:.3e}, torch f32 - f64 {y:.3e}, norm {norm:.3e}")
        worst = max(worst, e / norm)
        assert e <= 4 * y + 2.0**-23 * norm, \
            f"{k}: fused gradient is {e:.3e} from the float64 arm, torch f32's own distance is {y:.3e} (norm {norm:.3e})"
    print(f"largest ||g_fused - g_f64|| / ||g_f64|| over the parameters: {worst:.3e}")


@pytest.fixture(scope="module")
def trained():
    """Both recorded runs, three steps each, twice: {name: [(log, predictor state, encoder before / after, opt)]}."""
    out = {}
    for name in ("a", "b"):
        runs = []
        for _ in range(2):
            tr, enc, pred, opt, sched, wds = _trainer(name)
            enc0 = {k: v.detach().clone() for k, v in enc.state_dict().items()}
            log = []
            for i in range(fx.load()["micro"]["steps"]):
                clips, actions, states, extr = _batch(name, i)
                lr, wd = sched.step(), wds.step()
                l, jl, sl = tr.train_step(clips, actions, states, extr if pred.use_extrinsics else None).tolist()
                log.append(dict(loss=l, jloss=jl, sloss=sl, lr=lr, wd=wd))
            runs.append((log, {k: v.detach().cpu().clone() for k, v in pred.state_dict().items()}, enc0,
                         {k: v.detach().clone() for k, v in enc.state_dict().items()}, opt.state_dict()))
        out[name] = runs
    return out


@pytest.mark.parametrize("name", ["a", "b"])
def test_three_steps_inside_the_reference_envelope(trained, name):
    run = fx.load()["runs"][name]
    G = run["G"]
    log, final, enc0, enc1, _ = trained[name][0]
    for got, want in zip(log, run["steps"]):
        assert abs(got["lr"] - want["lr"]) <= 1e-12 and abs(got["wd"] - want["wd"]) <= 1e-12
        for q in ("jloss", "sloss"):
            d = abs(got[q] - want[q])
            print(f"{name} {q}: {got[q]:.6f} reference {want[q]:.6f} diff {d:.3e} G_max {G[q][1]:.3e}")
            assert d <= 1.5 * G[q][1], (q, got[q], want[q], G[q])
        assert abs(got["loss"] - (got["jloss"] + got["sloss"])) <= 1e-6 * abs(got["loss"])
    # The final weights: G (mean, max) of the quantity as a whole, and G per tensor: the mean over every element,
    # the maximum over the sign-safe elements. AdamW's first updates are about lr * sign(g) whatever |g|, so an
    # element whose gradient is within the precision's own noise of zero moves by up to 2 lr per step one way or
    # the other, on both sides. The fixture marks, from the reference's two runs alone, the elements with
    # |g_fp32| <= 4 |g_bf16 - g_fp32| at any step (the planning fixture's margin for a decision the bf16 gap may
    # flip); on this micro model that is most of them (run a 91 %, run b 74 %), e.g. element 29 of
    # blocks.1.norm2.weight: g = -1.0e-4 in fp32, -3.5e-5 under bf16 at step 1, which the HIP run moves the other
    # way (1.28e-3 against that tensor's own G_max 7.3e-4). Those are held to the quantity's G_max, which the
    # reference's bf16 run saturates the same way; every other element to its tensor's.
    import numpy as np

    assert list(final) == list(run["final_predictor"])
    diffs = {k: (final[k].double() - want.double()).abs() for k, want in run["final_predictor"].items()}
    numel = sum(d.numel() for d in diffs.values())
    g_mean = sum(G["final_predictor"][k][0] * d.numel() for k, d in diffs.items()) / numel
    g_max = max(v[1] for v in G["final_predictor"].values())
    d_mean = sum(d.sum().item() for d in diffs.values()) / numel
    d_max = max(d.max().item() for d in diffs.values())
    print(f"{name} final weights: mean diff {d_mean:.3e} (G {g_mean:.3e}), max diff {d_max:.3e} (G {g_max:.3e})")
    assert d_mean <= 1.5 * g_mean and d_max <= 1.5 * g_max, (d_mean, g_mean, d_max, g_max)
    n_safe = 0
    for k, d in diffs.items():
        gmean, gmax = G["final_predictor"][k]
        assert d.mean().item() <= 1.5 * gmean, (k, d.mean().item(), gmean)
        unsafe = torch.from_numpy(np.unpackbits(run["sign_unsafe"][k].numpy())[:d.numel()].astype(bool)).view(d.shape)
        safe = d[~unsafe]
        n_safe += safe.numel()
        if safe.numel():
            j = int(torch.where(unsafe, torch.zeros_like(d), d).reshape(-1).argmax())
            print(f"{name} {k}: {safe.numel()} of {d.numel()} sign-safe, max diff {safe.max().item():.3e} (element {j}), "
                  f"tensor G_max {gmax:.3e}; over all elements {d.max().item():.3e}")
            assert safe.max().item() <= 1.5 * gmax, (k, j, safe.max().item(), gmax)
    assert 0 < n_safe < numel
    assert all(torch.equal(enc0[k], enc1[k]) for k in enc0)  # the frozen encoder is bit-identical


@pytest.mark.parametrize("name", ["a", "b"])
def test_three_steps_are_reproducible_and_lay_out_the_optimizer_state(trained, name):
    (log1, w1, _, _, opt1), (log2, w2, _, _, _) = trained[name]
    assert log1 == log2
    assert all(torch.equal(w1[k], w2[k]) for k in w1)
    rec = fx.load()["runs"][name]["opt"]
    assert [len(g["params"]) for g in opt1["param_groups"]] == rec["group_sizes"]
    assert [sorted(k for k in g if k != "params") for g in opt1["param_groups"]] == rec["group_keys"]
    assert sorted(opt1["state"]) == rec["state_ids"]  # no encoder state; no extrinsics state where they are unused
    assert [float(opt1["state"][k]["step"]) for k in sorted(opt1["state"])] == rec["state_steps"]


# ------------------------------------------------------------------------------------------------ the app
class _Interrupted(Exception):
    pass


def test_main_end_to_end_and_resume(tmp_path, monkeypatch):
    from vjepa2_amd import droid
    from vjepa2_amd import vision_transformer as vt
    from vjepa2_amd.schedulers import WSDSchedule

    monkeypatch.setattr(vt, "vit_micro", fx.vit_micro, raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    run = fx.load()["runs"]["a"]
    args = {k: dict(v) if isinstance(v, dict) else v for k, v in run["args"].items()}
    args["app"] = "vjepa_droid"
    args["meta"]["pretrain_checkpoint"] = fx.checkpoint("a", str(tmp_path / "micro_pretrained.pt"))
    args["data"]["num_samples"] = 64
    args["optimization"].update(epochs=2, ipe=2, warmup=0.5, anneal=0.5)

    def launch(folder):
        a = dict(args, folder=str(tmp_path / folder))
        p = tmp_path / f"{folder}.yaml"
        p.write_text(yaml.dump(a))
        return droid.main(droid.load_params(str(p)))

    full = launch("full")
    assert len(full) == 4
    ck = torch.load(tmp_path / "full" / "latest.pt", weights_only=True)
    assert sorted(ck) == run["ck_keys"] and ck["epoch"] == 2 and ck["scaler"] is None
    assert (ck["batch_size"], ck["world_size"], ck["lr"]) == (run["ck_meta"]["batch_size"], 1, run["ck_meta"]["lr"])
    assert all(k.startswith("module.") for k in ck["predictor"]) and list(ck["encoder"]) == list(ck["target_encoder"])
    assert all(torch.equal(ck["encoder"][k], ck["target_encoder"][k]) for k in ck["encoder"])  # one encoder, two keys
    rec = run["opt"]
    assert [len(g["params"]) for g in ck["opt"]["param_groups"]] == rec["group_sizes"]
    assert [sorted(k for k in g if k != "params") for g in ck["opt"]["param_groups"]] == rec["group_keys"]
    assert sorted(ck["opt"]["state"]) == rec["state_ids"]
    assert all(float(s["step"]) == 4.0 for s in ck["opt"]["state"].values())
    with open(tmp_path / "full" / "log_r0.csv") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["epoch", "itr", "loss", "iter-time(ms)", "gpu-time(ms)", "dataload-time(ms)"]
    assert [r[:2] for r in rows[1:]] == [["1", "0"], ["1", "1"], ["2", "0"], ["2", "1"]]
    assert [r[2] for r in rows[1:]] == [f"{v:.5f}" for v in full]

    # the same run, stopped after the first epoch's checkpoint, then started again
    real_save = droid.save_checkpoint

    def save_then_stop(*a, **kw):
        real_save(*a, **kw)
        raise _Interrupted

    monkeypatch.setattr(droid, "save_checkpoint", save_then_stop)
    with pytest.raises(_Interrupted):
        launch("resumed")
    monkeypatch.setattr(droid, "save_checkpoint", real_save)
    assert torch.load(tmp_path / "resumed" / "latest.pt", weights_only=True)["epoch"] == 1
    resumed = launch("resumed")
    assert len(resumed) == 2  # epoch 2 only
    assert torch.equal(torch.tensor(resumed[0]), torch.tensor(full[2])), (resumed, full)
    assert torch.equal(torch.tensor(resumed), torch.tensor(full[2:]))
    ck2 = torch.load(tmp_path / "resumed" / "latest.pt", weights_only=True)
    assert ck2["epoch"] == 2
    assert all(torch.equal(ck2["predictor"][k], ck["predictor"][k]) for k in ck["predictor"])
    # the schedulers were advanced by start_epoch * ipe steps: the last rate is the fourth step's
    co = args["optimization"]
    s = WSDSchedule(type("O", (), dict(param_groups=[{}]))(), warmup_steps=1, anneal_steps=1, T_max=4,
                    start_lr=co["start_lr"], ref_lr=co["lr"], final_lr=co["final_lr"])
    want = [s.step() for _ in range(4)][-1]
    assert ck2["opt"]["param_groups"][1]["lr"] == want == ck["opt"]["param_groups"][1]["lr"]
    with open(tmp_path / "resumed" / "log_r0.csv") as f:
        rows = list(csv.reader(f))
    assert [r[:2] for r in rows[1:]] == [["1", "0"], ["1", "1"], ["2", "0"], ["2", "1"]]
