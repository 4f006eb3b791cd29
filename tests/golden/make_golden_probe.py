"""Generate tests/golden/probe_steps.pt by running the REFERENCE's frozen-encoder probe training
(evals/video_classification_frozen/eval.py) on CPU.

Like make_golden.py this runs in the build container only, executes the reference read-only mounted at
/root/reference and copies none of its text: the fixture holds inputs, recorded results and settings.

Stubs: ``timm.models.layers.drop_path`` (inert: the probe has no stochastic depth) and
``evals.video_classification_frozen.utils.make_transforms`` (torchvision is absent; no clip is decoded).

With those, eval.py imports. Its ``run_one_epoch`` returns only the epoch's best accuracy and reads the
CUDA allocator, so the per-iteration quantities are recorded by driving the same sequence from its
imported pieces: ``AttentiveClassifier`` (src/models/attentive_pooler.py), eval.py's own ``init_opt``
(torch.optim.AdamW + WarmupCosineLRSchedule + CosineWDSchedule) and ``AverageMeter``
(src/utils/logging.py), in run_one_epoch's order (eval.py:301-341): schedulers, every classifier on every
view, ``torch.nn.CrossEntropyLoss()`` per view, the view-averaged ``F.softmax`` top-1, one backward per
view loss, the optimizers, zero_grad. The encoder is replaced by fixed tokens (its output is an input
of the probe step). The same four iterations run twice: in fp32, and with the classifiers' forward
under ``torch.autocast("cpu", dtype=torch.bfloat16)`` (the reference's mixed-precision branch with the
device's 16-bit type; loss scale 1; the loss and softmax then see 16-bit logits, as in the reference).
The gap between the two runs is the envelope G the HIP path is held to (tests/test_gpu_probe.py).

Size. Three classifiers of width 64 and depth 2 are 3 x 47 k parameters even at mlp_ratio 1, so the
initial weights, iteration-0 gradients, final weights and both AdamW moments in fp32 would be ~3 MB.
To stay under 1 MB in one file:
  * the initial state_dict()s are NOT stored: they are a function of cfg["init_seed"] (constructor +
    perturbation draws, restated in tests/probe_fixture.py) and the fixture keeps each tensor's
    (sum, sum of squares) so a loader can tell that it rebuilt the same weights;
  * tokens are rounded to bf16 before either run and stored as bf16 (exact);
  * iteration-0 gradients are stored as bf16 (2^-9 relative, against a 4e-2 bound), the final fp32-run
    weights as fp16 differences from the initial weights (|d| ~ 1e-3: about 1e-6 absolute);
  * of the bf16 run's final weights only the distance to the fp32 run's is kept (G_w per head), measured
    to the fp32 run's weights AS STORED (initial + fp16 difference), the same point a test measures from;
  * the optimizers' param_groups are stored for every head, the moment tensors for head 1 only (bf16).

Usage:  python tests/golden/make_golden_probe.py     (writes tests/golden/probe_steps.pt)
"""

import contextlib
import os
import sys
import types

sys.dont_write_bytecode = True  # never write __pycache__ into the reference tree
REF = os.environ.get("VJEPA_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

timm = types.ModuleType("timm")
timm_models = types.ModuleType("timm.models")
timm_layers = types.ModuleType("timm.models.layers")
timm_layers.drop_path = lambda x, drop_prob=0.0, training=False, scale_by_keep=True: x
timm.models = timm_models
timm_models.layers = timm_layers
sys.modules.update({"timm": timm, "timm.models": timm_models, "timm.models.layers": timm_layers})
sys.path.insert(0, REF)
ut_mod = types.ModuleType("evals.video_classification_frozen.utils")
ut_mod.make_transforms = lambda **kw: (lambda x: x)
sys.modules["evals.video_classification_frozen.utils"] = ut_mod

import evals.video_classification_frozen.eval as ev  # noqa: E402
from src.models.attentive_pooler import AttentiveClassifier  # noqa: E402
from src.utils.logging import AverageMeter  # noqa: E402

torch.set_num_threads(8)

CFG = dict(embed_dim=64, num_heads=2, depth=2, mlp_ratio=1.0, num_classes=11, B=3, V=2, N=32, ipe=4, num_epochs=2,
           iters=4, init_seed=31, opt_state_head=1)
MULTIHEAD = [dict(lr=1e-3, start_lr=2e-4, final_lr=0.0, weight_decay=0.01, final_weight_decay=0.01, warmup=0.0),
             dict(lr=3e-3, start_lr=1e-4, final_lr=1e-5, weight_decay=0.1, final_weight_decay=0.4, warmup=0.5),
             dict(lr=5e-4, start_lr=5e-4, final_lr=1e-4, weight_decay=0.4, final_weight_decay=0.05, warmup=1.0)]


def _classifier():
    c = CFG
    return AttentiveClassifier(embed_dim=c["embed_dim"], num_heads=c["num_heads"], depth=c["depth"],
                               mlp_ratio=c["mlp_ratio"], num_classes=c["num_classes"],
                               use_activation_checkpointing=True)


def _init_states():
    """One seed, then per head: the constructor's draws, then 0.05 * randn_like per parameter in
    parameters() order (non-trivial LayerNorm / bias / query values)."""
    torch.manual_seed(CFG["init_seed"])
    states = []
    for _ in MULTIHEAD:
        m = _classifier()
        with torch.no_grad():
            for p in m.parameters():
                p.add_(0.05 * torch.randn_like(p))
        states.append({k: v.detach().clone() for k, v in m.state_dict().items()})
    return states


def _inputs(seed):
    g = torch.Generator().manual_seed(seed)
    c = CFG
    tokens = [[torch.randn(c["B"], c["N"], c["embed_dim"], generator=g).bfloat16() for _ in range(c["V"])]
              for _ in range(c["iters"] + 1)]  # the last entry is the validation iteration
    labels = [torch.randint(0, c["num_classes"], (c["B"],), generator=g) for _ in range(c["iters"] + 1)]
    return tokens, labels


def _run(init_states, tokens, labels, bf16):
    c = CFG
    clfs = []
    for sd in init_states:
        m = _classifier()
        m.load_state_dict(sd)
        clfs.append(m)
    opt_kwargs = [dict(ref_wd=k["weight_decay"], final_wd=k["final_weight_decay"], start_lr=k["start_lr"],
                       ref_lr=k["lr"], final_lr=k["final_lr"], warmup=k["warmup"]) for k in MULTIHEAD]
    opts, _, scheds, wd_scheds = ev.init_opt(classifiers=clfs, opt_kwargs=opt_kwargs, iterations_per_epoch=c["ipe"],
                                             num_epochs=c["num_epochs"], use_bfloat16=False)
    criterion = torch.nn.CrossEntropyLoss()
    cast = (lambda: torch.autocast("cpu", dtype=torch.bfloat16)) if bf16 else contextlib.nullcontext
    rec = dict(losses=[], top1=[], pred=[], lr=[], wd=[], meter=[], margin=[])
    meters = [AverageMeter() for _ in clfs]
    for itr in range(c["iters"] + 1):
        training = itr < c["iters"]
        if not training:
            meters = [AverageMeter() for _ in clfs]
        for m in clfs:
            m.train(mode=training)
        if training:
            [s.step() for s in scheds]
            [s.step() for s in wd_scheds]
            rec["lr"].append([o.param_groups[0]["lr"] for o in opts])
            rec["wd"].append([o.param_groups[0]["weight_decay"] for o in opts])
        lab = labels[itr]
        with cast(), torch.set_grad_enabled(training):
            outputs = [[m(o.float()) for o in tokens[itr]] for m in clfs]
        if itr == 0:
            rec["logits0"] = [torch.cat([o.detach().float() for o in co], 0) for co in outputs]
        losses = [[criterion(o, lab) for o in co] for co in outputs]
        with torch.no_grad():
            probs = [sum([F.softmax(o, dim=1) for o in co]) / len(co) for co in outputs]
            pred = [p.max(dim=1).indices for p in probs]
            top1 = [float(100.0 * p.eq(lab).sum() / len(lab)) for p in pred]
            for t1m, t1a in zip(meters, top1):
                t1m.update(t1a)
            top2 = [p.float().topk(2, dim=1).values for p in probs]
            rec["margin"].append(min(float((t[:, 0] / t[:, 1]).min()) for t in top2))
        rec["losses"].append(torch.tensor([[float(x) for x in li] for li in losses], dtype=torch.float64))
        rec["top1"].append(top1)
        rec["pred"].append(torch.stack(pred))
        rec["meter"].append([m.avg for m in meters])
        if training:
            [[lij.backward() for lij in li] for li in losses]
            if itr == 0:
                rec["grads0"] = [{n: p.grad.detach().clone() for n, p in m.named_parameters()} for m in clfs]
            [o.step() for o in opts]
            [o.zero_grad() for o in opts]
    rec["losses"] = torch.stack(rec["losses"])  # [iters + 1, heads, views]
    rec["pred"] = torch.stack(rec["pred"])      # [iters + 1, heads, B]
    rec["weights"] = [{k: v.detach().clone() for k, v in m.state_dict().items()} for m in clfs]
    rec["opt"] = [o.state_dict() for o in opts]
    return rec


def _flat(sd):
    return torch.cat([v.reshape(-1).double() for v in sd.values()])


def gen_probe_steps():
    c = CFG
    init_states = _init_states()
    init_sums = [{k: (v.double().sum().item(), v.double().pow(2).sum().item()) for k, v in sd.items()}
                 for sd in init_states]
    # a seed whose fp32 and bf16 runs agree on every sample's top-1 on at least 3 of the 5 iterations
    for seed in range(40, 140):
        tokens, labels = _inputs(seed)
        f32 = _run(init_states, tokens, labels, bf16=False)
        b16 = _run(init_states, tokens, labels, bf16=True)
        agree = [bool(torch.equal(f32["pred"][i], b16["pred"][i])) for i in range(c["iters"] + 1)]
        print(f"seed {seed}: top-1 agreement per iteration {agree}, fp32 top-1 / top-2 margins {f32['margin']}")
        # ... and whose agreeing iterations are decided by more than 16-bit rounding: fp32 top-1 / top-2 >= 1.01
        if sum(agree) >= 3 and all(m >= 1.01 for a, m in zip(agree, f32["margin"]) if a):
            break
    else:
        raise SystemExit("no seed found")
    # the fp32 run's final weights as the fixture stores them (fp16 differences from the initial weights):
    # the point both the bf16 run here and the HIP run in the test are measured against
    wdelta = [{k: (w[k] - i[k]).half() for k in w} for w, i in zip(f32["weights"], init_states)]
    stored = [{k: i[k] + dl[k].float() for k in i} for i, dl in zip(init_states, wdelta)]
    print("fp16 storage of the final weights: mean |stored - exact|",
          [(_flat(a) - _flat(b)).abs().mean().item() for a, b in zip(stored, f32["weights"])])
    gaps = dict(
        loss=(b16["losses"] - f32["losses"]).abs().mean().item(),
        logits=[(a - b).abs().mean().item() for a, b in zip(b16["logits0"], f32["logits0"])],
        weights=[(_flat(a) - _flat(b)).abs().mean().item() for a, b in zip(b16["weights"], stored)])
    print("envelope G (reference bf16 autocast vs its fp32):", gaps)
    print("fp32 losses", f32["losses"].flatten().tolist())
    print("bf16 losses", b16["losses"].flatten().tolist())
    print("fp32 top-1", f32["top1"], "bf16 top-1", b16["top1"])
    small = ("losses", "top1", "pred", "meter", "logits0", "margin")
    h = c["opt_state_head"]
    out = dict(cfg=dict(CFG), multihead_kwargs=[dict(k) for k in MULTIHEAD], seed=seed, init_sums=init_sums,
               tokens=tokens, labels=labels, agree=agree, gaps=gaps,
               f32={k: f32[k] for k in small + ("lr", "wd")}, bf16={k: b16[k] for k in small})
    out["f32"]["grads0"] = [{n: g.bfloat16() for n, g in gd.items()} for gd in f32["grads0"]]
    out["f32"]["wdelta"] = wdelta
    out["f32"]["opt_groups"] = [o["param_groups"] for o in f32["opt"]]
    out["f32"]["opt_state"] = {pid: dict(step=st["step"].clone(), exp_avg=st["exp_avg"].bfloat16(),
                                         exp_avg_sq=st["exp_avg_sq"].bfloat16())
                               for pid, st in f32["opt"][h]["state"].items()}
    path = os.path.join(OUT, "probe_steps.pt")
    torch.save(out, path)
    print(f"wrote {path} ({os.path.getsize(path) / 1e3:.1f} kB)")
    torch.load(path, weights_only=True)  # tensors and scalars only


if __name__ == "__main__":
    gen_probe_steps()
