"""Generate tests/golden/anticipation_steps.pt by running the REFERENCE's frozen action-anticipation eval
(evals/action_anticipation_frozen) on CPU.

Like make_golden_probe.py this runs in the build container only, executes the reference read-only mounted at
/root/reference and copies none of its text: the fixture holds inputs, recorded results and settings.

Stub: ``timm.models.layers.drop_path`` (inert: no stochastic depth here). With it the reference's
``losses``, ``metrics``, ``models`` and ``modelcustom.vit_encoder_predictor_concat_ar`` import and run on the
CPU. ``ClassMeanRecall`` all-reduces its counters, so a one-rank gloo group on a file store is opened.

(a) wrapper: a tiny RoPE encoder (4 frames of 16 x 16, patch 8: N = 8 tokens) and RoPE predictor (16 frames:
    32 positions) with seeded + perturbed weights, ``AnticipativeWrapper`` with num_steps 1 and 2 on a clip
    batch with three different anticipation times, in fp32 and under ``torch.autocast("cpu", bfloat16)``.
    Weights are not stored: they are a function of cfg["seed"], and per-tensor (sum, sum of squares) let a
    loader tell that it rebuilt the same ones.
(b) probe: three ``AttentiveClassifier``s (models.py; depth 2, width 64, 2 heads; the pooler's mlp_ratio is set
    to 1 through the name models.py looks up, to keep the fixture small; 7 verbs, 9 nouns, 13 actions) driven
    in eval.py's order (:479-535, :629-665): schedulers, forward of every classifier, ``sigmoid_focal_loss``
    per head, loss = verb + noun + action, backward, AdamW, zero_grad, ``ClassMeanRecall`` per head; four
    training iterations and one validation iteration whose metrics get non-trivial valid-class sets (the
    validation labels lie inside them, as labels of a validation set do). The metric is called one sample at
    a time, which changes none of its sums and shows each sample's hit flag as the counter that moved. Run
    twice, in fp32 and with the classifiers' forward under bf16 autocast (the losses then see 16-bit logits).
    A seed is kept whose two runs agree on every hit flag in at least 3 of the 5 iterations and where, in those
    iterations, the label's logit is further than 4 G_logits (mean |bf16 - fp32| of the iteration-0 logits) from
    the k-th and (k+1)-th largest valid logits of its row.
(c) label maps: epickitchens.py:227-241's set arithmetic on a small list of (verb, noun) pairs. The annotation
    reader needs pandas, which is absent, so the same expressions are evaluated here on the pair lists.

Usage:  python tests/golden/make_golden_anticipation.py     (writes tests/golden/anticipation_steps.pt)
"""

import contextlib
import functools
import os
import sys
import tempfile
import types

sys.dont_write_bytecode = True  # never write __pycache__ into the reference tree
REF = os.environ.get("VJEPA_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

timm = types.ModuleType("timm")
timm_models = types.ModuleType("timm.models")
timm_layers = types.ModuleType("timm.models.layers")
timm_layers.drop_path = lambda x, drop_prob=0.0, training=False, scale_by_keep=True: x
timm.models = timm_models
timm_models.layers = timm_layers
sys.modules.update({"timm": timm, "timm.models": timm_models, "timm.models.layers": timm_layers})
sys.path.insert(0, REF)

import evals.action_anticipation_frozen.models as ref_models  # noqa: E402
import evals.action_anticipation_frozen.modelcustom.vit_encoder_predictor_concat_ar as ref_wrap  # noqa: E402
import src.models.predictor as vpred  # noqa: E402
import src.models.vision_transformer as vit  # noqa: E402
from evals.action_anticipation_frozen.losses import sigmoid_focal_loss  # noqa: E402
from evals.action_anticipation_frozen.metrics import ClassMeanRecall  # noqa: E402
from evals.action_anticipation_frozen.utils import CosineWDSchedule, WarmupCosineLRSchedule  # noqa: E402
from src.models.attentive_pooler import AttentivePooler  # noqa: E402

torch.set_num_threads(8)
HEADS = ("verb", "noun", "action")
K = 5

WCFG = dict(seed=51, img_size=16, patch_size=8, clip_frames=4, pred_frames=16, tubelet_size=2, embed_dim=64,
            enc_depth=2, pred_depth=2, num_heads=2, pred_embed_dim=64, mlp_ratio=2.0, num_mask_tokens=2, fps=4,
            num_output_frames=2, times=[0.0, 0.5, 1.5])
CFG = dict(embed_dim=64, num_heads=2, depth=2, mlp_ratio=1.0, verbs=7, nouns=9, actions=13, B=4, N=24, ipe=4,
           num_epochs=2, iters=4, init_seed=37, k=K, alpha=0.25, gamma=2.0)
MULTIHEAD = [dict(lr=1e-3, start_lr=2e-4, final_lr=0.0, weight_decay=0.01, final_weight_decay=0.01, warmup=0.0),
             dict(lr=3e-3, start_lr=1e-4, final_lr=1e-5, weight_decay=0.1, final_weight_decay=0.4, warmup=0.5),
             dict(lr=5e-4, start_lr=5e-4, final_lr=1e-4, weight_decay=0.4, final_weight_decay=0.05, warmup=1.0)]
VALID = dict(verb=[0, 2, 3, 5, 6], noun=[1, 2, 4, 6, 7, 8], action=[0, 1, 3, 4, 7, 8, 10, 12])
PAIRS = dict(train=[(3, 10), (3, 4), (0, 10), (7, 2), (3, 10), (12, 4), (0, 2), (7, 7), (5, 10), (12, 300), (41, 2)],
             val=[(3, 4), (9, 9), (0, 10), (7, 4), (12, 300), (3, 10), (41, 2), (41, 7), (0, 2)])


def _sums(sd):
    return {k: (v.double().sum().item(), v.double().pow(2).sum().item()) for k, v in sd.items()}


def _perturb(m):
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.05 * torch.randn_like(p))


# ------------------------------------------------------------------------------------------------ (a)
def gen_wrapper():
    c = WCFG
    norm = functools.partial(torch.nn.LayerNorm, eps=1e-6)
    torch.manual_seed(c["seed"])
    enc = vit.VisionTransformer(img_size=c["img_size"], patch_size=c["patch_size"], num_frames=c["clip_frames"],
                                tubelet_size=c["tubelet_size"], embed_dim=c["embed_dim"], depth=c["enc_depth"],
                                num_heads=c["num_heads"], mlp_ratio=c["mlp_ratio"], qkv_bias=True, use_rope=True,
                                uniform_power=True, norm_layer=norm)
    pred = vpred.vit_predictor(img_size=c["img_size"], patch_size=c["patch_size"], num_frames=c["pred_frames"],
                               tubelet_size=c["tubelet_size"], embed_dim=c["embed_dim"],
                               predictor_embed_dim=c["pred_embed_dim"], depth=c["pred_depth"], num_heads=c["num_heads"],
                               uniform_power=True, use_mask_tokens=True, num_mask_tokens=c["num_mask_tokens"],
                               zero_init_mask_tokens=False, use_rope=True)
    _perturb(enc)
    _perturb(pred)
    enc.eval(), pred.eval()
    g = torch.Generator().manual_seed(c["seed"] + 1)
    clips = torch.randn(len(c["times"]), 3, c["clip_frames"], c["img_size"], c["img_size"], generator=g).bfloat16()
    times = torch.tensor(c["times"], dtype=torch.float32)
    out = dict(cfg=dict(c), clips=clips, times=times, enc_sums=_sums(enc.state_dict()),
               pred_sums=_sums(pred.state_dict()), f32={}, bf16={}, gaps={})
    for steps in (1, 2):
        w = ref_wrap.AnticipativeWrapper(encoder=enc, predictor=pred, frames_per_second=c["fps"],
                                         crop_size=c["img_size"], patch_size=c["patch_size"],
                                         tubelet_size=c["tubelet_size"], num_output_frames=c["num_output_frames"],
                                         num_steps=steps)
        with torch.no_grad():
            y32 = w(clips.float(), times)
            with torch.autocast("cpu", dtype=torch.bfloat16):
                y16 = w(clips.float(), times).float()
        d = (y16 - y32).abs()
        out["f32"][steps], out["bf16"][steps] = y32, y16.bfloat16()
        out["gaps"][steps] = dict(mean=d.mean().item(), max=d.max().item())
        print(f"wrapper num_steps {steps}: output {tuple(y32.shape)}, |bf16 - fp32| mean {d.mean():.3e} max {d.max():.3e}, "
              f"mean |y| {y32.abs().mean():.3e}")
    return out


# ------------------------------------------------------------------------------------------------ (b)
def _classifier():
    c = CFG
    ref_models.AttentivePooler = functools.partial(AttentivePooler, mlp_ratio=c["mlp_ratio"])
    try:
        return ref_models.AttentiveClassifier(
            verb_classes={i: i for i in range(c["verbs"])}, noun_classes={i: i for i in range(c["nouns"])},
            action_classes={i: i for i in range(c["actions"])}, embed_dim=c["embed_dim"], num_heads=c["num_heads"],
            depth=c["depth"], use_activation_checkpointing=True)
    finally:
        ref_models.AttentivePooler = AttentivePooler


def _init_states(n=len(MULTIHEAD)):
    """One seed, then per classifier: the constructor's draws, then 0.05 * randn_like per parameter in
    parameters() order."""
    torch.manual_seed(CFG["init_seed"])
    states = []
    for _ in range(n):
        m = _classifier()
        _perturb(m)
        states.append({k: v.detach().clone() for k, v in m.state_dict().items()})
    return states


def _action_only_sums():
    """The action-only variant (no verb classes): keys and seeded init only."""
    c = CFG
    torch.manual_seed(c["init_seed"] + 1)
    ref_models.AttentivePooler = functools.partial(AttentivePooler, mlp_ratio=c["mlp_ratio"])
    try:
        m = ref_models.AttentiveClassifier(verb_classes={}, noun_classes={},
                                           action_classes={i: i for i in range(c["actions"])},
                                           embed_dim=c["embed_dim"], num_heads=c["num_heads"], depth=c["depth"],
                                           use_activation_checkpointing=True)
    finally:
        ref_models.AttentivePooler = AttentivePooler
    return _sums(m.state_dict())


def _inputs(seed):
    g = torch.Generator().manual_seed(seed)
    c = CFG
    n = c["iters"] + 1  # the last entry is the validation iteration
    tokens = [torch.randn(c["B"], c["N"], c["embed_dim"], generator=g).bfloat16() for _ in range(n)]
    labels = []
    for it in range(n):
        lab = {}
        for h in HEADS:
            C = c[h + "s"]
            if it < c["iters"]:
                lab[h] = torch.randint(0, C, (c["B"],), generator=g)
            else:  # validation labels lie inside the valid sets
                v = torch.tensor(VALID[h])
                lab[h] = v[torch.randint(0, len(v), (c["B"],), generator=g)]
        labels.append(lab)
    return tokens, labels


def _init_opt(clfs):
    """eval.py's init_opt (utils.py): AdamW with one decayed group carrying the mc_* constants + both schedules."""
    c = CFG
    opts, scheds, wds = [], [], []
    for m, k in zip(clfs, MULTIHEAD):
        groups = [dict(params=(p for n, p in m.named_parameters()), mc_warmup_steps=int(k["warmup"] * c["ipe"]),
                       mc_start_lr=k["start_lr"], mc_ref_lr=k["lr"], mc_final_lr=k["final_lr"],
                       mc_ref_wd=k["weight_decay"], mc_final_wd=k["final_weight_decay"])]
        o = torch.optim.AdamW(groups)
        opts.append(o)
        scheds.append(WarmupCosineLRSchedule(o, T_max=int(c["num_epochs"] * c["ipe"])))
        wds.append(CosineWDSchedule(o, T_max=int(c["num_epochs"] * c["ipe"])))
    return opts, scheds, wds


def _margin(logits, label, valid):
    """min over the row's k-th and (k+1)-th largest valid logits of |x_label - that logit| (inf where the row
    has no such rank)."""
    x = logits.float()
    C = x.numel()
    idx = list(range(C)) if valid is None else [i for i in valid]
    order = sorted(idx, key=lambda i: float(x[i]), reverse=True)
    xl = float(x[int(label)])
    out = float("inf")
    for r in (K - 1, K):  # the k-th and (k+1)-th largest: the two sides of the top-k boundary
        if r < len(order) and order[r] != int(label):
            out = min(out, abs(xl - float(x[order[r]])))
    return out


def _run(init_states, tokens, labels, bf16):
    c = CFG
    clfs = []
    for sd in init_states:
        m = _classifier()
        m.load_state_dict(sd)
        clfs.append(m)
    opts, scheds, wd_scheds = _init_opt(clfs)
    cast = (lambda: torch.autocast("cpu", dtype=torch.bfloat16)) if bf16 else contextlib.nullcontext
    dev = torch.device("cpu")
    counts = dict(verb=c["verbs"], noun=c["nouns"], action=c["actions"])
    rec = dict(losses=[], hits=[], tp=[], fn=[], metrics=[], lr=[], wd=[], margin=[])
    loggers = {h: [ClassMeanRecall(num_classes=counts[h], device=dev, k=K) for _ in clfs] for h in HEADS}
    for itr in range(c["iters"] + 1):
        training = itr < c["iters"]
        if not training:
            loggers = {h: [ClassMeanRecall(num_classes=counts[h], device=dev, k=K) for _ in clfs] for h in HEADS}
        for m in clfs:
            m.train(mode=training)
        if training:
            [s.step() for s in scheds]
            [s.step() for s in wd_scheds]
            rec["lr"].append([o.param_groups[0]["lr"] for o in opts])
            rec["wd"].append([o.param_groups[0]["weight_decay"] for o in opts])
        lab = labels[itr]
        with cast(), torch.set_grad_enabled(training):
            outputs = [m(tokens[itr].float()) for m in clfs]
        if itr == 0:
            rec["logits0"] = [{h: o[h].detach().float().clone() for h in HEADS} for o in outputs]
        with torch.set_grad_enabled(training):
            per = [[sigmoid_focal_loss(o[h].float(), lab[h]) for h in HEADS] for o in outputs]
            loss = [a + b + d for a, b, d in per]
        rec["losses"].append(torch.tensor([[float(x) for x in li] for li in per], dtype=torch.float64))
        if training:
            [L.backward() for L in loss]
            if itr == 0:
                rec["grads0"] = [{n: p.grad.detach().clone() for n, p in m.named_parameters()} for m in clfs]
            [o.step() for o in opts]
            [o.zero_grad() for o in opts]
        hits = torch.zeros(len(clfs), len(HEADS), c["B"], dtype=torch.int32)
        last = {}
        margin = float("inf")
        with torch.no_grad():
            for i, o in enumerate(outputs):
                for s, h in enumerate(HEADS):
                    valid = None if training else set(VALID[h])
                    m = loggers[h][i]
                    for b in range(c["B"]):
                        before = float(m.TP[lab[h][b]])
                        last[(h, i)] = m(o[h][b:b + 1].detach().float(), lab[h][b:b + 1], valid_classes=valid)
                        hits[i, s, b] = int(float(m.TP[lab[h][b]]) - before)
                        margin = min(margin, _margin(o[h][b].detach(), lab[h][b], None if training else VALID[h]))
        rec["hits"].append(hits)
        rec["margin"].append(margin)
        rec["tp"].append([{h: loggers[h][i].TP.to(torch.int32).clone() for h in HEADS} for i in range(len(clfs))])
        rec["fn"].append([{h: loggers[h][i].FN.to(torch.int32).clone() for h in HEADS} for i in range(len(clfs))])
        rec["metrics"].append([{h: dict(recall=float(last[(h, i)]["recall"]), accuracy=float(last[(h, i)]["accuracy"]))
                                for h in HEADS} for i in range(len(clfs))])
    rec["losses"] = torch.stack(rec["losses"])  # [iters + 1, classifiers, heads]
    rec["hits"] = torch.stack(rec["hits"])      # [iters + 1, classifiers, heads, B]
    rec["weights"] = [{k: v.detach().clone() for k, v in m.state_dict().items()} for m in clfs]
    return rec


def _flat(sd):
    return torch.cat([v.reshape(-1).double() for v in sd.values()])


def gen_probe():
    c = CFG
    init_states = _init_states()
    init_sums = [_sums(sd) for sd in init_states]
    for seed in range(60, 260):
        tokens, labels = _inputs(seed)
        f32 = _run(init_states, tokens, labels, bf16=False)
        b16 = _run(init_states, tokens, labels, bf16=True)
        dl = torch.cat([(b16["logits0"][i][h] - f32["logits0"][i][h]).abs().flatten()
                        for i in range(len(init_states)) for h in HEADS])
        g_logits = dict(mean=dl.mean().item(), max=dl.max().item())
        agree = [bool(torch.equal(f32["hits"][i], b16["hits"][i])) for i in range(c["iters"] + 1)]
        qualify = [a and m > 4 * g_logits["mean"] for a, m in zip(agree, f32["margin"])]
        print(f"seed {seed}: hit agreement {agree}, fp32 margins {[round(m, 5) for m in f32['margin']]}, "
              f"G_logits {g_logits}, qualify {qualify}")
        if sum(qualify) >= 3:
            break
    else:
        raise SystemExit("no seed found")
    wdelta = [{k: (w[k] - i[k]).half() for k in w} for w, i in zip(f32["weights"], init_states)]
    stored = [{k: i[k] + d[k].float() for k in i} for i, d in zip(init_states, wdelta)]
    dloss = (b16["losses"] - f32["losses"]).abs()
    gaps = dict(loss=dict(mean=dloss.mean().item(), max=dloss.max().item()), logits=g_logits,
                weights=[(_flat(a) - _flat(b)).abs().mean().item() for a, b in zip(b16["weights"], stored)],
                weights_max=[(_flat(a) - _flat(b)).abs().max().item() for a, b in zip(b16["weights"], stored)])
    print("envelope G (reference bf16 autocast vs its fp32):", gaps)
    print("fp32 losses", f32["losses"].flatten().tolist())
    print("fp32 metrics (last training iteration, validation)", f32["metrics"][c["iters"] - 1], f32["metrics"][-1])
    small = ("losses", "hits", "tp", "fn", "metrics", "margin")
    out = dict(cfg=dict(CFG), multihead_kwargs=[dict(k) for k in MULTIHEAD], valid={h: list(v) for h, v in VALID.items()},
               seed=seed, init_sums=init_sums, action_only_sums=_action_only_sums(), tokens=tokens, labels=labels,
               agree=agree, qualify=qualify, gaps=gaps,
               f32={k: f32[k] for k in small + ("lr", "wd")}, bf16={k: b16[k] for k in small})
    out["f32"]["logits0"] = [{h: v.bfloat16() for h, v in d.items()} for d in f32["logits0"]]
    out["bf16"]["logits0"] = [{h: v.bfloat16() for h, v in d.items()} for d in b16["logits0"]]
    out["f32"]["grads0"] = [{n: g.bfloat16() for n, g in gd.items()} for gd in f32["grads0"]]
    out["f32"]["wdelta"] = wdelta
    return out


# ------------------------------------------------------------------------------------------------ (c)
def gen_labels():
    """epickitchens.py:227-241 on (verb, noun) pair lists instead of the two DataFrame columns."""
    tp, vp = PAIRS["train"], PAIRS["val"]
    tactions = set([(v, n) for v, n in tp])
    tverbs = set([v for v, _ in tactions])
    tnouns = set([n for _, n in tactions])
    keep = [(v, n) in tactions for v, n in vp]
    kept = [p for p, k in zip(vp, keep) if k]
    verb_classes = {k: i for i, k in enumerate(tverbs)}
    noun_classes = {k: i for i, k in enumerate(tnouns)}
    action_classes = {k: i for i, k in enumerate(tactions)}
    return dict(train=[list(p) for p in tp], val=[list(p) for p in vp], keep=keep,
                verbs=[[k, i] for k, i in verb_classes.items()], nouns=[[k, i] for k, i in noun_classes.items()],
                actions=[[k[0], k[1], i] for k, i in action_classes.items()],
                val_verbs=sorted(set([verb_classes[v] for v, _ in kept])),
                val_nouns=sorted(set([noun_classes[n] for _, n in kept])),
                val_actions=sorted(set([action_classes[a] for a in kept])))


def main():
    with tempfile.TemporaryDirectory() as td:
        dist.init_process_group("gloo", store=dist.FileStore(os.path.join(td, "store"), 1), rank=0, world_size=1)
        try:
            out = dict(wrapper=gen_wrapper(), probe=gen_probe(), labels=gen_labels())
        finally:
            dist.destroy_process_group()
    path = os.path.join(OUT, "anticipation_steps.pt")
    torch.save(out, path)
    print(f"wrote {path} ({os.path.getsize(path) / 1e3:.1f} kB)")
    torch.load(path, weights_only=True)  # tensors, scalars and settings only
    assert os.path.getsize(path) < 1_000_000


if __name__ == "__main__":
    main()
