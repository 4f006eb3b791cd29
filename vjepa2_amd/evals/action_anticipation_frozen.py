"""Frozen action-anticipation probe (drop-in for evals/action_anticipation_frozen/eval.py, its
modelcustom/vit_encoder_predictor_concat_ar.py, models.py, metrics.py and losses.py): the EK100 configs
configs/eval/vitl/ek100.yaml and configs/eval/vitg-384/ek100.yaml.

The frozen encoder's tokens are rolled forward by the frozen predictor to positions beyond the clip
(AnticipativeWrapper), encoder and predicted tokens are concatenated, and attentive probes with three
queries (verb, noun, action) are trained on them. `main(args_eval, resume_preempt)` reads the reference's
config keys (eval.py:52-126) and runs its epochs (eval.py:444-593, 596-735). The step is
AnticipationTrainer.train_step, MI355X-native:
  * the wrapper runs once, under no_grad, on the HIP encoder and predictor;
  * per classifier, the three sigmoid focal losses, their gradients and the three ClassMeanRecall updates are
    ONE kernel (vj_focal) with no host read-back: the reference's ten elementwise passes per loss and its
    per-sample `gt in p` membership test (one device-to-host sync per sample, metrics.py:37-41) become device
    counters that are read when the metrics are logged;
  * classifiers run one after the other, forward -> loss -> backward -> AdamW, so one classifier's
    activations are freed before the next one's are made (they share nothing but the wrapper's tokens, so the
    order of their updates changes no number);
  * every classifier's parameters live in one flat arena with one fused AdamW launch.
With optimization.use_focal_loss false the loss and its gradient come from vj_xent (CrossEntropyLoss, one
view) per head and vj_focal only counts (loss_kind 0).

Metrics. ClassMeanRecall counts a sample as a hit when its label is among the top 5 of its row, by rank
count; among equal logits the lower class index ranks first (torch.topk leaves ties unspecified). Validation
restricts the ranking to the classes seen in the validation annotations (the metric's valid_classes);
training ranks all classes.

Positions. The predictor's RoPE tables are sized from predictor.num_patches, so every future position id
must be below it: AnticipativeWrapper computes the anticipation steps on the host (the times arrive from the
loader as a CPU tensor) and raises ValueError before any launch otherwise. The EK100 configs are inside the
range (predictor num_frames 64, clips of 32 frames).

Precision: optimization.use_bfloat16 has the meaning it has for every probe here (evals/probe.py, which also
holds what this eval shares with the video and image evals): bf16 GEMM operands, loss scale 1, a
per-classifier device-side skip when a gradient holds an inf or NaN.
Multi-GPU probe training (world size > 1), real EK100 decoding and the COIN annotations are not implemented:
the data is a synthetic stand-in with the loader's sample layout (video, verb, noun, anticipation time).
"""

import csv
import logging
import os

import numpy as np
import torch
import torch.nn as nn

from .. import functions as fn
from .. import ops
from .. import predictor as vit_pred
from .. import vision_transformer as vit
from ..attentive_pooler import AttentivePooler
from ..distributed import env_world_size
from . import probe
from .probe import load_checkpoint  # noqa: F401  (resume() calls it; here as save_checkpoint's counterpart)
from .probe import (FrozenProbeTrainer, checked_labels, frozen, init_device, init_opt, load_pretrained, output_paths,
                    resume, save_checkpoint)

logger = logging.getLogger(__name__)
ANTICIPATION_MODULE = "evals.action_anticipation_frozen.modelcustom.vit_encoder_predictor_concat_ar"
HEADS = ("verb", "noun", "action")


# ------------------------------------------------------------------------------------------------
class AnticipativeWrapper(nn.Module):
    """modelcustom/vit_encoder_predictor_concat_ar.py:119-188: encoder tokens + the predictor's tokens for
    num_output_frames frames that lie anticipation_time seconds past the clip."""

    def __init__(self, encoder, predictor, frames_per_second=4, crop_size=224, patch_size=16, tubelet_size=2,
                 no_predictor=False, num_output_frames=2, num_steps=1, no_encoder=False):
        super().__init__()
        self.encoder = encoder
        self.predictor = predictor
        self.grid_size = crop_size // patch_size
        self.tubelet_size = tubelet_size
        self.no_predictor = no_predictor
        self.num_output_frames = max(num_output_frames, tubelet_size)
        self.frames_per_second = frames_per_second
        self.num_steps = num_steps
        self.no_encoder = no_encoder
        assert not (self.no_predictor and self.no_encoder), "Anticipative wrapper must use predictor or encoder"

    def target_positions(self, anticipation_times, N):
        """(:157-170) on the host: (context ids [B, N], target ids [B, N_pred]) as CPU int64 tensors. Raises
        ValueError when a target id falls outside [N, predictor.num_patches): the RoPE tables end there, and
        ids below N would collide with the context's."""
        t = torch.as_tensor(anticipation_times)
        if t.is_cuda:
            t = t.cpu()  # a host sync: loaders deliver the times on the CPU
        B = t.shape[0]
        steps = (t * self.frames_per_second / self.tubelet_size).to(torch.int64)
        skip = N + int(self.grid_size**2) * steps
        N_pred = int(self.grid_size**2 * (self.num_output_frames // self.tubelet_size))
        tgt = torch.arange(N_pred).unsqueeze(0).repeat(B, 1) + skip.unsqueeze(1).repeat(1, N_pred)
        ctxt = torch.arange(N).unsqueeze(0).repeat(B, 1)
        limit = int(self.predictor.num_patches)
        lo, hi = int(tgt.min()), int(tgt.max())
        if lo < N or hi >= limit:
            raise ValueError(f"anticipation target position ids [{lo}, {hi}] leave the predictor's range [{N}, {limit}) "
                             f"(num_frames {getattr(self.predictor, 'num_frames', '?')}): anticipation times "
                             f"{t.tolist()} s at {self.frames_per_second} fps, tubelet {self.tubelet_size}")
        return ctxt, tgt

    def forward(self, x, anticipation_times):
        """x [B, C, T, H, W], anticipation_times [B] seconds -> [B, N (+ num_steps * N_pred), D]."""
        x = self.encoder(x)
        if self.no_predictor:
            return x
        B, N, D = x.size()
        if getattr(self.predictor, "predictor_pos_embed", None) is not None:
            raise NotImplementedError("future positions need a RoPE predictor (use_rope): a sincos predictor's "
                                      "position table is not wired for ids beyond the clip")
        ctxt, tgt = self.target_positions(anticipation_times, N)  # raises before any predictor launch
        N_pred = tgt.shape[1]
        ctxt, tgt = ctxt.to(x.device), tgt.to(x.device)
        acc = [] if self.no_encoder else [x]
        for _ in range(self.num_steps):
            x_pred = self.predictor(x, masks_x=ctxt, masks_y=tgt).to(x.dtype)
            acc.append(x_pred)
            x = torch.cat([x[:, N_pred:, :], x_pred], dim=1)
        return torch.cat(acc, dim=1)


def init_module(module_name, device, frames_per_clip, frames_per_second, resolution, checkpoint, model_kwargs,
                wrapper_kwargs):
    """models.py:71-110 + modelcustom/vit_encoder_predictor_concat_ar.py:37-116: the HIP encoder and predictor
    from checkpoint[checkpoint_key] (non-strict, DDP / wrapper prefixes stripped) inside AnticipativeWrapper;
    frozen, in eval mode, on `device`."""
    if module_name != ANTICIPATION_MODULE:
        raise NotImplementedError(f"model module {module_name!r}: only {ANTICIPATION_MODULE} is ported")
    logger.info("Loading pretrained model from %s", checkpoint)
    ck = torch.load(checkpoint, map_location="cpu", weights_only=True)
    enc_kwargs = dict(model_kwargs["encoder"])
    encoder = vit.__dict__[enc_kwargs.get("model_name")](img_size=resolution, num_frames=frames_per_clip, **enc_kwargs)
    load_pretrained(encoder, ck[enc_kwargs.get("checkpoint_key")], "model")
    prd_kwargs = dict(model_kwargs["predictor"])
    predictor = vit_pred.__dict__[prd_kwargs.get("model_name")](
        img_size=resolution, embed_dim=encoder.embed_dim, patch_size=encoder.patch_size,
        tubelet_size=encoder.tubelet_size, **prd_kwargs)
    load_pretrained(predictor, ck[prd_kwargs.get("checkpoint_key")], "predictor")
    del ck
    model = AnticipativeWrapper(encoder=encoder, predictor=predictor, frames_per_second=frames_per_second,
                                crop_size=resolution, patch_size=encoder.patch_size, tubelet_size=encoder.tubelet_size,
                                **(wrapper_kwargs or {}))
    model.embed_dim = encoder.embed_dim
    return frozen(model, device)


# ------------------------------------------------------------------------------------------------
class AttentiveClassifier(nn.Module):
    """models.py:19-68: a three-query attentive pooler (one query when action-only) and one nn.Linear per
    query (mlp_ratio: the pooler's, 4 in the reference). The three Linears keep nn.Linear's default init, as
    in the reference (its _init_weights is the pooler's own). The reference's host-side NaN test of the input (:50-52) is not made: it is a device
    read-back per classifier per iteration; use_bfloat16's finite check guards the update instead."""

    def __init__(self, verb_classes, noun_classes, action_classes, embed_dim, num_heads, depth,
                 use_activation_checkpointing=False, mlp_ratio=4.0):
        super().__init__()
        self.num_verb_classes = len(verb_classes)
        num_noun_classes = len(noun_classes)
        num_action_classes = len(action_classes)
        self.action_only = self.num_verb_classes == 0
        self.pooler = AttentivePooler(num_queries=1 if self.action_only else 3, embed_dim=embed_dim,
                                      num_heads=num_heads, mlp_ratio=mlp_ratio, depth=depth,
                                      use_activation_checkpointing=use_activation_checkpointing)
        if not self.action_only:
            self.verb_classifier = nn.Linear(embed_dim, self.num_verb_classes, bias=True)
            self.noun_classifier = nn.Linear(embed_dim, num_noun_classes, bias=True)
        self.action_classifier = nn.Linear(embed_dim, num_action_classes, bias=True)

    @property
    def heads(self):
        return ("action",) if self.action_only else HEADS

    def forward(self, x):
        """x [B, N, D] -> dict of f32 logits [B, C_head]."""
        x = self.pooler(x)  # [B, nq, D]
        if self.action_only:
            return dict(action=fn.run_linear(x[:, 0, :].contiguous(), self.action_classifier, out_dtype=torch.float32))
        x = x.transpose(0, 1).contiguous()  # [3, B, D]: one copy, three contiguous GEMM operands
        return dict(verb=fn.run_linear(x[0], self.verb_classifier, out_dtype=torch.float32),
                    noun=fn.run_linear(x[1], self.noun_classifier, out_dtype=torch.float32),
                    action=fn.run_linear(x[2], self.action_classifier, out_dtype=torch.float32))


def init_classifier(embed_dim, num_heads, num_blocks, device, num_classifiers, action_classes, verb_classes,
                    noun_classes):
    """models.py:113-136."""
    return [AttentiveClassifier(verb_classes=verb_classes, noun_classes=noun_classes, action_classes=action_classes,
                                embed_dim=embed_dim, num_heads=num_heads, depth=num_blocks,
                                use_activation_checkpointing=True).to(device) for _ in range(num_classifiers)]


# ------------------------------------------------------------------------------------------------
class ClassMeanRecall:
    """metrics.py:12-57 with the counting on the device: int32 TP / FN per class that vj_focal adds to
    (ops.focal's tp / fn); result() reads them back and does the reference's float32 arithmetic."""

    def __init__(self, num_classes, device, k=5):
        self.num_classes = num_classes
        self.TP = torch.zeros(num_classes, dtype=torch.int32, device=device)
        self.FN = torch.zeros(num_classes, dtype=torch.int32, device=device)
        self.k = k

    @staticmethod
    def compute(TP, FN, eps=1e-8):
        """metrics.py:51-57 from given counts (any integer or float tensors), in float32 on the CPU."""
        TP, FN = TP.detach().cpu().to(torch.float32), FN.detach().cpu().to(torch.float32)
        nch = torch.sum((TP + FN) > 0)
        recall = 100.0 * torch.sum(TP / (TP + FN + eps)) / nch
        total = int(torch.sum(TP + FN))
        topk = 100.0 * torch.sum(TP) / total if total else torch.tensor(float("nan"))
        return dict(recall=float(recall), accuracy=float(topk))

    def result(self, eps=1e-8):
        """dict(recall = mean class recall %, accuracy = top-k accuracy %): a host sync."""
        return self.compute(self.TP, self.FN, eps)


def unify_labels(train_pairs, val_pairs):
    """epickitchens.py:227-241 from (verb_class, noun_class) int pairs: validation actions unseen in training
    are dropped; class ids enumerate Python sets (of ints, of int tuples) in the sets' own iteration order.
    Returns dict(verbs, nouns, actions: class dicts; val_verbs, val_nouns, val_actions: sets of class ids;
    val_keep: per validation pair whether it stays)."""
    tactions = set([(int(v), int(n)) for v, n in train_pairs])
    tverbs = set([v for v, _ in tactions])
    tnouns = set([n for _, n in tactions])
    val_pairs = [(int(v), int(n)) for v, n in val_pairs]
    keep = [p in tactions for p in val_pairs]
    kept = [p for p, k in zip(val_pairs, keep) if k]
    verb_classes = {k: i for i, k in enumerate(tverbs)}
    noun_classes = {k: i for i, k in enumerate(tnouns)}
    action_classes = {k: i for i, k in enumerate(tactions)}
    return dict(verbs=verb_classes, nouns=noun_classes, actions=action_classes,
                val_verbs=set([verb_classes[v] for v, _ in kept]), val_nouns=set([noun_classes[n] for _, n in kept]),
                val_actions=set([action_classes[a] for a in kept]), val_keep=keep)


def read_annotation_pairs(path):
    """The (verb_class, noun_class) column pairs of an EK100 annotation CSV (epickitchens.py:224-228)."""
    with open(path, newline="") as f:
        return [(int(r["verb_class"]), int(r["noun_class"])) for r in csv.DictReader(f)]


# ------------------------------------------------------------------------------------------------
class AnticipationTrainer(FrozenProbeTrainer):
    """The anticipation probe step (eval.py:470-535, 622-665) over arena-owned classifiers, one by one."""

    def __init__(self, model, classifiers, optimizers, scalers=None, schedulers=None, wd_schedulers=None,
                 use_bfloat16=False, use_focal_loss=True, alpha=0.25, gamma=2.0, k=5):
        super().__init__(classifiers, optimizers, scalers, schedulers, wd_schedulers, use_bfloat16)
        self.model = model
        self.use_focal_loss = bool(use_focal_loss)
        self.alpha, self.gamma, self.k = alpha, gamma, k  # sigmoid_focal_loss's defaults, ClassMeanRecall's k
        self.heads = self.classifiers[0].heads
        self.metrics = {True: None, False: None}  # training / validation: {head: [ClassMeanRecall per classifier]}
        # the last step's losses [classifiers, heads] (device) and hit flags [classifiers, heads, B] (device);
        # on_logits is given the classifier's dict of logits
        self.last_losses, self.last_hits = None, None

    def _linear(self, c, head):
        return getattr(c, f"{head}_classifier")

    def reset_metrics(self, training):
        """New counters, as the reference makes new ClassMeanRecall objects per epoch (eval.py:465-467, 618-620)."""
        dev = next(self.classifiers[0].parameters()).device
        self.metrics[training] = {h: [ClassMeanRecall(self._linear(c, h).out_features, dev, k=self.k)
                                      for c in self.classifiers] for h in self.heads}

    def results(self, training):
        """eval.py:574-593: per head the best classifier's accuracy and recall (reads the counters back)."""
        out = {}
        for h, ms in self.metrics[training].items():
            rs = [m.result() for m in ms]
            out[h] = dict(accuracy=max(r["accuracy"] for r in rs), recall=max(r["recall"] for r in rs))
        return out

    def train_step(self, clips, anticipation_times, labels):
        """One training iteration (eval.py:479-535). labels: {head: [B] unified class ids}. Returns the
        losses [classifiers, heads] (device); a classifier's loss is their sum."""
        self._begin(True)
        with torch.no_grad():
            x = self.model(clips, anticipation_times).detach()
        return self._classifiers(x, labels, None, training=True)

    def validate(self, clips, anticipation_times, labels, valid=None):
        """One validation iteration (eval.py:629-665). valid: {head: bool / uint8 device mask [C] of the classes
        that count for the ranking} or None."""
        self._begin(False)
        with torch.no_grad():
            x = self.model(clips, anticipation_times).detach()
            return self._classifiers(x, labels, valid, training=False)

    def _classifiers(self, x, labels, valid, training):
        if self.metrics[training] is None:
            self.reset_metrics(training)
        heads, n, dev = self.heads, len(self.heads), x.device
        B = x.shape[0]
        labels = [checked_labels(labels[h], self._linear(self.classifiers[0], h).out_features, dev, what=h)
                  for h in heads]
        masks = None if valid is None else [valid.get(h) for h in heads]
        losses = torch.empty(len(self.classifiers), n, dtype=torch.float32, device=dev)
        hits = torch.empty(len(self.classifiers), n, B, dtype=torch.int32, device=dev)
        row_loss = torch.empty(n * B, dtype=torch.float32, device=dev)
        pred = torch.empty(B, dtype=torch.int32, device=dev)
        correct = torch.empty(1, dtype=torch.int32, device=dev)
        for i, (c, opt) in enumerate(zip(self.classifiers, self.opts)):
            out = c(x)
            logits = [out[h] for h in heads]
            if self.on_logits is not None:
                self.on_logits(i, out)
            tp = [self.metrics[training][h][i].TP for h in heads]
            fn_ = [self.metrics[training][h][i].FN for h in heads]
            dls = [torch.empty_like(lg) for lg in logits] if training else None
            if self.use_focal_loss:
                ops.focal(logits, labels, tp, fn_, valid=masks, alpha=self.alpha, gamma=self.gamma, k=self.k,
                          want_grad=training, out=(losses[i], row_loss, dls, hits[i]))
            else:
                for s, (lg, lb) in enumerate(zip(logits, labels)):
                    ops.xent(lg, lb, views=1, want_grad=training,
                             out=(losses[i, s:s + 1], row_loss[:B], None if dls is None else dls[s], pred, correct))
                ops.focal(logits, labels, tp, fn_, valid=masks, k=self.k, loss_kind=0, out=(None, None, None, hits[i]))
            if training:
                torch.autograd.backward(logits, dls)
                self._update(i, opt)
            del out, logits, dls  # this classifier's activations go before the next one's are made
        self._end(training)
        self.last_losses, self.last_hits = losses, hits
        return losses


# ------------------------------------------------------------------------------------------------
class SyntheticAnticipationDataset(torch.utils.data.Dataset):
    """Samples in the layout the reference's EK100 loader delivers (epickitchens.py:199): (video [3, F, S, S],
    verb, noun, anticipation_time), verb / noun the RAW annotation classes (mapped by unify_labels's dicts in
    the epoch loop, eval.py:490-498). The time of sample i is drawn uniformly from anticipation_time_sec =
    [lo, hi]. Deterministic per index."""

    def __init__(self, pairs, frames_per_clip, crop_size, anticipation_time_sec, seed_offset=0):
        self.pairs = [(int(v), int(n)) for v, n in pairs]
        self.fpc, self.crop, self.seed_offset = frames_per_clip, crop_size, seed_offset
        self.times = [float(t) for t in anticipation_time_sec]

    @staticmethod
    def make_pairs(num_samples, num_verbs, num_nouns, seed_offset=0):
        """Raw (verb, noun) annotation pairs for a run without annotation files."""
        i = np.arange(num_samples)
        return list(zip(((i * 5 + 1 + seed_offset) % num_verbs).tolist(), ((i * 7 + 2) % num_nouns).tolist()))

    def __len__(self):
        return len(self.pairs)

    def __getitem__(self, i):
        g = torch.Generator().manual_seed(self.seed_offset + 4000 + i)
        v, n = self.pairs[i]
        video = torch.randn(3, self.fpc, self.crop, self.crop, generator=g) + 0.5 * np.sin(1.0 + v) + 0.25 * np.cos(n)
        lo, hi = self.times[0], self.times[-1]
        at = lo + (hi - lo) * float(torch.rand((), generator=g))
        return video.float(), v, n, np.float32(at)


def make_dataloader(pairs, batch_size, frames_per_clip, crop_size, anticipation_time_sec, num_workers=0,
                    seed_offset=0):
    ds = SyntheticAnticipationDataset(pairs, frames_per_clip, crop_size, anticipation_time_sec, seed_offset=seed_offset)
    return torch.utils.data.DataLoader(ds, batch_size=batch_size, shuffle=False, num_workers=num_workers,
                                       drop_last=True, persistent_workers=num_workers > 0)


def _class_mask(ids, num_classes, device):
    m = torch.zeros(num_classes, dtype=torch.uint8)
    if ids:
        m[sorted(ids)] = 1
    return m.to(device)


def run_one_epoch(trainer, device, training, data_loader, classes, valid=None, log_every=10):
    """eval.py:444-593 / 596-735: one pass over the loader; returns {head: dict(accuracy, recall)}. The
    metrics are read back from the device only when they are logged and at the end."""
    trainer.reset_metrics(training)
    n = len(data_loader)
    for itr, (clips, verbs, nouns, times) in enumerate(data_loader):
        labels = dict(action=torch.tensor([classes["actions"][(int(v), int(n_))] for v, n_ in zip(verbs, nouns)]))
        if "verb" in trainer.heads:
            labels["verb"] = torch.tensor([classes["verbs"][int(v)] for v in verbs])
            labels["noun"] = torch.tensor([classes["nouns"][int(n_)] for n_ in nouns])
        clips = clips.to(device, non_blocking=True)
        if training:
            trainer.train_step(clips, times, labels)
        else:
            trainer.validate(clips, times, labels, valid=valid)
        if itr % log_every == 0 or itr == n - 1:
            r = trainer.results(training)
            logger.info("[%5d] acc %s recall %s [mem: %.2e]", itr, {h: round(v["accuracy"], 1) for h, v in r.items()},
                        {h: round(v["recall"], 1) for h, v in r.items()}, torch.cuda.max_memory_allocated() / 1024.0**2)
    return trainer.results(training)


CSV_COLUMNS = ("epoch", "train-acc", "train-acc-verb", "train-acc-noun", "train-recall", "train-recall-verb",
               "train-recall-noun", "val-acc", "val-acc-verb", "val-acc-noun", "val-recall", "val-recall-verb",
               "val-recall-noun")
CSV_COLUMNS_ACTION_ONLY = ("epoch", "train-acc", "train-recall", "val-acc", "val-recall")


def _csv_row(epoch, train, val, verb_noun):
    if verb_noun:
        vals = [m[h][q] for m in (train, val) for q in ("accuracy", "recall") for h in ("action", "verb", "noun")]
    else:
        vals = [m["action"][q] for m in (train, val) for q in ("accuracy", "recall")]
    return [str(epoch)] + ["%.5f" % v for v in vals]


def read_config(args_eval, resume_preempt=False):
    """The reference's keys (eval.py:52-126); data: the section itself, for the synthetic dataset's four."""
    c = probe.read_config(args_eval, resume_preempt)
    args_data = args_eval.get("experiment").get("data")
    c.update(data=args_data, dataset=args_data.get("dataset"),
             num_workers=args_data.get("num_workers", 0),  # synthetic data: no decode to hide
             frames_per_clip=args_data.get("frames_per_clip"), frames_per_second=args_data.get("frames_per_second"),
             train_anticipation_time_sec=args_data.get("train_anticipation_time_sec"),
             val_anticipation_time_sec=args_data.get("anticipation_time_sec"),
             train_annotations_path=args_data.get("dataset_train"), val_annotations_path=args_data.get("dataset_val"),
             use_focal_loss=args_eval.get("experiment").get("optimization").get("use_focal_loss", False))
    return c


def main(args_eval, resume_preempt=False):
    """eval.py:52-441. Returns the validation metrics {head: dict(accuracy, recall)} of the last epoch run."""
    c = read_config(args_eval, resume_preempt)
    val_only, batch_size, num_epochs, use_bfloat16 = c["val_only"], c["batch_size"], c["num_epochs"], c["use_bfloat16"]
    args_data = c["data"]

    world_size, rank = env_world_size(), 0
    if world_size > 1:
        raise NotImplementedError(f"action_anticipation_frozen on the HIP path runs on one GPU (world size "
                                  f"{world_size} requested): the classifiers' gradient all-reduce and the TP / FN "
                                  "all-reduce (metrics.py:47-48) are not wired")
    if c["module_name"] != ANTICIPATION_MODULE:
        raise NotImplementedError(f"model module {c['module_name']!r}: only {ANTICIPATION_MODULE} is ported")
    if c["dataset"] in ["COIN_anticipation"]:
        raise NotImplementedError("the COIN anticipation annotations (action-only labels) are not ported")
    device = init_device("the anticipation probe")
    folder, log_file, latest_path = output_paths(c["pretrain_folder"], "action_anticipation_frozen", c["eval_tag"],
                                                 rank)
    os.makedirs(folder, exist_ok=True)
    with open(log_file, "a", newline="") as f:  # CSVLogger prints its header when it is made (logging.py:51-57)
        csv.writer(f).writerow(CSV_COLUMNS)

    # annotations: (verb, noun) pairs from the CSVs when both exist, else synthetic ones
    train_path, val_path = c["train_annotations_path"], c["val_annotations_path"]
    if train_path and val_path and os.path.exists(train_path) and os.path.exists(val_path):
        train_pairs = read_annotation_pairs(train_path)
        val_pairs = read_annotation_pairs(val_path)
    else:
        n_train = int(args_data.get("num_samples", 64 * batch_size))
        n_val = int(args_data.get("num_val_samples", n_train))
        nv, nn_ = int(args_data.get("num_verbs", 97)), int(args_data.get("num_nouns", 300))
        train_pairs = SyntheticAnticipationDataset.make_pairs(n_train, nv, nn_)
        val_pairs = SyntheticAnticipationDataset.make_pairs(n_val, nv, nn_, seed_offset=1)
    classes = unify_labels(train_pairs, val_pairs)
    val_pairs = [p for p, k in zip(val_pairs, classes["val_keep"]) if k]
    verb_classes, noun_classes, action_classes = classes["verbs"], classes["nouns"], classes["actions"]

    model = init_module(module_name=c["module_name"], frames_per_clip=c["frames_per_clip"],
                        frames_per_second=c["frames_per_second"], resolution=c["resolution"],
                        checkpoint=c["checkpoint"], model_kwargs=c["args_model"], wrapper_kwargs=c["args_wrapper"],
                        device=device)
    classifiers = init_classifier(embed_dim=model.embed_dim, num_heads=c["num_heads"], verb_classes=verb_classes,
                                  noun_classes=noun_classes, action_classes=action_classes,
                                  num_blocks=c["num_probe_blocks"], device=device,
                                  num_classifiers=len(c["opt_kwargs"]))
    kw = dict(batch_size=batch_size, frames_per_clip=c["frames_per_clip"], crop_size=c["resolution"],
              num_workers=c["num_workers"])
    train_loader = make_dataloader(train_pairs, anticipation_time_sec=c["train_anticipation_time_sec"], **kw)
    val_loader = make_dataloader(val_pairs, anticipation_time_sec=c["val_anticipation_time_sec"], seed_offset=1 << 20,
                                 **kw)
    ipe = len(train_loader)
    logger.info("Dataloader created... iterations per epoch: %d (val %d)", ipe, len(val_loader))

    optimizer, scaler, scheduler, wd_scheduler = init_opt(classifiers=classifiers, opt_kwargs=c["opt_kwargs"],
                                                          iterations_per_epoch=ipe, num_epochs=num_epochs,
                                                          use_bfloat16=use_bfloat16)
    trainer = AnticipationTrainer(model, classifiers, optimizer, scaler, scheduler, wd_scheduler,
                                  use_bfloat16=use_bfloat16, use_focal_loss=c["use_focal_loss"])
    valid = dict(verb=_class_mask(classes["val_verbs"], len(verb_classes), device),
                 noun=_class_mask(classes["val_nouns"], len(noun_classes), device),
                 action=_class_mask(classes["val_actions"], len(action_classes), device))

    start_epoch = 0
    if c["resume_checkpoint"] and os.path.exists(latest_path):
        start_epoch = resume(latest_path, classifiers, optimizer, scaler, scheduler, wd_scheduler, ipe, val_only)

    val_metrics = None
    for epoch in range(start_epoch, num_epochs):
        logger.info("Epoch %d", epoch)
        if not val_only:
            train_metrics = run_one_epoch(trainer, device, True, train_loader, classes)
        val_metrics = run_one_epoch(trainer, device, False, val_loader, classes, valid=valid)
        if val_only:
            logger.info("val %s", val_metrics)
            return val_metrics
        logger.info("[%5d] train %s val %s", epoch + 1, train_metrics, val_metrics)
        with open(log_file, "a", newline="") as f:
            csv.writer(f).writerow(_csv_row(epoch + 1, train_metrics, val_metrics, True))
        save_checkpoint(latest_path, classifiers, optimizer, scaler, epoch + 1, batch_size, world_size)
    return val_metrics
