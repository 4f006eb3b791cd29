"""Frozen-encoder video-classification probe (drop-in for evals/video_classification_frozen/eval.py and
its modelcustom/vit_encoder_multiclip.py:41-78 and vit_encoder_multiclip_multilevel.py:41-82 init_module):
the SSv2 / K400 / COIN configs of configs/eval/ (single-level wrapper) and the Diving48 / Jester ones
(multilevel wrapper: four tapped layers, each normed once into the classifiers' buffer by vj_layernorm_taps).

`main(args_eval, resume_preempt)` reads the reference's config keys (eval.py:48-108) and runs its epoch
(eval.py:283-356): frozen encoder forward -> every attentive classifier on every view -> per-view
CrossEntropyLoss, view-averaged softmax top-1 -> backward -> one AdamW per classifier. The step is
ProbeTrainer.train_step, MI355X-native:
  * the encoder runs once, under no_grad, through ClipAggregation on the HIP VisionTransformer;
  * each classifier sees its V views stacked as ONE batch of V*B (full-size GEMMs instead of V passes);
  * loss, dL/dlogits, the view-averaged softmax's argmax and the top-1 count are ONE kernel (vj_xent)
    per head, with no host read-back: the reference's float(...) per head per iteration (eval.py:329)
    becomes a device counter read when the accuracy is logged;
  * heads run one after the other, forward -> loss -> backward -> AdamW, so one head's activations are
    freed before the next head's are made. The reference keeps all heads' autograd graphs alive
    until the backward (eval.py:322-339); with 20 heads of 4 blocks over K400's 8 x 2048 tokens per
    view that is over 100 GB of activations. The heads share nothing but the encoder's tokens, so the
    order of their updates changes no number;
  * every classifier's parameters live in one flat arena with one fused AdamW launch (the reference
    puts ALL of a classifier's parameters, biases included, in a single decayed group, eval.py:471-483).
What this eval shares with the image and the anticipation evals (schedules, init_opt, the meter, latest.pt,
the config's common keys, the trainer base and its use_bfloat16 convention, the epoch loop) is evals/probe.py.
Multi-GPU probe training (world_size > 1) is not implemented.
"""

import csv
import logging
import os

import torch

from .. import ops
from .. import vision_transformer as vit
from ..attentive_pooler import AttentiveClassifier
from ..distributed import env_world_size
from ..multiclip import ClipAggregation, ClipAggregationMultilevel
from ..train import SyntheticLabelledVideoDataset
from . import probe
from .probe import load_checkpoint  # noqa: F401  (resume() calls it; here as save_checkpoint's counterpart)
from .probe import (FrozenProbeTrainer, TopOneMeter, checked_labels, frozen, init_device, init_opt, load_pretrained,
                    output_paths, resume, save_checkpoint)

logger = logging.getLogger(__name__)
MULTICLIP_MODULE = "evals.video_classification_frozen.modelcustom.vit_encoder_multiclip"
MULTILEVEL_MODULE = "evals.video_classification_frozen.modelcustom.vit_encoder_multiclip_multilevel"


class ProbeTrainer(FrozenProbeTrainer):
    """The probe step (eval.py:301-341) over arena-owned classifiers, head by head."""

    def __init__(self, encoder, classifiers, optimizers, scalers=None, schedulers=None, wd_schedulers=None,
                 use_bfloat16=False):
        super().__init__(classifiers, optimizers, scalers, schedulers, wd_schedulers, use_bfloat16)
        self.encoder = encoder
        H = len(self.classifiers)
        self.train_meter, self.val_meter = TopOneMeter(H), TopOneMeter(H)
        # the last step's per-head per-view losses [H, V] (device) and predictions [H, B] (device)
        self.last_losses, self.last_pred = None, None

    def _tokens(self, clips, clip_indices):
        stacked = getattr(self.encoder, "forward_stacked", None)
        if stacked is not None:  # the multilevel wrapper writes the views into one buffer: no cat
            with torch.no_grad():
                x, V = stacked(clips, clip_indices)
            return x.detach(), V
        with torch.no_grad():
            outputs = self.encoder(clips, clip_indices)
        V = len(outputs)
        x = outputs[0] if V == 1 else torch.cat(outputs, dim=0)  # [V*B, N, D]: row v*B + b
        return x.detach(), V

    def train_step(self, clips, clip_indices, labels):
        """One training iteration (eval.py:302-341): schedulers, encoder, then per head forward ->
        vj_xent -> backward -> inf check -> AdamW -> zero_grad. Returns the losses [H, V] (device)."""
        self._begin(True)
        x, V = self._tokens(clips, clip_indices)
        return self._heads(x, V, labels, training=True)

    def validate(self, clips, clip_indices, labels):
        """One validation iteration (eval.py:316-331): the same without gradients or updates."""
        self._begin(False)
        x, V = self._tokens(clips, clip_indices)
        with torch.no_grad():
            return self._heads(x, V, labels, training=False)

    def _heads(self, x, V, labels, training):
        H = len(self.classifiers)
        B = x.shape[0] // V
        dev = x.device
        labels = checked_labels(labels, self.classifiers[0].linear.out_features, dev)
        losses = torch.empty(H, V, dtype=torch.float32, device=dev)
        correct = torch.empty(H, dtype=torch.int32, device=dev)
        preds = torch.empty(H, B, dtype=torch.int32, device=dev)
        row_loss = torch.empty(V * B, dtype=torch.float32, device=dev)
        for h, (c, opt) in enumerate(zip(self.classifiers, self.opts)):
            logits = c(x)  # [V*B, C] f32
            if self.on_logits is not None:
                self.on_logits(h, logits)
            dl = torch.empty_like(logits) if training else None
            ops.xent(logits, labels, views=V, want_grad=training,
                     out=(losses[h], row_loss, dl, preds[h], correct[h:h + 1]))
            if training:
                logits.backward(dl)
                self._update(h, opt)
            del logits, dl  # this head's activations go before the next head's are made
        self._end(training)
        (self.train_meter if training else self.val_meter).update(correct, B)
        self.last_losses, self.last_pred = losses, preds
        return losses


# ------------------------------------------------------------------------------------------------
def init_module(module_name, frames_per_clip, resolution, checkpoint, model_kwargs, wrapper_kwargs, device):
    """evals/video_classification_frozen/models.py + modelcustom/vit_encoder_multiclip.py:41-78: the HIP
    VisionTransformer `model_name`, weights from checkpoint[checkpoint_key] (non-strict, DDP / wrapper
    prefixes stripped), wrapped in ClipAggregation; frozen, in eval mode, on `device`. With the module
    name of modelcustom/vit_encoder_multiclip_multilevel.py:41-82 (Diving48, Jester) the encoder is built
    with wrapper_kwargs["out_layers"] and wrapped in ClipAggregationMultilevel."""
    multilevel = module_name == MULTILEVEL_MODULE
    if module_name is not None and module_name != MULTICLIP_MODULE and not multilevel:
        raise NotImplementedError(f"encoder module {module_name!r}: only {MULTICLIP_MODULE} and "
                                  f"{MULTILEVEL_MODULE} are ported")
    enc_kwargs = dict(model_kwargs["encoder"])
    ckp_key = enc_kwargs.get("checkpoint_key")
    if multilevel:
        enc_kwargs["out_layers"] = (wrapper_kwargs or {}).get("out_layers")
    model = vit.__dict__[enc_kwargs.get("model_name")](img_size=resolution, num_frames=frames_per_clip, **enc_kwargs)
    logger.info("Loading pretrained model from %s", checkpoint)
    ck = torch.load(checkpoint, map_location="cpu", weights_only=True)
    load_pretrained(model, ck[ckp_key], "model")
    del ck
    wrap = ClipAggregationMultilevel if multilevel else ClipAggregation
    return frozen(wrap(model, tubelet_size=model.tubelet_size, **(wrapper_kwargs or {})), device)


def make_dataloader(batch_size, num_samples, num_classes, img_size=224, frames_per_clip=16, num_segments=1,
                    num_views_per_segment=1, world_size=1, rank=0, num_workers=0, seed_offset=0):
    """eval.py:414-465 with the synthetic labelled dataset (decord / torchvision are absent)."""
    ds = SyntheticLabelledVideoDataset(num_samples, frames_per_clip, img_size, num_classes, num_segments=num_segments,
                                       num_views=num_views_per_segment, seed_offset=seed_offset)
    sampler = torch.utils.data.distributed.DistributedSampler(ds, num_replicas=world_size, rank=rank, shuffle=False)
    loader = torch.utils.data.DataLoader(ds, batch_size=batch_size, sampler=sampler, num_workers=num_workers,
                                         drop_last=False, persistent_workers=num_workers > 0)
    return loader, sampler


def _unpack(data, device):
    """eval.py:308-313: the loader's (clips, labels, clip_indices) as the step's arguments."""
    clips = [[dij.to(device, non_blocking=True) for dij in di] for di in data[0]]
    clip_indices = [d.to(device, non_blocking=True) for d in data[2]]
    return clips, clip_indices, data[1]


def run_one_epoch(trainer, device, training, data_loader, log_every=10):
    """eval.py:283-356: returns the best head's running top-1 (%)."""
    return probe.run_one_epoch(trainer, device, training, data_loader, _unpack, log_every)


def read_config(args_eval, resume_preempt=False):
    """The reference's keys (eval.py:48-108); data: the section itself, for the synthetic dataset's two."""
    c = probe.read_config(args_eval, resume_preempt, num_heads=16)
    args_data = args_eval.get("experiment").get("data")
    c.update(num_workers=args_eval.get("num_workers", 0),  # synthetic data: no decode to hide
             data=args_data, num_classes=args_data.get("num_classes"), num_segments=args_data.get("num_segments", 1),
             frames_per_clip=args_data.get("frames_per_clip", 16),
             num_views_per_segment=args_data.get("num_views_per_segment", 1))
    return c


def main(args_eval, resume_preempt=False):
    """eval.py:48-280. Returns the best head's validation accuracy (%) of the last epoch run."""
    c = read_config(args_eval, resume_preempt)
    val_only, batch_size, num_epochs, use_bfloat16 = c["val_only"], c["batch_size"], c["num_epochs"], c["use_bfloat16"]

    world_size, rank = env_world_size(), 0
    if world_size > 1:
        raise NotImplementedError(f"video_classification_frozen on the HIP path runs on one GPU (world size "
                                  f"{world_size} requested): the classifiers' gradient all-reduce and the "
                                  "accuracy all-reduce (eval.py:161, 329) are not wired")
    device = init_device("the frozen-encoder probe")
    folder, log_file, latest_path = output_paths(c["pretrain_folder"], "video_classification_frozen", c["eval_tag"],
                                                 rank)
    os.makedirs(folder, exist_ok=True)

    encoder = init_module(module_name=c["module_name"], frames_per_clip=c["frames_per_clip"],
                          resolution=c["resolution"], checkpoint=c["checkpoint"], model_kwargs=c["args_model"],
                          wrapper_kwargs=c["args_wrapper"], device=device)
    classifiers = [AttentiveClassifier(embed_dim=encoder.embed_dim, num_heads=c["num_heads"],
                                       depth=c["num_probe_blocks"], num_classes=c["num_classes"],
                                       use_activation_checkpointing=True).to(device) for _ in c["opt_kwargs"]]

    # synthetic stand-ins for dataset_train / dataset_val (data.num_samples / data.num_val_samples; the
    # training loader has one view per segment as eval.py:172)
    n_train = int(c["data"].get("num_samples", 64 * batch_size))
    n_val = int(c["data"].get("num_val_samples", n_train))
    kw = dict(batch_size=batch_size, num_classes=c["num_classes"], img_size=c["resolution"],
              frames_per_clip=c["frames_per_clip"], num_segments=c["num_segments"], world_size=world_size, rank=rank,
              num_workers=c["num_workers"])
    train_loader, train_sampler = make_dataloader(num_samples=n_train, num_views_per_segment=1, **kw)
    val_loader, _ = make_dataloader(num_samples=n_val, num_views_per_segment=c["num_views_per_segment"],
                                    seed_offset=1 << 20, **kw)
    ipe = len(train_loader)
    logger.info("Dataloader created... iterations per epoch: %d", ipe)

    optimizer, scaler, scheduler, wd_scheduler = init_opt(classifiers=classifiers, opt_kwargs=c["opt_kwargs"],
                                                          iterations_per_epoch=ipe, num_epochs=num_epochs,
                                                          use_bfloat16=use_bfloat16)
    trainer = ProbeTrainer(encoder, classifiers, optimizer, scaler, scheduler, wd_scheduler, use_bfloat16=use_bfloat16)

    start_epoch = 0
    if c["resume_checkpoint"] and os.path.exists(latest_path):
        start_epoch = resume(latest_path, classifiers, optimizer, scaler, scheduler, wd_scheduler, ipe, val_only)

    val_acc = None
    for epoch in range(start_epoch, num_epochs):
        logger.info("Epoch %d", epoch + 1)
        train_sampler.set_epoch(epoch)
        train_acc = -1.0 if val_only else run_one_epoch(trainer, device, True, train_loader)
        val_acc = run_one_epoch(trainer, device, False, val_loader)
        logger.info("[%5d] train: %.3f%% test: %.3f%%", epoch + 1, train_acc, val_acc)
        with open(log_file, "a", newline="") as f:  # epoch, train acc, val acc (eval.py:136, 275), no header row
            csv.writer(f).writerow([epoch + 1, f"{train_acc:.5f}", f"{val_acc:.5f}"])
        if val_only:
            return val_acc
        save_checkpoint(latest_path, classifiers, optimizer, scaler, epoch + 1, batch_size, world_size)
    return val_acc
