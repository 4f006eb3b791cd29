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
Precision: optimization.use_bfloat16 selects the reference's autocast + GradScaler branch
(eval.py:306, 334-337). The reference autocasts to float16 there and scales the loss; the HIP path
computes bf16 GEMM operands (fp32's exponent range: loss scale fixed at 1, train.GradScalerFlag) and
keeps GradScaler.step's behaviour that matters: a head whose gradients hold an inf / NaN skips its
update, decided per head on the device. Without use_bfloat16 the same kernels run and the check is off.
Multi-GPU probe training (world_size > 1) is not implemented.
"""

import csv
import logging
import math
import os

import numpy as np
import torch

from .. import ops
from .. import vision_transformer as vit
from ..arena import FlatArena, FusedAdamW, readiness_order
from ..attentive_pooler import AttentiveClassifier
from ..functions import join_wgrad_stream, refresh_weight_transposes
from ..multiclip import ClipAggregation, ClipAggregationMultilevel
from ..train import GradScalerFlag, SyntheticLabelledVideoDataset

logger = logging.getLogger(__name__)
_GLOBAL_SEED = 0
_MC_KEYS = ("mc_warmup_steps", "mc_start_lr", "mc_ref_lr", "mc_final_lr", "mc_ref_wd", "mc_final_wd")
MULTICLIP_MODULE = "evals.video_classification_frozen.modelcustom.vit_encoder_multiclip"
MULTILEVEL_MODULE = "evals.video_classification_frozen.modelcustom.vit_encoder_multiclip_multilevel"


# ------------------------------------------------------------------------------------------------
# eval.py:490-537 (NOT vjepa2_amd/schedulers.py: these read their constants from the param group)
class WarmupCosineLRSchedule:
    """eval.py:490-515: linear warm-up from mc_start_lr to mc_ref_lr over mc_warmup_steps, then a
    cosine to mc_final_lr over T_max - warmup steps, never below mc_final_lr."""

    def __init__(self, optimizer, T_max, last_epoch=-1):
        self.optimizer = optimizer
        self.T_max = T_max
        self._step = 0.0

    def step(self):
        self._step += 1
        for group in self.optimizer.param_groups:
            ref_lr, final_lr, start_lr = group.get("mc_ref_lr"), group.get("mc_final_lr"), group.get("mc_start_lr")
            warmup_steps = group.get("mc_warmup_steps")
            T_max = self.T_max - warmup_steps
            if self._step < warmup_steps:
                progress = float(self._step) / float(max(1, warmup_steps))
                new_lr = start_lr + progress * (ref_lr - start_lr)
            else:
                progress = float(self._step - warmup_steps) / float(max(1, T_max))
                new_lr = max(final_lr, final_lr + (ref_lr - final_lr) * 0.5 * (1.0 + math.cos(math.pi * progress)))
            group["lr"] = new_lr


class CosineWDSchedule:
    """eval.py:518-537: cosine from mc_ref_wd to mc_final_wd over T_max steps, clamped at mc_final_wd."""

    def __init__(self, optimizer, T_max):
        self.optimizer = optimizer
        self.T_max = T_max
        self._step = 0.0

    def step(self):
        self._step += 1
        progress = self._step / self.T_max
        for group in self.optimizer.param_groups:
            ref_wd, final_wd = group.get("mc_ref_wd"), group.get("mc_final_wd")
            new_wd = final_wd + (ref_wd - final_wd) * 0.5 * (1.0 + math.cos(math.pi * progress))
            new_wd = max(final_wd, new_wd) if final_wd <= ref_wd else min(final_wd, new_wd)
            group["weight_decay"] = new_wd


def init_opt(classifiers, iterations_per_epoch, opt_kwargs, num_epochs, use_bfloat16=False):
    """eval.py:468-487. Per classifier: one flat arena, one fused AdamW whose single (decayed) param
    group carries the mc_* schedule constants and is numbered in named_parameters() order, so its
    state_dict() loads into the reference's torch.optim.AdamW and back."""
    optimizers, schedulers, wd_schedulers, scalers = [], [], [], []
    for c, kwargs in zip(classifiers, opt_kwargs):
        named = list(c.named_parameters())
        device = named[0][1].device
        arena = FlatArena(readiness_order(named), device, name="classifier")
        opt = FusedAdamW([arena], wd_exclude=[None], ref_groups=[named])
        opt.param_groups[0].update(mc_warmup_steps=int(kwargs.get("warmup") * iterations_per_epoch),
                                   mc_start_lr=kwargs.get("start_lr"), mc_ref_lr=kwargs.get("ref_lr"),
                                   mc_final_lr=kwargs.get("final_lr"), mc_ref_wd=kwargs.get("ref_wd"),
                                   mc_final_wd=kwargs.get("final_wd"))
        optimizers.append(opt)
        schedulers.append(WarmupCosineLRSchedule(opt, T_max=int(num_epochs * iterations_per_epoch)))
        wd_schedulers.append(CosineWDSchedule(opt, T_max=int(num_epochs * iterations_per_epoch)))
        scalers.append(GradScalerFlag() if use_bfloat16 else None)
    return optimizers, scalers, schedulers, wd_schedulers


def load_opt_state(opt, sd):
    """FusedAdamW.load_state_dict plus the mc_* keys of the saved group (torch's load_state_dict
    replaces the whole group, eval.py:375)."""
    opt.load_state_dict(sd)
    for g, sg in zip(opt.param_groups, sd["param_groups"]):
        for k in _MC_KEYS:
            if k in sg:
                g[k] = sg[k]


# ------------------------------------------------------------------------------------------------
class TopOneMeter:
    """src/utils/logging.py AverageMeter as eval.py:328-331 feeds it, per head: the unweighted mean of
    the per-iteration percentages 100 * correct / batch_size. The counts stay on the device (one
    int32 [heads] tensor per iteration) until avg() is asked for."""

    def __init__(self, heads):
        self.heads = heads
        self.reset()

    def reset(self):
        self.sum = np.zeros(self.heads, dtype=np.float64)
        self.count = 0
        self._pending = []

    def update(self, correct, batch_size):
        self._pending.append((correct, batch_size))

    def avg(self):
        """[heads] float64 (reads the pending counts back: a host sync)."""
        if self._pending:
            cnt = torch.stack([c for c, _ in self._pending]).cpu().numpy()
            for row, (_, bs) in zip(cnt, self._pending):
                # 100.0 * int64 tensor / batch_size is float32 arithmetic in the reference
                self.sum += (np.float32(100.0) * row.astype(np.float32) / np.float32(bs)).astype(np.float64)
                self.count += 1
            self._pending = []
        return self.sum / max(1, self.count)


class ProbeTrainer:
    """The probe step (eval.py:301-341) over arena-owned classifiers, head by head."""

    def __init__(self, encoder, classifiers, optimizers, scalers=None, schedulers=None, wd_schedulers=None,
                 use_bfloat16=False):
        self.encoder = encoder
        self.classifiers = list(classifiers)
        self.opts = list(optimizers)
        self.scalers = list(scalers) if scalers is not None else [None] * len(self.opts)
        self.schedulers = list(schedulers) if schedulers is not None else []
        self.wd_schedulers = list(wd_schedulers) if wd_schedulers is not None else []
        self.use_bfloat16 = bool(use_bfloat16)
        H = len(self.classifiers)
        self.train_meter, self.val_meter = TopOneMeter(H), TopOneMeter(H)
        # the last step's values, for logging and tests: per-head LR / WD as applied, per-head per-view
        # losses [H, V] (device), predictions [H, B] (device)
        self.last_lr, self.last_wd, self.last_losses, self.last_pred = [], [], None, None
        # debug hooks (tests): on_logits(h, logits) after a head's forward, on_grads(h) when its
        # gradients are complete and before its update
        self.on_logits = None
        self.on_grads = None

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

    def _labels(self, labels, device):
        if not labels.is_cuda:  # loaders deliver CPU labels: validated here, once for every head
            lo, hi = int(labels.min()), int(labels.max())
            C = self.classifiers[0].linear.out_features
            if lo < 0 or hi >= C:
                raise IndexError(f"label {hi if hi >= C else lo} out of range for {C} classes")
            labels = labels.to(device, non_blocking=True)
        return labels

    def train_step(self, clips, clip_indices, labels):
        """One training iteration (eval.py:302-341): schedulers, encoder, then per head forward ->
        vj_xent -> backward -> inf check -> AdamW -> zero_grad. Returns the losses [H, V] (device)."""
        for s in self.schedulers:
            s.step()
        for s in self.wd_schedulers:
            s.step()
        self.last_lr = [o.param_groups[0]["lr"] for o in self.opts]
        self.last_wd = [o.param_groups[0]["weight_decay"] for o in self.opts]
        for c in self.classifiers:
            c.train(True)
        x, V = self._tokens(clips, clip_indices)
        return self._heads(x, V, labels, training=True)

    def validate(self, clips, clip_indices, labels):
        """One validation iteration (eval.py:316-331): the same without gradients or updates."""
        for c in self.classifiers:
            c.train(False)
        x, V = self._tokens(clips, clip_indices)
        with torch.no_grad():
            return self._heads(x, V, labels, training=False)

    def _heads(self, x, V, labels, training):
        H = len(self.classifiers)
        B = x.shape[0] // V
        dev = x.device
        labels = self._labels(labels, dev)
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
                join_wgrad_stream()
                for a in opt.arenas:
                    a.finalize_grads()
                if self.on_grads is not None:
                    self.on_grads(h)
                found = opt.check_finite() if self.use_bfloat16 else None
                opt.step(found_inf=found)
                opt.zero_grad()
            del logits, dl  # this head's activations go before the next head's are made
        if training:
            refresh_weight_transposes()  # the next backward's W^T operands, one launch
        (self.train_meter if training else self.val_meter).update(correct, B)
        self.last_losses, self.last_pred = losses, preds
        return losses

    def sync_bf16(self):
        for o in self.opts:
            for a in o.arenas:
                a.sync_bf16()


# ------------------------------------------------------------------------------------------------
def _strip(sd):
    out = {}
    for k, v in sd.items():
        out[k.replace("module.", "").replace("backbone.", "")] = v
    return out


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
    pretrained = _strip(ck[ckp_key])
    for k, v in model.state_dict().items():
        if k not in pretrained:
            logger.info('key "%s" could not be found in loaded state dict', k)
        elif pretrained[k].shape != v.shape:
            logger.info('key "%s" is of different shape in model and loaded state dict', k)
            pretrained[k] = v
    msg = model.load_state_dict(pretrained, strict=False)
    logger.info("loaded pretrained model with msg: %s", msg)
    del ck
    wrap = ClipAggregationMultilevel if multilevel else ClipAggregation
    model = wrap(model, tubelet_size=model.tubelet_size, **(wrapper_kwargs or {}))
    model = model.to(device).eval()
    for p in model.parameters():
        p.requires_grad = False
    return model


def make_dataloader(batch_size, num_samples, num_classes, img_size=224, frames_per_clip=16, num_segments=1,
                    num_views_per_segment=1, world_size=1, rank=0, num_workers=0, seed_offset=0):
    """eval.py:414-465 with the synthetic labelled dataset (decord / torchvision are absent)."""
    ds = SyntheticLabelledVideoDataset(num_samples, frames_per_clip, img_size, num_classes, num_segments=num_segments,
                                       num_views=num_views_per_segment, seed_offset=seed_offset)
    sampler = torch.utils.data.distributed.DistributedSampler(ds, num_replicas=world_size, rank=rank, shuffle=False)
    loader = torch.utils.data.DataLoader(ds, batch_size=batch_size, sampler=sampler, num_workers=num_workers,
                                         drop_last=False, persistent_workers=num_workers > 0)
    return loader, sampler


def _env_world_size():
    """The world size a launcher asked for (distributed.init_distributed's sources), without joining a
    process group: the larger of an initialised group's and the environment's."""
    env = os.environ
    world = 1
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        world = torch.distributed.get_world_size()
    if "RANK" in env and "WORLD_SIZE" in env:
        world = max(world, int(env["WORLD_SIZE"]))
    elif "SLURM_NTASKS" in env:
        world = max(world, int(env["SLURM_NTASKS"]))
    return world


def save_checkpoint(path, classifiers, optimizers, scalers, epoch, batch_size, world_size):
    """eval.py:225-238: the reference's keys; classifier keys with DistributedDataParallel's prefix."""
    torch.save({"classifiers": [{"module." + k: v.detach().cpu().clone() for k, v in c.state_dict().items()}
                                for c in classifiers],
                "opt": [o.state_dict() for o in optimizers],
                "scaler": None if scalers[0] is None else [s.state_dict() for s in scalers],
                "epoch": epoch, "batch_size": batch_size, "world_size": world_size}, path)


def load_checkpoint(r_path, classifiers, opt, scaler, val_only=False):
    """eval.py:359-382 (tensor-only checkpoint: weights_only=True); classifier keys with or without
    the 'module.' prefix."""
    ck = torch.load(r_path, map_location="cpu", weights_only=True)
    for c, sd in zip(classifiers, ck["classifiers"]):
        c.load_state_dict({(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()})
    for o in opt:
        for a in o.arenas:
            a.sync_bf16()
    if val_only:
        return classifiers, opt, scaler, 0
    for o, sd in zip(opt, ck["opt"]):
        load_opt_state(o, sd)
    if scaler is not None and scaler[0] is not None and ck.get("scaler") is not None:
        for s, sd in zip(scaler, ck["scaler"]):
            s.load_state_dict(sd)
    return classifiers, opt, scaler, ck["epoch"]


def run_one_epoch(trainer, device, training, data_loader, log_every=10):
    """eval.py:283-356: returns the best head's running top-1 (%). The accuracy is read back from the
    device only when it is logged and at the end."""
    meter = trainer.train_meter if training else trainer.val_meter
    meter.reset()
    for itr, data in enumerate(data_loader):
        clips = [[dij.to(device, non_blocking=True) for dij in di] for di in data[0]]
        clip_indices = [d.to(device, non_blocking=True) for d in data[2]]
        labels = data[1]
        if training:
            trainer.train_step(clips, clip_indices, labels)
        else:
            trainer.validate(clips, clip_indices, labels)
        if itr % log_every == 0:
            agg = meter.avg()
            logger.info("[%5d] %.3f%% [%.3f%% %.3f%%] [mem: %.2e]", itr, agg.max(), agg.mean(), agg.min(),
                        torch.cuda.max_memory_allocated() / 1024.0**2)
    return float(meter.avg().max())


def main(args_eval, resume_preempt=False):
    """eval.py:48-280. Returns the best head's validation accuracy (%) of the last epoch run."""
    val_only = args_eval.get("val_only", False)
    pretrain_folder = args_eval.get("folder", None)
    resume_checkpoint = args_eval.get("resume_checkpoint", False) or resume_preempt
    eval_tag = args_eval.get("tag", None)
    num_workers = args_eval.get("num_workers", 0)  # synthetic data: no decode to hide

    args_pretrain = args_eval.get("model_kwargs")
    checkpoint = args_pretrain.get("checkpoint")
    module_name = args_pretrain.get("module_name")
    args_model = args_pretrain.get("pretrain_kwargs")
    args_wrapper = args_pretrain.get("wrapper_kwargs")
    args_exp = args_eval.get("experiment")
    args_classifier = args_exp.get("classifier")
    num_probe_blocks = args_classifier.get("num_probe_blocks", 1)
    num_heads = args_classifier.get("num_heads", 16)
    args_data = args_exp.get("data")
    num_classes = args_data.get("num_classes")
    resolution = args_data.get("resolution", 224)
    num_segments = args_data.get("num_segments", 1)
    frames_per_clip = args_data.get("frames_per_clip", 16)
    num_views_per_segment = args_data.get("num_views_per_segment", 1)
    args_opt = args_exp.get("optimization")
    batch_size = args_opt.get("batch_size")
    num_epochs = args_opt.get("num_epochs")
    use_bfloat16 = args_opt.get("use_bfloat16")
    opt_kwargs = [dict(ref_wd=kw.get("weight_decay"), final_wd=kw.get("final_weight_decay"),
                       start_lr=kw.get("start_lr"), ref_lr=kw.get("lr"), final_lr=kw.get("final_lr"),
                       warmup=kw.get("warmup")) for kw in args_opt.get("multihead_kwargs")]

    world_size, rank = _env_world_size(), 0
    if world_size > 1:
        raise NotImplementedError(f"video_classification_frozen on the HIP path runs on one GPU (world size "
                                  f"{world_size} requested): the classifiers' gradient all-reduce and the "
                                  "accuracy all-reduce (eval.py:161, 329) are not wired")
    if not torch.cuda.is_available():
        raise RuntimeError("the frozen-encoder probe on the HIP path needs an MI355X (no CPU path)")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    np.random.seed(_GLOBAL_SEED)
    torch.manual_seed(_GLOBAL_SEED)

    folder = os.path.join(pretrain_folder, "video_classification_frozen/")
    if eval_tag is not None:
        folder = os.path.join(folder, eval_tag)
    os.makedirs(folder, exist_ok=True)
    log_file = os.path.join(folder, f"log_r{rank}.csv")
    latest_path = os.path.join(folder, "latest.pt")

    encoder = init_module(module_name=module_name, frames_per_clip=frames_per_clip, resolution=resolution,
                          checkpoint=checkpoint, model_kwargs=args_model, wrapper_kwargs=args_wrapper, device=device)
    classifiers = [AttentiveClassifier(embed_dim=encoder.embed_dim, num_heads=num_heads, depth=num_probe_blocks,
                                       num_classes=num_classes, use_activation_checkpointing=True).to(device)
                   for _ in opt_kwargs]

    # synthetic stand-ins for dataset_train / dataset_val (data.num_samples / data.num_val_samples; the
    # training loader has one view per segment as eval.py:172)
    n_train = int(args_data.get("num_samples", 64 * batch_size))
    n_val = int(args_data.get("num_val_samples", n_train))
    kw = dict(batch_size=batch_size, num_classes=num_classes, img_size=resolution, frames_per_clip=frames_per_clip,
              num_segments=num_segments, world_size=world_size, rank=rank, num_workers=num_workers)
    train_loader, train_sampler = make_dataloader(num_samples=n_train, num_views_per_segment=1, **kw)
    val_loader, _ = make_dataloader(num_samples=n_val, num_views_per_segment=num_views_per_segment,
                                    seed_offset=1 << 20, **kw)
    ipe = len(train_loader)
    logger.info("Dataloader created... iterations per epoch: %d", ipe)

    optimizer, scaler, scheduler, wd_scheduler = init_opt(classifiers=classifiers, opt_kwargs=opt_kwargs,
                                                          iterations_per_epoch=ipe, num_epochs=num_epochs,
                                                          use_bfloat16=use_bfloat16)
    trainer = ProbeTrainer(encoder, classifiers, optimizer, scaler, scheduler, wd_scheduler, use_bfloat16=use_bfloat16)

    start_epoch = 0
    if resume_checkpoint and os.path.exists(latest_path):
        *_, start_epoch = load_checkpoint(latest_path, classifiers, optimizer, scaler, val_only=val_only)
        for _ in range(start_epoch * ipe):
            [s.step() for s in scheduler]
            [s.step() for s in wd_scheduler]

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
