"""What the three frozen-probe evals (video_classification_frozen, image_classification_frozen,
action_anticipation_frozen) share, each piece once: the reference's schedules and init_opt (eval.py:468-537
of the video eval; the other two evals' copies are the same code), the accuracy meter, latest.pt, the
non-strict pretrained load, the config keys the three eval.py files read alike, the set-up and resume steps
of their main()s, the host-side label check, the classifier-by-classifier trainer base and the top-1 epoch
loop. Each eval module adds its own encoder wrapper, token production, loss loop, data and log format.

Precision (the trainers' use_bfloat16): bf16 GEMM operands at loss scale 1 (train.GradScalerFlag) and
GradScaler.step's behaviour that matters: a classifier whose gradients hold an inf / NaN skips its update,
decided per classifier on the device. Without use_bfloat16 the same kernels run and the check is off.
"""

import logging
import math
import os

import numpy as np
import torch

from ..arena import FlatArena, FusedAdamW, readiness_order
from ..functions import join_wgrad_stream, refresh_weight_transposes
from ..train import GradScalerFlag

logger = logging.getLogger(__name__)
_GLOBAL_SEED = 0
_MC_KEYS = ("mc_warmup_steps", "mc_start_lr", "mc_ref_lr", "mc_final_lr", "mc_ref_wd", "mc_final_wd")


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


# ------------------------------------------------------------------------------------------------
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


def resume(latest_path, classifiers, optimizers, scalers, schedulers, wd_schedulers, ipe, val_only=False):
    """eval.py:212-223: latest.pt into the classifiers and optimizers, both scheduler lists replayed to the
    saved epoch's first iteration. Returns the epoch to start at (0 under val_only)."""
    *_, start_epoch = load_checkpoint(latest_path, classifiers, optimizers, scalers, val_only=val_only)
    for _ in range(start_epoch * ipe):
        [s.step() for s in schedulers]
        [s.step() for s in wd_schedulers]
    return start_epoch


# ------------------------------------------------------------------------------------------------
def load_pretrained(model, state_dict, what):
    """modelcustom/vit_encoder_multiclip.py:57-68: `state_dict` with the DDP / wrapper prefixes stripped, into
    `model`, non-strict; a key that is missing or of another shape is logged and keeps the model's own value."""
    pretrained = {k.replace("module.", "").replace("backbone.", ""): v for k, v in state_dict.items()}
    for k, v in model.state_dict().items():
        if k not in pretrained:
            logger.info('key "%s" could not be found in loaded state dict', k)
        elif pretrained[k].shape != v.shape:
            logger.info('key "%s" is of different shape in model and loaded state dict', k)
            pretrained[k] = v
    msg = model.load_state_dict(pretrained, strict=False)
    logger.info("loaded pretrained %s with msg: %s", what, msg)


def frozen(model, device):
    """`model` on `device`, in eval mode, no parameter asking for a gradient."""
    model = model.to(device).eval()
    for p in model.parameters():
        p.requires_grad = False
    return model


# ------------------------------------------------------------------------------------------------
def read_config(args_eval, resume_preempt=False, num_heads=None):
    """The keys the three eval.py files read alike (video eval.py:48-108). num_heads: the default of
    classifier.num_heads, which the evals do not share. Each eval adds its own keys to the dict."""
    args_pretrain = args_eval.get("model_kwargs")
    args_exp = args_eval.get("experiment")
    args_classifier = args_exp.get("classifier")
    args_opt = args_exp.get("optimization")
    return dict(
        val_only=args_eval.get("val_only", False), pretrain_folder=args_eval.get("folder", None),
        resume_checkpoint=args_eval.get("resume_checkpoint", False) or resume_preempt,
        eval_tag=args_eval.get("tag", None),
        checkpoint=args_pretrain.get("checkpoint"), module_name=args_pretrain.get("module_name"),
        args_model=args_pretrain.get("pretrain_kwargs"), args_wrapper=args_pretrain.get("wrapper_kwargs"),
        num_probe_blocks=args_classifier.get("num_probe_blocks", 1),
        num_heads=args_classifier.get("num_heads", num_heads),
        resolution=args_exp.get("data").get("resolution", 224),
        batch_size=args_opt.get("batch_size"), num_epochs=args_opt.get("num_epochs"),
        use_bfloat16=args_opt.get("use_bfloat16"),
        opt_kwargs=[dict(ref_wd=kw.get("weight_decay"), final_wd=kw.get("final_weight_decay"),
                         start_lr=kw.get("start_lr"), ref_lr=kw.get("lr"), final_lr=kw.get("final_lr"),
                         warmup=kw.get("warmup")) for kw in args_opt.get("multihead_kwargs")])


def init_device(what):
    """The one GPU an eval runs on, made current, then the reference's two seeds (eval.py:41-42)."""
    if not torch.cuda.is_available():
        raise RuntimeError(f"{what} on the HIP path needs an MI355X (no CPU path)")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    np.random.seed(_GLOBAL_SEED)
    torch.manual_seed(_GLOBAL_SEED)
    return device


def output_paths(pretrain_folder, eval_name, eval_tag, rank=0):
    """eval.py:126-132: (folder, log file, latest.pt). Naming them makes nothing."""
    folder = os.path.join(pretrain_folder, eval_name + "/")
    if eval_tag is not None:
        folder = os.path.join(folder, eval_tag)
    return folder, os.path.join(folder, f"log_r{rank}.csv"), os.path.join(folder, "latest.pt")


def checked_labels(labels, num_classes, device, what=""):
    """`labels` on `device`. Loaders deliver CPU labels: those are range-checked here, on the host, once for
    every classifier (a device tensor is taken as it is). what: the head's name for the message."""
    if not labels.is_cuda:
        lo, hi = int(labels.min()), int(labels.max())
        if lo < 0 or hi >= num_classes:
            raise IndexError(f"{what + ' ' if what else ''}label {hi if hi >= num_classes else lo} out of range "
                             f"for {num_classes} classes")
        labels = labels.to(device, non_blocking=True)
    return labels


# ------------------------------------------------------------------------------------------------
class FrozenProbeTrainer:
    """What a probe step does around its losses (eval.py:301-341), over arena-owned classifiers that are
    updated one after the other. A subclass produces the frozen model's tokens and runs its loss kernel per
    classifier between _begin() and _end(), calling _update() when a classifier's backward has been issued."""

    def __init__(self, classifiers, optimizers, scalers=None, schedulers=None, wd_schedulers=None,
                 use_bfloat16=False):
        self.classifiers = list(classifiers)
        self.opts = list(optimizers)
        self.scalers = list(scalers) if scalers is not None else [None] * len(self.opts)
        self.schedulers = list(schedulers) if schedulers is not None else []
        self.wd_schedulers = list(wd_schedulers) if wd_schedulers is not None else []
        self.use_bfloat16 = bool(use_bfloat16)
        # the last training step's per-classifier LR / WD as applied, for logging and tests
        self.last_lr, self.last_wd = [], []
        # debug hooks (tests): on_logits(i, logits) after classifier i's forward, on_grads(i) when its
        # gradients are complete and before its update
        self.on_logits = None
        self.on_grads = None

    def _begin(self, training):
        """Training: both schedulers step (eval.py:302-305). Either way the classifiers' mode is set."""
        if training:
            for s in self.schedulers:
                s.step()
            for s in self.wd_schedulers:
                s.step()
            self.last_lr = [o.param_groups[0]["lr"] for o in self.opts]
            self.last_wd = [o.param_groups[0]["weight_decay"] for o in self.opts]
        for c in self.classifiers:
            c.train(training)

    def _update(self, i, opt):
        """Classifier i's gradients -> inf check -> AdamW -> zero_grad (eval.py:334-341)."""
        join_wgrad_stream()
        for a in opt.arenas:
            a.finalize_grads()
        if self.on_grads is not None:
            self.on_grads(i)
        found = opt.check_finite() if self.use_bfloat16 else None
        opt.step(found_inf=found)
        opt.zero_grad()

    def _end(self, training):
        if training:
            refresh_weight_transposes()  # the next backward's W^T operands, one launch

    def sync_bf16(self):
        for o in self.opts:
            for a in o.arenas:
                a.sync_bf16()


def run_one_epoch(trainer, device, training, data_loader, unpack, log_every):
    """eval.py:283-356 over a ProbeTrainer-like `trainer`: returns the best head's running top-1 (%). The
    accuracy is read back from the device only when it is logged and at the end. unpack(data, device) gives
    the step's (clips, clip_indices, labels) from what the loader delivers."""
    meter = trainer.train_meter if training else trainer.val_meter
    meter.reset()
    for itr, data in enumerate(data_loader):
        clips, clip_indices, labels = unpack(data, device)
        if training:
            trainer.train_step(clips, clip_indices, labels)
        else:
            trainer.validate(clips, clip_indices, labels)
        if itr % log_every == 0:
            agg = meter.avg()
            logger.info("[%5d] %.3f%% [%.3f%% %.3f%%] [mem: %.2e]", itr, agg.max(), agg.mean(), agg.min(),
                        torch.cuda.max_memory_allocated() / 1024.0**2)
    return float(meter.avg().max())
