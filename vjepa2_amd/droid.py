"""V-JEPA 2-AC post-training (drop-in for app/vjepa_droid/train.py + app/vjepa_droid/utils.py): the
action-conditioned predictor is trained on the representations of a frozen encoder.

`main(args, resume_preempt)` reads the reference's YAML keys (meta / model / data / data_aug / loss /
optimization; configs/train/vitg16/droid-256px-8f.yaml unchanged) and runs the reference's step (train.py:
403-470). The step itself is ACTrainer.train_step, built from paths that exist elsewhere in the package:
  * targets: every frame becomes a doubled 2-frame tubelet (as planning.WorldModel.encode), the frozen encoder
    runs without grad on its bf16 forward path, the extra F.layer_norm is vj_plan_frame;
  * teacher forcing: one differentiable VisionTransformerPredictorAC.forward over frames 0 .. T-2;
  * roll-out: auto_steps - 1 further forwards over the growing sequence [h_0, zn_1, ..., zn_n], each recomputing
    the whole sequence as the reference does (training through the K/V cache is not built);
  * the loss side (layer_norm of the prediction, the slice of h, mean(|z - h| ** p) / p and their autograd) is
    functions.ACLossFn on the vj_acloss.hip kernels; its backward also carries the gradient that flows from the
    roll-out back into the teacher-forced pass (zn_tf's first frame starts the roll-out);
  * weight gradients accumulate across the predictor passes into the predictor's flat arenas
    (functions.wgrad_buf / grad_buf), zeroed lazily once per step; FusedAdamW steps the two predictor arenas.
The optimizer keeps the reference's four parameter groups (encoder wd, predictor wd, encoder no-wd, predictor
no-wd; utils.py:215-234) in state_dict(); the encoder groups own no gradient and never gain state, exactly as in
the reference, whose context encoder is in the optimizer but not in the step.

One MI355X (world_size 1). The real DROID loader (h5py / decord / pandas) is out of scope: SyntheticDroidDataset
returns samples of the same structure. `app: vjepa_droid` is not dispatched by vjepa2_amd.main yet; this module
is its own entry point:

    python -m vjepa2_amd.droid --fname configs/train/vitg16/droid-256px-8f.yaml
"""

import argparse
import copy
import csv
import logging
import os
import time
import types

import numpy as np
import torch

from . import ops
from . import vision_transformer as video_vit
from .ac_predictor import vit_ac_predictor
from .arena import FlatArena, FusedAdamW, readiness_order, wd_split
from .distributed import env_world_size
from .functions import ACLossFn, join_wgrad_stream, refresh_weight_transposes
from .planning import poses_to_diff
from .schedulers import CosineWDSchedule, WSDSchedule
from .train import GradScalerFlag, gpu_timer

logger = logging.getLogger(__name__)
_GLOBAL_SEED = 0
F32 = torch.float32


# ------------------------------------------------------------------------------------------------
# app/vjepa_droid/utils.py equivalents
def init_video_model(device, patch_size=16, max_num_frames=16, tubelet_size=2, model_name="vit_base", crop_size=224,
                     pred_depth=6, pred_num_heads=None, pred_embed_dim=384, uniform_power=False, use_sdpa=False,
                     use_rope=False, use_silu=False, use_pred_silu=False, wide_silu=False, pred_is_frame_causal=True,
                     use_activation_checkpointing=False, return_all_tokens=False, action_embed_dim=7,
                     use_extrinsics=False, old_pred=False):
    """app/vjepa_droid/utils.py:127-194 (same construction order -> same initial weights per seed).
    use_activation_checkpointing is accepted and ignored (activations are kept, no numerics change)."""
    if not use_rope:
        raise NotImplementedError("V-JEPA 2-AC post-training on the HIP path needs model.use_rope: true (the AC "
                                  "predictor without RoPE is not built; every DROID config uses RoPE)")
    encoder = video_vit.__dict__[model_name](img_size=crop_size, patch_size=patch_size, num_frames=max_num_frames,
                                             tubelet_size=tubelet_size, uniform_power=uniform_power,
                                             use_sdpa=use_sdpa, use_silu=use_silu, wide_silu=wide_silu,
                                             use_activation_checkpointing=use_activation_checkpointing,
                                             use_rope=use_rope)
    predictor = vit_ac_predictor(img_size=crop_size, patch_size=patch_size, num_frames=max_num_frames,
                                 tubelet_size=tubelet_size, embed_dim=encoder.embed_dim,
                                 predictor_embed_dim=pred_embed_dim, action_embed_dim=action_embed_dim,
                                 depth=pred_depth, is_frame_causal=pred_is_frame_causal,
                                 num_heads=encoder.num_heads if pred_num_heads is None else pred_num_heads,
                                 uniform_power=uniform_power, use_rope=use_rope, use_sdpa=use_sdpa,
                                 use_silu=use_pred_silu, wide_silu=wide_silu, use_extrinsics=use_extrinsics,
                                 use_activation_checkpointing=use_activation_checkpointing)
    encoder.to(device)
    predictor.to(device)
    return encoder, predictor


def init_opt(encoder, predictor, iterations_per_epoch, start_lr, ref_lr, warmup, anneal, num_epochs, wd=1e-6,
             final_wd=1e-6, final_lr=0.0, mixed_precision=False, betas=(0.9, 0.999), eps=1e-8, zero_init_bias_wd=True,
             enc_lr_scale=1.0):
    """app/vjepa_droid/utils.py:197-253. The predictor's two parameter groups become two flat arenas under the
    fused HIP AdamW; the encoder's two groups are kept (empty arenas, the reference's numbering in
    state_dict()) but own no gradient: the step never produces one, in the reference either."""
    device = next(predictor.parameters()).device
    pred_wd, pred_nowd = wd_split(readiness_order(predictor.named_parameters()))
    arenas = [FlatArena([], device, grads=False, opt_state=False, name="encoder"),
              FlatArena(pred_wd, device, name="predictor"),
              FlatArena([], device, grads=False, opt_state=False, name="encoder_nowd"),
              FlatArena(pred_nowd, device, name="predictor_nowd")]
    enc_groups, pred_groups = wd_split(encoder.named_parameters()), wd_split(predictor.named_parameters())
    ref_groups = [enc_groups[0], pred_groups[0], enc_groups[1], pred_groups[1]]
    optimizer = FusedAdamW(arenas, wd_exclude=[None, None, zero_init_bias_wd, zero_init_bias_wd], betas=betas,
                           eps=eps, ref_groups=ref_groups)
    for i in (0, 2):
        optimizer.param_groups[i]["lr_scale"] = enc_lr_scale
    scheduler = WSDSchedule(optimizer, warmup_steps=int(warmup * iterations_per_epoch),
                            anneal_steps=int(anneal * iterations_per_epoch), start_lr=start_lr, ref_lr=ref_lr,
                            final_lr=final_lr, T_max=int(num_epochs * iterations_per_epoch))
    wd_scheduler = CosineWDSchedule(optimizer, ref_wd=wd, final_wd=final_wd,
                                    T_max=int(num_epochs * iterations_per_epoch))
    scaler = GradScalerFlag() if mixed_precision else None
    return optimizer, scaler, scheduler, wd_scheduler


def _strip(sd):
    """Checkpoint keys without the DDP / wrapper prefixes (utils.py:40: k.replace("backbone.", ""))."""
    return {k.replace("module.", "").replace("backbone.", ""): v for k, v in sd.items()}


def _load_weights(module, sd):
    """load_state_dict(strict=False) (utils.py:41), then the bf16 shadows of arena-owned parameters."""
    msg = module.load_state_dict(_strip(sd), strict=False)
    for a in {id(p._vj_arena): p._vj_arena for p in module.parameters() if getattr(p, "_vj_arena", None)}.values():
        a.sync_bf16()
    return msg


def load_pretrained(r_path, encoder=None, predictor=None, target_encoder=None, context_encoder_key="encoder",
                    target_encoder_key="target_encoder", load_predictor=False, load_encoder=True):
    """app/vjepa_droid/utils.py:22-66 (tensor-only checkpoints: loaded with weights_only=True). When encoder and
    target_encoder are one module (equal keys) it is loaded once."""
    ck = torch.load(r_path, map_location="cpu", weights_only=True)
    epoch = ck["epoch"]
    if load_encoder:
        msg = _load_weights(encoder, ck[context_encoder_key])
        logger.info(f"loaded pretrained encoder from epoch {epoch} with msg: {msg}")
    if load_predictor:
        msg = _load_weights(predictor, ck["predictor"])
        logger.info(f"loaded pretrained predictor from epoch {epoch} with msg: {msg}")
    if load_encoder and target_encoder is not None and target_encoder is not encoder:
        msg = _load_weights(target_encoder, ck[target_encoder_key])
        logger.info(f"loaded pretrained target encoder from epoch {epoch} with msg: {msg}")
    return encoder, predictor, target_encoder


def _prefixed(sd):
    return {"module." + k: v.detach().cpu().clone() for k, v in sd.items()}


def save_checkpoint(path, encoder, predictor, target_encoder, optimizer, scaler, epoch, loss, batch_size, world_size,
                    lr):
    """train.py:314-332 format (keys with DistributedDataParallel's "module." prefix). One shared encoder is
    written under both keys."""
    enc = _prefixed(encoder.state_dict())
    tgt = enc if target_encoder is encoder else _prefixed(target_encoder.state_dict())
    torch.save({"encoder": enc, "predictor": _prefixed(predictor.state_dict()), "opt": optimizer.state_dict(),
                "scaler": None if scaler is None else scaler.state_dict(), "target_encoder": tgt, "epoch": epoch,
                "loss": loss, "batch_size": batch_size, "world_size": world_size, "lr": lr}, path)


def load_checkpoint(r_path, encoder, predictor, target_encoder, opt=None, scaler=None):
    """app/vjepa_droid/utils.py:69-124."""
    ck = torch.load(r_path, map_location="cpu", weights_only=True)
    _load_weights(encoder, ck["encoder"])
    _load_weights(predictor, ck["predictor"])
    if target_encoder is not None and target_encoder is not encoder:
        _load_weights(target_encoder, ck["target_encoder"])
    if opt is not None:
        opt.load_state_dict(ck["opt"])
    if scaler is not None and ck.get("scaler") is not None:
        scaler.load_state_dict(ck["scaler"])
    return encoder, predictor, target_encoder, opt, scaler, ck["epoch"]


# ------------------------------------------------------------------------------------------------
class ACTrainer:
    """The V-JEPA 2-AC train step (app/vjepa_droid/train.py:403-470) on one MI355X.

    predictor: a VisionTransformerPredictorAC whose parameters live in `optimizer`'s arenas (init_opt);
    target_encoder: the frozen VisionTransformer (never written). LR / WD must already be set on the optimizer's
    param_groups (the schedulers). loss_side="torch" replaces ACLossFn by the reference's separate torch ops
    on the same HIP predictor (tools/bench_droid_step.py's second arm and the tests' isolation of the kernels)."""

    def __init__(self, predictor, target_encoder, optimizer, tokens_per_frame, auto_steps=1, loss_exp=1.0,
                 normalize_reps=True, mixed_precision=True, world_size=1, loss_side="hip"):
        if world_size != 1:
            raise NotImplementedError(f"V-JEPA 2-AC post-training on the HIP path runs on one GPU (world size "
                                      f"{world_size} requested): the predictor's gradient all-reduce is not wired")
        if loss_side not in ("hip", "torch"):
            raise ValueError(f"loss_side {loss_side!r}: 'hip' or 'torch'")
        self.pred, self.tgt, self.opt = predictor, target_encoder, optimizer
        self.hw = int(tokens_per_frame)
        self.auto_steps, self.loss_exp = int(auto_steps), float(loss_exp)
        self.normalize_reps, self.mixed_precision = bool(normalize_reps), bool(mixed_precision)
        self.loss_side = loss_side
        for p in target_encoder.parameters():
            p.requires_grad = False
        self.pred_arenas = [a for a in optimizer.arenas if a.grad is not None]
        # parameters the step never reaches have grad None in the reference: no update, no decay, no state
        self.unused = [] if predictor.use_extrinsics else list(predictor.extrinsics_encoder.parameters())
        self.found_inf = None

    # -- train.py:408-415
    def forward_target(self, clips):
        B, _, T, _, _ = clips.shape
        c = clips.permute(0, 2, 1, 3, 4).flatten(0, 1).unsqueeze(2).repeat(1, 1, 2, 1, 1)
        with torch.no_grad():
            t, _ = self.tgt.forward_ragged(c, None, out_dtype=F32, final_norm=True,
                                           bf16_residual=self.mixed_precision and self.tgt.bf16_residual_ok())
        h = t.view(B, -1, t.shape[-1])
        if h.shape[1] != T * self.hw:
            raise ValueError(f"{h.shape[1]} target tokens per clip, expected {T} frames of {self.hw}")
        if self.normalize_reps:
            out = torch.empty_like(h)
            ops.plan_frame(h, dst=out, normalize=True)
            h = out
        return h

    def _loss(self, z, h, normalize, want_zn=True):
        """(loss, zn) of one predictor pass; h None: normalise only; want_zn False: the loss alone."""
        if self.loss_side == "hip":
            if h is None and not normalize:
                return None, z
            return ACLossFn.apply(z, h, normalize, self.loss_exp, 1e-5, want_zn)
        zn = torch.nn.functional.layer_norm(z, (z.size(-1),)) if normalize else z
        if h is None:
            return None, zn
        return torch.mean(torch.abs(zn - h) ** self.loss_exp) / self.loss_exp, zn

    # -- train.py:417-449
    def forward_losses(self, clips, actions, states, extrinsics):
        hw = self.hw
        T = clips.shape[2]
        steps = min(self.auto_steps, T)
        if steps > T - 1 or steps < 1:
            raise ValueError(f"auto_steps {steps} needs {steps + 1} frames per clip, the clips have {T}")
        h = self.forward_target(clips)
        ext = None if extrinsics is None else extrinsics[:, :-1]
        z_tf = self.pred(h[:, :-hw], actions, states[:, :-1], ext)
        jloss, zn_tf = self._loss(z_tf, h[:, hw:], self.normalize_reps)
        seq = torch.cat([h[:, :hw], zn_tf[:, :hw]], dim=1)
        for n in range(1, steps):
            ext = None if extrinsics is None else extrinsics[:, :n + 1]
            out = self.pred(seq, actions[:, :n + 1], states[:, :n + 1], ext)
            _, zn = self._loss(out[:, -hw:], None, self.normalize_reps)
            seq = torch.cat([seq, zn], dim=1)
        # the rolled frames are normalised already: the loss alone
        sloss, _ = self._loss(seq[:, hw:], h[:, hw:(steps + 1) * hw], False, want_zn=False)
        return jloss, sloss

    def train_step(self, clips, actions, states, extrinsics=None):
        """clips [B, C, T, H, W], actions [B, T-1, 7], states [B, T, 7], extrinsics [B, T, 6] on the device.
        Returns a device tensor (loss, jloss, sloss): nothing is read back here."""
        if self.pred.use_extrinsics and extrinsics is None:
            raise ValueError("the predictor uses extrinsics")
        jloss, sloss = self.forward_losses(clips, actions.float(), states.float(),
                                           None if extrinsics is None else extrinsics.float())
        loss = jloss + sloss
        loss.backward()
        join_wgrad_stream()
        for a in self.pred_arenas:
            a.finalize_grads()
        found = None
        if self.mixed_precision:  # GradScaler.step's inf / NaN skip, decided on the device
            if self.found_inf is None:
                self.found_inf = torch.zeros(1, dtype=torch.int32, device=clips.device)
            found = self.found_inf.zero_()
            for a in self.pred_arenas:
                ops.check_finite(a.grad, found)
        self.opt.step(found_inf=found, exclude=self.unused)
        self.opt.zero_grad()
        refresh_weight_transposes()
        return torch.stack([loss.detach(), jloss.detach(), sloss.detach()])


# ------------------------------------------------------------------------------------------------
# data (the reference's DROIDVideoDataset needs h5py / decord / pandas: synthetic samples of its structure)
class SyntheticDroidDataset(torch.utils.data.Dataset):
    """(clip [C, T, H, W], actions [T-1, 7], states [T, 7], extrinsics [T, 6]), a function of (seed, index):
    a noise clip, a random-walk end-effector trajectory (x, y, z, roll, pitch, yaw, gripper), its frame-to-frame
    pose differences (planning.poses_to_diff) as actions, random extrinsics."""

    def __init__(self, num_samples, frames_per_clip, crop_size, seed=5000):
        self.n, self.fpc, self.crop, self.seed = int(num_samples), int(frames_per_clip), int(crop_size), int(seed)

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        g = torch.Generator().manual_seed(self.seed + int(i))
        T = self.fpc
        clip = torch.randn(3, T, self.crop, self.crop, generator=g)
        start = (torch.rand(7, generator=g) - 0.5) * torch.tensor([0.6, 0.6, 0.6, 1.0, 1.0, 1.0, 1.0]) \
            + torch.tensor([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.5])
        steps = 0.05 * torch.randn(T - 1, 7, generator=g)
        states = torch.cat([start[None], start[None] + torch.cumsum(steps, 0)], 0)
        states[:, 6] = states[:, 6].clamp(0.0, 1.0)
        extrinsics = 0.5 * torch.randn(T, 6, generator=g)
        actions = torch.stack([poses_to_diff(states[t].double(), states[t + 1].double())
                               for t in range(T - 1)]).float()
        return clip, actions, states, extrinsics


def init_data(batch_size, frames_per_clip, crop_size, rank=0, world_size=1, num_workers=0, num_samples=None,
              seed=0, **kw):
    """app/vjepa_droid/droid.py init_data's role: (loader, sampler). The sampler shuffles by (seed, epoch), so
    an epoch's batches are the same in a resumed run as in an uninterrupted one."""
    ds = SyntheticDroidDataset(num_samples or 100_000, frames_per_clip, crop_size)
    sampler = torch.utils.data.distributed.DistributedSampler(ds, num_replicas=world_size, rank=rank, shuffle=True,
                                                              seed=seed)
    dl = torch.utils.data.DataLoader(ds, batch_size=batch_size, sampler=sampler, num_workers=num_workers,
                                     drop_last=True, persistent_workers=num_workers > 0)
    return dl, sampler


def check_data_aug(cfgs_data_aug):
    """The synthetic clips take no augmentation; only the DROID config's values (all off) are accepted."""
    on = [k for k in ("auto_augment", "motion_shift", "horizontal_flip") if cfgs_data_aug.get(k, False)]
    if float(cfgs_data_aug.get("reprob", 0.0)) > 0:
        on.append("reprob")
    if on:
        raise NotImplementedError(f"data_aug {on}: not built on the HIP path (the DROID config turns them off)")


# ------------------------------------------------------------------------------------------------
def settings(args):
    """The YAML keys the app uses with the reference's defaults (train.py:59-150), as a namespace; `model` holds
    init_video_model's keyword arguments."""
    meta, cm, cd, cl, co = (args.get(k) for k in ("meta", "model", "data", "loss", "optimization"))
    s = types.SimpleNamespace()
    s.folder = args.get("folder", ".")
    s.r_file = meta.get("resume_checkpoint", None)
    s.p_file = meta.get("pretrain_checkpoint", None)
    s.load_predictor = meta.get("load_predictor", False)
    s.context_encoder_key = meta.get("context_encoder_key", "encoder")
    s.target_encoder_key = meta.get("target_encoder_key", "target_encoder")
    s.load_encoder = meta.get("load_encoder", True)
    s.seed = meta.get("seed", _GLOBAL_SEED)
    s.save_every_freq = meta.get("save_every_freq", -1)
    s.which_dtype = str(meta.get("dtype", "float32")).lower()
    s.mixed_precision = s.which_dtype in ("bfloat16", "float16")
    # one copy of the encoder weights on the device when both checkpoint keys name the same weights (the DROID
    # config): the context encoder is in the optimizer and the checkpoint, never in the step
    s.shared_encoder = s.context_encoder_key == s.target_encoder_key
    s.dataset_fpcs = cd.get("dataset_fpcs")
    s.max_num_frames = max(s.dataset_fpcs)
    s.batch_size = cd.get("batch_size")
    s.tubelet_size = cd.get("tubelet_size")
    s.crop_size = cd.get("crop_size", 256)
    s.patch_size = cd.get("patch_size")
    s.num_samples = cd.get("num_samples")  # this build's key: the synthetic data set's length
    s.loss_exp = cl.get("loss_exp")
    s.normalize_reps = cl.get("normalize_reps")
    s.auto_steps = min(cl.get("auto_steps", 1), s.max_num_frames)
    s.tokens_per_frame = int((s.crop_size // s.patch_size) ** 2)
    s.ipe = co.get("ipe", None)
    s.wd, s.final_wd = float(co.get("weight_decay")), float(co.get("final_weight_decay"))
    s.num_epochs, s.anneal, s.warmup = co.get("epochs"), co.get("anneal"), co.get("warmup")
    s.start_lr, s.lr, s.final_lr = co.get("start_lr"), co.get("lr"), co.get("final_lr")
    s.enc_lr_scale = co.get("enc_lr_scale", 1.0)
    s.betas, s.eps = co.get("betas", (0.9, 0.999)), co.get("eps", 1.0e-8)
    # The reference builds both models for 512 frames (train.py:196), which only sizes the predictor's
    # frame-causal mask (256 frames of HW + 2 tokens: 66048^2 entries at 256 px). The mask is sized here for
    # the clips of this run, doubled as the reference doubles every frame; no parameter's shape depends on it.
    s.model = dict(
        patch_size=s.patch_size, max_num_frames=s.tubelet_size * s.max_num_frames, tubelet_size=s.tubelet_size,
        model_name=cm.get("model_name"), crop_size=s.crop_size, pred_depth=cm.get("pred_depth"),
        pred_num_heads=cm.get("pred_num_heads", None), pred_embed_dim=cm.get("pred_embed_dim"), action_embed_dim=7,
        pred_is_frame_causal=cm.get("pred_is_frame_causal", True), use_extrinsics=cm.get("use_extrinsics", False),
        use_sdpa=meta.get("use_sdpa", False), use_silu=cm.get("use_silu", False),
        use_pred_silu=cm.get("use_pred_silu", False), wide_silu=cm.get("wide_silu", True),
        use_rope=cm.get("use_rope", False), uniform_power=cm.get("uniform_power", False),
        use_activation_checkpointing=cm.get("use_activation_checkpointing", False))
    return s


def main(args, resume_preempt=False):
    """app/vjepa_droid/train.py:54-524 on ACTrainer. Returns the per-iteration losses. resume_preempt is accepted
    and unused, as in the reference's main (train.py:54, 294): the run resumes whenever latest.pt exists."""
    c = settings(args)
    # the app's own refusals before anything is put on the device; nothing is written before the models are built
    # (a predictor variant that VisionTransformerPredictorAC refuses raises from init_video_model)
    world_size, rank = env_world_size(), 0
    if world_size > 1:
        raise NotImplementedError(f"V-JEPA 2-AC post-training on the HIP path runs on one GPU (world size "
                                  f"{world_size} requested): the predictor's gradient all-reduce is not wired")
    check_data_aug(args.get("data_aug") or {})
    if not c.model["use_rope"]:
        raise NotImplementedError("V-JEPA 2-AC post-training on the HIP path needs model.use_rope: true (the AC "
                                  "predictor without RoPE is not built; every DROID config uses RoPE)")
    if not torch.cuda.is_available():
        raise RuntimeError("V-JEPA 2-AC post-training on the HIP path needs an MI355X (no CPU path)")
    if c.which_dtype == "float16":
        logger.warning("float16 autocast requested: the HIP path computes bf16 GEMM operands instead")

    np.random.seed(c.seed)
    torch.manual_seed(c.seed)
    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", 0)))
    torch.cuda.set_device(device)
    log_file = os.path.join(c.folder, f"log_r{rank}.csv")
    latest_path = os.path.join(c.folder, "latest.pt")
    resume_path = os.path.join(c.folder, c.r_file) if c.r_file is not None else latest_path
    if not os.path.exists(resume_path):
        resume_path = None

    encoder, predictor = init_video_model(device=device, **c.model)
    target_encoder = encoder if c.shared_encoder else copy.deepcopy(encoder)
    loader, sampler = init_data(batch_size=c.batch_size, frames_per_clip=c.max_num_frames, crop_size=c.crop_size,
                                rank=rank, world_size=world_size, num_workers=0, num_samples=c.num_samples,
                                seed=c.seed)
    ipe = len(loader) if c.ipe is None else c.ipe
    optimizer, scaler, scheduler, wd_scheduler = init_opt(
        encoder=encoder, predictor=predictor, wd=c.wd, final_wd=c.final_wd, start_lr=c.start_lr, ref_lr=c.lr,
        final_lr=c.final_lr, enc_lr_scale=c.enc_lr_scale, iterations_per_epoch=ipe, anneal=c.anneal, warmup=c.warmup,
        num_epochs=c.num_epochs, mixed_precision=c.mixed_precision, betas=c.betas, eps=c.eps)
    if c.p_file is not None:
        load_pretrained(r_path=c.p_file, encoder=encoder, predictor=predictor, target_encoder=target_encoder,
                        context_encoder_key=c.context_encoder_key, target_encoder_key=c.target_encoder_key,
                        load_predictor=c.load_predictor, load_encoder=c.load_encoder)
    trainer = ACTrainer(predictor, target_encoder, optimizer, c.tokens_per_frame, auto_steps=c.auto_steps,
                        loss_exp=c.loss_exp, normalize_reps=c.normalize_reps, mixed_precision=c.mixed_precision,
                        world_size=world_size)

    start_epoch = 0
    if os.path.exists(latest_path) and resume_path is not None:
        *_, start_epoch = load_checkpoint(resume_path, encoder, predictor, target_encoder, optimizer, scaler)
        for _ in range(start_epoch * ipe):
            scheduler.step()
            wd_scheduler.step()

    os.makedirs(c.folder, exist_ok=True)
    if not os.path.exists(log_file):
        with open(log_file, "a", newline="") as f:
            csv.writer(f).writerow(["epoch", "itr", "loss", "iter-time(ms)", "gpu-time(ms)", "dataload-time(ms)"])
    losses = []
    for epoch in range(start_epoch, c.num_epochs):
        logger.info("Epoch %d", epoch + 1)
        sampler.set_epoch(epoch)  # an epoch's batches are a function of (seed, epoch): a resumed run sees the same
        loader_it = iter(loader)
        loss_sum = 0.0
        for itr in range(ipe):
            t0 = time.time()
            try:
                sample = next(loader_it)
            except StopIteration:
                loader_it = iter(loader)
                sample = next(loader_it)
            clips = sample[0].to(device, non_blocking=True)
            actions, states, extrinsics = (s.to(device, dtype=torch.float, non_blocking=True) for s in sample[1:4])
            data_ms = (time.time() - t0) * 1000.0

            def step():
                new_lr = scheduler.step()
                new_wd = wd_scheduler.step()
                # the one read-back of the step: the three losses, for the log (train.py:464-467)
                return trainer.train_step(clips, actions, states, extrinsics).tolist(), new_lr, new_wd

            ((loss, jloss, sloss), new_lr, new_wd), gpu_ms = gpu_timer(step)
            losses.append(loss)
            loss_sum += loss
            with open(log_file, "a", newline="") as f:
                csv.writer(f).writerow([epoch + 1, itr, f"{loss:.5f}", int((time.time() - t0) * 1000), int(gpu_ms),
                                        int(data_ms)])
            if itr % 10 == 0 or itr == ipe - 1:
                logger.info("[%d, %5d] loss: %.3f [%.2f, %.2f] [wd: %.2e] [lr: %.2e] [mem: %.2e] [gpu: %.1f ms]",
                            epoch + 1, itr, loss, jloss, sloss, new_wd, new_lr,
                            torch.cuda.max_memory_allocated() / 1024.0**2, gpu_ms)
            assert not np.isnan(loss), "loss is nan"
        avg = loss_sum / max(1, ipe)
        save_checkpoint(latest_path, encoder, predictor, target_encoder, optimizer, scaler, epoch + 1, avg,
                        c.batch_size, world_size, c.lr)
        if c.save_every_freq > 0 and epoch % c.save_every_freq == 0:
            save_checkpoint(os.path.join(c.folder, f"e{epoch}.pt"), encoder, predictor, target_encoder, optimizer,
                            scaler, epoch + 1, avg, c.batch_size, world_size, c.lr)
    return losses


def load_params(fname):
    """The launcher's YAML loading (vjepa2_amd.main.load_params; the launcher itself does not dispatch this app
    yet)."""
    from .main import load_params as _load

    return _load(fname)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description="V-JEPA 2-AC post-training on one MI355X")
    ap.add_argument("--fname", required=True, help="YAML config (the reference's droid-256px-8f.yaml layout)")
    ap.add_argument("--folder", default=None, help="override the config's output folder")
    a = ap.parse_args()
    logging.basicConfig(level=logging.INFO)
    params = load_params(a.fname)
    if a.folder is not None:
        params["folder"] = a.folder
    main(params)
