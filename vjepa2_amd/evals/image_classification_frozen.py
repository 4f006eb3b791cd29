"""Frozen-encoder image-classification probe (drop-in for evals/image_classification_frozen/eval.py and
its modelcustom/vit_encoder.py:38-83 init_module): the IN1K configs of configs/eval/.

`main(args_eval, resume_preempt)` reads the reference's config keys (eval.py:56-103) and runs its epoch
(eval.py:263-324): schedulers, the frozen encoder under no_grad on the image repeated along time, every
attentive classifier, CrossEntropyLoss, top-1 as 100 * correct / len(imgs) into a per-head average,
backward, one AdamW per classifier. That is the video probe's step with ONE view, so the step is
video_classification_frozen.ProbeTrainer (vj_xent with views=1, the arena AdamW, the bf16 convention of
evals/probe.py), and the schedules, init_opt, the meter, the checkpoint functions and the epoch loop are
evals/probe.py's, as they are for the video eval.
The encoder is the HIP VisionTransformer's forward(); the image repeat (eval: 0.2 GB at the IN1K shape,
against an encoder pass hundreds of times that) is a stride-0 expand that the patch embed reads.
Data is synthetic (timm, torchvision and an image folder are absent): data.num_samples /
data.num_val_samples images of SyntheticLabelledImageDataset.
Multi-GPU probe training (world_size > 1) is not ported.
"""

import logging
import math
import os

import torch

from .. import vision_transformer as vit
from ..attentive_pooler import AttentiveClassifier
from ..distributed import env_world_size
from . import probe
from .probe import load_checkpoint  # noqa: F401  (resume() calls it; here as save_checkpoint's counterpart)
from .probe import frozen, init_device, init_opt, load_pretrained, resume, save_checkpoint
from .video_classification_frozen import ProbeTrainer

logger = logging.getLogger(__name__)
IMAGE_MODULE = "evals.image_classification_frozen.modelcustom.vit_encoder"


class ImageAsVideoEncoder(torch.nn.Module):
    """modelcustom/vit_encoder.py:55-66: the video encoder behind a pre-hook that repeats an image
    img_as_video_nframes times along a new time axis."""

    def __init__(self, model, img_as_video_nframes):
        super().__init__()
        self.model = model
        self.nframes = int(img_as_video_nframes)
        self.embed_dim = model.embed_dim
        self.num_heads = model.num_heads

    def forward(self, imgs):
        """imgs [B, C, H, W] -> [B, N, D] f32."""
        if imgs.ndim != 4:
            raise ValueError(f"expected an image batch [B, C, H, W], got {tuple(imgs.shape)}")
        return self.model(imgs.unsqueeze(2).expand(-1, -1, self.nframes, -1, -1))


class _OneViewEncoder:
    """ProbeTrainer's encoder protocol (clips, clip_indices) -> list over views, for one image batch."""

    def __init__(self, encoder):
        self.encoder = encoder

    def __call__(self, imgs, clip_indices=None):
        return [self.encoder(imgs)]


def init_module(module_name, resolution, checkpoint, model_kwargs, wrapper_kwargs, device):
    """evals/image_classification_frozen/models.py + modelcustom/vit_encoder.py:38-83. The reference passes
    input_size=resolution (NOT img_size), which the constructor swallows in **kwargs: the model keeps
    img_size=224 whatever the images' size. A RoPE model takes its grid from the input; a sincos model
    interpolates its 14x14 table. Kept. Weights non-strict with the DDP / wrapper prefixes stripped;
    frozen, in eval mode, on `device`."""
    if module_name is not None and module_name != IMAGE_MODULE:
        raise NotImplementedError(f"encoder module {module_name!r}: only {IMAGE_MODULE} is ported")
    nframes = (wrapper_kwargs or {}).get("img_as_video_nframes")
    enc_kwargs = dict(model_kwargs["encoder"])
    ckp_key = enc_kwargs.get("checkpoint_key")
    model = vit.__dict__[enc_kwargs.get("model_name")](input_size=resolution, num_frames=nframes, **enc_kwargs)
    logger.info("Loading pretrained model from %s", checkpoint)
    ck = torch.load(checkpoint, map_location="cpu", weights_only=True)
    load_pretrained(model, ck[ckp_key], "model")
    del ck
    return frozen(ImageAsVideoEncoder(model, nframes), device)


class SyntheticLabelledImageDataset(torch.utils.data.Dataset):
    """(img [3, S, S], label) as the reference's ImageFolder loader delivers them (eval.py:287);
    deterministic per index, unit-scale noise plus the faint label-dependent offset of
    train.SyntheticLabelledVideoDataset."""

    def __init__(self, num_samples, img_size, num_classes, seed_offset=0):
        self.n, self.size, self.classes, self.seed_offset = num_samples, img_size, num_classes, seed_offset
        self.labels = (torch.arange(num_samples) * 7 + 3 + seed_offset) % num_classes

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        g = torch.Generator().manual_seed(self.seed_offset + 2000 + i)
        label = int(self.labels[i])
        shift = 0.5 * math.sin(1.0 + label)
        return torch.randn(3, self.size, self.size, generator=g) + shift, label


def make_dataloader(batch_size, num_samples, num_classes, img_size=224, world_size=1, rank=0, num_workers=0,
                    seed_offset=0):
    """eval.py:354-404 with the synthetic dataset (src/datasets/imagenet1k.py: DistributedSampler, drop_last
    False)."""
    ds = SyntheticLabelledImageDataset(num_samples, img_size, num_classes, seed_offset=seed_offset)
    sampler = torch.utils.data.distributed.DistributedSampler(ds, num_replicas=world_size, rank=rank, shuffle=False)
    loader = torch.utils.data.DataLoader(ds, batch_size=batch_size, sampler=sampler, num_workers=num_workers,
                                         drop_last=False, persistent_workers=num_workers > 0)
    return loader, sampler


class CSVLog:
    """src/utils/logging.py CSVLogger as eval.py:131, 255 uses it: the header line 'epoch,loss,acc' when
    the logger is made (appended, as the reference does on every start), then one line per epoch of
    epoch (%d), train accuracy (%.5f), validation accuracy (%.5f)."""

    def __init__(self, fname):
        self.fname = fname
        with open(fname, "+a") as f:
            print("epoch,loss,acc", file=f)

    def log(self, epoch, train_acc, val_acc):
        with open(self.fname, "+a") as f:
            print("%d,%.5f,%.5f" % (epoch, train_acc, val_acc), file=f)


def _unpack(data, device):
    """eval.py:287: the loader's (imgs, labels) as ProbeTrainer's (clips, clip_indices, labels)."""
    return data[0].to(device, non_blocking=True), None, data[1]


def run_one_epoch(trainer, device, training, data_loader, log_every=20):
    """eval.py:263-324: returns the best head's running top-1 (%)."""
    return probe.run_one_epoch(trainer, device, training, data_loader, _unpack, log_every)


def read_config(args_eval, resume_preempt=False):
    """The reference's keys (eval.py:56-103) plus the synthetic dataset's two."""
    c = probe.read_config(args_eval, resume_preempt, num_heads=16)
    args_data = args_eval.get("experiment").get("data")
    c.update(num_workers=args_eval.get("num_workers", 0),
             dataset_name=args_data.get("dataset_name"), num_classes=args_data.get("num_classes"),
             root_path=args_data.get("root_path", None), image_folder=args_data.get("image_folder", None),
             normalization=args_data.get("normalization", None),
             num_samples=args_data.get("num_samples"), num_val_samples=args_data.get("num_val_samples"))
    return c


def output_paths(pretrain_folder, eval_tag, rank=0):
    """eval.py:121-127: (folder, log file, latest.pt)."""
    return probe.output_paths(pretrain_folder, "image_classification_frozen", eval_tag, rank)


def main(args_eval, resume_preempt=False):
    """eval.py:49-260. Returns the best head's validation accuracy (%) of the last epoch run."""
    world_size, rank = env_world_size(), 0
    if world_size > 1:  # first: before the config is read, the checkpoint opened or a folder made
        raise NotImplementedError(f"image_classification_frozen on the HIP path runs on one GPU (world size "
                                  f"{world_size} requested): the multi-GPU run is not ported")
    c = read_config(args_eval, resume_preempt)
    val_only, batch_size, num_epochs, use_bfloat16 = c["val_only"], c["batch_size"], c["num_epochs"], c["use_bfloat16"]
    device = init_device("the frozen-encoder probe")
    folder, log_file, latest_path = output_paths(c["pretrain_folder"], c["eval_tag"], rank)
    os.makedirs(folder, exist_ok=True)
    csv_logger = CSVLog(log_file)

    encoder = init_module(module_name=c["module_name"], resolution=c["resolution"], checkpoint=c["checkpoint"],
                          model_kwargs=c["args_model"], wrapper_kwargs=c["args_wrapper"], device=device)
    classifiers = [AttentiveClassifier(embed_dim=encoder.embed_dim, num_heads=c["num_heads"],
                                       depth=c["num_probe_blocks"], num_classes=c["num_classes"],
                                       use_activation_checkpointing=True).to(device) for _ in c["opt_kwargs"]]

    n_train = int(c["num_samples"] if c["num_samples"] is not None else 64 * batch_size)
    n_val = int(c["num_val_samples"] if c["num_val_samples"] is not None else n_train)
    kw = dict(batch_size=batch_size, num_classes=c["num_classes"], img_size=c["resolution"], world_size=world_size,
              rank=rank, num_workers=c["num_workers"])
    train_loader, train_sampler = make_dataloader(num_samples=n_train, **kw)
    val_loader, _ = make_dataloader(num_samples=n_val, seed_offset=1 << 20, **kw)
    ipe = len(train_loader)
    logger.info("Dataloader created... iterations per epoch: %d", ipe)

    optimizer, scaler, scheduler, wd_scheduler = init_opt(classifiers=classifiers, opt_kwargs=c["opt_kwargs"],
                                                          iterations_per_epoch=ipe, num_epochs=num_epochs,
                                                          use_bfloat16=use_bfloat16)
    trainer = ProbeTrainer(_OneViewEncoder(encoder), classifiers, optimizer, scaler, scheduler, wd_scheduler,
                           use_bfloat16=use_bfloat16)

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
        csv_logger.log(epoch + 1, train_acc, val_acc)
        if val_only:
            return val_acc
        save_checkpoint(latest_path, classifiers, optimizer, scaler, epoch + 1, batch_size, world_size)
    return val_acc
