"""Multi-clip frozen-encoder wrapper of the video-classification evals
(evals/video_classification_frozen/modelcustom/vit_encoder_multiclip.py:87-162, ClipAggregation):
every (clip, view) goes through the encoder as one batch, the tokens of a view's clips are
concatenated along time, and an optional 1-D temporal sincos embedding is added at each clip's frame
indices. The encoder is the HIP VisionTransformer; the optional embedding add is vj_add_rows.

ClipAggregationMultilevel is the wrapper of the Diving48 / Jester configs
(modelcustom/vit_encoder_multiclip_multilevel.py:85-155): the encoder's out_layers are tapped and their
normed tokens concatenated along the token axis before the same regrouping. Each tap's LayerNorm is
written once, by vj_layernorm_taps, into the buffer the classifiers read.
"""

import os

import numpy as np
import torch
import torch.nn as nn

from . import ops


def get_1d_sincos_pos_embed(embed_dim, grid_size):
    """src/models/utils/pos_embs.py:96-105 (float64 numpy, cls_token=False): [grid_size, embed_dim]."""
    pos = np.arange(grid_size, dtype=float)
    omega = np.arange(embed_dim // 2, dtype=np.float64)
    omega /= embed_dim / 2.0
    omega = 1.0 / 10000**omega
    out = np.einsum("m,d->md", pos.reshape(-1), omega)
    return np.concatenate([np.sin(out), np.cos(out)], axis=1)


class ClipAggregation(nn.Module):
    """vit_encoder_multiclip.py:87-162: process each clip independently and concatenate all tokens."""

    def __init__(self, model, tubelet_size=2, max_frames=128, use_pos_embed=False):
        super().__init__()
        self.model = model
        self.tubelet_size = tubelet_size
        self.embed_dim = embed_dim = model.embed_dim
        self.num_heads = model.num_heads
        self.pos_embed = None
        if use_pos_embed:
            max_T = max_frames // tubelet_size
            self.pos_embed = nn.Parameter(torch.zeros(1, max_T, embed_dim), requires_grad=False)
            sincos = get_1d_sincos_pos_embed(embed_dim, max_T)
            with torch.no_grad():
                self.pos_embed.copy_(torch.from_numpy(sincos).float().unsqueeze(0))

    def forward(self, x, clip_indices=None):
        """x: list over clips of lists over views of [B, C, F, H, W]; clip_indices: list over clips of
        [B, F] frame indices. Returns a list over views of [B, num_clips * T * S, D] (f32)."""
        num_clips = len(x)
        num_views = len(x[0])
        B, C, Fr, H, W = x[0][0].size()
        xb = torch.cat([torch.cat(xi, dim=0) for xi in x], dim=0)
        outputs = self.model(xb)  # [num_clips * num_views * B, N, D]
        _, N, D = outputs.size()
        T = Fr // self.tubelet_size
        S = N // T
        eff_B = B * num_views
        views = []
        for j in range(num_views):
            # [num_clips, B, T*S, D] of this view -> [B, num_clips*T*S, D] (time-major concatenation)
            o = torch.stack([outputs[i * eff_B + j * B:i * eff_B + (j + 1) * B] for i in range(num_clips)], 1)
            o = o.reshape(B, num_clips * T * S, D).contiguous()
            if self.pos_embed is not None and clip_indices is not None:
                # row (b, c, t, s) += pos_embed[clip_indices[c][b, t * tubelet]] (apply_masks of the table)
                idx = torch.stack([ci[:, ::self.tubelet_size] for ci in clip_indices], 1)  # [B, clips, T]
                # CPU indices (the eval loaders' clip_indices) are validated here and raise as the
                # reference's gather would; device indices are not read back (no host sync per forward)
                # unless VJ_CHECK_INDICES=1 (debug): vj_add_rows never reads a table row outside
                # [0, rows) and leaves such a row unchanged
                if not idx.is_cuda or os.environ.get("VJ_CHECK_INDICES", "0") == "1":
                    lo, hi = int(idx.min()), int(idx.max())
                    if lo < 0 or hi >= self.pos_embed.shape[1]:
                        raise IndexError(f"clip index {hi if hi >= self.pos_embed.shape[1] else lo} out of range "
                                         f"for the temporal pos_embed of {self.pos_embed.shape[1]} frames")
                idx = idx.to(device=o.device, dtype=torch.int32)
                idx = idx.reshape(B, num_clips * T, 1).expand(B, num_clips * T, S).reshape(-1).contiguous()
                table = self.pos_embed[0].detach().float().contiguous()
                ops.add_rows(o.view(-1, D), table, idx=idx)
            views.append(o)
        return views


def multilevel_dst_blocks(num_clips, num_views, B, L):
    """Where ClipAggregationMultilevel puts each (encoder batch row, tap): a list over taps l of lists over
    encoder rows g = i*V*B + j*B + b (clip i, view j, sample b) of the block ((j*B + b)*clips + i)*L + l,
    blocks counted in units of one sample's N tokens in the [V*B, clips*L*N, D] buffer. This is the
    reference's row order (vit_encoder_multiclip_multilevel.py:123-141: cat over levels along tokens, then
    per view the clips along time) inside a sample, and ProbeTrainer's row v*B + b across views."""
    eff_B = num_views * B
    return [[((g % eff_B) * num_clips + g // eff_B) * L + l for g in range(num_clips * eff_B)] for l in range(L)]


def multilevel_pos_rows(clip_indices, tubelet_size, L, N, T):
    """The temporal pos-embed row of every token row of one view, [B, clips * L * N] (the dtype of
    clip_indices). The reference derives S = (L*N) // T from the CONCATENATED token count
    (vit_encoder_multiclip_multilevel.py:126-128, 140, 148), so row r of a clip's L*N rows takes frame
    index (r // S) * tubelet of that clip whatever level it came from: kept exactly."""
    S = (L * N) // T
    if T * S != L * N:
        raise ValueError(f"{L} levels of {N} tokens do not split into {T} temporal indices")
    idx = torch.stack([ci[:, ::tubelet_size] for ci in clip_indices], 1)  # [B, clips, T]
    Bc, clips, Tc = idx.shape
    if Tc != T:
        raise ValueError(f"clip_indices give {Tc} temporal indices per clip, the clips have {T}")
    return idx.reshape(Bc, clips * T, 1).expand(Bc, clips * T, S).reshape(Bc, clips * T * S)


class ClipAggregationMultilevel(nn.Module):
    """vit_encoder_multiclip_multilevel.py:85-155 (ClipAggregation of the Diving48 / Jester configs): the
    encoder returns its out_layers' normed tokens, concatenated along the token axis, then regrouped per
    view as in ClipAggregation. Here every tapped layer's LayerNorm is written once, by
    vj_layernorm_taps, into the one [V*B, clips*L*N, D] buffer the classifiers read (multilevel_dst_blocks);
    the reference's four copies of that tensor (LayerNorm outputs, cat over levels, per-view regroup, cat
    over views) are never made."""

    def __init__(self, model, tubelet_size=2, max_frames=128, use_pos_embed=False, out_layers=None):
        super().__init__()
        if not getattr(model, "tap_layers", None) or not model.tap_layers():
            raise ValueError("ClipAggregationMultilevel needs an encoder built with out_layers")
        self.model = model
        self.tubelet_size = tubelet_size
        self.embed_dim = embed_dim = model.embed_dim
        self.num_heads = model.num_heads
        self.pos_embed = None
        if use_pos_embed:
            max_T = max_frames // tubelet_size
            self.pos_embed = nn.Parameter(torch.zeros(1, max_T, embed_dim), requires_grad=False)
            sincos = get_1d_sincos_pos_embed(embed_dim, max_T)
            with torch.no_grad():
                self.pos_embed.copy_(torch.from_numpy(sincos).float().unsqueeze(0))

    @torch.no_grad()
    def forward_stacked(self, x, clip_indices=None):
        """x, clip_indices as forward(). Returns (f32 [V*B, clips*L*N, D] with row v*B + b = sample b of
        view v, V): the buffer forward()'s views are slices of, allocated once per call."""
        num_clips = len(x)
        num_views = len(x[0])
        B, C, Fr, H, W = x[0][0].size()
        xb = torch.cat([torch.cat(xi, dim=0) for xi in x], dim=0)
        _, Tp, Hp, Wp, _, _ = self.model._geometry(xb)
        N, L, D = Tp * Hp * Wp, len(self.model.tap_layers()), self.embed_dim
        buf = torch.empty(num_views * B, num_clips * L * N, D, dtype=torch.float32, device=xb.device)
        self.model.forward_taps(xb, buf.view(-1, D), multilevel_dst_blocks(num_clips, num_views, B, L))
        if self.pos_embed is not None and clip_indices is not None:
            idx = multilevel_pos_rows(clip_indices, self.tubelet_size, L, N, Fr // self.tubelet_size)
            # CPU indices are validated here and raise as the reference's gather would; device indices are
            # not read back unless VJ_CHECK_INDICES=1 (as ClipAggregation: vj_add_rows leaves a row whose
            # table id is out of range unchanged)
            if not idx.is_cuda or os.environ.get("VJ_CHECK_INDICES", "0") == "1":
                lo, hi = int(idx.min()), int(idx.max())
                if lo < 0 or hi >= self.pos_embed.shape[1]:
                    raise IndexError(f"clip index {hi if hi >= self.pos_embed.shape[1] else lo} out of range "
                                     f"for the temporal pos_embed of {self.pos_embed.shape[1]} frames")
            idx = idx.to(device=buf.device, dtype=torch.int32)
            idx = idx.unsqueeze(0).expand(num_views, *idx.shape).reshape(-1).contiguous()  # every view alike
            table = self.pos_embed[0].detach().float().contiguous()
            ops.add_rows(buf.view(-1, D), table, idx=idx)
        return buf, num_views

    def forward(self, x, clip_indices=None):
        """x: list over clips of lists over views of [B, C, F, H, W]; clip_indices: list over clips of
        [B, F] frame indices. Returns the reference's list over views of [B, num_clips * L * N, D] (f32):
        row-slices of forward_stacked()'s buffer."""
        buf, V = self.forward_stacked(x, clip_indices)
        B = buf.shape[0] // V
        return [buf[j * B:(j + 1) * B] for j in range(V)]
