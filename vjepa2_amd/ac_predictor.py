"""V-JEPA 2-AC action-conditioned predictor (src/models/ac_predictor.py:17-200) on the HIP kernels:
same constructor signature, init RNG order and state_dict() keys as the reference.

The reference interleaves, per frame, the action / state (/ extrinsics) tokens in front of the frame's
H*W tokens (ac_predictor.py:161-172) and runs ACBlocks with a frame-causal attention mask
(build_action_block_causal_attention_mask, modules.py:12-23). Here:
 * the embeddings are HIP GEMMs (the 7-wide encoders' reduction dim zero-padded to 8);
 * the interleaved sequence is assembled by row scatters (vj_gather_rows, scatter mode) from the
   embedding outputs, and its backward is the matching gathers;
 * every block is the fused HIP block (functions.run_block) on a TokenLayout whose RoPE ids put each
   frame's conditioning tokens at (frame, 0, 0) (depth rotation only, ACRoPEAttention :184-200) and
   whose attention is frame-causal over blocks of cond + H*W tokens (vj_attn_fwd_fc / vj_attn_bwd_fc);
 * the frame tokens are gathered back out (ac_predictor.py:187-189) before predictor_norm / proj.
"""

import math
from functools import partial

import torch
import torch.nn as nn

from . import functions as fn
from . import ops
from .modules import ACBlock, ac_token_layout, build_action_block_causal_attention_mask, trunc_normal_


class _ScatterRowsFn(torch.autograd.Function):
    """seq[idx_i] = src_i for several sources (every row of seq written exactly once); backward gathers."""

    @staticmethod
    def forward(ctx, S, idxs, *srcs):
        D = srcs[0].shape[1]
        seq = torch.empty(S, D, dtype=torch.float32, device=srcs[0].device)
        for src, idx in zip(srcs, idxs):
            ops.scatter_rows(src.float().contiguous(), idx, seq)
        ctx.idxs = idxs
        return seq

    @staticmethod
    def backward(ctx, dseq):
        dseq = dseq.contiguous()
        return (None, None) + tuple(ops.gather_rows(dseq, idx) for idx in ctx.idxs)


class ACRolloutCache:
    """Per-block keys and values of the frames a rollout has fed so far (VisionTransformerPredictorAC.new_cache /
    forward_cached). The predictor's attention is frame-causal: the hidden states of frames 0 .. t-1, and so
    their keys and values in every block, do not depend on frame t, and a rollout that appends one frame per
    step needs only the new frame's rows through the GEMMs.

    kv[i]: block i's bf16 [batch, max_frames * n_t, 2 * H * hd] buffer (K | V columns, RoPE applied to K),
    n_t = cond + H*W tokens per frame, sample-major so a sequence's keys are contiguous. Allocated once:
    depth * batch * max_frames * n_t * 2 * D * 2 bytes (DROID planning, 400 samples, 2 frames, n_t 258,
    D 1024, 24 blocks: 400 * 2 * 258 * 4096 B * 24 = 20.3 GB). `frames` is a host counter: the rows of frames
    >= `frames` are stale and never read (vj_attn_fwd_kv sees the first frames * n_t rows only), so rewind()
    and reset() do no device work."""

    def __init__(self, depth, batch, max_frames, n_t, width, hw, grid_w, cond, device):
        self.batch, self.max_frames, self.n_t, self.cond = int(batch), int(max_frames), int(n_t), int(cond)
        self.hw, self.grid_w = int(hw), int(grid_w)
        self.frames = 0
        self.kv = [torch.empty(self.batch, self.max_frames * self.n_t, 2 * width, dtype=torch.bfloat16, device=device)
                   for _ in range(depth)]
        self._layouts = {}

    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in self.kv)

    def rewind(self, t):
        """Forget the frames from t on (0 <= t <= frames): the next forward_cached appends at frame t."""
        t = int(t)
        if not 0 <= t <= self.frames:
            raise ValueError(f"rewind({t}): the cache holds {self.frames} frames")
        self.frames = t

    def reset(self):
        self.rewind(0)

    def layout(self, t0, tn):
        """ac_token_layout's TokenLayout for the rows of frames t0 .. t0 + tn - 1 alone: the same RoPE ids those
        rows have in the full sequence, ids_mod (and so the RoPE tables) sized for max_frames whatever t0."""
        lay = self._layouts.get((t0, tn))
        if lay is None:
            dev = self.kv[0].device
            t = torch.arange(t0, t0 + tn, device=dev)[:, None]
            j = torch.arange(self.n_t, device=dev)[None, :]
            ids = torch.where(j < self.cond, t * self.hw, t * self.hw + (j - self.cond))
            ids = ids.reshape(1, -1).expand(self.batch, -1).reshape(-1).to(torch.int32).contiguous()
            lay = fn.TokenLayout([(self.batch, tn * self.n_t)], ids=ids, ids_mod=self.max_frames * self.hw,
                                 tpf=self.hw, tpr=self.grid_w, fblk=self.n_t)
            self._layouts[(t0, tn)] = lay
        return lay


class VisionTransformerPredictorAC(nn.Module):
    """ac_predictor.py:17-190."""

    def __init__(self, img_size=(224, 224), patch_size=16, num_frames=1, tubelet_size=2, embed_dim=768,
                 predictor_embed_dim=1024, depth=24, num_heads=16, mlp_ratio=4.0, qkv_bias=True, qk_scale=None,
                 drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.0, norm_layer=nn.LayerNorm, init_std=0.02,
                 uniform_power=True, use_silu=False, wide_silu=True, is_frame_causal=True,
                 use_activation_checkpointing=False, use_rope=True, action_embed_dim=7, use_extrinsics=False,
                 **kwargs):
        super().__init__()
        self.is_frame_causal = is_frame_causal
        self.use_extrinsics = use_extrinsics
        self.predictor_embed = nn.Linear(embed_dim, predictor_embed_dim, bias=True)
        self.action_encoder = nn.Linear(action_embed_dim, predictor_embed_dim, bias=True)
        self.state_encoder = nn.Linear(action_embed_dim, predictor_embed_dim, bias=True)
        self.extrinsics_encoder = nn.Linear(action_embed_dim - 1, predictor_embed_dim, bias=True)
        if type(img_size) is int:
            img_size = (img_size, img_size)
        self.img_height, self.img_width = img_size
        self.patch_size = patch_size
        self.num_frames = num_frames
        self.tubelet_size = tubelet_size
        self.is_video = num_frames > 1
        self.grid_height = img_size[0] // self.patch_size
        self.grid_width = img_size[1] // self.patch_size
        self.use_activation_checkpointing = use_activation_checkpointing
        dpr = [x.item() for x in torch.linspace(0, drop_path_rate, depth)]
        self.uniform_power = uniform_power
        self.use_rope = use_rope
        if not use_rope:
            raise NotImplementedError("the AC predictor without RoPE is not on the HIP path (configs use RoPE)")
        self.predictor_blocks = nn.ModuleList([
            ACBlock(use_rope=use_rope, grid_size=self.grid_height, dim=predictor_embed_dim, num_heads=num_heads,
                    mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale, drop=drop_rate,
                    act_layer=nn.SiLU if use_silu else nn.GELU, wide_silu=wide_silu, attn_drop=attn_drop_rate,
                    drop_path=dpr[i], norm_layer=norm_layer) for i in range(depth)])
        self.predictor_norm = norm_layer(predictor_embed_dim)
        self.predictor_proj = nn.Linear(predictor_embed_dim, embed_dim, bias=True)
        self.init_std = init_std
        self.apply(self._init_weights)
        self._rescale_blocks()
        attn_mask = None
        if self.is_frame_causal:
            attn_mask = build_action_block_causal_attention_mask(self.num_frames // self.tubelet_size,
                                                                 self.grid_height, self.grid_width,
                                                                 add_tokens=3 if use_extrinsics else 2)
        self.attn_mask = attn_mask
        self._idx_cache = {}

    def _init_weights(self, m):
        """ac_predictor.py:124-131."""
        if isinstance(m, nn.Linear):
            trunc_normal_(m.weight, std=self.init_std)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    def _rescale_blocks(self):
        """ac_predictor.py:133-139."""
        for layer_id, layer in enumerate(self.predictor_blocks):
            layer.attn.proj.weight.data.div_(math.sqrt(2.0 * (layer_id + 1)))
            layer.mlp.fc2.weight.data.div_(math.sqrt(2.0 * (layer_id + 1)))

    def _indices(self, B, T, cond, device):
        """Rows of the interleaved [B*T*(cond + H*W)] sequence taken by each source (int32, device)."""
        key = (B, T, cond, str(device))
        c = self._idx_cache.get(key)
        if c is None:
            hw = self.grid_height * self.grid_width
            n_t = cond + hw
            base = (torch.arange(B * T, device=device) * n_t)[:, None]
            conds = [(base + i).reshape(-1).to(torch.int32).contiguous() for i in range(cond)]
            frame = (base + cond + torch.arange(hw, device=device)[None, :]).reshape(-1).to(torch.int32).contiguous()
            c = (conds, frame)
            self._idx_cache[key] = c
        return c

    def forward(self, x, actions, states, extrinsics=None):
        """ac_predictor.py:141-190: x [B, T*H*W, embed_dim] context tokens, actions / states [B, T, 7]
        (extrinsics [B, T, 6]) -> [B, T*H*W, embed_dim] (f32)."""
        B, N_ctxt, C = x.shape
        hw = self.grid_height * self.grid_width
        T = N_ctxt // hw
        cond = 3 if self.use_extrinsics else 2
        e = fn.run_linear(x.reshape(B * N_ctxt, C), self.predictor_embed, out_dtype=torch.float32)
        a = fn.run_linear(actions.reshape(B * T, -1), self.action_encoder, out_dtype=torch.float32)
        s = fn.run_linear(states.reshape(B * T, -1), self.state_encoder, out_dtype=torch.float32)
        srcs = [a, s]
        if self.use_extrinsics:
            srcs.append(fn.run_linear(extrinsics.reshape(B * T, -1), self.extrinsics_encoder, out_dtype=torch.float32))
        conds, frame = self._indices(B, T, cond, x.device)
        S = B * T * (cond + hw)
        seq = _ScatterRowsFn.apply(S, conds + [frame], *srcs, e)
        if self.attn_mask is not None and T > self.num_frames // self.tubelet_size:
            raise ValueError("more frames than the frame-causal mask was built for (ac_predictor.py:174)")
        lay = ac_token_layout(B, T, self.grid_height, self.grid_width, cond, self.attn_mask is not None, x.device)
        for blk in self.predictor_blocks:
            seq = fn.run_block(seq, blk, lay)
        rows = fn.gather_rows(seq, frame)
        y = fn.run_layernorm(rows, self.predictor_norm, out_dtype=torch.bfloat16)
        out = fn.run_linear(y, self.predictor_proj, out_dtype=torch.float32)
        return out.reshape(B, T * hw, -1)

    def new_cache(self, batch, max_frames):
        """An ACRolloutCache for forward_cached: `batch` sequences of up to `max_frames` frames. One bf16
        [batch, max_frames * n_t, 2 * predictor_embed_dim] buffer per block (sizes: ACRolloutCache)."""
        if not self.is_frame_causal:
            raise ValueError("new_cache: the predictor is not frame-causal (is_frame_causal=False): earlier frames "
                             "see later ones, so their keys and values cannot be cached")
        if max_frames < 1 or batch < 1:
            raise ValueError(f"new_cache: batch {batch} and max_frames {max_frames} must be >= 1")
        if max_frames > self.num_frames // self.tubelet_size:
            raise ValueError(f"new_cache: max_frames {max_frames} exceeds the {self.num_frames // self.tubelet_size} "
                             "frames the frame-causal mask was built for (num_frames // tubelet_size)")
        cond = 3 if self.use_extrinsics else 2
        hw = self.grid_height * self.grid_width
        width = self.predictor_embed.weight.shape[0]
        return ACRolloutCache(len(self.predictor_blocks), batch, max_frames, cond + hw, width, hw, self.grid_width,
                              cond, self.predictor_embed.weight.device)

    def forward_cached(self, x_new, actions_new, states_new, extrinsics_new=None, *, cache):
        """forward() one chunk of frames at a time: x_new [B, Tn*H*W, embed_dim], actions_new / states_new
        [B, Tn, 7] (extrinsics_new [B, Tn, 6]) are frames t0 .. t0 + Tn - 1 of a sequence whose first
        t0 = cache.frames frames earlier calls fed. Returns [B, Tn*H*W, embed_dim] (f32), mathematically rows
        [t0*H*W, (t0 + Tn)*H*W) of forward() over all t0 + Tn frames, and advances cache.frames by Tn. Only the
        new rows go through the GEMMs; their attention reads the earlier frames' keys and values from the
        cache. Inference only, frame-causal predictors only, no active dropout / drop_path."""
        hw = self.grid_height * self.grid_width
        B, N_new, C = x_new.shape
        Tn = N_new // hw
        cond = 3 if self.use_extrinsics else 2
        # every refusal before any device work, the cache untouched
        if not isinstance(cache, ACRolloutCache):
            raise TypeError("forward_cached: cache must be an ACRolloutCache (predictor.new_cache)")
        if not self.is_frame_causal:
            raise ValueError("forward_cached: the predictor is not frame-causal (is_frame_causal=False): the cached "
                             "keys and values of earlier frames would be invalid")
        if torch.is_grad_enabled():
            ins = [t for t in (x_new, actions_new, states_new, extrinsics_new) if t is not None]
            if any(t.requires_grad for t in ins) or any(p.requires_grad for p in self.parameters()):
                raise RuntimeError("forward_cached is inference only (there is no backward through the cache): call it "
                                   "under torch.no_grad(), or with no input or parameter requiring grad")
        for i, blk in enumerate(self.predictor_blocks):
            why = fn.cached_block_refusal(blk)
            if why is not None:
                raise RuntimeError(f"forward_cached: block {i}: {why}; the cached forward is the deterministic "
                                   "inference path (call eval(), drop rates 0)")
        if Tn < 1 or N_new != Tn * hw:
            raise ValueError(f"forward_cached: {N_new} tokens are not whole frames of {hw}")
        if B != cache.batch:
            raise ValueError(f"forward_cached: batch {B} != cache.batch {cache.batch}")
        if (cache.n_t, cache.cond, len(cache.kv)) != (cond + hw, cond, len(self.predictor_blocks)):
            raise ValueError("forward_cached: the cache was made for another predictor")
        t0 = cache.frames
        if t0 + Tn > cache.max_frames:
            raise ValueError(f"forward_cached: {t0} cached + {Tn} new frames exceed the cache's max_frames "
                             f"{cache.max_frames}")
        if actions_new.shape[:2] != (B, Tn) or states_new.shape[:2] != (B, Tn):
            raise ValueError(f"forward_cached: actions / states must be [{B}, {Tn}, 7]")
        if self.use_extrinsics and extrinsics_new is None:
            raise ValueError("forward_cached: the predictor uses extrinsics")
        n_t = cond + hw
        e = fn.run_linear(x_new.reshape(B * N_new, C), self.predictor_embed, out_dtype=torch.float32)
        a = fn.run_linear(actions_new.reshape(B * Tn, -1), self.action_encoder, out_dtype=torch.float32)
        s = fn.run_linear(states_new.reshape(B * Tn, -1), self.state_encoder, out_dtype=torch.float32)
        srcs = [a, s]
        if self.use_extrinsics:
            srcs.append(fn.run_linear(extrinsics_new.reshape(B * Tn, -1), self.extrinsics_encoder,
                                      out_dtype=torch.float32))
        conds, frame = self._indices(B, Tn, cond, x_new.device)
        seq = _ScatterRowsFn.apply(B * Tn * n_t, conds + [frame], *srcs, e)
        lay = cache.layout(t0, Tn)
        for blk, kv in zip(self.predictor_blocks, cache.kv):
            seq = fn.block_forward_cached(seq, blk, lay, kv, t0 * n_t)
        rows = fn.gather_rows(seq, frame)
        y = fn.run_layernorm(rows, self.predictor_norm, out_dtype=torch.bfloat16)
        out = fn.run_linear(y, self.predictor_proj, out_dtype=torch.float32)
        cache.frames = t0 + Tn
        return out.reshape(B, Tn * hw, -1)


def vit_ac_predictor(**kwargs):
    """ac_predictor.py:193-200."""
    return VisionTransformerPredictorAC(mlp_ratio=4, qkv_bias=True, norm_layer=partial(nn.LayerNorm, eps=1e-6),
                                        **kwargs)
