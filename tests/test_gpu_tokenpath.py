"""GPU: the token-path kernels of csrc/vj_ops.hip outside the GEMM / attention / row-op regime, called at the C
entry points (vjepa2_amd._lib.call) with every operand inside a poisoned buffer and every output inside a
sentinel buffer with slack on both sides (tests/test_gpu_gemm_strided.py's OutFrame / _in_vec; integer outputs:
_IntOut below). Every index handed to a kernel is in range: a wrong offset shows as a wrong value or a touched
guard, never as a fault. References and bounds: tests/kernel_refs.py (checked on the CPU by
tests/test_kernel_refs.py).

Branches launched, per kernel:
  k_im2col<false>, k_im2col<true>  kdim / 4 = 4 (one partial wave), 144, 384 and 400 (two trips of the
                               256-thread loop, the second partial); tub 1 / 2 / 3; p = 4, 8, 16 and 20 (col % p
                               with p no power of two); C = 1 .. 3; a one-token grid; B = 1 and 3; idx NULL,
                               sorted, unsorted with repeats, K = 1, and R = B K - 3 (the tail rows keep the
                               sentinel). Unlisted tokens are NaN: the kernel reads only what idx names. +-0,
                               f32 subnormals, +-inf and 3.4e38 (-> bf16 inf) bitwise; NaN as NaN.
  k_pred_index                 n = 2, 255, 256, 257, 1479 and 16384 (64 KiB of dynamic LDS); the merge-path branch
                               (sorted rows, ids shared by mx and my, an equal pair straddling the K boundary)
                               and the counting branch (one unsorted row in mx, one in my, repeats inside mx);
                               bmod 0 / B / B / 2 / 1; loss_rows NULL or not; row0 0 and 17 (pos[:row0] untouched)
  k_mask_count, k_mask_emit    N = 30 (most threads own no token), 231, 256, 257 (two tokens per thread, trailing
                               threads empty) and 2048; blocks 1x1x1, full duration, mid size; npred 1 / 2 / 4
                               with identical, overlapping and far-corner boxes; max_ctx = duration, duration - 1
                               and 1; modes 0 / 1 / 2; k_enc the batch minimum and 1; plus the host and device
                               collators side by side on 2x2 and 3x3 grids
  k_video_transform            one-row, one-column and one-pixel boxes, the far corner, an identity resize
                               (bitwise), a 4.8x downscale, 2048-wide and 600-tall crops (index precision), both
                               flips, C = 1 and 3, totals that are no multiple of 256; against float64 with the
                               derived bound, and bitwise unchanged when every byte outside the boxes changes
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

import kernel_refs as kr  # noqa: E402
from test_gpu_gemm_strided import BF16, DEV, F32, OutFrame, _in_vec  # noqa: E402
from test_gpu_rowops import _ovec, _same  # noqa: E402

I32, I64 = torch.int32, torch.int64
INT_SENT = {I32: 0x7FC12345, I64: 0x7FC1234512345678}
PAD = 16  # elements of slack on both sides of an integer buffer


def _call(name, *args):
    from vjepa2_amd import _lib

    return _lib.call(name, *args)


def _st():
    return torch.cuda.current_stream().cuda_stream


class _IntOut:
    """n integer outputs inside a sentinel buffer with PAD elements of slack on both sides."""

    def __init__(self, n, dtype):
        self.n, self.sent = n, INT_SENT[dtype]
        self.buf = torch.full((n + 2 * PAD,), self.sent, dtype=dtype, device=DEV)
        self.ptr = self.buf[PAD:].data_ptr()

    def read(self, what):
        raw = self.buf.cpu()
        guard = torch.cat([raw[:PAD], raw[PAD + self.n:]])
        assert bool((guard == self.sent).all()), f"{what}: slack around the output was written"
        return raw[PAD:PAD + self.n].clone()


def _in_ints(t, poison):
    """An integer / byte operand as a 16-B aligned slice of a longer buffer holding `poison` elsewhere."""
    buf = torch.full((t.numel() + 2 * PAD,), poison, dtype=t.dtype)
    buf[PAD:PAD + t.numel()] = t.reshape(-1)
    out = buf.to(DEV)[PAD:PAD + t.numel()]
    assert out.data_ptr() % 16 == 0
    return out


# ------------------------------------------------------------------------------------------------
# im2col
SPECIALS = [0.0, -0.0, 1e-40, -1e-40, float("inf"), float("-inf"), 3.4e38, -3.4e38]


def _im2col_idx(kind, B, N, g):
    """-> (idx int64 [B, K] or None, K, R)."""
    if kind == "all":
        return None, N, B * N
    if kind == "sorted":
        K = max(1, N // 2)
        return torch.stack([torch.randperm(N, generator=g)[:K].sort().values for _ in range(B)]), K, B * K
    if kind == "one":
        return torch.randint(0, N, (B, 1), generator=g), 1, B
    idx = torch.randint(0, N, (B, 5), generator=g)
    idx[:, 3] = idx[:, 0]                      # a repeated id
    idx[:, 1], idx[:, 2] = N - 1, 0            # descending somewhere
    return idx, 5, B * 5 - (3 if kind == "short" else 0)


def _im2col_launch(clip_dev, idx_dev, R, K, B, geom, f32, what):
    C, Tf, Hf, Wf, tub, p = geom
    kdim = C * tub * p * p
    fo = OutFrame(B * K, kdim, kdim, F32 if f32 else BF16)
    _call("vj_im2col_tubelet_f32" if f32 else "vj_im2col_tubelet", R, K, None if idx_dev is None else idx_dev.data_ptr(),
          B, C, Tf, Hf, Wf, tub, p, clip_dev.data_ptr(), fo.win.data_ptr(), _st())
    torch.cuda.synchronize()
    bits = fo.read(what)
    assert bool((bits[R:] == fo.sent).all()), f"{what}: rows past R were written"
    return bits[:R].view(F32 if f32 else BF16)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("geom", kr.IM2COL_GEOMS, ids=lambda g: "x".join(map(str, g)))
def test_im2col_gathers_listed_tokens_bitwise(geom, B):
    C, Tf, Hf, Wf, tub, p = geom
    N = kr.im2col_tokens(geom)
    g = torch.Generator().manual_seed(1000 * B + Hf * Wf)
    for kind in ("all", "sorted", "unsorted", "one", "short"):
        idx, K, R = _im2col_idx(kind, B, N, g)
        clip = torch.randn(B, C, Tf, Hf, Wf, generator=g)
        sp = torch.randint(0, 50, clip.shape, generator=g)
        for i, v in enumerate(SPECIALS):
            clip[sp == i] = v
        flat = None if idx is None else idx.reshape(-1)
        rows = torch.arange(R)
        toks = (rows % K) if idx is None else flat[:R]
        listed = kr.im2col_token_mask(clip.shape, (rows // K).tolist(), toks.tolist(), tub, p)
        clip[~listed] = float("nan")  # whatever the kernel may not read
        clip_dev = _in_vec(clip.reshape(-1))
        idx_dev = None if idx is None else _in_ints(flat, -(1 << 40))
        for f32 in (False, True):
            what = f"im2col {geom} B={B} idx={kind} {'f32' if f32 else 'bf16'}"
            if R == 0:
                continue
            got = _im2col_launch(clip_dev, idx_dev, R, K, B, geom, f32, what)
            exp = kr.im2col_ref(clip if f32 else clip.bfloat16(), flat, K, tub, p, R=R)
            assert not bool(exp.isnan().any())
            assert not bool(got.isnan().any()), f"{what}: a pixel of an unlisted token was read"
            it = I32 if f32 else torch.int16
            _same(got.view(it), exp.contiguous().view(it), what)


def test_im2col_nan_pixels_stay_nan():
    geom, B = kr.IM2COL_GEOMS[0], 2
    C, Tf, Hf, Wf, tub, p = geom
    N = kr.im2col_tokens(geom)
    g = torch.Generator().manual_seed(4)
    clip = torch.randn(B, C, Tf, Hf, Wf, generator=g)
    clip[torch.rand(clip.shape, generator=g) < 0.01] = float("nan")
    clip_dev = _in_vec(clip.reshape(-1))
    for f32 in (False, True):
        got = _im2col_launch(clip_dev, None, B * N, N, B, geom, f32, "im2col NaN")
        exp = kr.im2col_ref(clip if f32 else clip.bfloat16(), None, N, tub, p)
        assert bool(exp.isnan().any()) and bool(kr.same_bits_or_nan(got, exp).all())


# ------------------------------------------------------------------------------------------------
# vj_pred_index
PRED_FAMILIES = [(3, 1, 1, 5), (4, 100, 155, 400), (4, 100, 156, 400), (4, 100, 157, 400), (4, 513, 966, 2048),
                 (2, 8192, 8192, 16384)]  # (B, K, Kp, N); the last: n = 16384, sorted rows only


def _pred_masks(B, K, Kp, N, ordering, g):
    rows = lambda k, lo, hi: torch.stack([lo + torch.randperm(hi - lo, generator=g)[:k].sort().values  # noqa: E731
                                          for _ in range(B)])
    if ordering == "straddle":  # mx below my in every row, the last id of mx equal to the first of my
        mx, my = rows(K, 0, N // 2), rows(Kp, N // 2, N)
        my[:, 0] = mx[:, K - 1]
        return mx, my
    mx, my = rows(K, 0, N), rows(Kp, 0, N)  # drawn independently: ids shared by mx and my
    if ordering == "unsorted_mx":
        mx[1 % B] = mx[1 % B].flip(0)
    elif ordering == "unsorted_my":
        my[2 % B] = my[2 % B].flip(0)
    elif ordering == "repeat_unsorted":
        mx[0] = mx[0].flip(0)
        if K > 1:
            mx[0, 1] = mx[0, 0]
            mx[B - 1, K - 1] = mx[B - 1, 0]
    return mx, my


@pytest.mark.parametrize("fam", PRED_FAMILIES, ids=lambda f: "-".join(map(str, f)))
def test_pred_index_matches_stable_argsort(fam):
    B, K, Kp, N = fam
    n = K + Kp
    big = n == 16384
    g = torch.Generator().manual_seed(n)
    for ordering in ("sorted", "straddle") + (() if big else ("unsorted_mx", "unsorted_my", "repeat_unsorted")):
        mx, my = _pred_masks(B, K, Kp, N, ordering, g)
        mxd, myd = _in_ints(mx, -(1 << 40)), _in_ints(my, -(1 << 40))
        for bmod in sorted({0, B, max(1, B // 2), 1}):
            for with_loss in (True, False):
                for row0 in (0, 17):
                    what = f"pred_index {fam} {ordering} bmod={bmod} loss_rows={with_loss} row0={row0}"
                    ref = kr.pred_index_ref(mx, my, row0, bmod, N)
                    out = dict(pos=_IntOut(row0 + B * n, I32), ctx_dst=_IntOut(B * K, I32), tgt_rows=_IntOut(B * Kp, I32),
                               loss_rows=_IntOut(B * Kp, I32))
                    _call("vj_pred_index", B, K, Kp, mxd.data_ptr(), myd.data_ptr(), row0, bmod, N, out["pos"].ptr,
                          out["ctx_dst"].ptr, out["tgt_rows"].ptr, out["loss_rows"].ptr if with_loss else None, _st())
                    torch.cuda.synchronize()
                    got = {k: o.read(f"{what} {k}") for k, o in out.items()}
                    assert bool((got["pos"][:row0] == INT_SENT[I32]).all()), f"{what}: pos[:row0] was written"
                    _same(got["pos"][row0:], ref["pos"][row0:], f"{what} pos")
                    _same(got["ctx_dst"], ref["ctx_dst"], f"{what} ctx_dst")
                    _same(got["tgt_rows"], ref["tgt_rows"], f"{what} tgt_rows")
                    if with_loss:
                        _same(got["loss_rows"], ref["loss_rows"], f"{what} loss_rows")
                    else:
                        assert bool((got["loss_rows"] == INT_SENT[I32]).all())


# ------------------------------------------------------------------------------------------------
# masks
MASK_GRIDS = [(2, 3, 5), (3, 7, 11), (4, 8, 8), (1, 1, 257), (8, 16, 16)]


def _mask_boxes(grid, size, npred, g):
    """int32 [3, npred, 3] (start, top, left): sample 0 identical boxes at the origin; sample 1 the far corner
    and boxes overlapping it; sample 2 random positions."""
    hi = [grid[i] - size[i] for i in range(3)]
    far = torch.tensor(hi)
    s1 = torch.stack([(far - j).clamp(min=0) for j in range(npred)])
    s2 = torch.stack([torch.tensor([int(torch.randint(0, h + 1, (1,), generator=g)) for h in hi]) for _ in range(npred)])
    return torch.stack([torch.zeros(npred, 3, dtype=torch.int64), s1, s2]).to(I32)


@pytest.mark.parametrize("grid", MASK_GRIDS, ids=lambda g: "x".join(map(str, g)))
def test_mask_count_emit_forced_boxes(grid):
    D, H, W = grid
    N, B = D * H * W, 3
    g = torch.Generator().manual_seed(N)
    distinct = 0
    for size in [(1, 1, 1), (D, max(1, H // 2), max(1, W // 5)), (max(1, D // 2), max(1, H // 3), max(1, W // 4))]:
        for npred in (1, 2, 4):
            boxes = _mask_boxes(grid, size, npred, g)
            bdev = _in_ints(boxes, 1 << 20)
            for max_ctx in sorted({D, max(1, D - 1), 1}):
                what = f"masks grid={grid} size={size} npred={npred} max_ctx={max_ctx}"
                counts, _, _ = kr.masks_ref(grid, size, boxes, max_ctx, 0)
                assert int(counts.min()) >= 1
                distinct += len(set(counts.tolist())) == B
                oc = _IntOut(B, I32)
                _call("vj_mask_count", B, D, H, W, npred, bdev.data_ptr(), *size, max_ctx, oc.ptr, _st())
                torch.cuda.synchronize()
                _same(oc.read(what + " counts").long(), counts, what + " counts")
                k_min, k_pred = int(counts.min()), int(N - counts.max())
                for mode in (0, 1, 2):
                    for k_enc in sorted({k_min, min(k_min, 1)}):
                        w2 = f"{what} mode={mode} k_enc={k_enc} k_pred={k_pred}"
                        _, enc, pred = kr.masks_ref(grid, size, boxes, max_ctx, mode, k_enc, k_pred)
                        assert enc.shape[1] == (N - k_pred if mode == 2 else k_enc)
                        assert pred.shape[1] == (N - k_enc if mode == 1 else k_pred)
                        oe, op = _IntOut(enc.numel(), I64), _IntOut(pred.numel(), I64)
                        _call("vj_mask_emit", B, D, H, W, npred, bdev.data_ptr(), *size, max_ctx, mode, k_enc, k_pred,
                              oe.ptr, op.ptr, _st())
                        torch.cuda.synchronize()
                        _same(oe.read(w2 + " enc"), enc.reshape(-1), w2 + " enc")
                        _same(op.read(w2 + " pred"), pred.reshape(-1), w2 + " pred")
    assert distinct > 0, "no draw gave the three samples different counts"


MASK_CFG = dict(aspect_ratio=[0.75, 1.5], num_blocks=2, spatial_scale=[0.4, 0.7], temporal_scale=[0.5, 1.0])
MASK_OPTIONS = [dict(full_complement=True), dict(full_complement=True, max_temporal_keep=0.5),
                dict(pred_full_complement=True), dict(pred_full_complement=True, max_temporal_keep=0.5),
                dict(pred_full_complement=True, max_keep=3), dict(pred_full_complement=True, max_temporal_keep=0.5, max_keep=3)]


@pytest.mark.parametrize("crop,fpc", [(32, 2), (32, 4), (48, 2), (48, 4)])
@pytest.mark.parametrize("opt", MASK_OPTIONS, ids=lambda o: "-".join(o))
def test_small_grid_collators_host_vs_device(crop, fpc, opt):
    """2x2 and 3x3 token grids, one and two frames deep (N = 4 .. 18): the device build against the host collate
    on the same draws, five collates each, consuming the same RNG stream."""
    from vjepa2_amd.masks import MaskCollator, materialize

    cfgs = [dict(MASK_CFG, **opt)]
    host = MaskCollator(cfgs, [fpc], crop_size=crop, patch_size=16, tubelet_size=2)
    dev = MaskCollator(cfgs, [fpc], crop_size=crop, patch_size=16, tubelet_size=2, device_masks=True)
    batch = [(torch.zeros(1), 0, [torch.arange(fpc)]) for _ in range(3)]
    for i in range(5):
        torch.manual_seed(500 + i)
        (_, he, hp), = host(batch)
        after_host = torch.rand(1)
        torch.manual_seed(500 + i)
        entry, = dev(batch)
        _, de, dp = materialize(entry, DEV)
        assert torch.equal(torch.rand(1), after_host), "the draws consumed a different RNG stream"
        for a, b in zip(he + hp, de + dp):
            assert b.is_cuda and b.dtype == I64 and torch.equal(a, b.cpu()), (crop, fpc, opt, i)


# ------------------------------------------------------------------------------------------------
# video transform
def _video_launch(frames, params, S, mean, stdv, what):
    B, T, H, W, C = frames.shape
    total = B * C * T * S * S
    fo = _ovec(total)
    # every operand stays referenced until the kernel has run: a freed block would be handed to the next one
    fr, pr, mv, sv = _in_ints(frames, 0xA5), _in_ints(params, 0), _in_vec(mean), _in_vec(stdv)
    _call("vj_video_transform", B, T, H, W, C, S, fr.data_ptr(), pr.data_ptr(), mv.data_ptr(), sv.data_ptr(),
          fo.win.data_ptr(), _st())
    torch.cuda.synchronize()
    del fr, pr, mv, sv
    return fo.read(what).view(F32).reshape(B, C, T, S, S)


@pytest.mark.parametrize("name", list(kr.VIDEO_CASES))
def test_video_transform_vs_float64(name):
    frames, params, S, mean, stdv = kr.video_inputs(name)
    B, T, H, W, C = frames.shape
    got = _video_launch(frames, params, S, mean, stdv, f"video {name}")
    ref, bound = kr.video_ref64(frames, params, S, mean, stdv)
    ratio = (got.double() - ref).abs() / bound
    print(f"video {name}: largest error / bound {float(ratio.max()):.4f}")
    assert bool((ratio <= 1.0).all()), (name, float(ratio.max()), [int(v) for v in (ratio > 1.0).nonzero()[0]])
    # every byte outside the crop boxes re-randomised: nothing outside a box is read
    other = torch.randint(0, 256, frames.shape, generator=torch.Generator().manual_seed(99), dtype=torch.uint8)
    for b in range(B):
        ci, cj, ch, cw, flip = (int(v) for v in params[b])
        other[b, :, ci:ci + ch, cj:cj + cw] = frames[b, :, ci:ci + ch, cj:cj + cw]
        if (ch, cw) == (S, S):  # an identity resize: exact
            crop = frames[b, :, ci:ci + ch, cj:cj + cw].float().permute(3, 0, 1, 2)
            crop = crop.flip(-1) if flip else crop
            ident = (crop - mean[:, None, None, None]) / stdv[:, None, None, None]
            _same(got[b].view(I32), ident.contiguous().view(I32), f"video {name} identity resize of sample {b}")
    again = _video_launch(other, params, S, mean, stdv, f"video {name} re-randomised")
    _same(again.view(I32), got.view(I32), f"video {name}: bytes outside the crop boxes changed the output")
