"""CPU: the references and bounds of tests/kernel_refs.py hold on their own, on the inputs the GPU tests use
(tests/test_gpu_tokenpath.py, tests/test_gpu_variants.py).

  * an f32 numpy restatement of k_swiglu_fwd / k_swiglu_bwd and of k_video_transform (source index rounded twice,
    multiply then subtract, and once, as a fused multiply-add) lies inside the stated bound of its float64
    reference: a correct kernel passes the GPU check;
  * a tap shifted by one pixel, a dropped x2 offset and a threshold taken from a double p break the same checks:
    the checks can fail;
  * masks_ref equals the host MaskCollator for the same draws (small grids, every complement mode,
    max_temporal_keep, max_keep) and the lists the reference generated (tests/golden/masks.pt);
  * im2col_ref and pred_index_ref agree with independent formulations (unfold; a counting rank);
  * drop_thresh takes the f32 value of p, as the library does.
"""

import numpy as np
import pytest
import torch

import kernel_refs as kr
from test_dropout import drop_thresh, vj_dropout_mask_ref
from test_host_logic import VITL, gold


# ------------------------------------------------------------------------------------------------
def _swiglu_ratios(x12, dh, what):
    ref = kr.swiglu_ref64(x12, dh)
    out, d1, d2 = kr.swiglu_restate_f32(x12, dh)
    return (kr.check_swiglu(out, ref["v"], ref["bound"], ref["m"], f"{what} fwd"),
            kr.check_swiglu(d1, ref["v1"], ref["bound1"], ref["m1"], f"{what} dx1"),
            kr.check_swiglu(d2, ref["v2"], ref["bound2"], ref["m2"], f"{what} dx2"))


@pytest.mark.parametrize("shape", kr.SWIGLU_SMALL + [kr.SWIGLU_LARGE])
def test_swiglu_restatement_within_bound(shape):
    """Every edge value of SWIGLU_EDGES sits in row 0; of the large shape the first 1024 rows (2.1M elements)."""
    x12, dh = kr.swiglu_inputs(*shape)
    r = _swiglu_ratios(x12[:1024], dh[:1024], f"swiglu {shape}")
    assert max(r) <= 1.0, r


def test_swiglu_checks_can_fail():
    x12, dh = kr.swiglu_inputs(37, 344)
    ref = kr.swiglu_ref64(x12, dh)
    out, d1, d2 = kr.swiglu_restate_f32(x12, dh)
    with pytest.raises(AssertionError):  # x2 read one column to the left (a dropped or wrong h offset)
        wrong, _, _ = kr.swiglu_restate_f32(torch.cat([x12[:, :344], x12[:, 343:-1]], 1), dh)
        kr.check_swiglu(wrong, ref["v"], ref["bound"], ref["m"], "shifted x2")
    with pytest.raises(AssertionError):  # one bf16 ulp off everywhere
        kr.check_swiglu((d2.float() * (1 + 2.0 ** -7)).bfloat16(), ref["v2"], ref["bound2"], ref["m2"], "scaled dx2")
    with pytest.raises(AssertionError):  # dx1 and dx2 swapped
        kr.check_swiglu(d2, ref["v1"], ref["bound1"], ref["m1"], "swapped halves")


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(kr.VIDEO_CASES))
def test_video_restatement_within_bound(name):
    inp = kr.video_inputs(name)
    ref, bound = kr.video_ref64(*inp)
    for fused in (False, True):
        got = kr.video_restate_f32(*inp, fused=fused).double()
        ratio = float(((got - ref).abs() / bound).max())
        assert ratio <= 1.0, (name, fused, ratio)
    assert float(bound.max()) <= 2.3e-3


def test_video_identity_resize_is_exact():
    frames, params, S, mean, stdv = kr.video_inputs("b-C3-S16-flip0")
    assert tuple(params[1][:4].tolist()) == (4, 7, 16, 16) and S == 16
    got = kr.video_restate_f32(frames, params, S, mean, stdv, fused=True)[1]
    crop = frames[1, :, 4:20, 7:23].float().permute(3, 0, 1, 2)
    if params[1][4]:
        crop = crop.flip(-1)
    assert torch.equal(got, (crop - mean[:, None, None, None]) / stdv[:, None, None, None])


def test_video_check_can_fail():
    """The clamp ch for ch - 1 (a tap one row below the crop) and a crop origin off by one column both exceed
    the bound by orders of magnitude."""
    frames, params, S, mean, stdv = kr.video_inputs("a-C3-S17-flip0")
    ref, bound = kr.video_ref64(frames, params, S, mean, stdv)
    shifted = params.clone()
    shifted[0, 1] += 1  # the whole-frame box read one column to the right (39 columns stay in range)
    shifted[0, 3] -= 1
    got = kr.video_restate_f32(frames, shifted, S, mean, stdv, fused=True).double()
    assert float(((got - ref).abs() / bound)[0].max()) > 50.0


# ------------------------------------------------------------------------------------------------
MASK_CFG = dict(aspect_ratio=[0.75, 1.5], num_blocks=2, spatial_scale=[0.4, 0.7], temporal_scale=[0.5, 1.0])
MASK_OPTIONS = [dict(), dict(max_temporal_keep=0.5), dict(full_complement=True),
                dict(full_complement=True, max_temporal_keep=0.5), dict(pred_full_complement=True),
                dict(pred_full_complement=True, max_temporal_keep=0.5, max_keep=3), dict(max_keep=2, num_blocks=4)]


def _sample(fpc):
    return (torch.zeros(1), 0, [torch.arange(fpc)])


def _spec_lists(spec):
    """masks_ref on a MaskSpec's draws, with MaskSpec.build's lengths (batch minima, max_keep)."""
    counts, _, _ = kr.masks_ref(spec.grid, spec.size, spec.boxes, spec.max_ctx, 0)
    N = spec.grid[0] * spec.grid[1] * spec.grid[2]
    k_enc, k_pred = int(counts.min()), int(N - counts.max())
    if spec.max_keep is not None:
        k_enc = min(k_enc, int(spec.max_keep))
    _, e, p = kr.masks_ref(spec.grid, spec.size, spec.boxes, spec.max_ctx, spec.mode, k_enc, k_pred)
    return (p, e) if spec.inv_block else (e, p)


@pytest.mark.parametrize("crop,fpc", [(32, 2), (32, 4), (48, 4), (64, 8), (112, 16)])
@pytest.mark.parametrize("opt", MASK_OPTIONS, ids=lambda o: "-".join(o) or "plain")
def test_masks_ref_matches_host_collate(crop, fpc, opt):
    from vjepa2_amd.masks import MaskCollator

    cfgs = [dict(MASK_CFG, **opt)]
    host = MaskCollator(cfgs, [fpc], crop_size=crop, patch_size=16, tubelet_size=2)
    draw = MaskCollator(cfgs, [fpc], crop_size=crop, patch_size=16, tubelet_size=2, device_masks=True)
    for i in range(5):
        torch.manual_seed(77 + i)
        (_, he, hp), = host([_sample(fpc) for _ in range(3)])
        torch.manual_seed(77 + i)
        (_, specs, none), = draw([_sample(fpc) for _ in range(3)])
        assert none is None
        e, p = _spec_lists(specs[0])
        assert torch.equal(e, he[0]) and torch.equal(p, hp[0]), (crop, fpc, opt, i)


@pytest.mark.parametrize("tag", ["vitl", "small"])
def test_masks_ref_matches_golden(tag):
    from vjepa2_amd.masks import MaskCollator

    g = gold("masks.pt")[tag]
    torch.manual_seed(239)
    mc = MaskCollator(VITL, [g["fpc"]], crop_size=g["crop"], patch_size=16, tubelet_size=2, device_masks=True)
    for it in g["iters"]:
        (_, specs, _), = mc([_sample(g["fpc"]) for _ in range(g["B"])])
        built = [_spec_lists(s) for s in specs]
        for a, b in zip([e for e, _ in built] + [p for _, p in built], it["enc"] + it["pred"]):
            assert a.dtype == torch.int64 and torch.equal(a, b)


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", kr.IM2COL_GEOMS)
def test_im2col_ref_matches_unfold(geom):
    C, Tf, Hf, Wf, tub, p = geom
    clip = torch.randn(2, C, Tf, Hf, Wf, generator=torch.Generator().manual_seed(Hf))
    N = kr.im2col_tokens(geom)
    u = clip.unfold(2, tub, tub).unfold(3, p, p).unfold(4, p, p)  # [B, C, T', H', W', tub, p, p]
    full = u.permute(0, 2, 3, 4, 1, 5, 6, 7).reshape(2 * N, -1)
    assert torch.equal(kr.im2col_ref(clip, None, N, tub, p), full)
    idx = torch.randint(0, N, (2, 5), generator=torch.Generator().manual_seed(1))
    rows = (torch.arange(2)[:, None] * N + idx).reshape(-1)
    assert torch.equal(kr.im2col_ref(clip, idx.reshape(-1), 5, tub, p), full[rows])
    assert torch.equal(kr.im2col_ref(clip, idx.reshape(-1), 5, tub, p, R=7), full[rows[:7]])


def test_pred_index_ref_matches_counting_rank():
    g = torch.Generator().manual_seed(9)
    B, K, Kp, N, row0 = 4, 7, 5, 40, 17
    mx, my = torch.randint(0, N, (B, K), generator=g), torch.randint(0, N, (B, Kp), generator=g)
    mx[1, 3] = mx[1, 0]
    my[2, 0] = mx[2, K - 1]
    for bmod in (0, 4, 2, 1):
        ref = kr.pred_index_ref(mx, my, row0, bmod, N)
        assert bool((ref["pos"][:row0] == -1).all())
        for b in range(B):
            ids = torch.cat([mx[b], my[b]]).tolist()
            n = K + Kp
            for i, v in enumerate(ids):
                rank = sum((w < v) or (w == v and j < i) for j, w in enumerate(ids))
                dst = row0 + b * n + rank
                assert int(ref["pos"][dst]) == v
                if i < K:
                    assert int(ref["ctx_dst"][b * K + i]) == dst
                else:
                    assert int(ref["tgt_rows"][b * Kp + i - K]) == dst
                    assert int(ref["loss_rows"][b * Kp + i - K]) == (b % (bmod or B)) * N + v


def test_pred_index_rejects_bad_arguments_before_any_launch():
    """Null operands, negative sizes and n > 16384 return an error with a message (validation precedes any device
    work, so this needs no GPU); loss_rows may be null."""
    from vjepa2_amd import _lib

    lib = _lib.load()
    p = 4096  # never dereferenced: every call below is rejected on the host
    for args, msg in [((2, 4, 4, None, p, 0, 0, 8, p, p, p, p), "null argument"),
                      ((2, 4, 4, p, None, 0, 0, 8, p, p, p, p), "null argument"),
                      ((2, 4, 4, p, p, 0, 0, 8, None, p, p, None), "null argument"),
                      ((2, 4, 4, p, p, 0, 0, 8, p, None, p, None), "null argument"),
                      ((2, 4, 4, p, p, 0, 0, 8, p, p, None, None), "null argument"),
                      ((-1, 4, 4, p, p, 0, 0, 8, p, p, p, p), "size out of range"),
                      ((2, -4, 4, p, p, 0, 0, 8, p, p, p, p), "size out of range"),
                      ((2, 4, 4, p, p, -1, 0, 8, p, p, p, p), "size out of range"),
                      ((2, 4, 4, p, p, 0, -2, 8, p, p, p, p), "size out of range"),
                      ((2, 2 ** 31 - 1, 2, p, p, 0, 0, 8, p, p, p, p), "size out of range"),
                      ((2, 8192, 8193, p, p, 0, 0, 8, p, p, p, p), "sequence length 16385 out of range"),
                      ((2, 0, 0, p, p, 0, 0, 8, p, p, p, p), "sequence length 0 out of range")]:
        rc = lib.vj_pred_index(*args, None)
        assert rc != 0 and msg in _lib.last_error(), (args, rc, _lib.last_error())


# ------------------------------------------------------------------------------------------------
def test_drop_thresh_rounds_the_f32_value_of_p():
    """vj_dropout receives p as a float: 0.3f = 0.300000011920929, whose threshold lies 51 above the double's."""
    assert drop_thresh(0.3) == int(float(np.float32(0.3)) * 4294967296.0 + 0.5)
    assert drop_thresh(0.3) - int(0.3 * 4294967296.0 + 0.5) == 51
    assert drop_thresh(0.5) == 1 << 31 and drop_thresh(0.0) == 0
    keep = kr.dropout_keep(5, 4, 8, 0.3)
    assert torch.equal(keep, torch.from_numpy(vj_dropout_mask_ref(5, np.arange(4), np.arange(8), 0.3)))


@pytest.mark.parametrize("p,seed,at", kr.DROPOUT_GAP_CASES)
def test_dropout_gap_cases_separate_the_two_thresholds(p, seed, at):
    """At these seeds exactly the named element of a [300, 520] mask depends on whether p is rounded to f32
    before the threshold is taken: the GPU test on them fails for a library (or a reference) that uses the double."""
    u_ge = lambda t: vj_dropout_mask_ref_at(seed, 300, 520, t)  # noqa: E731
    t32 = drop_thresh(p)
    t64 = int(p * 4294967296.0 + 0.5)
    assert t32 - t64 in (51, 55)
    diff = np.argwhere(u_ge(t64) != u_ge(t32))
    assert diff.tolist() == [list(at)]
    assert not bool(kr.dropout_keep(seed, 300, 520, p)[at])


def vj_dropout_mask_ref_at(seed, rows, cols, thresh):
    """The keep mask for an explicit integer threshold (the hash of test_dropout.py)."""
    from test_dropout import M32, _mix

    r = np.arange(rows, dtype=np.uint64)[:, None]
    c = np.arange(cols, dtype=np.uint64)[None, :]
    return _mix((_mix(np.uint64(seed) ^ ((r * 0x9E3779B1) & M32)) + c * 0x85EBCA77) & M32) >= thresh


def test_rowscale_and_dropout_refs_follow_the_documented_roundings():
    g = torch.Generator().manual_seed(2)
    y, r = torch.randn(5, 8, generator=g), torch.randn(5, 8, generator=g)
    s = torch.tensor([0.0, 1 / 0.9, 1 / 0.9, 0.0, 1 / 0.9]).bfloat16().float()
    b = (y.bfloat16().double() * s.double()[:, None]).float().bfloat16()
    assert torch.equal(kr.rowscale_ref(y, s), b)
    assert torch.equal(kr.rowscale_ref(y, s, r), r + b.float())
    assert torch.equal(kr.rowscale_ref(y, s, r.bfloat16()), (r.bfloat16().float() + b.float()).bfloat16())
    assert torch.equal(kr.dropout_ref(y, 0.0, 7), y.bfloat16())
    out = kr.dropout_ref(y, 0.5, 7)
    keep = kr.dropout_keep(7, 5, 8, 0.5)
    assert torch.equal(out, torch.where(keep, (y.bfloat16().float() * 2).bfloat16(), torch.zeros(()).bfloat16() * y.bfloat16()))
