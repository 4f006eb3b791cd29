"""CPU: host logic of the multilevel eval encoder wrapper (vjepa2_amd/multiclip.py
ClipAggregationMultilevel, ops.layernorm_taps, video_classification_frozen.init_module): the destination
map against the reference's op sequence emulated in torch, the reference's pos-index rule and temporal
table against tests/golden/multilevel.pt, the module-name dispatch and the wrapper's host refusals."""

import os

import pytest
import torch
import torch.nn as nn

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _gold():
    return torch.load(os.path.join(GOLD, "multilevel.pt"), weights_only=True)


def _reference_sequence(levels, clips, V, B, T):
    """vit_encoder_multiclip_multilevel.py:123-141 on a list over levels of [clips*V*B, n, D] (n = T
    temporal indices x some spatial tokens), then ProbeTrainer's cat over views: [V*B, clips*L*n, D]."""
    o = torch.cat(levels, dim=1)
    _, LN, D = o.shape
    S = LN // T
    eff_B = B * V
    views = []
    for j in range(V):
        per_clip = [o[i * eff_B:(i + 1) * eff_B][j * B:(j + 1) * B].reshape(B, T, S, D) for i in range(clips)]
        views.append(torch.cat(per_clip, dim=1).flatten(1, 2))
    return torch.cat(views, dim=0)


@pytest.mark.parametrize("clips,V,B,L,n", [(1, 1, 1, 1, 1), (2, 2, 2, 2, 8), (4, 3, 2, 4, 5)])
def test_destination_map_matches_reference_sequence(clips, V, B, L, n):
    """Every (level, encoder row, token) carries its own id through the reference's cat / slice / reshape /
    cat; the map must send block (l, g) to the rows where those ids end up."""
    from vjepa2_amd.multiclip import multilevel_dst_blocks

    G = clips * V * B
    levels = [(torch.arange(G * n, dtype=torch.float64) + l * G * n).reshape(G, n, 1) for l in range(L)]
    T = {1: 1, 8: 4, 5: 5}[n]  # temporal indices per clip (n = T x spatial tokens)
    want = _reference_sequence(levels, clips, V, B, T).reshape(-1)  # [V*B * clips*L*n]
    dst = multilevel_dst_blocks(clips, V, B, L)
    assert len(dst) == L and all(len(d) == G for d in dst)
    flat = [b for d in dst for b in d]
    assert sorted(flat) == list(range(G * L))  # a bijection onto the buffer's blocks
    got = torch.full((G * L * n,), -1.0, dtype=torch.float64)
    for l in range(L):
        for g in range(G):
            got[dst[l][g] * n:dst[l][g] * n + n] = levels[l][g, :, 0]
    assert torch.equal(got, want)


@pytest.mark.parametrize("case", ["taps_0_2", "taps_1"])
def test_pos_index_rule_matches_reference(case):
    """The reference takes S = (L*N) // T from the concatenated token count, so with two levels ALL of a
    clip's level-0 rows (both temporal indices) take the clip's first frame index and all level-1 rows its
    second: what the reference added (outs - outs_nopos of the fixture) is pos_embed at multilevel_pos_rows."""
    from vjepa2_amd.multiclip import multilevel_pos_rows

    g = _gold()
    c = g["cases"][case]
    cfg = g["cfg"]
    L = len(c["out_layers"])
    T = cfg["num_frames"] // cfg["tubelet_size"]
    N = T * (cfg["img_size"] // cfg["patch_size"]) ** 2
    rows = multilevel_pos_rows(g["clip_indices"], cfg["tubelet_size"], L, N, T)  # [B, clips*L*N]
    assert rows.shape == (2, 2 * L * N)
    want = g["pos_embed"][0][rows]  # [B, clips*L*N, D]
    for o, o0 in zip(c["outs"], c["outs_nopos"]):
        added = o.double() - o0.double()
        # o = fl(o0 + p): |added - p| <= half an ulp of |o| (|o| < 16 here: 2^-21 ~ 4.8e-7 at most ... 1e-5 is 20x)
        assert float(o.abs().max()) < 16
        assert (added - want.double()).abs().max() < 1e-5
    if L == 2:  # the rule mixes levels: the per-level S = N // T would give another table row somewhere
        naive = torch.stack([ci[:, ::cfg["tubelet_size"]] for ci in g["clip_indices"]], 1)  # [B, clips, T]
        naive = naive.reshape(2, 2, 1, T, 1).expand(2, 2, L, T, N // T).reshape(2, -1)
        assert not torch.equal(naive, rows)


def _micro(**kw):
    from vjepa2_amd import vision_transformer as vit

    return vit.VisionTransformer(embed_dim=64, depth=3, num_heads=1, mlp_ratio=4, qkv_bias=True,
                                 norm_layer=lambda dim: nn.LayerNorm(dim, eps=1e-6), **kw)


def test_temporal_table_bit_for_bit_and_attributes():
    from vjepa2_amd.multiclip import ClipAggregationMultilevel

    g = _gold()
    enc = _micro(img_size=32, num_frames=4, patch_size=16, tubelet_size=2, use_rope=True, uniform_power=True,
                 out_layers=[0, 2])
    agg = ClipAggregationMultilevel(enc, tubelet_size=2, max_frames=16, use_pos_embed=True, out_layers=[0, 2])
    assert torch.equal(agg.pos_embed, g["pos_embed"]) and not agg.pos_embed.requires_grad
    assert agg.embed_dim == 64 and agg.num_heads == 1
    assert ClipAggregationMultilevel(enc).pos_embed is None
    assert enc.tap_layers() == [0, 2]
    with pytest.raises(ValueError, match="out_layers"):
        ClipAggregationMultilevel(_micro(img_size=32, num_frames=4, use_rope=True))


def test_init_module_dispatch(tmp_path, monkeypatch):
    """The multilevel module name builds the encoder with wrapper_kwargs' out_layers inside
    ClipAggregationMultilevel; the single-level name still gives ClipAggregation; any other is refused."""
    from vjepa2_amd import multiclip
    from vjepa2_amd import vision_transformer as vit
    from vjepa2_amd.evals import video_classification_frozen as app

    monkeypatch.setattr(vit, "vit_micro", lambda patch_size=16, **kw: _micro(patch_size=patch_size, **kw),
                        raising=False)
    enc_kw = dict(model_name="vit_micro", checkpoint_key="target_encoder", tubelet_size=2, use_rope=True,
                  uniform_power=True)
    torch.manual_seed(0)
    src = _micro(img_size=32, num_frames=4, use_rope=True, uniform_power=True)
    ckpt = tmp_path / "pretrained.pt"
    torch.save({"target_encoder": {"module.backbone." + k: v for k, v in src.state_dict().items()}}, ckpt)
    kw = dict(frames_per_clip=4, resolution=32, checkpoint=str(ckpt), model_kwargs=dict(encoder=enc_kw), device="cpu")
    m = app.init_module(module_name=app.MULTILEVEL_MODULE,
                        wrapper_kwargs=dict(max_frames=16, use_pos_embed=False, out_layers=[1, 2]), **kw)
    assert isinstance(m, multiclip.ClipAggregationMultilevel) and not m.training
    assert m.model.out_layers == [1, 2] and m.model.tap_layers() == [1, 2] and m.pos_embed is None
    assert not any(p.requires_grad for p in m.parameters())
    assert torch.equal(m.model.blocks[2].mlp.fc1.weight, src.blocks[2].mlp.fc1.weight)
    assert hasattr(m, "forward_stacked")
    s = app.init_module(module_name=app.MULTICLIP_MODULE, wrapper_kwargs=dict(max_frames=16), **kw)
    assert type(s) is multiclip.ClipAggregation and s.model.out_layers is None and not hasattr(s, "forward_stacked")
    with pytest.raises(NotImplementedError, match="are ported"):
        app.init_module(module_name="evals.video_classification_frozen.modelcustom.something_else",
                        wrapper_kwargs={}, **kw)


def test_layernorm_taps_host_refusals():
    """ops.layernorm_taps checks dtypes, shapes and the destination map on the host, before any upload;
    then it needs device tensors (no CPU path)."""
    from vjepa2_amd import ops

    D, n, G = 8, 3, 2
    x, w, b = torch.zeros(G * n, D), torch.ones(D), torch.zeros(D)
    out = torch.zeros(4 * n + 1, D)  # 4 whole blocks
    with pytest.raises(IndexError, match="dst_block value 4 out of range for 4 blocks"):
        ops.layernorm_taps(x, w, b, 1e-6, out, n, [0, 4])
    with pytest.raises(IndexError, match="dst_block value -1 out of range"):
        ops.layernorm_taps(x, w, b, 1e-6, out, n, [-1, 2])
    with pytest.raises(ValueError, match="repeats a destination block"):
        ops.layernorm_taps(x, w, b, 1e-6, out, n, [3, 3])
    with pytest.raises(ValueError, match="1 destination blocks for 2 groups"):
        ops.layernorm_taps(x, w, b, 1e-6, out, n, [1])
    with pytest.raises(ValueError, match="not whole groups"):
        ops.layernorm_taps(x, w, b, 1e-6, out, 4, [0])
    with pytest.raises(TypeError, match="x must be f32 or bf16"):
        ops.layernorm_taps(x.half(), w, b, 1e-6, out, n, [0, 1])
    with pytest.raises(TypeError, match="out must be f32"):
        ops.layernorm_taps(x, w, b, 1e-6, out.bfloat16(), n, [0, 1])
    with pytest.raises(TypeError, match="weight and bias must be f32"):
        ops.layernorm_taps(x, w.bfloat16(), b, 1e-6, out, n, [0, 1])
    with pytest.raises(TypeError, match="host sequence of ints"):
        ops.layernorm_taps(x, w, b, 1e-6, out, n, torch.tensor([0.0, 1.0]))
    with pytest.raises(ValueError, match="x is 8 wide, out 12"):
        ops.layernorm_taps(x, w, b, 1e-6, torch.zeros(12, 12), n, [0, 1])
    with pytest.raises(ValueError, match="row-major"):
        ops.layernorm_taps(x.t().contiguous().t(), w, b, 1e-6, out, n, [0, 1])
    with pytest.raises(RuntimeError, match="no CPU path"):  # a valid call but for the device
        ops.layernorm_taps(x, w, b, 1e-6, out, n, torch.tensor([2, 0]))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.tap_blocks([1, 0], 2, "cpu")
