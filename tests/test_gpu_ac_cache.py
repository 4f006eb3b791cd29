"""GPU: VisionTransformerPredictorAC.forward_cached (frame-by-frame forward over a per-block K/V cache) against
the reference's recorded outputs (tests/golden/ac_predictor.pt: B 2, 3 frames of 4 tokens, head dim 32) and
against the full HIP forward().

Two bounds, neither measured on the cached path: rel_l1(cached, reference) < 1e-2, the bound
test_ac_predictor_matches_reference holds forward() to; and rel_l1(cached, forward()) <= D0 = rel_l1(forward(),
reference) on the `causal` fixture: the cache may add no more error than forward() itself has. Configurations
without a usable recording (the edited sequence of the rewind test, `causal_silu_dp` in eval(), whose recording
was made with drop_path draws, and the width-1024 model) are held to the second bound with the same D0."""

import functools
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda"
HW = 4  # tokens per frame of the fixtures (32 px, 16 px patches)
CHUNKS = [(1, 1, 1), (2, 1), (1, 2), (3,)]


def rel_l1(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).abs().mean() / b.abs().mean().clamp_min(1e-12)).item()


@functools.lru_cache(maxsize=None)
def _gold():
    return torch.load(os.path.join(GOLD, "ac_predictor.pt"), weights_only=True)


def _model(which, **over):
    from vjepa2_amd.ac_predictor import vit_ac_predictor

    g = _gold()[which]
    m = vit_ac_predictor(**dict(g["cfg"], **over)).to(DEV)
    m.load_state_dict(g["state"])
    return m.eval()


def _inputs(which):
    g = _gold()[which]
    ins = [g[k].to(DEV) for k in ("x", "actions", "states")]
    return ins + [g["ext"].to(DEV) if g["cfg"]["use_extrinsics"] else None]


def _full(m, x, a, s, e):
    with torch.no_grad():
        return m(x, a, s, e)


def _cached(m, x, a, s, e, chunks, cache=None, hw=HW):
    """forward_cached over `chunks` frames at a time from cache.frames on; the outputs concatenated."""
    cache = cache if cache is not None else m.new_cache(x.shape[0], sum(chunks))
    outs, t = [], 0
    with torch.no_grad():
        for n in chunks:
            f0 = cache.frames
            outs.append(m.forward_cached(x[:, t * hw:(t + n) * hw], a[:, t:t + n], s[:, t:t + n],
                                         None if e is None else e[:, t:t + n], cache=cache))
            assert cache.frames == f0 + n and tuple(outs[-1].shape) == (x.shape[0], n * hw, x.shape[2])
            t += n
    return torch.cat(outs, 1)


@functools.lru_cache(maxsize=None)
def _d0():
    """rel_l1(forward(), reference) of the `causal` fixture: the full HIP forward's own distance."""
    y = _full(_model("causal"), *_inputs("causal"))
    return rel_l1(y, _gold()["causal"]["y"])


@pytest.mark.parametrize("chunks", CHUNKS, ids=lambda c: "-".join(map(str, c)))
@pytest.mark.parametrize("which", ["causal", "causal_ext"])
def test_chunked_forward_matches_reference_and_full_forward(which, chunks):
    m, ins = _model(which), _inputs(which)
    y_ref = _gold()[which]["y"]
    y_full = _full(m, *ins)
    y = _cached(m, *ins, chunks)
    assert y.dtype == torch.float32 and y.shape == y_full.shape
    d_ref, d_full, own = rel_l1(y, y_ref), rel_l1(y, y_full), rel_l1(y_full, y_ref)
    print(f"{which} {chunks}: cached vs reference {d_ref:.3e}, cached vs forward() {d_full:.3e}, forward() vs "
          f"reference {own:.3e}")
    assert d_ref < 1e-2, d_ref
    assert d_full <= own, (d_full, own)


def test_rewind_replaces_the_later_frames():
    """3 frames, rewind(1), two different frames: equals forward() on the edited 3-frame sequence; frame 0's
    keys and values are the ones the first pass left."""
    m = _model("causal")
    x, a, s, e = _inputs("causal")
    cache = m.new_cache(2, 3)
    _cached(m, x, a, s, e, (1, 1, 1), cache=cache)
    assert cache.frames == 3
    g = torch.Generator().manual_seed(11)
    x2, a2, s2 = x.clone(), a.clone(), s.clone()
    x2[:, HW:] = torch.randn(2, 2 * HW, x.shape[2], generator=g).to(DEV) * x.std()
    a2[:, 1:] = torch.randn(2, 2, 7, generator=g).to(DEV) * a.std()
    s2[:, 1:] = torch.randn(2, 2, 7, generator=g).to(DEV) * s.std()
    cache.rewind(1)
    assert cache.frames == 1
    with torch.no_grad():
        y1 = m.forward_cached(x2[:, HW:2 * HW], a2[:, 1:2], s2[:, 1:2], cache=cache)
        y2 = m.forward_cached(x2[:, 2 * HW:], a2[:, 2:], s2[:, 2:], cache=cache)
    assert cache.frames == 3
    want = _full(m, x2, a2, s2, None)
    got = torch.cat([y1, y2], 1)
    d = rel_l1(got, want[:, HW:])
    print(f"rewind: cached vs forward() on the edited sequence {d:.3e} (bound {_d0():.3e})")
    assert d <= _d0(), (d, _d0())
    assert rel_l1(want[:, HW:], _full(m, x, a, s, None)[:, HW:]) > 0.05  # the edit matters
    with pytest.raises(ValueError, match="holds 3 frames"):
        cache.rewind(4)
    with pytest.raises(ValueError):
        cache.rewind(-1)
    cache.reset()
    assert cache.frames == 0
    assert torch.equal(_cached(m, x, a, s, e, (3,), cache=cache), _cached(m, x, a, s, e, (3,)))


def test_two_caches_are_independent():
    """A second cache used in between changes nothing: both interleaved rollouts give the bits they give alone."""
    m = _model("causal")
    x, a, s, e = _inputs("causal")
    xb, ab_, sb = x.flip(0).contiguous() * 0.5, a.flip(0).contiguous(), s.flip(0).contiguous() + 0.1
    alone_a = _cached(m, x, a, s, e, (1, 1, 1))
    alone_b = _cached(m, xb, ab_, sb, None, (1, 1, 1))
    assert not torch.equal(alone_a, alone_b)
    ca, cb = m.new_cache(2, 3), m.new_cache(2, 3)
    ya, yb = [], []
    for t in range(3):
        ya.append(_cached(m, x[:, t * HW:(t + 1) * HW], a[:, t:t + 1], s[:, t:t + 1], None, (1,), cache=ca))
        yb.append(_cached(m, xb[:, t * HW:(t + 1) * HW], ab_[:, t:t + 1], sb[:, t:t + 1], None, (1,), cache=cb))
    assert torch.equal(torch.cat(ya, 1), alone_a)
    assert torch.equal(torch.cat(yb, 1), alone_b)


def test_swiglu_blocks_in_eval():
    """causal_silu_dp (SwiGLU MLPs, drop_path 0.5 on block 1) in eval(): cached against forward()."""
    m, ins = _model("causal_silu_dp"), _inputs("causal_silu_dp")
    y_full = _full(m, *ins)
    for chunks in ((1, 1, 1), (2, 1)):
        d = rel_l1(_cached(m, *ins, chunks), y_full)
        print(f"causal_silu_dp {chunks}: cached vs forward() {d:.3e} (bound {_d0():.3e})")
        assert d <= _d0(), (chunks, d, _d0())


def test_width_1024_head_dim_64():
    """Predictor width 1024, 16 heads (head dim 64: the DROID attention kernel), depth 2, B 3, 3 frames."""
    from vjepa2_amd.ac_predictor import vit_ac_predictor

    torch.manual_seed(17)
    m = vit_ac_predictor(img_size=32, patch_size=16, num_frames=6, tubelet_size=2, embed_dim=96,
                         predictor_embed_dim=1024, depth=2, num_heads=16, action_embed_dim=7).to(DEV).eval()
    g = torch.Generator().manual_seed(18)
    x = torch.randn(3, 3 * HW, 96, generator=g).to(DEV)
    a, s = torch.randn(3, 3, 7, generator=g).to(DEV), torch.randn(3, 3, 7, generator=g).to(DEV)
    y_full = _full(m, x, a, s, None)
    y = _cached(m, x, a, s, None, (1, 1, 1))
    d = rel_l1(y, y_full)
    print(f"width 1024: cached vs forward() {d:.3e} (bound {_d0():.3e})")
    assert torch.isfinite(y).all() and d <= _d0(), (d, _d0())


def test_refusals_leave_the_cache_alone():
    m = _model("causal")
    x, a, s, _ = _inputs("causal")
    cache = m.new_cache(2, 3)
    _cached(m, x, a, s, None, (1,), cache=cache)
    one = (x[:, HW:2 * HW], a[:, 1:2], s[:, 1:2])

    def refused(exc, match, fn):
        with pytest.raises(exc, match=match):
            fn()
        assert cache.frames == 1

    # gradient mode with parameters (or an input) requiring grad
    refused(RuntimeError, "inference only", lambda: m.forward_cached(*one, cache=cache))
    for p in m.parameters():
        p.requires_grad_(False)
    refused(RuntimeError, "inference only",
            lambda: m.forward_cached(one[0].clone().requires_grad_(True), one[1], one[2], cache=cache))
    m.forward_cached(*one, cache=cache)  # grad mode on, nothing requires grad: fine
    cache.rewind(1)
    with torch.no_grad():
        refused(ValueError, "batch 1 != cache.batch 2",
                lambda: m.forward_cached(*(t[:1] for t in one), cache=cache))
        refused(ValueError, "max_frames 3",
                lambda: m.forward_cached(x, a, s, cache=cache))  # 1 cached + 3 new frames
        # training mode with an active drop_path / dropout
        dp = _model("causal_silu_dp").train()
        refused(RuntimeError, "drop_path is active", lambda: dp.forward_cached(*one, cache=cache))
        dr = _model("causal", drop_rate=0.1).train()
        refused(RuntimeError, "dropout is active", lambda: dr.forward_cached(*one, cache=cache))
        # a predictor that is not frame-causal has no valid cache
        nc = _model("causal", is_frame_causal=False)
        refused(ValueError, "not frame-causal", lambda: nc.forward_cached(*one, cache=cache))
        refused(ValueError, "not frame-causal", lambda: nc.new_cache(2, 3))
        # more frames than the frame-causal mask covers (num_frames // tubelet_size = 3)
        refused(ValueError, "exceeds the 3 frames", lambda: m.new_cache(2, 4))
        y = m.forward_cached(*one, cache=cache)  # the cache still works
    assert cache.frames == 2 and torch.isfinite(y).all()
