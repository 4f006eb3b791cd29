"""CPU: the host side of the AC predictor's rollout cache (no GPU here, so anything that reached a kernel would
raise "no CPU path" instead): the frame counter, the step layouts' RoPE ids against ac_token_layout's, the size,
and that every refusal of forward_cached comes before any device work and leaves the counter alone."""

import pytest
import torch

CFG = dict(img_size=32, patch_size=16, num_frames=6, tubelet_size=2, embed_dim=96, predictor_embed_dim=64, depth=2,
           num_heads=2, action_embed_dim=7)


def _model(**over):
    from vjepa2_amd.ac_predictor import vit_ac_predictor

    torch.manual_seed(0)
    return vit_ac_predictor(**dict(CFG, **over)).eval()


def test_cache_counter_size_and_layouts():
    from vjepa2_amd.modules import ac_token_layout

    m = _model(use_extrinsics=True)
    cache = m.new_cache(5, 3)
    n_t = 3 + 4
    assert (cache.batch, cache.max_frames, cache.n_t, cache.frames) == (5, 3, n_t, 0)
    assert len(cache.kv) == 2 and all(t.shape == (5, 3 * n_t, 128) and t.dtype == torch.bfloat16 for t in cache.kv)
    assert cache.nbytes() == 2 * 5 * 3 * n_t * 128 * 2
    full = ac_token_layout(5, 3, 2, 2, 3, True, "cpu")
    ids = full.ids.reshape(5, 3, n_t)
    for t0, tn in ((0, 1), (1, 1), (2, 1), (0, 2), (1, 2), (0, 3)):
        lay = cache.layout(t0, tn)
        assert torch.equal(lay.ids.reshape(5, tn, n_t), ids[:, t0:t0 + tn])
        assert (lay.ids_mod, lay.tpf, lay.tpr, lay.fblk, lay.npos) == (full.ids_mod, full.tpf, full.tpr, n_t, full.npos)
        assert lay.groups == [(5, tn * n_t)] and cache.layout(t0, tn) is lay
    cache.frames = 2
    cache.rewind(2)
    cache.rewind(1)
    assert cache.frames == 1
    for bad in (2, -1):
        with pytest.raises(ValueError, match="holds 1 frames"):
            cache.rewind(bad)
    cache.reset()
    assert cache.frames == 0
    with pytest.raises(ValueError, match="exceeds the 3 frames"):
        m.new_cache(5, 4)
    with pytest.raises(ValueError, match="not frame-causal"):
        _model(is_frame_causal=False).new_cache(5, 3)


def test_refusals_come_before_any_device_work():
    m = _model()
    cache = m.new_cache(2, 3)
    cache.frames = 1
    x, a, s = torch.zeros(2, 4, 96), torch.zeros(2, 1, 7), torch.zeros(2, 1, 7)

    def refused(exc, match, fn):
        with pytest.raises(exc, match=match):
            fn()
        assert cache.frames == 1

    refused(RuntimeError, "inference only", lambda: m.forward_cached(x, a, s, cache=cache))
    with torch.no_grad():
        refused(ValueError, "batch 3 != cache.batch 2",
                lambda: m.forward_cached(torch.zeros(3, 4, 96), torch.zeros(3, 1, 7), torch.zeros(3, 1, 7), cache=cache))
        refused(ValueError, "max_frames 3",
                lambda: m.forward_cached(torch.zeros(2, 12, 96), torch.zeros(2, 3, 7), torch.zeros(2, 3, 7), cache=cache))
        refused(ValueError, "not whole frames", lambda: m.forward_cached(torch.zeros(2, 5, 96), a, s, cache=cache))
        refused(RuntimeError, "drop_path is active",
                lambda: _model(drop_path_rate=0.5).train().forward_cached(x, a, s, cache=cache))
        refused(RuntimeError, "dropout is active",
                lambda: _model(drop_rate=0.1).train().forward_cached(x, a, s, cache=cache))
        refused(ValueError, "not frame-causal",
                lambda: _model(is_frame_causal=False).forward_cached(x, a, s, cache=cache))
        refused(TypeError, "ACRolloutCache", lambda: m.forward_cached(x, a, s, cache=None))
        # an accepted call goes on to the kernels, which have no CPU path
        refused(RuntimeError, "no CPU path", lambda: m.forward_cached(x, a, s, cache=cache))
    # drop_path in eval() is inactive: accepted (and then stopped by the missing device only)
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU path"):
        _model(drop_path_rate=0.5).forward_cached(x, a, s, cache=cache)


def test_world_model_switch_is_a_setter():
    from vjepa2_amd.planning import WorldModel

    wm = WorldModel(encoder=None, predictor=_model(), tokens_per_frame=4, transform=None, device="cpu")
    assert wm.kv_cache is False and wm._cache is None
    assert wm.set_kv_cache(True) is wm and wm.kv_cache is True
    c = wm._rollout_cache(6, 2)
    assert (c.batch, c.max_frames) == (6, 2) and wm._rollout_cache(6, 2) is c
    assert wm._rollout_cache(6, 3) is not c and wm._rollout_cache(4, 3).batch == 4
    with pytest.raises(ValueError, match="exceeds the 3 frames"):
        wm._rollout_cache(4, 4)
    assert wm.set_kv_cache(False)._cache is None
