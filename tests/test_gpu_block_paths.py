"""Every composition path of functions.block_forward / block_backward (and the standalone attn_module_* /
mlp_module_*) against the float64 reference of tests/block_refs.py, per row of every tensor, under the bound
C * E(t) measured against the bf16 emulation (block_refs' docstring). Each case runs twice with the same seeds
and draws and must repeat bitwise. Dropout seeds are replayed through functions._drop_seed, DropPath draws
through blk.drop_path.sample. Dense layouts go through Block.forward, the ragged / action-conditioned layouts
and the forward-only bf16 cases through functions.run_block with a TokenLayout."""

import functools

import pytest
import torch
import torch.nn as nn

import block_refs as br

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ------------------------------------------------------------------------------------------------
# spies on ops: one event string per call, in host order


class Spy:
    NAMES = ("linear_fwd", "rowscale_add", "rowscale_bf16", "dropout", "cast_bf16", "colsum", "layernorm_bwd",
             "linear_dgrad", "swiglu_bwd")

    def __init__(self):
        from vjepa2_amd import ops

        self.ops, self.events, self.phase, self.saved = ops, [], "fwd", {}
        self.epi = {getattr(ops, n): n for n in ("EPI_BF16", "EPI_BF16_RESID", "EPI_F32", "EPI_F32_RESID", "EPI_GELU")}

    def _tag(self, name, a, kw):
        dt = lambda t: "bf16" if t.dtype == torch.bfloat16 else "f32"  # noqa: E731
        arg = lambda i, k, d=None: kw[k] if k in kw else (a[i] if len(a) > i else d)  # noqa: E731
        if name == "linear_fwd":
            return "linear_fwd:" + self.epi[arg(3, "epi", self.ops.EPI_BF16)]
        if name == "rowscale_add":
            return "rowscale_add:" + dt(arg(2, "resid"))
        if name == "dropout":
            resid, aux = arg(3, "resid"), arg(4, "aux")
            return "dropout:resid:" + dt(resid) if resid is not None else ("dropout:aux" if aux is not None else
                                                                          "dropout:plain")
        if name == "layernorm_bwd":
            return "layernorm_bwd:" + ("sum" if arg(9, "sum_in") is not None else "nosum")
        if name == "linear_dgrad":
            return "dgrad" + (":gelu" if arg(3, "gelu_grad") is not None else "") + (
                ":resid" if arg(5, "resid") is not None else "")
        return name

    def __enter__(self):
        for n in self.NAMES:
            real = self.saved[n] = getattr(self.ops, n)

            def wrap(*a, _n=n, _real=real, **kw):
                self.events.append((self.phase, self._tag(_n, a, kw)))
                return _real(*a, **kw)

            setattr(self.ops, n, wrap)
        return self

    def __exit__(self, *exc):
        for n, real in self.saved.items():
            setattr(self.ops, n, real)
        return False

    def of(self, phase):
        return [e for p, e in self.events if p == phase]


def routes(events_fwd, events_bwd, dy_bf16):
    """The composition routes a run took, from its ops events."""
    out = set()
    for i, e in enumerate(events_fwd):
        if e in ("linear_fwd:EPI_F32_RESID", "linear_fwd:EPI_BF16_RESID"):
            out.add("out:fused:" + ("f32" if "F32" in e else "bf16"))
        elif e.startswith("rowscale_add:"):
            both = i > 0 and events_fwd[i - 1] == "dropout:plain"
            out.add(("out:dropout+droppath:" if both else "out:droppath:") + e.split(":")[1])
        elif e.startswith("dropout:resid:"):
            out.add("out:dropout:" + e.split(":")[2])
    # the backward of a block: [dY of the MLP branch] LayerNorm-2 backward [proj dY] LayerNorm-1 backward
    segs, cur = [], []
    for e in events_bwd:
        if e.startswith("layernorm_bwd"):
            segs.append((cur, e))
            cur = []
        else:
            cur.append(e)
    for k in range(0, len(segs), 2):
        seg, ln2 = segs[k]
        first = next((i for i, e in enumerate(seg) if e.startswith("dgrad")), len(seg))  # _mlp_backward starts
        src = [e for e in seg[:first] if e in ("cast_bf16", "rowscale_bf16", "dropout:plain", "colsum")]
        out.add("dy:" + ("+".join(src) if src else ("bf16" if dy_bf16 else "twin")))
        out.add("bias:fused" if ln2.endswith(":sum") else "bias:colsum")
        assert ln2.endswith(":sum") or "colsum" in segs[k + 1][0], "unfused proj bias gradient without a colsum"
        if "swiglu_bwd" in seg:
            out.add("mlp:swiglu")
        else:
            out.add("mlp:gelu")
            out.add("fc2dgrad:dropout" if "dropout:aux" in seg else "fc2dgrad:gelu")
            assert ("dgrad:gelu" in seg) != ("dropout:aux" in seg)
    return out


REQUIRED_ROUTES = {
    # _branch_out: fused epilogue, drop_path, dropout, both; in both residual dtypes where the matrix reaches them
    "out:fused:f32", "out:fused:bf16", "out:droppath:f32", "out:droppath:bf16", "out:dropout:f32", "out:dropout:bf16",
    "out:dropout+droppath:f32",
    # block_backward's dY of the MLP branch: the cast, the bf16 stream, the twin, drop_path, the dropout branch
    # (with p > 0, with drop_path before it, and with p = 0 under SwiGLU)
    "dy:cast_bf16", "dy:bf16", "dy:twin", "dy:rowscale_bf16+colsum", "dy:dropout:plain+colsum",
    "dy:rowscale_bf16+dropout:plain+colsum", "dy:cast_bf16+colsum",
    "bias:fused", "bias:colsum", "fc2dgrad:gelu", "fc2dgrad:dropout", "mlp:gelu", "mlp:swiglu",
}


# ------------------------------------------------------------------------------------------------
# running a block on the HIP path


def _token_layout(name):
    from vjepa2_amd import functions as fn
    from vjepa2_amd import modules

    lay = br.layout(name)
    if name == "L3":
        tl = modules.ac_token_layout(B=2, T=3, H=4, W=4, cond=2, causal=True, device=DEV)
        assert tl.fblk == lay.fblk == 18 and tl.groups == [tuple(g) for g in lay.groups]
        assert torch.equal(tl.ids.cpu().long(), lay.ids) and (tl.ids_mod, tl.tpf, tl.tpr) == lay[2:5]
        return tl
    ids = lay.ids.to(torch.int32).to(DEV) if lay.ids is not None else None
    return fn.TokenLayout(lay.groups, ids=ids, ids_mod=lay.ids_mod, tpf=lay.tpf, tpr=lay.tpr, fblk=lay.fblk)


def _make_block(P, mlp="gelu", layout="L1", qkv_bias=True, sdpa=True, qk_scale=None, drop=0.0, attn_drop=0.0,
                dpath=False):
    from vjepa2_amd import modules

    cls = modules.ACBlock if layout == "L3" else modules.Block
    blk = cls(br.D, br.H, mlp_ratio=4.0, qkv_bias=qkv_bias, qk_scale=qk_scale, drop=drop, attn_drop=attn_drop,
              drop_path=br.DROP_PATH_P if dpath else 0.0, act_layer=nn.GELU if mlp == "gelu" else nn.SiLU,
              wide_silu=mlp == "swiglu_wide", norm_layer=lambda d: nn.LayerNorm(d, eps=br.EPS), use_sdpa=sdpa,
              grid_size=4, use_rope=br.layout(layout).ids is not None).to(DEV)
    blk.load_state_dict(P)
    return blk.train()


def _case_block(case):
    return _make_block(br.inputs(case.name).P, case.mlp, case.layout, case.qkv_bias, case.sdpa, case.qk_scale,
                       case.drop, case.attn_drop, case.dpath)


class _Replay:
    """functions._drop_seed hands out block_refs.SEEDS in order; each block's DropPath replays `draws`."""

    def __init__(self, blks, draws=None):
        from vjepa2_amd import functions as fn

        self.fn, self.blks, self.draws = fn, blks, draws

    def __enter__(self):
        self.real = self.fn._drop_seed
        seeds = iter(br.SEEDS)
        self.fn._drop_seed = lambda: next(seeds)
        if self.draws is not None:
            for b in self.blks:
                pending = [d.float() for d in self.draws]
                b.drop_path.sample = lambda n, device, _p=pending: _p.pop(0).to(device)
        return self

    def __exit__(self, *exc):
        self.fn._drop_seed = self.real
        return False


def _forward(x, blk, layout):
    """x [T, D] through the block: Block.forward for the dense layouts it can express (f32 or trained bf16
    input), functions.run_block with a TokenLayout otherwise."""
    from vjepa2_amd import functions as fn

    lay = br.layout(layout)
    if layout in ("L2", "L4") and torch.is_grad_enabled():
        (B, N), = lay.groups
        return blk(x.view(B, N, -1)).reshape(x.shape)
    return fn.run_block(x, blk, _token_layout(layout))


def _collect(y, x, blks, prefix=False):
    out = {"y": y.detach().clone()}
    if x.grad is not None:
        out["dx"] = x.grad.clone()
        for i, b in enumerate(blks):
            for n, p in b.named_parameters():
                if p.grad is not None:
                    out[(f"d{i}." if prefix else "d") + n] = p.grad.clone()
    torch.cuda.synchronize()
    return out


def _run_once(case, blk, dys=None):
    """One forward (+ one backward per dy, each after a forward of its own) of a matrix case with spies on."""
    inp = br.inputs(case.name)
    dt = torch.bfloat16 if case.bf16 else torch.float32
    blk.zero_grad(set_to_none=True)
    x = inp.x.to(DEV, dt).requires_grad_(not case.fwd_only)
    dys = (inp.dy,) if dys is None else dys
    with Spy() as spy, _Replay([blk], inp.draws):
        if case.fwd_only:
            with torch.no_grad():
                y = _forward(x, blk, case.layout)
        else:
            for dy in dys:
                spy.phase = "fwd"
                y = _forward(x, blk, case.layout)
                spy.phase = "bwd"
                y.backward(dy.to(DEV, dt))
    assert y.dtype == dt and (case.fwd_only or x.grad.dtype == dt)
    return _collect(y, x, [blk]), spy


def _assert_bitwise(a, b, label):
    assert set(a) == set(b), label
    for k in a:
        assert torch.equal(a[k], b[k]), f"{label}: {k} differs between two runs with the same seeds"


@functools.lru_cache(None)
def hip_case(name):
    """(outputs, routes) of a matrix case on the HIP path; run twice, bitwise repeatable."""
    case = br.CASES[name]
    blk = _case_block(case)
    out, spy = _run_once(case, blk)
    again, _ = _run_once(case, blk)
    _assert_bitwise(out, again, name)
    return out, routes(spy.of("fwd"), spy.of("bwd"), case.bf16)


@functools.lru_cache(None)
def hip_chain(halve):
    """Two stacked blocks on case 1's inputs; halve: a tensor hook between the blocks halves the gradient in
    place. Returns (outputs, routes, number of ops.cast_bf16 calls in the backward)."""
    from vjepa2_amd import functions as fn

    inp = br.inputs("c01_gelu_f32")
    blks = [_make_block(br.make_params("gelu", True, 7 + i)) for i in range(2)]
    lay = _token_layout("L1")
    res = []

    def halve_in_place(g):
        g.mul_(0.5)

    for _ in range(2):
        for b in blks:
            b.zero_grad(set_to_none=True)
        x = inp.x.to(DEV).requires_grad_(True)
        with Spy() as spy:
            h = fn.run_block(x, blks[0], lay)
            if halve:
                h.register_hook(halve_in_place)
            y = fn.run_block(h, blks[1], lay)
            spy.phase = "bwd"
            y.backward(inp.dy.to(DEV))
        res.append(_collect(y, x, blks, prefix=True))
    _assert_bitwise(res[0], res[1], "chain")
    return res[0], routes(spy.of("fwd"), spy.of("bwd"), False), spy.of("bwd").count("cast_bf16")


# ------------------------------------------------------------------------------------------------
# tests


@pytest.mark.parametrize("name", [c.name for c in br.MATRIX])
def test_block_case(name):
    """Cases 1 - 12, 14, 15: y, dx and every parameter gradient (y alone where forward-only) within C * E of the
    float64 reference on every row; bitwise repeatable."""
    out, _ = hip_case(name)
    ref = br.run_case(name)
    assert set(out) == set(ref)
    br.check(out, ref, br.run_case(name, "all"), name)


def test_frozen_output_biases():
    """Case 13: attn.proj.bias and mlp.fc2.bias frozen: their .grad stays None, everything else is case 1's,
    bitwise (the fused bias sums are simply not taken)."""
    case = br.CASES["c01_gelu_f32"]
    blk = _case_block(case)
    blk.attn.proj.bias.requires_grad_(False)
    blk.mlp.fc2.bias.requires_grad_(False)
    out, _ = _run_once(case, blk)
    assert blk.attn.proj.bias.grad is None and blk.mlp.fc2.bias.grad is None
    full, _ = hip_case(case.name)
    assert set(full) - set(out) == {"dattn.proj.bias", "dmlp.fc2.bias"}
    for k in out:
        assert torch.equal(out[k], full[k]), k


def test_stacked_blocks_use_the_twin():
    """Case 16, unmodified chain: the second block's LayerNorm-1 backward supplies block one's bf16 dY, so the
    only cast of the backward is that of the incoming dy."""
    out, rts, casts = hip_chain(False)
    assert casts == 1 and "dy:twin" in rts, (casts, rts)
    br.check(out, br.run_chain(), br.run_chain("all"), "c16_chain")


def test_stale_twin_is_refused():
    """Case 16 with the gradient between the blocks halved in place: the version check falls back to the cast
    and the result is the reference's with the halved gradient."""
    out, rts, casts = hip_chain(True)
    assert casts == 2 and "dy:twin" not in rts, (casts, rts)
    br.check(out, br.run_chain(None, 0.5), br.run_chain("all", 0.5), "c16_chain_halved")


def test_two_backward_passes_accumulate():
    """Case 17: two passes with different dy into the same .grad give the sum of the two references."""
    case = br.CASES["c01_gelu_f32"]
    inp = br.inputs(case.name)
    blk = _case_block(case)
    out, _ = _run_once(case, blk, dys=(inp.dy, inp.dy2))
    again, _ = _run_once(case, blk, dys=(inp.dy, inp.dy2))
    _assert_bitwise(out, again, "accumulate")
    br.check(out, br.run_accumulate(), br.run_accumulate("all"), "c17_accumulate")


def _make_sublayer(name):
    from vjepa2_amd import modules

    s = br.SUBLAYERS[name]
    if s["kind"] == "attn":
        kw = dict(num_heads=br.H, qkv_bias=True, qk_scale=s["qk_scale"], proj_drop=s["proj_drop"], use_sdpa=s["sdpa"])
        rope = br.layout(s["layout"]).ids is not None
        mod = modules.RoPEAttention(br.D, grid_size=4, **kw) if rope else modules.Attention(br.D, **kw)
    elif s["mlp"] == "gelu":
        mod = modules.MLP(br.D, 4 * br.D, drop=s["drop"])
    else:
        mod = modules.SwiGLUFFN(br.D, 4 * br.D, wide_silu=True)
    mod.load_state_dict(br.sublayer_inputs(name)[2])
    return mod.to(DEV).train()


@pytest.mark.parametrize("name", list(br.SUBLAYERS))
def test_standalone_module(name):
    """Case 18: the standalone modules through functions.run_sublayer vs the matching piece of the reference."""
    from vjepa2_amd import functions as fn

    x0, dy, _, _, _ = br.sublayer_inputs(name)
    mod = _make_sublayer(name)
    lay = _token_layout(br.SUBLAYERS[name]["layout"]) if br.SUBLAYERS[name]["kind"] == "attn" else None
    res = []
    for _ in range(2):
        mod.zero_grad(set_to_none=True)
        x = x0.to(DEV).requires_grad_(True)
        with _Replay([]):
            y = fn.run_sublayer(x, mod, lay)
            y.backward(dy.to(DEV))
        res.append(_collect(y, x, [mod]))
    _assert_bitwise(res[0], res[1], name)
    ref = br.run_sublayer(name)
    assert set(res[0]) == set(ref)
    br.check(res[0], ref, br.run_sublayer(name, "all"), "c18_" + name)


def test_route_coverage():
    """Set cover over the whole matrix (and the stacked chain): every composition route of _branch_out,
    block_backward's dY sources, both bias-gradient forms, both fc2 data-gradient forms and both MLP kinds is
    reached at least once. Not per-case call counts: a later fusion may reroute a case."""
    reached = {}
    for c in br.MATRIX:
        for r in hip_case(c.name)[1]:
            reached.setdefault(r, []).append(c.name)
    for r in hip_chain(False)[1]:
        reached.setdefault(r, []).append("chain")
    print("\n".join(f"{r}: {' '.join(v)}" for r, v in sorted(reached.items())))
    assert not REQUIRED_ROUTES - set(reached), sorted(REQUIRED_ROUTES - set(reached))
