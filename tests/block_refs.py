"""Float64 reference, bf16 emulation and deliberately wrong variants ("mutants") of one transformer block
on a packed [T, D] batch: the layer vjepa2_amd/functions.py composes from the HIP kernels (block_forward /
block_backward, _branch_out / _branch_grad, _mlp_forward / _mlp_backward, attn_module_* / mlp_module_*).
A helper, not collected: tests/test_block_refs.py (CPU) anchors the reference to the reference project's
recorded fixtures and proves that every mutant breaks the bound; tests/test_gpu_block_paths.py holds the HIP
path to the same bound on the same inputs. Nothing here imports vjepa2_amd.

Reference (`block_graph`, plain torch in float64, backward by autograd): LayerNorm, QKV (optional bias),
optional 3-axis RoPE (oracle.vjepa_oracle.apply_rope_qk), softmax attention per sequence with an optional
frame-causal mask (j // fblk <= i // fblk) and an optional dropout matrix on the probabilities, proj, the
branch dropout mask, the per-sequence DropPath factor repeated over the sequence's tokens, the residual add,
LayerNorm, the GELU MLP with its two dropout masks or SwiGLU (fc3(silu(fc1 x) * fc2 x)), mask, factor and add
again. Masks (test_dropout.vj_dropout_mask_ref; attention rows = token * H + head) and draws are arguments.

Emulation: the same function with a rounding hook R(t, point): bf16 in the forward, the gradient to bf16 in
the backward, at the rounding points functions.py and include/vjepa_hip.h document:
    GEMM operands    LayerNorm outputs ("ln"), weights ("w", forward only: weight gradients are f32), the
                     (rotated) q, k, v ("qkv"), the probabilities ("p"), the attention output ("o"), the
                     GELU / SwiGLU activation and its dropped form ("act")
    other points     the bf16 pre-activations of fc1 (GELU) and fc1 | fc2 (SwiGLU) ("pre"), the branch
                     outputs of the drop_path / dropout forms bf16(bf16(y) * z) ("branch"), the bf16
                     residual stream where a case uses it ("resid")
    gradients        every hook rounds its gradient; a bwd-only hook ("grad") on each branch output is the
                     bf16 dY the backward GEMMs read.
Placement "all" rounds at every point; placement "gemm" rounds the forward at the GEMM operands only (the
gradients at every hook, since they all feed backward GEMMs). The emulation is a yardstick for how much
error bf16 rounding buys at these shapes, not a bit model of the kernels (no f32 accumulation order, no bf16
GELU', f64 RoPE angles, probabilities' gradient rounded where the kernels round dS).

Error measure, per row r of a 2-D tensor (tokens for y / dx, output channels for weight gradients; a vector
is one row):
    e_r(got) = |got_r - ref_r|_2 / max(|ref_r|_2, |ref|_F / sqrt(rows))
    E(t)     = max(max_r e_r(emulation "all"), E_FLOOR)
and the HIP path must satisfy e_r(HIP) <= C * E(t) on every row of every tensor. C is measured against the
emulation, not chosen from the code under test: the largest e_r(HIP) / E(t) over the whole matrix, rounded up
to the next of 1.5, 2, 3.

Measured on an MI355X, the largest e_r(HIP) / E(t) per case (the tensor it falls on):
    c01_gelu_f32          1.118 dmlp.fc1.weight     c09_swiglu_droppath    1.163 dnorm2.weight
    c02_gelu_bf16         1.174 dnorm2.bias         c10_swiglu_dropout     1.239 dmlp.fc2.weight
    c03_nobias_nosdpa_..  1.030 dmlp.fc1.bias       c11_frame_causal       1.217 dmlp.fc1.weight
    c04_droppath          1.267 dnorm1.bias         c12_T1056              1.066 dnorm2.bias
    c05_dropout           1.232 y                   c14_fwd_bf16_dropout   1.001 y
    c06_dropout_droppath  1.172 dattn.qkv.weight    c15_fwd_bf16_droppath  1.090 y
    c07_attn_drop_only    1.176 dnorm1.weight       c16 chain / halved     1.186 d0.norm2.weight
    c08_swiglu_wide       1.105 y                   c17 accumulate         1.172 dattn.qkv.weight
    c08_swiglu_narrow     1.257 dattn.proj.weight   c18 standalone modules 1.172 / 1.097 / 1.106 / 1.234
The largest is 1.267, so C = 1.5. No case came near 3; no route produced wrong values. The emulation's own
two placements differ by up to 1.4998 E (d1.attn.proj.weight of the stacked chain, one output channel of small
norm; 1.18 E on every other tensor; tests/test_block_refs.py), so C is no tighter than the yardstick's ambiguity.
E itself: 1.5e-3 ... 1.4e-2 on every tensor of every case (bias gradients lowest, qkv weight rows highest).

Mutants of the float64 reference, each a plausible composition bug:
    M1  the output Linear's bias gradient is summed from the residual gradient dxo, not from the scaled /
        dropped branch dY (active: drop_path or branch dropout on that branch)
    M2  the MLP branch uses the attention branch's DropPath draws (drop_path)
    M3  draws repeated over the wrong lengths: the lengths are rotated by one sequence (drop_path, ragged)
    M4  the two MLP dropouts share one seed (GELU MLP with drop > 0)
    M5  the backward of the MLP branch's dropout applies the proj mask (GELU MLP with drop > 0, backward)
    M6  the residual gradient is left out of dxm: LayerNorm-2's backward runs without dres_in (backward)
    M7  the output Linear's weight gradient is taken against a stale dY, that of a previous call (backward)
    M8  the attention scale is hd ** -0.5 where the module asks for its qk_scale (no SDPA, qk_scale set)
Each must exceed C E by a factor 4 on at least one tensor in every case where it is active. Smallest
max_t e_r / (C E) per mutant over its active cases (tests/test_block_refs.py prints them):
    M1 10.1 (c14, forward only; 17.6 ... 273 elsewhere)   M2 104   M3 112   M4 65   M5 134   M6 77   M7 123   M8 42
"""

import functools
import math
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from oracle import vjepa_oracle as orc
from test_dropout import vj_dropout_mask_ref

F64 = torch.float64
D, H, HD, EPS = 128, 2, 64, 1e-6
C = 1.5  # measured: see the docstring
# Floor of E(t). Where no bf16 rounding reaches a tensor the emulation is exact (the fc2 bias gradient of a bf16
# stream is the column sum of the bf16 dy itself), yet the kernels sum in f32 where the reference sums in f64: a
# sum of T <= 1056 terms of either sign carries up to about sqrt(T) 2^-24 = 2e-6 of its own size. 2^-16 covers
# that with room and is 1 / 256 of one bf16 rounding, so it hides nothing the measure is after.
E_FLOOR = 2.0 ** -16

GEMM_POINTS = ("ln", "w", "qkv", "p", "o", "act")
OTHER_POINTS = ("pre", "branch", "resid")


# ------------------------------------------------------------------------------------------------
# rounding hook


class _Round(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t, fwd, bwd):
        ctx.bwd = bwd
        return t.bfloat16().to(t.dtype) if fwd else t.view_as(t)

    @staticmethod
    def backward(ctx, g):
        return (g.bfloat16().to(g.dtype) if ctx.bwd else g), None, None


def make_hook(mode):
    """mode None: the exact reference; "all" / "gemm": the two emulation placements."""
    if mode is None:
        return lambda t, point, fwd=True, bwd=True: t
    assert mode in ("all", "gemm")

    def R(t, point, fwd=True, bwd=True):
        assert point in GEMM_POINTS + OTHER_POINTS + ("grad",), point
        if mode == "gemm" and point in OTHER_POINTS:
            fwd = False
        return _Round.apply(t, fwd, bwd)

    return R


class _Mask(torch.autograd.Function):
    """t * zf in the forward, g * zb in the backward (zb is zf unless a mutant swaps it)."""

    @staticmethod
    def forward(ctx, t, zf, zb):
        ctx.zb = zb
        return t * zf

    @staticmethod
    def backward(ctx, g):
        return g * ctx.zb, None, None


class _StaleW(torch.autograd.Function):
    """h W^T whose weight gradient is taken against `stale` instead of the incoming dY (M7)."""

    @staticmethod
    def forward(ctx, h, w, stale):
        ctx.save_for_backward(h, w, stale)
        return h @ w.t()

    @staticmethod
    def backward(ctx, g):
        h, w, stale = ctx.saved_tensors
        return g @ w, stale.t() @ h, None


class _ScaleGrad(torch.autograd.Function):
    """Identity whose gradient is multiplied by `f` (the in-place tensor hook of the stale-twin case)."""

    @staticmethod
    def forward(ctx, t, f):
        ctx.f = f
        return t.view_as(t)

    @staticmethod
    def backward(ctx, g):
        return g * ctx.f, None


# ------------------------------------------------------------------------------------------------
# layouts and cases

Layout = namedtuple("Layout", "groups ids ids_mod tpf tpr fblk")


def seq_lens(groups):
    return [ln for n, ln in groups for _ in range(n)]


@functools.lru_cache(None)
def layout(name):
    """ids: int64 [T] RoPE token ids, or None (no RoPE)."""
    if name == "L1":  # ragged; explicit ascending subsets of a 5-frame 4 x 4 grid
        g = torch.Generator().manual_seed(101)
        ids = [torch.randperm(80, generator=g)[:48].sort().values for _ in range(2)] + [torch.arange(80)]
        return Layout(((2, 48), (1, 80)), torch.cat(ids), 80, 16, 4, 0)
    if name == "L2":
        return Layout(((3, 32),), None, 32, 1, 1, 0)
    if name == "L3":  # action-conditioned: B = 2, T = 3 frames of cond = 2 + 4 x 4 tokens, frame-causal
        B, T, hw, cond = 2, 3, 16, 2
        n_t = cond + hw
        ids = torch.tensor([t * hw + max(j - cond, 0) for t in range(T) for j in range(n_t)])
        return Layout(((B, T * n_t),), ids.repeat(B), T * hw, hw, 4, n_t)
    if name == "L4":  # T = 1056 >= 1024: the 256-row GEMMs and the fused RoPE epilogue
        return Layout(((4, 264),), torch.arange(264).repeat(4), 264, 16, 4, 0)
    raise KeyError(name)


# mlp: "gelu" | "swiglu_wide" | "swiglu_narrow"; dpath: active DropPath with the draws DRAWS
Case = namedtuple("Case", "name layout mlp bf16 qkv_bias sdpa qk_scale drop attn_drop dpath fwd_only")


def _case(name, layout="L1", mlp="gelu", bf16=False, qkv_bias=True, sdpa=True, qk_scale=None, drop=0.0, attn_drop=0.0,
          dpath=False, fwd_only=False):
    return Case(name, layout, mlp, bf16, qkv_bias, sdpa, qk_scale, drop, attn_drop, dpath, fwd_only)


MATRIX = (
    _case("c01_gelu_f32"),
    _case("c02_gelu_bf16", bf16=True),
    _case("c03_nobias_nosdpa_qkscale", layout="L2", qkv_bias=False, sdpa=False, qk_scale=0.2),
    _case("c04_droppath", dpath=True),
    _case("c05_dropout", drop=0.15),
    _case("c06_dropout_droppath", drop=0.15, dpath=True),
    _case("c07_attn_drop_only", sdpa=False, attn_drop=0.1),
    _case("c08_swiglu_wide", mlp="swiglu_wide"),
    _case("c08_swiglu_narrow", mlp="swiglu_narrow"),
    _case("c09_swiglu_droppath", mlp="swiglu_narrow", dpath=True),
    _case("c10_swiglu_dropout", mlp="swiglu_wide", drop=0.15),
    _case("c11_frame_causal", layout="L3"),
    _case("c12_T1056", layout="L4"),
    _case("c14_fwd_bf16_dropout", bf16=True, drop=0.15, fwd_only=True),
    _case("c15_fwd_bf16_droppath", bf16=True, dpath=True, fwd_only=True),
)
CASES = {c.name: c for c in MATRIX}

# per-sequence DropPath factors (keep = 0.5) of the attention and the MLP branch: each drops a sequence, they
# differ between the branches and between the sequences
DROP_PATH_P = 0.5
DRAWS = {3: ((0.0, 2.0, 2.0), (2.0, 0.0, 2.0))}
SEEDS = (11, 22, 33, 44)  # handed out in the order attention, proj, MLP activation, MLP output


def hidden_width(mlp):
    return {"gelu": 4 * D, "swiglu_narrow": 4 * D, "swiglu_wide": (int(2 * 4 * D / 3) + 7) // 8 * 8}[mlp]


def drop_probs(case):
    """(attention, proj, MLP) dropout probabilities of a training-mode block (modules.py): SDPA takes the
    proj_drop probability, the non-SDPA branch attn_drop; SwiGLUFFN has no dropout."""
    pa = case.drop if case.sdpa else case.attn_drop
    return pa, case.drop, (case.drop if case.mlp == "gelu" else 0.0)


def case_seeds(case):
    pa, pp, pm = drop_probs(case)
    it = iter(SEEDS)
    return tuple(next(it) if p > 0 else 0 for p in (pa, pp, pm, pm))


def make_params(mlp, qkv_bias, seed):
    """f32 state dict of a Block (the reference's parameter names): unit-scale activations, so both branches
    weigh as much as the residual stream."""
    g = torch.Generator().manual_seed(seed)
    hid = hidden_width(mlp)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    P = {}
    for n in ("norm1", "norm2"):
        P[n + ".weight"] = 1 + 0.1 * rn(D)
        P[n + ".bias"] = 0.1 * rn(D)
    lin = [("attn.qkv", 3 * D, D), ("attn.proj", D, D), ("mlp.fc1", hid, D)]
    lin += [("mlp.fc2", D, hid)] if mlp == "gelu" else [("mlp.fc2", hid, D), ("mlp.fc3", D, hid)]
    for n, o, i in lin:
        P[n + ".weight"] = rn(o, i) * i ** -0.5
        if n != "attn.qkv" or qkv_bias:
            P[n + ".bias"] = 0.1 * rn(o)
    order = ["norm1", "attn.qkv", "attn.proj", "norm2", "mlp.fc1", "mlp.fc2", "mlp.fc3"]
    return {k: P[k] for n in order for k in (n + ".weight", n + ".bias") if k in P}


def mask_scale(seed, p, rows, cols):
    """keep / (1 - p) of vj_dropout's mask, float64 [rows, cols]."""
    keep = vj_dropout_mask_ref(seed, np.arange(rows), np.arange(cols), p)
    return torch.from_numpy(keep).to(F64) / (1 - p)


def attn_mask_scales(seed, p, groups, nheads):
    """Per sequence [H, L, L]: mask row = token * H + head, column = key within the sequence."""
    out, t0 = [], 0
    for ln in seq_lens(groups):
        rows = (np.arange(t0, t0 + ln)[None, :] * nheads + np.arange(nheads)[:, None]).reshape(-1)
        keep = vj_dropout_mask_ref(seed, rows, np.arange(ln), p)
        out.append(torch.from_numpy(keep).to(F64).reshape(nheads, ln, ln) / (1 - p))
        t0 += ln
    return out


Inputs = namedtuple("Inputs", "x dy dy2 P cfg masks draws")
Cfg = namedtuple("Cfg", "H groups ids tpf tpr fblk scale eps swiglu bf16")


@functools.lru_cache(None)
def inputs(name):
    """Everything a case feeds the block, f32 (x and dy rounded to bf16 where the case's stream is bf16).
    dy2: a second output gradient (the stale dY of M7, the second backward of the accumulation case)."""
    case = CASES[name]
    lay = layout(case.layout)
    T = sum(n * ln for n, ln in lay.groups)
    g = torch.Generator().manual_seed(1000 + sum(map(ord, name)))
    x, dy, dy2 = (torch.randn(T, D, generator=g) for _ in range(3))
    if case.bf16:
        x, dy, dy2 = (t.bfloat16().float() for t in (x, dy, dy2))
    P = make_params(case.mlp, case.qkv_bias, 7)
    scale = HD ** -0.5 if case.sdpa or lay.fblk or not case.qk_scale else case.qk_scale
    cfg = Cfg(H, lay.groups, lay.ids, lay.tpf, lay.tpr, lay.fblk, scale, EPS, case.mlp != "gelu", case.bf16)
    pa, pp, pm = drop_probs(case)
    sa, sp, sm1, sm2 = case_seeds(case)
    masks = {"za": attn_mask_scales(sa, pa, lay.groups, H) if pa > 0 else None,
             "zp": mask_scale(sp, pp, T, D) if pp > 0 else None,
             "zm1": mask_scale(sm1, pm, T, hidden_width(case.mlp)) if pm > 0 else None,
             "zm2": mask_scale(sm2, pm, T, D) if pm > 0 else None}
    draws = None
    if case.dpath:
        draws = tuple(torch.tensor(d, dtype=F64) for d in DRAWS[len(seq_lens(lay.groups))])
    return Inputs(x, dy, dy2, P, cfg, masks, draws)


# ------------------------------------------------------------------------------------------------
# the block


def _linear(h, P, name, R):
    y = h @ R(P[name + ".weight"], "w", bwd=False).t()
    return y + P[name + ".bias"] if name + ".bias" in P else y


def attention(h, P, cfg, za, R, mut=None, pre="attn."):
    """h [T, D] (the bf16 LayerNorm output in the emulation) -> the attention output o [T, D]."""
    T, Dm = h.shape
    nh = cfg.H
    hd = Dm // nh
    qkv = _linear(h, P, pre + "qkv", R)
    q, k, v = (qkv[:, i * Dm:(i + 1) * Dm].reshape(T, nh, hd).transpose(0, 1) for i in range(3))  # [H, T, hd]
    if cfg.ids is not None:
        q, k = orc.apply_rope_qk(q[None], k[None], cfg.ids, cfg.tpf, cfg.tpr)
        q, k = q[0], k[0]
    q, k, v = R(q, "qkv"), R(k, "qkv"), R(v, "qkv")
    scale = hd ** -0.5 if mut == "M8" else cfg.scale
    outs, t0 = [], 0
    for si, ln in enumerate(seq_lens(cfg.groups)):
        s = (q[:, t0:t0 + ln] @ k[:, t0:t0 + ln].transpose(-1, -2)) * scale
        if cfg.fblk:
            f = torch.arange(ln) // cfg.fblk
            s = s.masked_fill(f[None, :] > f[:, None], float("-inf"))
        p = torch.softmax(s, -1)
        if za is not None:
            p = p * za[si]
        outs.append((R(p, "p") @ v[:, t0:t0 + ln]).transpose(0, 1).reshape(ln, Dm))
        t0 += ln
    return R(torch.cat(outs, 0), "o")


def mlp_hidden(h, P, cfg, zm1, R, pre="mlp."):
    """h -> (the output Linear's input, that Linear's name)."""
    if cfg.swiglu:
        x1, x2 = R(_linear(h, P, pre + "fc1", R), "pre"), R(_linear(h, P, pre + "fc2", R), "pre")
        return R(F.silu(x1) * x2, "act"), pre + "fc3"
    act = R(F.gelu(R(_linear(h, P, pre + "fc1", R), "pre")), "act")
    if zm1 is not None:
        act = R(act * zm1, "act")
    return act, pre + "fc2"


def branch_out(inp, P, name, resid, z, factor, R, cfg, mut=None, z_bwd=None, stale=None, detach_resid=False):
    """resid + factor * z * (inp W^T + b): dropout mask z (z_bwd in the backward), then the DropPath row
    factors; each product rounded as the kernels' bf16(bf16(y) * z)."""
    w = R(P[name + ".weight"], "w", bwd=False)
    y = _StaleW.apply(inp, w, stale) if mut == "M7" and stale is not None else inp @ w.t()
    b = P.get(name + ".bias")
    outside = mut == "M1" and (z is not None or factor is not None)
    if b is not None and not outside:
        y = y + b
    if z is not None or factor is not None:
        y = R(y, "branch")
        if z is not None:
            y = R(_Mask.apply(y, z, z if z_bwd is None else z_bwd), "branch")
        if factor is not None:
            y = R(y * factor[:, None], "branch")
    y = R(y, "grad", fwd=False)
    if b is not None and outside:
        y = y + b
    out = (resid.detach() if detach_resid else resid) + y if resid is not None else y
    return R(out, "resid") if cfg.bf16 and resid is not None else out


def row_factors(draws, groups, mut=None):
    """(attention, MLP) per-token DropPath factors: each sequence's draw repeated over its tokens."""
    if draws is None:
        return None, None
    lens = torch.tensor(seq_lens(groups))
    if mut == "M3":
        lens = lens.roll(1)
    da, dm = draws
    if mut == "M2":
        dm = da
    return da.repeat_interleave(lens), dm.repeat_interleave(lens)


def block_graph(x, P, cfg, masks=None, draws=None, R=None, mut=None, stale=None):
    """x f64 [T, D] (in a graph) -> y. P: f64 parameters by the Block's state-dict names."""
    R = R or make_hook(None)
    m = masks or {}
    fa, fm = row_factors(draws, cfg.groups, mut)
    if cfg.bf16:
        x = R(x, "resid", fwd=False)  # bf16 dx
    ln1 = R(F.layer_norm(x, x.shape[1:], P["norm1.weight"], P["norm1.bias"], cfg.eps), "ln")
    o = attention(ln1, P, cfg, m.get("za"), R, mut)
    x_mid = branch_out(o, P, "attn.proj", x, m.get("zp"), fa, R, cfg, mut)
    ln2 = R(F.layer_norm(x_mid, x.shape[1:], P["norm2.weight"], P["norm2.bias"], cfg.eps), "ln")
    hidden, out_name = mlp_hidden(ln2, P, cfg, m.get("zm1"), R)
    zm2 = m.get("zm2")
    if mut == "M4" and zm2 is not None:
        zm2 = m["zm1"][:, :zm2.shape[1]]  # the first seed's mask on the output's columns
    z_bwd = m.get("zp") if mut == "M5" and zm2 is not None else None
    return branch_out(hidden, P, out_name, x_mid, zm2, fm, R, cfg, mut, z_bwd=z_bwd, stale=stale,
                      detach_resid=mut == "M6")


def _leaf(t):
    return t.detach().to(F64).clone().requires_grad_(True)


def run_graph(fn, x, dys, P):
    """fn(x leaf, P leaves) -> y; backward once per dy in dys, gradients summed. Returns {"y", "dx", "d<p>"}."""
    xl = _leaf(x)
    Pl = {k: _leaf(v) for k, v in P.items()}
    y = fn(xl, Pl)
    out = {"y": y.detach()}
    if dys:
        for i, dy in enumerate(dys):
            y.backward(dy.to(F64), retain_graph=i + 1 < len(dys))
        out["dx"] = xl.grad
        out.update({"d" + k: v.grad for k, v in Pl.items()})
    return out


@functools.lru_cache(None)
def run_case(name, emul=None, mut=None):
    """Reference (emul None), emulation ("all" / "gemm") or mutant of a matrix case."""
    case, inp = CASES[name], inputs(name)
    R = make_hook(emul)
    stale = inp.dy2.to(F64) if mut == "M7" else None
    return run_graph(lambda x, P: block_graph(x, P, inp.cfg, inp.masks, inp.draws, R, mut, stale), inp.x,
                     () if case.fwd_only else (inp.dy,), inp.P)


def mutant_active(mut, name):
    case, lay = CASES[name], layout(CASES[name].layout)
    pa, pp, pm = drop_probs(case)
    return {"M1": case.dpath or pp > 0, "M2": case.dpath, "M3": case.dpath and len(set(seq_lens(lay.groups))) > 1,
            "M4": pm > 0, "M5": pm > 0 and not case.fwd_only, "M6": not case.fwd_only, "M7": not case.fwd_only,
            "M8": bool(case.qk_scale) and not case.sdpa and not lay.fblk}[mut]


MUTANTS = ("M1", "M2", "M3", "M4", "M5", "M6", "M7", "M8")


# ------------------------------------------------------------------------------------------------
# two stacked blocks, repeated backward passes, standalone modules


@functools.lru_cache(None)
def run_chain(emul=None, grad_factor=1.0):
    """Two stacked blocks (case 1's layout and inputs, parameters "0.*" and "1.*"); grad_factor scales the
    gradient between the blocks (the in-place hook of the stale-twin case)."""
    inp = inputs("c01_gelu_f32")
    P = {f"{i}.{k}": v for i in range(2) for k, v in make_params("gelu", True, 7 + i).items()}
    R = make_hook(emul)

    def fn(x, Pl):
        for i in range(2):
            x = block_graph(x, {k[2:]: v for k, v in Pl.items() if k[0] == str(i)}, inp.cfg, R=R)
            if i == 0 and grad_factor != 1.0:
                x = _ScaleGrad.apply(x, grad_factor)
        return x

    return run_graph(fn, inp.x, (inp.dy,), P)


@functools.lru_cache(None)
def run_accumulate(emul=None):
    """Case 1 with two backward passes (dy, then dy2) into the same gradients."""
    inp = inputs("c01_gelu_f32")
    R = make_hook(emul)
    return run_graph(lambda x, P: block_graph(x, P, inp.cfg, R=R), inp.x, (inp.dy, inp.dy2), inp.P)


# standalone modules (functions.run_sublayer): name -> (kind, layout, options)
SUBLAYERS = {
    "rope_attn_projdrop": dict(kind="attn", layout="L1", sdpa=True, proj_drop=0.15, qk_scale=None),
    "attn_nosdpa": dict(kind="attn", layout="L2", sdpa=False, proj_drop=0.0, qk_scale=0.2),
    "mlp_drop": dict(kind="mlp", layout="L1", mlp="gelu", drop=0.15),
    "swiglu": dict(kind="mlp", layout="L1", mlp="swiglu_wide", drop=0.0),
}


@functools.lru_cache(None)
def sublayer_inputs(name):
    """(x, dy, P without the block prefix, cfg, masks) of a standalone module; x f32, cast to bf16 by the module."""
    s = SUBLAYERS[name]
    lay = layout(s["layout"])
    T = sum(n * ln for n, ln in lay.groups)
    g = torch.Generator().manual_seed(2000 + sum(map(ord, name)))
    x, dy = torch.randn(T, D, generator=g), torch.randn(T, D, generator=g)
    it = iter(SEEDS)
    if s["kind"] == "attn":
        full = make_params("gelu", True, 17)
        P = {k[5:]: v for k, v in full.items() if k.startswith("attn.")}
        scale = HD ** -0.5 if s["sdpa"] or not s["qk_scale"] else s["qk_scale"]
        cfg = Cfg(H, lay.groups, lay.ids, lay.tpf, lay.tpr, lay.fblk, scale, EPS, False, False)
        pp = s["proj_drop"]
        pa = pp if s["sdpa"] else 0.0  # SDPA's dropout_p is the proj_drop probability
        sa = next(it) if pa > 0 else 0
        sp = next(it) if pp > 0 else 0
        masks = {"za": attn_mask_scales(sa, pa, lay.groups, H) if pa > 0 else None,
                 "z_out": mask_scale(sp, pp, T, D) if pp > 0 else None}
    else:
        full = make_params(s["mlp"], True, 19)
        P = {k[4:]: v for k, v in full.items() if k.startswith("mlp.")}
        cfg = Cfg(H, lay.groups, None, 1, 1, 0, 0.0, EPS, s["mlp"] != "gelu", False)
        pm = s["drop"]
        sm1, sm2 = (next(it), next(it)) if pm > 0 else (0, 0)
        masks = {"zm1": mask_scale(sm1, pm, T, hidden_width(s["mlp"])) if pm > 0 else None,
                 "z_out": mask_scale(sm2, pm, T, D) if pm > 0 else None}
    return x, dy, P, cfg, masks


@functools.lru_cache(None)
def run_sublayer(name, emul=None):
    """The matching piece of the reference: bf16 input cast ("ln": the module's GEMM operand), attention + proj
    or the MLP, the output dropout; f32 output."""
    x, dy, P, cfg, masks = sublayer_inputs(name)
    R = make_hook(emul)

    def fn(xl, Pl):
        h = R(xl, "ln")
        if SUBLAYERS[name]["kind"] == "attn":
            inp, out_name = attention(h, Pl, cfg, masks["za"], R, pre=""), "proj"
        else:
            inp, out_name = mlp_hidden(h, Pl, cfg, masks["zm1"], R, pre="")
        return branch_out(inp, Pl, out_name, None, masks["z_out"], None, R, cfg)

    return run_graph(fn, x, (dy,), P)


# ------------------------------------------------------------------------------------------------
# error measure


def row_err(got, ref):
    """e_r of every row (a vector is one row)."""
    got, ref = got.detach().to(F64).cpu(), ref.detach().to(F64).cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if ref.dim() == 1:
        got, ref = got[None], ref[None]
    got, ref = got.reshape(got.shape[0], -1), ref.reshape(ref.shape[0], -1)
    den = torch.maximum(ref.norm(dim=1), ref.norm() / math.sqrt(ref.shape[0]))
    return (got - ref).norm(dim=1) / den.clamp_min(1e-300)


def yardstick(ref, emu):
    """E(t) per tensor."""
    return {k: max(float(row_err(emu[k], ref[k]).max()), E_FLOOR) for k in ref}


def ratios(got, ref, E):
    """max_r e_r(got) / E(t) per tensor."""
    out = {}
    for k in ref:
        e = float(row_err(got[k], ref[k]).max())
        out[k] = e / E[k]
    return out


def check(got, ref, emu, label, c=None):
    """Assert e_r(got) <= c E(t) on every row of every tensor; prints the ratios. Returns the largest."""
    c = C if c is None else c
    E = yardstick(ref, emu)
    r = ratios(got, ref, E)
    worst = max(r, key=r.get)
    print(f"{label}: worst {worst} {r[worst]:.3f} x E | " + " ".join(f"{k}={v:.2f}" for k, v in r.items()))
    bad = {k: (round(v, 3), f"E={E[k]:.2e}") for k, v in r.items() if not v <= c}
    assert not bad, f"{label}: e_r > {c} E: {bad}"
    return r[worst]

