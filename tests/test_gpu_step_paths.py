"""Every route of the train step (train.JEPATrainer.forward_loss / compute_grads / apply_update over
VisionTransformer.forward_ragged and the predictor's forward_ragged) against the float64 step of
tests/step_refs.py, per row of every tensor, under the bound C_STEP * E(t) measured against the bf16 emulation
(step_refs' docstring). The models come from the project's constructors (1-D parameters and qkv weights perturbed
by step_refs.perturb_) inside the wrappers, with init_opt and JEPATrainer, as the apps build them; the reference
is evaluated at the weights read back from the trainer."""

import copy
import functools

import pytest
import torch
import torch.nn as nn

import step_refs as sr

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64


def _trainer(case):
    from vjepa2_amd.predictor import vit_predictor
    from vjepa2_amd.train import JEPATrainer, init_opt
    from vjepa2_amd.vision_transformer import VisionTransformer
    from vjepa2_amd.wrappers import MultiSeqWrapper, PredictorMultiSeqWrapper

    torch.manual_seed(239)
    enc = VisionTransformer(img_size=sr.IMG, patch_size=sr.PATCH, num_frames=sr.FRAMES, tubelet_size=sr.TUB,
                            embed_dim=sr.ED, depth=sr.EDEPTH, num_heads=sr.EH, mlp_ratio=4, qkv_bias=True,
                            use_rope=case.rope, use_silu=case.swiglu, wide_silu=True, use_sdpa=True,
                            norm_layer=lambda d: nn.LayerNorm(d, eps=1e-6))
    pred = vit_predictor(img_size=sr.IMG, use_mask_tokens=True, patch_size=sr.PATCH, num_frames=sr.FRAMES,
                         tubelet_size=sr.TUB, embed_dim=sr.ED, predictor_embed_dim=sr.PD, depth=sr.PDEPTH,
                         num_heads=sr.PH, num_mask_tokens=sr.NTOK, zero_init_mask_tokens=False, use_rope=case.rope,
                         use_silu=case.swiglu, wide_silu=True, use_sdpa=True)
    assert case.swiglu == hasattr(enc.blocks[0].mlp, "fc3") == hasattr(pred.predictor_blocks[0].mlp, "fc3")
    sr.perturb_(enc.state_dict(), 6)  # the state dict's tensors share the parameters' storage
    sr.perturb_(pred.state_dict(), 7)
    enc, pred = MultiSeqWrapper(enc).to(DEV), PredictorMultiSeqWrapper(pred).to(DEV)
    tgt = copy.deepcopy(enc)
    opt, _, _, _ = init_opt(enc, pred, iterations_per_epoch=10, start_lr=sr.LR1, ref_lr=sr.LR1, warmup=0, num_epochs=1,
                            wd=sr.WD1, final_wd=sr.WD1, mixed_precision=case.mixed)
    for g in opt.param_groups:
        g["lr"] = sr.LR1
        if not g.get("WD_exclude", False):
            g["weight_decay"] = sr.WD1
    return JEPATrainer(enc, pred, tgt, opt, mixed_precision=case.mixed, loss_exp=case.loss_exp, fp8_target=case.fp8)


def _state(mod):
    torch.cuda.synchronize()
    return {k: v.detach().float().cpu().clone() for k, v in mod.state_dict().items()}


def _args(groups):
    return ([c.to(DEV) for c, _, _ in groups], [[m.to(DEV) for m in me] for _, me, _ in groups],
            [[m.to(DEV) for m in mp] for _, _, mp in groups])


def _grads(tr):
    torch.cuda.synchronize()
    out = {}
    for tag, mod in (("e.", tr.enc), ("p.", tr.pred)):
        for k, p in mod.named_parameters():
            if p.grad is not None:
                out[tag + k] = p.grad.detach().float().cpu().clone()
    return out


class _Spy:
    """Records ops.jepa_loss's (zp, dz) per call and functions.wgrad_buf's accumulate flag per write."""

    def __enter__(self):
        from vjepa2_amd import functions as fn
        from vjepa2_amd import ops

        self.fn, self.ops, self.loss_calls, self.acc = fn, ops, [], []
        self.real = (ops.jepa_loss, fn.wgrad_buf)

        def jepa_loss(z, *a, **kw):
            res = self.real[0](z, *a, **kw)
            self.loss_calls.append((z.detach().clone(), res[1].detach().clone()))
            return res

        def wgrad_buf(p):
            buf, acc = self.real[1](p)
            self.acc.append(acc)
            return buf, acc

        ops.jepa_loss, fn.wgrad_buf = jepa_loss, wgrad_buf
        return self

    def __exit__(self, *exc):
        self.ops.jepa_loss, self.fn.wgrad_buf = self.real
        return False


def _hip_step(tr, inp):
    """The HIP path's tensors of one step on `inp` (step_refs.run_inputs' keys) and what the spies saw."""
    from vjepa2_amd.functions import join_wgrad_stream

    clips, me, mp = _args(inp.groups)
    npairs = sum(len(m) for m in me)
    tr.opt.zero_grad()
    got = {}
    if tr.fp8_target:  # forward only
        with _Spy() as spy:
            loss, _, _ = tr.forward_loss(clips[0], me[0], mp[0], npairs=npairs)
        (zp, dz), = spy.loss_calls
        got.update(loss=loss.detach().float().cpu().reshape(1), zp0=zp.float().cpu(), dz0=dz.float().cpu())
        return got, spy
    for i in range(len(clips)):  # the linearised pass: compute_grads' loop with a seeded dy in dz's place
        _, zp, _ = tr.forward_loss(clips[i], me[i], mp[i], mask_index=i, npairs=npairs)
        assert zp.dtype == torch.bfloat16
        zp.backward(inp.dys[i].to(DEV, torch.bfloat16))
    join_wgrad_stream()
    for a in tr.opt.arenas:
        a.finalize_grads()
    got.update({"lin." + k: v for k, v in _grads(tr).items()})
    tr.opt.zero_grad()
    with _Spy() as spy:
        loss = tr.compute_grads(clips, me, mp)
    got.update({"g." + k: v for k, v in _grads(tr).items()})
    got["loss"] = loss.detach().float().cpu().reshape(1)
    assert len(spy.loss_calls) == len(clips)
    l1 = tr.loss_exp == 1
    for gi, (zp, dz) in enumerate(spy.loss_calls):
        got[f"zp{gi}"], got[("_dz" if l1 else "dz") + str(gi)] = zp.float().cpu(), dz.float().cpu()
    return got, spy


def _compare(case, tr, inp, label):
    """One step on the HIP path vs the float64 step at the same weights. Returns (largest ratio, its tensor)."""
    got, spy = _hip_step(tr, inp)
    n = len(inp.groups)
    dz_in = [got[f"_dz{gi}"].to(F64) for gi in range(n)] if case.loss_exp == 1 else None
    ref = sr.run_inputs(case, inp, None, None, dz_in)
    emu = sr.run_inputs(case, inp, "all", None, dz_in)
    for k in [k for k in got if k[:4] in ("lin.", "g.e.", "g.p.") and k not in ref]:
        # unused mask tokens (and anything frozen): no gradient where the reference has none
        assert float(got.pop(k).abs().max()) == 0.0, f"{label}: {k} has a gradient, the reference has none"
    worst = sr.check(got, ref, emu, label, case)
    bound = sr.loss_bound(ref)
    dl = abs(float(got["loss"]) - float(ref["loss"]))
    print(f"{label}: loss {float(got['loss']):.6f} vs {float(ref['loss']):.6f}: {dl:.2e} of the {bound:.2e} allowed")
    assert dl <= bound
    if case.loss_exp == 1:
        share, err = sr.l1_dz_err(case, inp, [got[f"zp{gi}"] for gi in range(n)],
                                  [got[f"_dz{gi}"] for gi in range(n)], ref, emu)
        print(f"{label}: tie band holds {share:.4f} of dz's elements; dz error outside it {err:.2e}")
        assert share <= sr.TIE_CAP and err <= sr.L1_DZ_TOL
    tokens = [i for i in range(sr.NTOK) if f"g.p.mask_tokens.{i}" in got]
    info = dict(ctx_bf16=tr.ctx_bf16_residual, tgt_bf16=tr.target_bf16_residual and not tr.fp8_target,
                fp8=tr.fp8_target, groups=getattr(tr, "_groups", None), tokens=tokens, acc=list(spy.acc), worst=worst)
    return info


@functools.lru_cache(None)
def hip_case(name):
    case = sr.CASES[name]
    first = sr.CASES["s01_mixed"] if case.second else case
    tr = _trainer(first)
    groups, dys = sr.make_groups(first, 1000 + sum(map(ord, first.name)))
    info0 = None
    if case.second:
        tok0 = [t.detach().cpu().clone() for t in tr.mask_tokens]
        tr.train_step(*_args(groups), sr.EMA1)
        info0 = dict(ow=[bool(getattr(p, "_vj_ow", False)) for a in tr.opt.arenas[:2] for p in a.params if p.dim() == 2],
                     moved=[not torch.equal(t.detach().cpu(), t0) for t, t0 in zip(tr.mask_tokens, tok0)])
        groups, dys = sr.make_groups(case, 4242)
    inp = sr.Inputs(_state(tr.enc), _state(tr.pred), _state(tr.tgt), groups, dys, None)
    info = _compare(case, tr, inp, name)
    info["first"] = info0
    return info


@pytest.mark.parametrize("name", [c.name for c in sr.MATRIX if not c.second])
def test_step_case(name):
    """s01 - s05, s07: zp per row and the loss from forward_loss, every parameter gradient of the linearised
    backward and of a fresh compute_grads on the true loss (both wrappers), dz; zero or no gradient where the
    reference has none. s08 (fp8 target): forward_loss alone: zp, dz and the loss, against the emulation with
    the documented e4m3 quantiser on the target's QKV / fc1 operands."""
    hip_case(name)


def test_second_step():
    """s06: after one train_step the second step's zp, loss and gradients against the float64 step at the
    weights read back from the arenas (the target at the HIP path's EMA'd weights): stale bf16 shadows or W^T
    copies (mutants S8, S9) would show here, optimizer drift does not."""
    hip_case("s06_second_step")


def test_route_coverage():
    """Each case took the route it is named for."""
    info = {c.name: hip_case(c.name) for c in sr.MATRIX}
    print("\n".join(f"{n}: {i['worst'][0]:.3f} E on {i['worst'][1]}" for n, i in info.items()))
    for c in sr.MATRIX:
        i = info[c.name]
        assert (i["ctx_bf16"], i["tgt_bf16"]) == sr.streams(c), c.name
        assert c.fp8 or i["groups"] == len(c.frames), c.name  # s08 runs forward_loss alone: no group count
        assert i["fp8"] == c.fp8, c.name
        assert c.fp8 or i["tokens"] == list(range(len(c.frames))), (c.name, i["tokens"])
    two = info["s05_two_groups"]["acc"]
    assert not two[0] and two[-1] and True in two and False in two  # group 0 overwrites, group 1 accumulates
    sec = info["s06_second_step"]
    assert all(sec["first"]["ow"]) and sec["first"]["moved"] == [True, False]
    assert not any(sec["acc"]), "the second step's first weight-gradient writes must overwrite (lazy zero)"


def test_update_is_adamw_and_ema_of_its_own_gradients():
    """apply_update after compute_grads: every parameter against float64 AdamW fed the arena's own gradients (the
    reference's grouping, step count 1, grad_scale 1), the target arenas against the EMA of the new parameters,
    every bf16 shadow against p.bfloat16(), the unused mask token and the pos_embeds bit for bit.

    Tolerances from vj_adamw's op sequence in f32 (2^-24 per rounding): p * decay (the product and the rounded
    constant) and the final add are 3 roundings of p's size; the update term u = neg_step * m / (sqrt(v) /
    bc2_sqrt + eps) carries m (2), v (3, halved by the root), the root, two divisions, the eps add and the
    rounded constants: under 16. The EMA t * mom + one_m * p is at most three roundings, of t * mom, one_m * p
    and the sum, with the constants as the kernel receives them (f32 mom, f32 1 - mom)."""
    case = sr.CASES["s03_sincos"]
    tr = _trainer(case)
    groups, _ = sr.make_groups(case, 77)
    before = (_state(tr.enc), _state(tr.pred), _state(tr.tgt))
    tr.compute_grads(*_args(groups))
    grads = _grads(tr)
    unused = "p.mask_tokens.1"
    assert float(grads.pop(unused).abs().max()) == 0.0
    tr.apply_update(sr.EMA1)
    after = (_state(tr.enc), _state(tr.pred), _state(tr.tgt))
    mom = float(torch.tensor(sr.EMA1, dtype=torch.float32))
    one_m = float(torch.tensor(1.0 - mom, dtype=torch.float32))
    ref_e, ref_p, _ = sr.adamw_ema(before[0], before[1], before[2], grads, sr.LR1, sr.WD1, mom)
    u24, worst = 2.0 ** -24, 0.0
    for tag, old, new, ref in (("e.", before[0], after[0], ref_e), ("p.", before[1], after[1], ref_p)):
        for k, r in ref.items():
            if tag + k not in grads:
                assert torch.equal(new[k], old[k]), f"{tag}{k} moved without a gradient"
                continue
            decay = 0.0 if ("bias" in k or r.dim() == 1) else sr.WD1
            u = (r - old[k].to(F64) * (1 - sr.LR1 * decay)).abs()
            tol = u24 * (3 * old[k].to(F64).abs() + 16 * u)
            err = (new[k].to(F64) - r).abs()
            worst = max(worst, float((err / tol.clamp_min(1e-300)).max()))
            assert bool((err <= tol).all()), f"{tag}{k}: {float((err / tol.clamp_min(1e-300)).max()):.2f} x the AdamW bound"
            assert float((new[k] - old[k]).abs().max()) > 0, f"{tag}{k} did not move"
    for k, t_old in before[2].items():
        if k in sr.FROZEN:
            assert torch.equal(after[2][k], t_old), k
            continue
        a, b = t_old.to(F64) * mom, one_m * after[0][k].to(F64)
        tol = u24 * (a.abs() + b.abs() + (a + b).abs())
        assert bool(((after[2][k].to(F64) - (a + b)).abs() <= tol).all()), f"target {k}: not the EMA of the new weights"
    print(f"AdamW: worst {worst:.2f} of the bound")
    torch.cuda.synchronize()
    for a in tr.opt.arenas + tr.tgt_arenas:
        for n, p in zip(a.names, a.params):
            assert torch.equal(p._vj_bf16, p.detach().bfloat16()), f"{a.name}.{n}: bf16 shadow is not p.bfloat16()"
