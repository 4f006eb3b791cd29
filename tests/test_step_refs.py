"""CPU checks of tests/step_refs.py: the float64 step reference reproduces the reference project's recorded
encoder, predictor and train-step fixtures, the bf16 emulation's two hook placements agree within the bound the
HIP path is held to, every mutant of the reference breaks that bound in every case where it is active, with a
margin, and the L1 tie band of s07 stays under its cap for the emulation."""

import os

import pytest
import torch

import block_refs as br
import step_refs as sr

GOLD = os.path.join(os.path.dirname(__file__), "golden")
F64 = torch.float64

# The fixtures are the reference project's own fp32 CPU run, so the float64 graph differs from them by that run's
# rounding: 2^-24 = 6e-8 per operation, accumulated over reductions of up to 1536 terms (the tubelet) and the
# two blocks. Measured per-row errors e_r, the largest per fixture: encoder_rope1 9.5e-7 on the outputs and 1.4e-6
# on the gradients (dblocks.0.attn.qkv.weight), encoder_rope0 8.8e-7 / 1.1e-6, predictor 3.8e-7 on the outputs,
# 5.1e-7 on dz and 1.3e-6 on the gradients; losses[0] of train_steps.pt to 6.8e-8 relative. The bound leaves a
# factor 4 over the largest for another BLAS's summation order; a composition error moves a row by parts in a
# hundred.
FIXTURE_TOL = 6e-6


def _gold(name):
    return torch.load(os.path.join(GOLD, name), weights_only=True)


def _leaf(sd, frozen):
    return {k: v.detach().to(F64).clone().requires_grad_(k != frozen) for k, v in sd.items()}


@pytest.mark.parametrize("rope", [1, 0])
def test_encoder_graph_reproduces_fixture(rope):
    """encoder_graph (all masks packed into one pass) vs the fixture's per-mask calls: outputs per row, the
    all-token output, and every parameter gradient of sum_m (out_m * gy_m).sum()."""
    g = _gold(f"encoder_rope{rope}.pt")
    m = sr.Model(1, None, 2, None, bool(rope), 2, None)
    P = _leaf(g["state"], "pos_embed")
    R = sr.make_hook(None)
    full = sr.encoder_graph(g["x"], P, None, m, R)
    out = sr.encoder_graph(g["x"], P, list(g["masks"]), m, R)
    D = out.shape[1]
    exp = torch.cat([o.reshape(-1, D) for o in g["outs"]])
    out.backward(torch.cat([gy.reshape(-1, D) for gy in g["gys"]]).to(F64))
    errs = {"full": float(br.row_err(g["full"].reshape(-1, D), full).max()), "outs": float(br.row_err(exp, out).max())}
    assert set(g["gparams"]) == {k for k, v in P.items() if v.grad is not None}
    errs.update({"d" + k: float(br.row_err(v, P[k].grad).max()) for k, v in g["gparams"].items()})
    print(f"encoder_rope{rope}", " ".join(f"{k}={v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) < FIXTURE_TOL, errs


def test_predictor_graph_reproduces_fixture():
    """predictor_graph, one pair per call with the fixture's mask_index, vs the recorded outputs, dz and the
    parameter gradients summed over the calls (the unused mask token has none)."""
    g = _gold("predictor.pt")
    m = sr.Model(None, 3, None, 2, True, 2, 2)
    P = _leaf(g["state"], "predictor_pos_embed")
    R, errs = sr.make_hook(None), {}
    for i, (inp, exp, gy) in enumerate(zip(g["ins"], g["outs"], g["gys"])):
        z = inp["z"].to(F64).reshape(-1, inp["z"].shape[-1]).requires_grad_(True)
        o = sr.predictor_graph(z, P, [inp["mx"]], [inp["my"]], m, inp["mask_index"], R)
        o.backward(gy.reshape(o.shape).to(F64))
        errs[f"out{i}"] = float(br.row_err(exp.reshape(o.shape), o).max())
        errs[f"dz{i}"] = float(br.row_err(inp["gz"].reshape(z.shape), z.grad).max())
    assert set(g["gparams"]) == {k for k, v in P.items() if v.grad is not None}
    errs.update({"d" + k: float(br.row_err(v, P[k].grad).max()) for k, v in g["gparams"].items()})
    print("predictor", " ".join(f"{k}={v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) < FIXTURE_TOL, errs


def test_step_graph_reproduces_first_train_step_loss():
    """step_graph (L1 loss, target = the initial encoder) vs losses[0] of the reference's recorded train run."""
    g = _gold("train_steps.pt")
    s = g["samples"][0]
    clips = torch.stack([torch.randn(3, 8, 64, 64, generator=torch.Generator().manual_seed(sd)) for sd in s["clip_seeds"]])
    enc = {k: v.to(F64) for k, v in g["init_encoder"].items()}
    pred = {k: v.to(F64) for k, v in g["init_predictor"].items()}
    m = sr.Model(1, 2, 2, 2, True, 4, 2)
    with torch.no_grad():
        loss = sr.step_graph(enc, pred, enc, [(clips.to(F64), list(s["enc"]), list(s["pred"]))], m, loss_exp=1.0)[0]
    rel = abs(float(loss) - g["losses"][0]) / g["losses"][0]
    print(f"train_steps losses[0]: {float(loss):.9f} vs {g['losses'][0]:.9f} (rel {rel:.1e})")
    assert rel < 1e-6  # one fp32 number: 2^-24 and its accumulation over a mean of 10^4 terms


NAMES = [c.name for c in sr.MATRIX]

# The emulation's own ambiguity: max_t max_r e_r(emulation "gemm") / E(t), measured per case: s01 1.337 (lin.e.
# blocks.1.attn.qkv.bias), s02 1.321, s03 1.444 (lin.e.blocks.1.attn.qkv.weight), s04 1.480 (lin.e.blocks.0.attn.
# proj.weight), s05 1.234, s06 1.279, s07 1.181, s08 0.970 (dz0). The record is the bound: a change of the graph or
# of the inputs that widens the spread past it fails here, and step_refs' docstring quotes it beside C_STEP.
SPREAD = 1.5


@pytest.mark.parametrize("name", NAMES)
def test_emulation_placements_agree(name):
    ref, emu, alt = sr.run(name), sr.run(name, "all"), sr.run(name, "gemm")
    E = br.yardstick(sr.measured(ref, sr.CASES[name]), sr.measured(emu, sr.CASES[name]))
    assert all(v < 0.1 for v in E.values()), E  # bf16 rounding, not a broken graph
    le = {m: abs(float(r["loss"] - ref["loss"])) / float(ref["loss"]) for m, r in (("all", emu), ("gemm", alt))}
    print(name, "E: min %.1e max %.1e" % (min(E.values()), max(E.values())), max(E, key=E.get),
          "loss error all %.2e gemm %.2e" % (le["all"], le["gemm"]))
    sr.check(alt, ref, emu, name + " gemm-only placement", sr.CASES[name], c=SPREAD)
    assert max(le.values()) <= sr.LOSS_E, le  # the record of step_refs.LOSS_E: no placement of any case exceeds it


# Smallest margins measured (max_t e_r / (C_STEP E), C_STEP = 2): S1 46 S2 inf (a gradient on the wrong mask token)
# S3 19.5 S4 113 S5 13.7 S6 75 S7 137 S8 82 S9 400 S10 32 S11 328; the test prints them per case.
MUTANT_MARGIN = 4.0


@pytest.mark.parametrize("mut", sr.MUTANTS)
def test_mutants_are_rejected(mut):
    """Every mutant misses C_STEP E by MUTANT_MARGIN on at least one tensor in every case where it is active."""
    active = [n for n in NAMES if sr.mutant_active(mut, n)]
    assert active, mut
    margins = {}
    for name in active:
        ref, emu, got = sr.run(name), sr.run(name, "all"), sr.run(name, None, mut)
        ref_m, got_m = sr.measured(ref, sr.CASES[name]), sr.measured(got, sr.CASES[name])
        if set(ref_m) != set(got_m):  # a gradient appears or vanishes: a miss by any margin
            margins[name] = (float("inf"), "keys")
            continue
        r = br.ratios(got_m, ref_m, br.yardstick(ref_m, sr.measured(emu, sr.CASES[name])))
        k = max(r, key=r.get)
        margins[name] = (r[k] / sr.C_STEP, k)
        if sr.CASES[name].loss_exp == 1:  # dz is held elementwise: the mutant's own zp and dz against h_ref
            _, err = sr.l1_dz_err(sr.CASES[name], sr.inputs(name), [got["zp0"]], [got["_dz0"]], ref, emu)
            margins[name] = max(margins[name], (err / sr.L1_DZ_TOL, "dz elementwise"))
    low = min(v for v, _ in margins.values())
    print(mut, "min margin %.1f:" % low, " ".join(f"{n}={v:.1f}({k})" for n, (v, k) in margins.items()))
    assert low >= MUTANT_MARGIN, margins


@pytest.mark.parametrize("mut", ["S1", "S9", "S11"])
def test_loss_alone_rejects(mut):
    """With the loss the only thing looked at, the wrong weighting (S1), the stale weights (S9) and the wrong loss
    scale (S11) miss loss_bound in every case where they are active. Smallest |dloss| / bound measured: S1 2.1
    (s02; 4.7 ... 43 elsewhere), S9 885, S11 9090."""
    over = {}
    for name in NAMES:
        if sr.mutant_active(mut, name):
            ref = sr.run(name)
            over[name] = abs(float(sr.run(name, None, mut)["loss"] - ref["loss"])) / sr.loss_bound(ref)
    print(mut, "loss alone, |dloss| / bound:", " ".join(f"{n}={v:.1f}" for n, v in over.items()))
    assert over and min(over.values()) > 1.0, over


def test_mutants_are_inert_where_inactive():
    for mut in ("S2", "S6", "S7", "S11"):
        ref, got = sr.run("s01_mixed"), sr.run("s01_mixed", None, mut)
        assert all(torch.equal(ref[k], got[k]) for k in sr.measured(ref, sr.CASES["s01_mixed"])), mut


def test_l1_tie_band_is_under_its_cap():
    """s07: the share of dz's elements whose sign the rounding of zp may decide stays under TIE_CAP for both
    emulations' zp, and outside the band their dz is sign(zp - h_ref) / (rows D npairs) to bf16 rounding."""
    name = "s07_l1"
    case, inp, ref, emu = sr.CASES[name], sr.inputs(name), sr.run(name), sr.run(name, "all")
    for mode in ("all", "gemm"):
        got = sr.run(name, mode)
        share, err = sr.l1_dz_err(case, inp, [got["zp0"]], [got["_dz0"]], ref, emu)
        print(f"{name} {mode}: tie band holds {share:.4f} of dz's elements; dz error outside it {err:.2e}")
        assert share <= sr.TIE_CAP and err <= sr.L1_DZ_TOL
