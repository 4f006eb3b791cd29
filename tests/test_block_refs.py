"""CPU checks of tests/block_refs.py: the float64 block reference reproduces the reference project's recorded
fixtures, the bf16 emulation's two hook placements agree within the bound the HIP path is held to, and every
mutant of the reference breaks that bound in every case where it is active, with a margin."""

import os

import pytest
import torch

import block_refs as br

GOLD = os.path.join(os.path.dirname(__file__), "golden")

# The fixtures are the reference project's own fp32 CPU run; the float64 reference differs from them by that
# run's rounding: about 2^-24 = 6e-8 per operation, accumulated over reductions of up to 4 D = 512 terms and the
# ten or so operations of a block. Measured per-row errors e_r (block_refs.row_err) over the five fixtures: at
# most 3.1e-7 on y, 3.2e-7 on dx and 9.8e-7 (dattn.qkv.weight of block_pred.pt) on the parameter gradients, 4
# to 16 x 2^-24. The bound leaves a factor 4 over the largest for another BLAS's summation order; a composition
# error moves a row by parts in a hundred, not in a million.
FIXTURE_TOL = 4e-6


@pytest.mark.parametrize("fixture", ["block_enc.pt", "block_pred.pt", "block_swiglu.pt", "block_droppath.pt",
                                     "block_swiglu_dp.pt"])
def test_reference_reproduces_fixture(fixture):
    """block_graph in float64 vs the recorded y, gx and gparams, per row, with the fixture's mask -> ids
    mapping (square grid: tokens_per_frame = grid^2, tokens_per_row = grid) and its drop-path draws."""
    g = torch.load(os.path.join(GOLD, fixture), weights_only=True)
    c = g["cfg"]
    B, N, Dm = g["x"].shape
    cfg = br.Cfg(c["heads"], ((B, N),), g["mask"].reshape(-1).long(), c["grid"] ** 2, c["grid"], 0,
                 (Dm // c["heads"]) ** -0.5, 1e-6, "mlp.fc3.weight" in g["state"], False)
    draws = tuple(d.double() for d in g["draws"]) if g.get("draws") else None
    out = br.run_graph(lambda x, P: br.block_graph(x, P, cfg, draws=draws), g["x"].reshape(B * N, Dm),
                       (g["gy"].reshape(B * N, Dm),), g["state"])
    exp = {"y": g["y"].reshape(B * N, Dm), "dx": g["gx"].reshape(B * N, Dm)}
    exp.update({"d" + k: v for k, v in g["gparams"].items()})
    assert set(exp) == set(out)
    errs = {k: float(br.row_err(exp[k], out[k]).max()) for k in exp}
    print(fixture, " ".join(f"{k}={v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) < FIXTURE_TOL, errs


def _emulation_pairs():
    for c in br.MATRIX:
        yield c.name, lambda e, n=c.name: br.run_case(n, e)
    yield "chain", br.run_chain
    yield "chain_halved", lambda e: br.run_chain(e, 0.5)
    yield "accumulate", br.run_accumulate
    for n in br.SUBLAYERS:
        yield "sub_" + n, lambda e, n=n: br.run_sublayer(n, e)


@pytest.mark.parametrize("name,run", list(_emulation_pairs()), ids=[n for n, _ in _emulation_pairs()])
def test_emulation_placements_agree(name, run):
    """The emulation with its hook at the GEMM operands only stays within C * E of the reference, E from the
    emulation with the hook at every point: C is no tighter than the yardstick's own ambiguity."""
    ref, emu, alt = run(None), run("all"), run("gemm")
    E = br.yardstick(ref, emu)
    assert all(v < 0.1 for v in E.values()), E  # bf16 rounding, not a broken graph
    print(name, "E:", " ".join(f"{k}={v:.1e}" for k, v in E.items()))
    br.check(alt, ref, emu, name + " gemm-only placement")


# Every mutant must miss the bound by this factor on at least one tensor, in every case where it is active. The
# smallest margins measured (max_t e_r / (C E), C = 1.5): M1 10.0, M2 104, M3 112, M4 65, M5 134, M6 77, M7 123,
# M8 42; the test prints them per case.
MUTANT_MARGIN = 4.0


@pytest.mark.parametrize("mut", br.MUTANTS)
def test_mutants_are_rejected(mut):
    active = [c.name for c in br.MATRIX if br.mutant_active(mut, c.name)]
    assert active, mut
    margins = {}
    for name in active:
        ref, emu = br.run_case(name), br.run_case(name, "all")
        r = br.ratios(br.run_case(name, None, mut), ref, br.yardstick(ref, emu))
        margins[name] = max(r.values()) / br.C
    print(mut, "min margin %.1f:" % min(margins.values()), " ".join(f"{k}={v:.1f}" for k, v in margins.items()))
    assert min(margins.values()) >= MUTANT_MARGIN, margins


def test_mutants_are_inert_where_inactive():
    """A mutant outside its active set is the reference itself (so `mutant_active` names the whole set)."""
    for mut in br.MUTANTS:
        for c in br.MATRIX:
            if not br.mutant_active(mut, c.name):
                ref, got = br.run_case(c.name), br.run_case(c.name, None, mut)
                assert all(torch.equal(ref[k], got[k]) for k in ref), (mut, c.name)
