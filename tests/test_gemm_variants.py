"""CPU: the case table of the strided GEMM tests (tests/test_gpu_gemm_strided.py) names every kernel
variant the 256-row GEMM's plan can pick.

STRIDED_CASES is shared with the GPU test: one row per (tile shape, waves, main-loop form) with the
operand layouts it runs, the shape and the VJ_GEMM_* knobs that force it, and the plan it declares. The GPU
test asserts that plan before each launch; the sweep here asserts that vj_gemm256_plan returns no (layout,
rows, cols, waves, form) the table lacks, so a new tile shape or main-loop form in plan256 fails this test
until the strided test gains a row for it. Host logic only (no device work)."""

import ctypes
import itertools
from collections import namedtuple

# operand layouts: (A K-major, B K-major); the name gives the major dimension of A then of B
LAYOUTS = {"KK": (1, 1), "KM": (1, 0), "MK": (0, 1), "MM": (0, 0)}
PLAN_KNOBS = ("VJ_GEMM_STG", "VJ_GEMM_STG64", "VJ_GEMM_BM192", "VJ_GEMM_2W", "VJ_GEMM_2W192")
ALL_KNOBS = PLAN_KNOBS + ("VJ_GEMM_GROUP", "VJ_GEMM_PXCD")
# vj_gemm_bf16's epilogues and vj_qkv_rope_gemm's (include/vjepa_hip.h)
EPI_BF16, EPI_F32, EPI_F32_RESID, EPI_GELU, EPI_GELU_BWD, EPI_ROPE, EPI_BF16_RESID = 0, 1, 2, 3, 4, 5, 7
DISPATCH_EPIS = (EPI_BF16, EPI_F32, EPI_F32_RESID, EPI_GELU, EPI_GELU_BWD, EPI_ROPE, EPI_BF16_RESID)

# knobs: per layout (besides VJ_GEMM_PXCD=1, which every strided case sets); plan: (rows, cols, waves, form),
# None = the 128 x 128 kernel of vj_gemm.hip (M < 1024)
Case = namedtuple("Case", "name M N K knobs plan")
_ALL4 = ("KK", "KM", "MK", "MM")
STRIDED_CASES = [
    Case("one_tile_256x256", 1032, 480, 72, {lay: {"VJ_GEMM_STG": "0", "VJ_GEMM_BM192": "0"} for lay in _ALL4},
         (256, 256, 8, 0)),
    Case("staggered_form1", 1032, 480, 96,
         {"KK": {"VJ_GEMM_STG": "1", "VJ_GEMM_STG64": "0", "VJ_GEMM_BM192": "0"}}, (256, 256, 8, 1)),
    Case("s64", 1032, 480, 192, {"KK": {"VJ_GEMM_BM192": "0"}}, (256, 256, 8, 2)),
    Case("tile_192x256", 1032, 480, 72, {"KK": {"VJ_GEMM_BM192": "1"}}, (192, 256, 8, 0)),
    Case("staged_256x128", 1032, 264, 72, {"KK": {"VJ_GEMM_2W": "0"}, "KM": {}, "MK": {}, "MM": {}},
         (256, 128, 8, 0)),
    Case("two_wg_192x128", 1032, 264, 72, {"KK": {}}, (192, 128, 4, 0)),
    Case("two_wg_256x128", 1032, 264, 40, {"KK": {"VJ_GEMM_2W192": "0"}}, (256, 128, 4, 0)),
    Case("tile_128x128", 264, 136, 72, {lay: {} for lay in _ALL4}, None),
]


def expected_plan(case, epi):
    """(rows, cols, waves, form) the case declares for an epilogue: the RoPE epilogue keeps 256-row tiles on
    the two-workgroup kernel (its table does not fit beside two 192 x 128 workgroups' stages)."""
    if case.plan is None:
        return None
    rows, cols, waves, form = case.plan
    if epi == EPI_ROPE and waves == 4:
        rows = 256
    return rows, cols, waves, form


def covered_variants(cases=None):
    """Every (layout, rows, cols, waves, form) a table row declares (the RoPE epilogue's 256-row form of the
    two-workgroup kernel counts through its own row, not through the 192-row one's RoPE launch)."""
    return {(lay,) + c.plan for c in (STRIDED_CASES if cases is None else cases) if c.plan for lay in c.knobs}


def plan(M, N, K, layout, epi, cus):
    """vj_gemm256_plan under the current environment: (rows, cols, waves, form), None where it declines."""
    from vjepa2_amd import _lib

    ak, bk = LAYOUTS[layout]
    out = (ctypes.c_int * 6)(*([-1] * 6))
    rc = _lib.load().vj_gemm256_plan(M, N, K, ak, bk, epi, cus, out)
    if rc == 3:  # VJ_ERR_UNSUPPORTED
        return None
    assert rc == 0, _lib.last_error()
    return tuple(out[:4])


def set_knobs(monkeypatch, knobs):
    """Exactly `knobs` of the VJ_GEMM_* environment (the library reads it per call)."""
    for k in ALL_KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)


def planned_variants(monkeypatch, Ms=(1032, 2100, 11712), Ns=(264, 480, 1024), Ks=(40, 72, 96, 192)):
    """The distinct (layout, rows, cols, waves, form) of vj_gemm256_plan(cus=256) over the shapes, the four
    layouts, the seven dispatch epilogues and every {unset, 0, 1} setting of the five plan knobs."""
    seen = set()
    probs = [(M, N, K, lay, epi) for M in Ms for N in Ns for K in Ks for lay in LAYOUTS for epi in DISPATCH_EPIS]
    for vals in itertools.product((None, "0", "1"), repeat=len(PLAN_KNOBS)):
        set_knobs(monkeypatch, {k: v for k, v in zip(PLAN_KNOBS, vals) if v is not None})
        for M, N, K, lay, epi in probs:
            p = plan(M, N, K, lay, epi, 256)
            assert p is not None, (M, N, K, lay, epi, vals)
            seen.add((lay,) + p)
    return seen


def test_strided_case_table_declares_the_plans(monkeypatch):
    """Each row's knobs give the plan it declares, for every epilogue, sized for 256 CUs (the GPU test asserts
    the same for its device's CU count before it launches)."""
    for c in STRIDED_CASES:
        for lay, knobs in c.knobs.items():
            set_knobs(monkeypatch, dict(knobs, VJ_GEMM_PXCD="1"))
            for epi in DISPATCH_EPIS:
                got = plan(c.M, c.N, c.K, lay, epi, 256)
                if c.plan is None:
                    assert c.M < 1024, c.name  # vj_gemm_bf16 offers the 256-row kernel M >= 1024 only
                else:
                    assert got == expected_plan(c, epi), (c.name, lay, epi, got)
    # the narrow RoPE GEMM keeps 256 x 128 tiles on 4 waves whatever VJ_GEMM_2W192 says
    for w192 in ({}, {"VJ_GEMM_2W192": "0"}, {"VJ_GEMM_2W192": "1"}):
        set_knobs(monkeypatch, dict(w192, VJ_GEMM_PXCD="1"))
        assert plan(1032, 264, 72, "KK", EPI_ROPE, 256) == (256, 128, 4, 0), w192


def test_strided_case_table_covers_every_planned_variant(monkeypatch):
    """No (layout, tile rows, tile columns, waves, main-loop form) of the plan lacks a row of the strided
    case table; and the check has teeth: without any one 256-row row of the table it fails."""
    seen = planned_variants(monkeypatch)
    missing = seen - covered_variants()
    assert not missing, f"vj_gemm256_plan picks variants the strided case table does not run: {sorted(missing)}"
    for drop in STRIDED_CASES:
        if drop.plan is not None:
            rest = [c for c in STRIDED_CASES if c is not drop]
            assert seen - covered_variants(rest), f"row {drop.name} adds no variant of its own"
