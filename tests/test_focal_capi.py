"""CPU: vj_focal validates its arguments before any device work (no GPU here), with a message for each
refusal, in the style of test_xent_capi.py; ops.focal has no CPU path and checks its bookkeeping on the host."""

import ctypes

import pytest


def _call(lib, B=3, nseg=2, C=(11, 7), ld=(11, 9), lddl=(11, 7), logits=(1, 1), labels=(1, 1), valid=None,
          dlogits=None, tp=(1, 1), fn=(1, 1), arrays=(), k=5, loss_kind=1, loss=1, row_loss=1, hit=1):
    """Non-null device pointers are never dereferenced on a refused call: any non-zero address stands in. The
    per-segment arrays are real host arrays (the entry point reads them); `arrays` names those passed as NULL."""
    n = max(1, min(nseg, 3))
    p = lambda v: ctypes.c_void_p(0x1000 * v) if v else None  # noqa: E731

    def ptrs(name, vals):
        if name in arrays or vals is None:
            return None
        return (ctypes.c_void_p * n)(*[0x1000 * v if v else None for v in vals[:n]])

    def nums(name, ty, vals):
        return None if name in arrays else (ty * n)(*vals[:n])

    return lib.vj_focal(B, nseg, ptrs("logits", logits), nums("ld", ctypes.c_long, ld), nums("C", ctypes.c_int, C),
                        ptrs("labels", labels), 1, ptrs("valid", valid), ptrs("dlogits", dlogits),
                        nums("lddl", ctypes.c_long, lddl), ptrs("tp", tp), ptrs("fn", fn), 0.25, 2.0, k, loss_kind,
                        p(loss), p(row_loss), p(hit), None)


def test_focal_argument_validation():
    from vjepa2_amd import _lib

    lib = _lib.load()
    err = _lib.last_error
    for bad in (0, 4, -1):
        assert _call(lib, nseg=bad) != 0 and "nseg must be 1..3" in err(), (bad, err())
    for bad in (2, -1):
        assert _call(lib, loss_kind=bad) != 0 and "loss_kind must be 0" in err(), (bad, err())
    for missing in ("logits", "ld", "C", "labels", "tp", "fn"):
        assert _call(lib, arrays=(missing,)) != 0 and "null operand" in err(), (missing, err())
    assert _call(lib, hit=0) != 0 and "null operand" in err(), err()
    for missing in ("loss", "row_loss"):
        assert _call(lib, **{missing: 0}) != 0 and "null loss operand" in err(), (missing, err())
    for missing in ("logits", "labels", "tp", "fn"):
        assert _call(lib, **{missing: (1, 0)}) != 0 and "null operand in segment 1" in err(), (missing, err())
    for bad in (dict(B=0), dict(B=-2), dict(k=0)):
        assert _call(lib, **bad) != 0 and "B and k must be >= 1" in err(), (bad, err())
    for bad in ((0, 7), (11, -3)):
        assert _call(lib, C=bad) != 0 and "C must be >= 1" in err(), (bad, err())
    assert _call(lib, ld=(11, 6)) != 0 and "segment 1 ld 6 < C 7" in err(), err()
    assert _call(lib, dlogits=(1, 1), lddl=(10, 7)) != 0 and "segment 0 dlogits stride 10 < C 11" in err(), err()
    assert _call(lib, dlogits=(1, 1), arrays=("lddl",)) != 0 and "dlogits stride 0 < C 11" in err(), err()
    assert _call(lib, B=1 << 30, nseg=3, C=(1, 1, 1), ld=(1, 1, 1), logits=(1, 1, 1), labels=(1, 1, 1), tp=(1, 1, 1),
                 fn=(1, 1, 1)) != 0 and "exceed int range" in err(), err()


def test_focal_wrapper_rejects_cpu_tensors_and_bad_shapes():
    """ops.focal: no CPU path; head counts are checked before anything else."""
    import torch

    from vjepa2_amd import ops

    x, lb, cnt = torch.zeros(4, 5), torch.zeros(4, dtype=torch.int64), torch.zeros(5, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.focal([x], [lb], [cnt], [cnt.clone()])
    with pytest.raises(ValueError, match="1..3 heads"):
        ops.focal([x] * 4, [lb] * 4, [cnt] * 4, [cnt] * 4)
    with pytest.raises(ValueError, match="1..3 heads"):
        ops.focal([x, x], [lb], [cnt, cnt], [cnt, cnt])
    with pytest.raises(ValueError, match="valid masks"):
        ops.focal([x], [lb], [cnt], [cnt], valid=[None, None])
