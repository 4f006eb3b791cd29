"""CPU: vj_xent validates its arguments before any device work (no GPU here), with a message for each
refusal, in the style of test_capi.py::test_library_metadata_and_errors."""

import ctypes


def _call(lib, V=2, B=3, C=11, logits=1, ld=11, labels=1, i64=1, loss=1, row_loss=1, dlogits=0, lddl=0, pred=1,
          correct=1):
    """Non-null pointers are never dereferenced on a refused call: any non-zero address stands in."""
    p = lambda v: ctypes.c_void_p(0x1000 * v) if v else None  # noqa: E731
    return lib.vj_xent(V, B, C, p(logits), ld, p(labels), i64, p(loss), p(row_loss), p(dlogits), lddl, p(pred),
                       p(correct), None)


def test_xent_argument_validation():
    from vjepa2_amd import _lib

    lib = _lib.load()
    for missing in ("logits", "labels", "loss", "row_loss", "pred", "correct"):
        rc = _call(lib, **{missing: 0})
        assert rc != 0 and "null operand" in _lib.last_error(), (missing, _lib.last_error())
    for bad in (dict(C=0), dict(B=0), dict(V=0), dict(C=-3), dict(V=-1)):
        rc = _call(lib, **bad)
        assert rc != 0 and "must be >= 1" in _lib.last_error(), (bad, _lib.last_error())
    rc = _call(lib, ld=10)
    assert rc != 0 and "ld 10 < C 11" in _lib.last_error(), _lib.last_error()
    rc = _call(lib, dlogits=1, lddl=7)
    assert rc != 0 and "dlogits stride 7 < C 11" in _lib.last_error(), _lib.last_error()
    rc = _call(lib, V=1 << 20, B=1 << 20)
    assert rc != 0 and "exceed int range" in _lib.last_error(), _lib.last_error()


def test_xent_wrapper_rejects_cpu_tensors_and_bad_shapes():
    """ops.xent: no CPU path; the label / view bookkeeping is checked on the host."""
    import pytest
    import torch

    from vjepa2_amd import ops

    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.xent(torch.zeros(4, 5), torch.zeros(4, dtype=torch.int64))
