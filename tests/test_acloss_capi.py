"""CPU: the AC post-training loss entry points (vj_ac_loss_fwd, vj_ac_loss_bwd, vj_ac_loss_reduce) validate their
arguments before any device work (no GPU here), with a message for each refusal, in the style of
test_plan_capi.py; the ops wrappers and ACLossFn have no CPU path."""

import ctypes

import pytest

P = lambda v: ctypes.c_void_p(0x1000 * v) if v else None  # noqa: E731  (never dereferenced on a refused call)


def _lib():
    from vjepa2_amd import _lib

    return _lib.load(), _lib.last_error


def _fwd(lib, B=2, R=4, D=96, z=1, zss=None, zrs=None, h=2, hss=None, hrs=None, normalize=1, p=1.0, zn=3, stats=4,
         rowsum=5):
    zrs = D if zrs is None else zrs
    zss = R * zrs if zss is None else zss
    hrs = D if hrs is None else hrs
    hss = R * hrs if hss is None else hss
    return lib.vj_ac_loss_fwd(B, R, D, P(z), zss, zrs, P(h), hss, hrs, normalize, 1e-5, p, P(zn), P(stats), P(rowsum),
                              None)


def _bwd(lib, B=2, R=4, D=96, z=1, zss=None, zrs=None, stats=2, h=3, hss=None, hrs=None, normalize=1, p=1.0, gzn=4,
         dz=5):
    zrs = D if zrs is None else zrs
    zss = R * zrs if zss is None else zss
    hrs = D if hrs is None else hrs
    hss = R * hrs if hss is None else hss
    return lib.vj_ac_loss_bwd(B, R, D, P(z), zss, zrs, P(stats), P(h), hss, hrs, normalize, p, 0.5, None, P(gzn), P(dz),
                              None)


@pytest.mark.parametrize("call,who", [(_fwd, "vj_ac_loss_fwd"), (_bwd, "vj_ac_loss_bwd")])
def test_shared_shape_and_stride_validation(call, who):
    lib, err = _lib()
    for bad in (dict(B=0), dict(R=0), dict(B=-1), dict(R=-2)):
        assert call(lib, **bad) != 0 and f"{who}: B and R must be >= 1" in err(), (bad, err())
    assert call(lib, B=1 << 20, R=1 << 11, zss=1 << 40, hss=1 << 40) != 0 and "exceeds 2^30" in err(), err()
    for bad in (0, 2, 98, 1023, -4):
        assert call(lib, D=bad, zrs=4096, hrs=4096) != 0 and "multiple of 4" in err(), (bad, err())
    assert call(lib, D=2052) != 0 and "D 2052 > 2048" in err(), err()
    assert call(lib, zrs=92) != 0 and "z row stride 92 < D 96" in err(), err()
    assert call(lib, zss=4 * 96 - 4) != 0 and "z sample stride 380 <" in err(), err()
    assert call(lib, hrs=92) != 0 and "h row stride 92 < D 96" in err(), err()
    assert call(lib, hss=4 * 96 - 4) != 0 and "h sample stride 380 <" in err(), err()
    for bad in (dict(zrs=98, zss=4 * 98), dict(zss=4 * 96 + 2), dict(hrs=98, hss=4 * 98), dict(hss=4 * 96 + 2)):
        assert call(lib, **bad) != 0 and "multiples of 4 floats" in err(), (bad, err())
    assert call(lib, normalize=1, stats=0) != 0 and f"{who}: normalize without stats" in err(), err()
    assert call(lib, p=0.0) != 0 and "loss exponent must be > 0" in err(), err()
    assert call(lib, p=-1.0) != 0 and "loss exponent must be > 0" in err(), err()


def test_ac_loss_fwd_argument_validation():
    lib, err = _lib()
    assert _fwd(lib, z=0) != 0 and "null operand (z)" in err(), err()
    assert _fwd(lib, zn=0, rowsum=0) != 0 and "nothing to do" in err(), err()
    assert _fwd(lib, h=0) != 0 and "rowsum without h" in err(), err()
    for which in range(3):  # z, h, zn off a 16-byte boundary
        ptr = [P(1), P(2), P(3)]
        ptr[which] = ctypes.c_void_p(0x1000 * (which + 1) + 8)
        assert lib.vj_ac_loss_fwd(2, 4, 96, ptr[0], 384, 96, ptr[1], 384, 96, 1, 1e-5, 1.0, ptr[2], P(4), P(5),
                                  None) != 0 and "16-byte aligned" in err(), (which, err())
    assert lib.vj_ac_loss_fwd(2, 4, 96, P(1), 384, 96, P(2), 384, 96, 1, 1e-5, 1.0, P(3), ctypes.c_void_p(0x4004),
                              P(5), None) != 0 and "stats must be 8-byte aligned" in err(), err()
    # a normalise-only call reads no h: its strides are not looked at, the next check is reached
    assert _fwd(lib, h=0, rowsum=0, hrs=1, hss=1, B=0) != 0 and "B and R must be >= 1" in err(), err()
    # without normalize no stats are needed
    assert _fwd(lib, normalize=0, stats=0, B=0) != 0 and "B and R must be >= 1" in err(), err()


def test_ac_loss_bwd_argument_validation():
    lib, err = _lib()
    assert _bwd(lib, z=0) != 0 and "null operand (z or dz)" in err(), err()
    assert _bwd(lib, dz=0) != 0 and "null operand (z or dz)" in err(), err()
    assert _bwd(lib, h=0, gzn=0) != 0 and "nothing to do" in err(), err()
    for which in range(4):  # z, h, gzn, dz off a 16-byte boundary
        ptr = [P(1), P(3), P(4), P(5)]
        ptr[which] = ctypes.c_void_p(0x1000 * (which + 1) + 4)
        assert lib.vj_ac_loss_bwd(2, 4, 96, ptr[0], 384, 96, P(2), ptr[1], 384, 96, 1, 1.0, 0.5, None, ptr[2], ptr[3],
                                  None) != 0 and "16-byte aligned" in err(), (which, err())
    assert lib.vj_ac_loss_bwd(2, 4, 96, P(1), 384, 96, ctypes.c_void_p(0x2004), P(3), 384, 96, 1, 1.0, 0.5, None, P(4),
                              P(5), None) != 0 and "stats must be 8-byte aligned" in err(), err()
    # a null gzn reads as zero and a null h as "no loss term": neither alone is refused
    assert _bwd(lib, gzn=0, B=0) != 0 and "B and R must be >= 1" in err(), err()
    assert _bwd(lib, h=0, B=0) != 0 and "B and R must be >= 1" in err(), err()
    assert _bwd(lib, normalize=0, stats=0, B=0) != 0 and "B and R must be >= 1" in err(), err()


def test_ac_loss_reduce_argument_validation():
    lib, err = _lib()
    assert lib.vj_ac_loss_reduce(8, None, 1.0, P(2), None) != 0 and "null operand" in err(), err()
    assert lib.vj_ac_loss_reduce(8, P(1), 1.0, None, None) != 0 and "null operand" in err(), err()
    for bad in (0, -5):
        assert lib.vj_ac_loss_reduce(bad, P(1), 1.0, P(2), None) != 0 and "n must be >= 1" in err(), (bad, err())


def test_wrappers_reject_cpu_tensors_and_bad_shapes():
    import torch

    from vjepa2_amd import ops
    from vjepa2_amd.functions import ACLossFn

    z, h = torch.zeros(2, 4, 96), torch.zeros(2, 4, 96)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.ac_loss_fwd(z, h)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.ac_loss_bwd(z, torch.zeros(8, 2), h)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ACLossFn.apply(z.requires_grad_(), h, True, 1.0, 1e-5)
