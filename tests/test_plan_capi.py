"""CPU: the four planning entry points (vj_cem_sample, vj_pose_step, vj_plan_frame, vj_cem_update) validate their
arguments before any device work (no GPU here), with a message for each refusal, in the style of
test_focal_capi.py; the ops wrappers have no CPU path."""

import ctypes

import pytest

P = lambda v: ctypes.c_void_p(0x1000 * v) if v else None  # noqa: E731  (never dereferenced on a refused call)


def _lib():
    from vjepa2_amd import _lib

    return _lib.load(), _lib.last_error


def _sample(lib, S=16, rollout=2, noise=1, mean=2, std=3, maxnorm=0.05, gclip=0.75, axis_on=None, axis_val=None,
            close_from=-1, actions=4):
    return lib.vj_cem_sample(S, rollout, P(noise), P(mean), P(std), maxnorm, gclip, axis_on, axis_val, close_from,
                             P(actions), None)


def _pose(lib, S=16, pose=1, ldp=7, action=2, lda=7, out=3, ldo=7):
    return lib.vj_pose_step(S, P(pose), ldp, P(action), lda, P(out), ldo, None)


def _frame(lib, S=16, R=4, D=96, src=1, ss=None, sr=None, normalize=1, dst=2, ds=None, goal=3, energy=4):
    sr = D if sr is None else sr
    ss = R * sr if ss is None else ss
    ds = R * D if ds is None else ds
    return lib.vj_plan_frame(S, R, D, P(src), ss, sr, normalize, 1e-5, P(dst), ds, P(goal), P(energy), None)


def _update(lib, S=16, rollout=2, k=4, energy=1, actions=2, mean=3, std=4, elite=5):
    return lib.vj_cem_update(S, rollout, k, P(energy), P(actions), 0.25, 0.95, 0.15, 0.15, P(mean), P(std), P(elite),
                             None)


def test_cem_sample_argument_validation():
    lib, err = _lib()
    for missing in ("noise", "mean", "std", "actions"):
        assert _sample(lib, **{missing: 0}) != 0 and "null operand" in err(), (missing, err())
    for bad in (dict(S=0), dict(S=-3), dict(rollout=0), dict(rollout=-1)):
        assert _sample(lib, **bad) != 0 and "S and rollout must be >= 1" in err(), (bad, err())
    assert _sample(lib, S=1 << 20, rollout=1 << 10) != 0 and "exceeds 2^26" in err(), err()
    assert lib.vj_cem_sample(16, 2, ctypes.c_void_p(0x1004), P(2), P(3), 0.05, 0.75, None, None, -1, P(4),
                             None) != 0 and "16-byte aligned" in err(), err()
    assert _sample(lib, maxnorm=-0.1) != 0 and "must be >= 0" in err(), err()
    assert _sample(lib, gclip=-0.1) != 0 and "must be >= 0" in err(), err()
    assert _sample(lib, close_from=-2) != 0 and "close_from must be -1" in err(), err()
    on = (ctypes.c_int * 4)(0, 1, 0, 0)
    assert _sample(lib, axis_on=on, axis_val=None) != 0 and "axis_on without axis_val" in err(), err()


def test_pose_step_argument_validation():
    lib, err = _lib()
    for missing in ("pose", "action", "out"):
        assert _pose(lib, **{missing: 0}) != 0 and "null operand" in err(), (missing, err())
    for bad in (0, -1):
        assert _pose(lib, S=bad) != 0 and "S must be >= 1" in err(), (bad, err())
    for bad in ("ldp", "lda", "ldo"):
        assert _pose(lib, **{bad: 6}) != 0 and "< 7" in err(), (bad, err())


def test_plan_frame_argument_validation():
    lib, err = _lib()
    assert _frame(lib, src=0) != 0 and "null operand (src)" in err(), err()
    assert _frame(lib, dst=0, energy=0) != 0 and "nothing to do" in err(), err()
    assert _frame(lib, goal=0) != 0 and "energy without goal" in err(), err()
    for bad in (dict(S=0), dict(R=0), dict(S=-1), dict(R=-2)):
        assert _frame(lib, **bad) != 0 and "S and R must be >= 1" in err(), (bad, err())
    for bad in (0, 2, 98, 1023, -4):
        assert _frame(lib, D=bad, sr=4096, ss=1 << 20, ds=1 << 20) != 0 and "multiple of 4" in err(), (bad, err())
    assert _frame(lib, D=2052) != 0 and "D 2052 > 2048" in err(), err()
    assert _frame(lib, sr=92) != 0 and "src row stride 92 < D 96" in err(), err()
    assert _frame(lib, ss=4 * 96 - 4) != 0 and "src sample stride 380 <" in err(), err()
    assert _frame(lib, ds=4 * 96 - 4) != 0 and "dst sample stride 380 < R * D = 384" in err(), err()
    assert _frame(lib, sr=98, ss=4 * 98) != 0 and "multiples of 4 floats" in err(), err()
    assert _frame(lib, ss=4 * 96 + 2) != 0 and "multiples of 4 floats" in err(), err()
    assert _frame(lib, ds=4 * 96 + 2) != 0 and "multiples of 4 floats" in err(), err()
    assert lib.vj_plan_frame(2, 4, 96, ctypes.c_void_p(0x1008), 384, 96, 1, 1e-5, P(2), 384, P(3), P(4),
                             None) != 0 and "16-byte aligned" in err(), err()
    # without dst its stride is not looked at; without energy the goal may be null
    assert _frame(lib, dst=0, ds=0, S=0) != 0 and "S and R must be >= 1" in err(), err()


def test_cem_update_argument_validation():
    lib, err = _lib()
    for missing in ("energy", "actions", "mean", "std"):
        assert _update(lib, **{missing: 0}) != 0 and "null operand" in err(), (missing, err())
    for bad in (dict(S=0), dict(rollout=0), dict(rollout=-1)):
        assert _update(lib, **bad) != 0 and "S and rollout must be >= 1" in err(), (bad, err())
    for bad in (1, 0, -1):
        assert _update(lib, k=bad) != 0 and "k must be >= 2" in err(), (bad, err())
    assert _update(lib, S=16, k=17) != 0 and "k 17 > S 16" in err(), err()
    assert _update(lib, S=4097, k=10) != 0 and "S 4097 > 4096" in err(), err()
    assert _update(lib, S=1, k=2) != 0 and "k 2 > S 1" in err(), err()


def test_wrappers_reject_cpu_tensors_and_bad_shapes():
    import torch

    from vjepa2_amd import ops

    S, r = 6, 2
    noise, mean, std = torch.zeros(r, S, 4), torch.zeros(r, 4), torch.ones(r, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.cem_sample(noise, mean, std, 0.05)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.pose_step(torch.zeros(S, 7), torch.zeros(S, 7))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.plan_frame(torch.zeros(S, 4, 96), goal=torch.zeros(4, 96))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.cem_update(torch.zeros(S), torch.zeros(S, r, 7), 2, mean, std)
