"""CPU: vj_attn_fwd_kv and vj_kv_append validate every argument before any device work (no GPU here: a launch
would fail differently), with a message naming each refusal, in the style of test_plan_capi.py; the ops
wrappers have no CPU path."""

import ctypes

import pytest

P = lambda v: ctypes.c_void_p(0x1000 * v) if v else None  # noqa: E731  (never dereferenced on a refused call)
ARG, UNSUPPORTED = 1, 3  # VJ_ERR_ARG, VJ_ERR_UNSUPPORTED


def _lib():
    from vjepa2_amd import _lib

    return _lib.load(), _lib.last_error


def _fwd(lib, nseq=3, qlen=6, klen=18, H=2, hd=32, q=1, ldq=192, q_off=0, kv=2, stride=24 * 128, ldkv=128, k_off=0,
         v_off=64, o=3, ldo=64, stats=4, scale=0.17, q_pos0=12, fblk=6):
    return lib.vj_attn_fwd_kv(nseq, qlen, klen, H, hd, P(q), ldq, q_off, P(kv), stride, ldkv, k_off, v_off, P(o), ldo,
                              P(stats), scale, q_pos0, fblk, None)


def _append(lib, nseq=3, nrows=6, width=128, src=1, lds=192, src_off=64, kv=2, stride=24 * 128, ldkv=128, dst_off=0,
            row0=12):
    return lib.vj_kv_append(nseq, nrows, width, P(src), lds, src_off, P(kv), stride, ldkv, dst_off, row0, None)


def test_attn_fwd_kv_argument_validation():
    lib, err = _lib()
    for missing in ("q", "kv", "o"):
        assert _fwd(lib, **{missing: 0}) == ARG and "null operand" in err(), (missing, err())
    for bad in (dict(nseq=0), dict(qlen=0), dict(klen=0), dict(nseq=-1)):
        assert _fwd(lib, **bad) == ARG and "must be >= 1" in err(), (bad, err())
    for hd in (48, 0, 128, -32):
        assert _fwd(lib, hd=hd) == ARG and "head_dim must be" in err(), (hd, err())
    for hd in (80, 88):  # the training forward's padded head dims are not built for the cached forward
        assert _fwd(lib, hd=hd, ldq=3 * 2 * hd, ldkv=4 * hd, v_off=2 * hd, ldo=2 * hd,
                    stride=24 * 4 * hd) == UNSUPPORTED and "not built for the cached forward" in err(), (hd, err())
    assert _fwd(lib, H=0) == ARG and "bad H" in err(), err()
    for fblk in (-1, -6):
        assert _fwd(lib, fblk=fblk) == ARG and "bad frame block" in err(), (fblk, err())
    # q_pos0 + qlen > klen: the new rows must already be in the cache
    for bad in (dict(q_pos0=13), dict(klen=17), dict(qlen=7), dict(q_pos0=-1)):
        assert _fwd(lib, **bad) == ARG and "q_pos0 + qlen > klen" in err(), (bad, err())
    for bad in (dict(ldq=196), dict(ldkv=132, stride=24 * 132), dict(ldo=68), dict(stride=24 * 128 + 4)):
        assert _fwd(lib, **bad) == ARG and "strides must be multiples of 8" in err(), (bad, err())
    for bad in (dict(q_off=4), dict(k_off=4), dict(v_off=68), dict(q_off=-8)):
        assert _fwd(lib, **bad) == ARG and "column offsets" in err(), (bad, err())
    for bad in (dict(ldq=56), dict(ldo=56), dict(ldkv=120, stride=24 * 120), dict(q_off=136)):
        assert _fwd(lib, **bad) == ARG and "shorter than its columns" in err(), (bad, err())
    # a sequence's slot holds kv_seq_stride / ldkv rows; one sequence may use any stride
    assert _fwd(lib, stride=17 * 128) == ARG and "exceeds the 17 rows" in err(), err()
    assert _fwd(lib, ldkv=1 << 22, stride=(1 << 22) * 512, klen=300, q_pos0=0) == ARG and "2 GB" in err(), err()
    assert lib.vj_attn_fwd_kv(3, 6, 18, 2, 32, ctypes.c_void_p(0x1008), 192, 0, P(2), 24 * 128, 128, 0, 64, P(3), 64,
                              None, 0.17, 12, 6, None) == ARG and "16-byte aligned" in err(), err()


def test_kv_append_argument_validation():
    lib, err = _lib()
    for missing in ("src", "kv"):
        assert _append(lib, **{missing: 0}) == ARG and "null operand" in err(), (missing, err())
    for bad in (dict(nseq=0), dict(nrows=0), dict(width=0), dict(nrows=-2)):
        assert _append(lib, **bad) == ARG and "nseq, nrows >= 1 and width >= 8" in err(), (bad, err())
    assert _append(lib, row0=-1) == ARG and "bad first row" in err(), err()
    for bad in (dict(width=124), dict(lds=196), dict(ldkv=132), dict(stride=24 * 128 + 2), dict(src_off=60),
                dict(dst_off=4), dict(src_off=-8)):
        assert _append(lib, **bad) == ARG and "multiples of 8" in err(), (bad, err())
    for bad in (dict(lds=184), dict(ldkv=120), dict(dst_off=8)):
        assert _append(lib, **bad) == ARG and "shorter than its columns" in err(), (bad, err())
    assert _append(lib, row0=19) == ARG and "exceed the 24 rows" in err(), err()  # rows 19 .. 24 of 24
    assert lib.vj_kv_append(3, 6, 128, ctypes.c_void_p(0x1004), 192, 64, P(2), 24 * 128, 128, 0, 12,
                            None) == ARG and "16-byte aligned" in err(), err()


def test_wrappers_reject_cpu_tensors_and_bad_shapes():
    import torch

    from vjepa2_amd import ops

    q = torch.zeros(18, 192, dtype=torch.bfloat16)
    kv = torch.zeros(3, 24, 128, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.attn_fwd_kv(q, kv, 18, 2, 32, 0.17, q_pos0=12, fblk=6)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.kv_append(q, kv, 12, 6, 64, 128)
