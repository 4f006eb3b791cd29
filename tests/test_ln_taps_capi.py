"""CPU: vj_layernorm_taps validates everything it can see without reading device memory before any device
work (no GPU here), with a message for each refusal, in the style of tests/test_xent_capi.py."""

import ctypes


def _call(lib, G=3, n=5, D=64, x=1, x_bf16=0, ldx=64, gamma=1, beta=1, eps=1e-6, out=1, ldo=64, R_out=40, dst=1,
          off=0):
    """Non-null pointers are never dereferenced on a refused call: any non-zero 16-B aligned address stands
    in (`off` bytes added to x's for the alignment refusal)."""
    p = lambda v, o=0: ctypes.c_void_p(0x1000 * v + o) if v else None  # noqa: E731
    return lib.vj_layernorm_taps(G, n, D, p(x, off), x_bf16, ldx, p(gamma), p(beta), eps, p(out), ldo, R_out, p(dst),
                                 None)


def test_layernorm_taps_argument_validation():
    from vjepa2_amd import _lib

    lib = _lib.load()

    def refused(fragment, **kw):
        rc = _call(lib, **kw)
        assert rc != 0 and fragment in _lib.last_error(), (kw, _lib.last_error())

    for missing in ("x", "out", "dst"):
        refused("null operand", **{missing: 0})
    refused("gamma/beta both or neither", gamma=0)
    refused("gamma/beta both or neither", beta=0)
    for bad in (dict(G=0), dict(n=0), dict(G=-2), dict(n=-1)):
        refused("G and n must be >= 1", **bad)
    for bad in (dict(D=0), dict(D=62, ldx=64), dict(D=2052, ldx=2052, ldo=2052), dict(D=-4)):
        refused("must be %4 and in [4, 2048]", **bad)
    refused("G * n = 1099511627776 rows exceed int range", G=1 << 20, n=1 << 20)
    refused("R_out = 4294967296 rows exceed int range", R_out=1 << 32)
    refused("R_out = -1 rows exceed int range", R_out=-1)
    refused("out has 2 blocks of 5 rows for 3 groups", R_out=14)
    refused("ldx 60 < D 64", ldx=60)
    refused("out stride 32 < D 64", ldo=32)
    refused("strides must be %4", ldx=66)
    refused("strides must be %4", ldo=70)
    refused("must be 16-B aligned", off=8)
    refused("must be 16-B aligned", x_bf16=1, off=4)


def test_layernorm_taps_is_declared_and_typed():
    """The entry is in the header, the ctypes table and the library (tests/test_capi.py holds the three sets
    together; this names the new member)."""
    from vjepa2_amd import _lib

    assert len(_lib.SIGNATURES["vj_layernorm_taps"]) == 14
    assert hasattr(_lib.load(), "vj_layernorm_taps")
