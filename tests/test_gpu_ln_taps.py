"""GPU: vj_layernorm_taps (ops.layernorm_taps) against ops.layernorm_fwd placed by torch indexing, bit for
bit: group boundaries inside a wave's rows (n = 1, 5, 37 against 4 rows per wave) and inside a block (16
rows), both input dtypes (each with the kernel vj_layernorm_fwd picks for it), padded strides on both
sides, a non-monotone destination map with unused blocks, and everything that must NOT be written: unused
blocks, pad columns, a stray tail row and guard rows before and after keep a sentinel bit pattern."""

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 0x5A5AC3C3  # as int32; not a value a LayerNorm of these inputs produces
GUARD = 3


def _dst(G):
    """Injective, non-monotone for G > 1, into 2G + 1 blocks (so G + 1 stay unused): 2 is a unit mod 2G + 1."""
    nb = 2 * G + 1
    d = [(2 * g + G) % nb for g in range(G)]
    assert len(set(d)) == G and (G == 1 or d != sorted(d))
    return d, nb


def _run(D, dtype, n, G, xpad, opad, gen, poison_row=None):
    from vjepa2_amd import ops

    ldx, ldo = D + xpad, D + opad
    xs = torch.randn(G * n, ldx, generator=gen, device=DEV) * 1.7 + 0.3
    if poison_row is not None:
        xs[poison_row, D // 2] = float("nan")
    xs = xs.to(dtype)
    x = xs[:, :D]
    w = torch.randn(D, generator=gen, device=DEV)
    b = torch.randn(D, generator=gen, device=DEV)
    dst, nb = _dst(G)
    R_out = nb * n + 1  # a tail row that belongs to no block
    store = torch.full((GUARD + R_out + GUARD, ldo), SENTINEL, dtype=torch.int32, device=DEV)
    out = store.view(torch.float32)[GUARD:GUARD + R_out, :D]
    ref = ops.layernorm_fwd(x, w, b, 1e-6, out_dtype=torch.float32, want_stats=False)[0]
    want = torch.full_like(store, SENTINEL)
    for g, blk in enumerate(dst):
        want[GUARD + blk * n:GUARD + blk * n + n, :D] = ref[g * n:(g + 1) * n].view(torch.int32)
    got = ops.layernorm_taps(x, w, b, 1e-6, out, n, dst)
    assert got is out
    return store, want, ref, dst


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("D", [64, 1024, 1408])
def test_taps_bitwise_and_untouched(D, dtype):
    gen = torch.Generator(device=DEV).manual_seed(D + (1 if dtype == torch.bfloat16 else 0))
    bad = []
    for n in (1, 4, 5, 37):
        for G in (1, 3, 7):
            for xpad, opad in ((0, 0), (8, 0), (0, 4), (8, 4)):
                store, want, ref, _ = _run(D, dtype, n, G, xpad, opad, gen)
                assert torch.isfinite(ref).all()
                if not torch.equal(store, want):
                    bad.append((n, G, xpad, opad, int((store != want).sum())))
    assert not bad, bad


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_nan_rows_stay_in_their_block(dtype):
    """A NaN input row gives a NaN output row where the map puts it, and nowhere else."""
    D, n, G = 1024, 5, 3
    gen = torch.Generator(device=DEV).manual_seed(11)
    row = 1 * n + 4  # the last row of group 1: in one wave with group 2's first rows
    store, want, ref, dst = _run(D, dtype, n, G, 8, 4, gen, poison_row=row)
    assert torch.isnan(ref[row]).all() and torch.isfinite(ref[:row]).all() and torch.isfinite(ref[row + 1:]).all()
    orow = GUARD + dst[1] * n + 4
    got = store.view(torch.float32)
    assert torch.isnan(got[orow, :D]).all()
    keep = torch.ones(store.shape[0], dtype=torch.bool, device=DEV)
    keep[orow] = False
    assert torch.equal(store[keep], want[keep])
    assert torch.equal(store[orow, D:], want[orow, D:])  # its pad columns too
    assert not torch.isnan(got[keep]).any()
