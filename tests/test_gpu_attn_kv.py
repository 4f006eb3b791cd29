"""GPU: vj_attn_fwd_kv (forward attention of appended queries over a K/V cache, with a query position offset)
and vj_kv_append, through the C ABI on framed buffers, against the float64 reference and the per-element
rounding bound of tests/attn_bounds.py (its forward bound E_o and constant C unchanged: attn_bounds._core takes
separate query and key lengths and a dense visibility matrix, which is written out here as
j // fblk <= (q_pos0 + i) // fblk).

Buffers (frames as in tests/test_gpu_attn_edges.py, whose Frame this file uses):
  * the new rows' q | k | v sit in a NaN-filled buffer, ld = 3 D + 56, columns 8, D + 24, 2 D + 40;
  * the cache is a flat NaN-sentinel buffer: guard elements, then nseq slots of kv_seq_stride = rows * ldkv + 72
    elements (rows: one frame more than the call uses), ldkv = 2 D + 40, K at column 8, V at D + 24, guard
    elements behind. Only the K / V windows of rows below q_pos0 are filled by the test; the K / V windows of the
    new rows are written by vj_kv_append (one call for K, one for V); every other element, and so every row at
    or past klen, keeps the NaN sentinel, which the attention must not let through;
  * O and stats are windows of sentinel-filled frames with guard rows and columns.
Checks: the append writes the new rows bit-exactly and nothing else; the attention leaves the cache as it was;
no guard element changes; O has no NaN and every element is within C E_o of the reference; stats is within the
edges test's bound (atol 2e-3, rtol 1e-4 in natural-log units); a second run and a run with stats = NULL give
the same O bits; the ops wrappers on packed tensors give the same bits as the framed calls."""

import functools
import math
import zlib
from collections import namedtuple

import pytest
import torch

import attn_bounds as ab
from test_gpu_attn_edges import BF16, DEV, F32, SENTINEL, Frame, _same_bits, _values

pytestmark = pytest.mark.gpu

KvCase = namedtuple("KvCase", "name hd fblk q_pos0 qlen rows")  # rows: allocated rows per sequence (> klen)
H, NSEQ = 2, 3
CGUARD = 4096  # sentinel elements in front of and behind the cache's slots
SENT16 = SENTINEL[BF16][1]


def _cases():
    out = []
    for hd in (32, 64):
        # (frame block, prior frames, new frames)
        for fblk, prior, new in ((6, 0, 1), (6, 2, 1), (6, 1, 2),  # (6, 1, 2): a block boundary inside the queries
                                 (258, 1, 1),  # klen 516: no multiple of 64, three 128-query tiles, the last ragged
                                 (130, 2, 1),  # klen 390
                                 (64, 3, 1)):  # exact tile multiples
            out.append(KvCase(f"fc{fblk}-p{prior}-n{new}-hd{hd}", hd, fblk, prior * fblk, new * fblk,
                              (prior + new + 1) * fblk))
        out.append(KvCase(f"dense-hd{hd}", hd, 0, 130, 70, 264))  # qlen 70, klen 200
    return out


CASES = _cases()
_ids = lambda c: c.name  # noqa: E731


def _dims(case):
    D = H * case.hd
    d = dict(D=D, ldq=3 * D + 56, q_off=8, ksrc=D + 24, vsrc=2 * D + 40, ldkv=2 * D + 40, k_off=8, v_off=D + 24,
             ldo=D + 24)
    assert all(v % 8 == 0 for v in d.values())
    d["stride"] = case.rows * d["ldkv"] + 72  # more than rows * ldkv
    d["klen"] = case.q_pos0 + case.qlen
    assert d["klen"] < case.rows and d["ldq"] != d["ldkv"] != d["ldo"]
    return d


@functools.lru_cache(maxsize=None)
def _inputs(case):
    """Seeded bf16 q [NSEQ, qlen, D], k, v [NSEQ, klen, D]; the last key of every sequence is pulled towards its
    last query (tests/attn_bounds.py: the edge key then carries weight). Shared, never modified."""
    g = torch.Generator().manual_seed(zlib.crc32(case.name.encode()))
    D, klen = H * case.hd, case.q_pos0 + case.qlen
    q = torch.randn(NSEQ, case.qlen, D, generator=g)
    k, v = torch.randn(NSEQ, klen, D, generator=g), torch.randn(NSEQ, klen, D, generator=g)
    k[:, -1] += math.log(klen + 1.0) * case.hd ** -0.5 * q[:, -1]
    return q.bfloat16(), k.bfloat16(), v.bfloat16()


def _visible(case):
    """The offset frame-causal mask, densely: query i (position q_pos0 + i) sees key j iff
    j // fblk <= (q_pos0 + i) // fblk; fblk = 0: every key."""
    klen = case.q_pos0 + case.qlen
    if not case.fblk:
        return torch.ones(case.qlen, klen, dtype=torch.bool)
    qi = (case.q_pos0 + torch.arange(case.qlen)) // case.fblk
    return (torch.arange(klen) // case.fblk)[None, :] <= qi[:, None]


@functools.lru_cache(maxsize=None)
def _reference(case):
    """float64 o, E_o [NSEQ * qlen, D] and lse [H, NSEQ * qlen] (natural log)."""
    q, k, v = (x.double() for x in _inputs(case))
    hd, T = case.hd, NSEQ * case.qlen
    vis = _visible(case)
    o, E = torch.zeros(T, H, hd, dtype=torch.float64), torch.zeros(T, H, hd, dtype=torch.float64)
    lse = torch.zeros(H, T, dtype=torch.float64)
    zero = torch.zeros(case.qlen, hd, dtype=torch.float64)
    for s in range(NSEQ):
        sl = slice(s * case.qlen, (s + 1) * case.qlen)
        for h in range(H):
            c = slice(h * hd, (h + 1) * hd)
            r = ab._core(q[s][:, c], k[s][:, c], v[s][:, c], zero, hd ** -0.5, vis=vis, bounds=True)
            o[sl, h], E[sl, h], lse[h, sl] = r["o"], r["E_o"], r["lse"]
    return o.reshape(T, -1), E.reshape(T, -1), lse


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Cache:
    """The flat sentinel-filled cache buffer of a case, rows below q_pos0 filled with the prior keys / values."""

    def __init__(self, case):
        d = _dims(case)
        self.case, self.d = case, d
        self.bits = torch.full((2 * CGUARD + NSEQ * d["stride"],), SENT16, dtype=torch.int16, device=DEV)
        _, k, v = _inputs(case)
        for name, src in (("k_off", k), ("v_off", v)):
            self.window(self.bits.view(BF16), 0, case.q_pos0, d[name]).copy_(src[:, :case.q_pos0].to(DEV))

    def window(self, flat, r0, r1, col):
        """[NSEQ, r1 - r0, D] strided view of rows r0 .. r1 - 1, columns col .. col + D - 1 of every slot."""
        d = self.d
        return flat.as_strided((NSEQ, r1 - r0, d["D"]), (d["stride"], d["ldkv"], 1), CGUARD + r0 * d["ldkv"] + col)

    def ptr(self):
        return self.bits[CGUARD:].data_ptr()

    def snapshot(self):
        return self.bits.cpu().clone()


def _append_framed(case, cache, fq):
    from vjepa2_amd._lib import call

    d = cache.d
    for src_off, dst_off in ((d["ksrc"], d["k_off"]), (d["vsrc"], d["v_off"])):
        call("vj_kv_append", NSEQ, case.qlen, d["D"], fq.ptr(), d["ldq"], src_off, cache.ptr(), d["stride"], d["ldkv"],
             dst_off, case.q_pos0, _stream())
    torch.cuda.synchronize()


def _attend_framed(case, cache, fq, with_stats=True):
    """One vj_attn_fwd_kv call into fresh O / stats frames: {"o": bits, "lse": bits or None} after the guard check."""
    from vjepa2_amd._lib import call

    d = cache.d
    T = NSEQ * case.qlen
    fo = Frame(T, d["ldo"], BF16, {"o": (8, d["D"])})
    fs = Frame(1, H * T + 16, F32, {"lse": (8, H * T)})
    call("vj_attn_fwd_kv", NSEQ, case.qlen, d["klen"], H, case.hd, fq.ptr(), d["ldq"], d["q_off"], cache.ptr(),
         d["stride"], d["ldkv"], d["k_off"], d["v_off"], fo.ptr(8), d["ldo"], fs.ptr(8) if with_stats else None,
         case.hd ** -0.5, case.q_pos0, case.fblk, _stream())
    torch.cuda.synchronize()
    res = fo.read(f"{case.name} o")
    st = fs.read(f"{case.name} stats", untouched=() if with_stats else ("lse",))
    res["lse"] = st["lse"] if with_stats else None
    return res


def _new_rows_frame(case):
    d = _dims(case)
    q, k, v = _inputs(case)
    T = NSEQ * case.qlen
    fq = Frame(T, d["ldq"], BF16, {"q": (d["q_off"], d["D"]), "k": (d["ksrc"], d["D"]), "v": (d["vsrc"], d["D"])})
    fq.put("q", q.reshape(T, -1))
    fq.put("k", k[:, case.q_pos0:].reshape(T, -1))
    fq.put("v", v[:, case.q_pos0:].reshape(T, -1))
    return fq


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_append_then_attend(case):
    d = _dims(case)
    _, k, v = _inputs(case)
    cache, fq = Cache(case), _new_rows_frame(case)
    before = cache.snapshot()
    _append_framed(case, cache, fq)
    after = cache.snapshot()
    # the append: the new rows' K / V windows hold the source bits, every other element is as it was (the older
    # rows bitwise, the gaps, the rows from klen on and the guards still the sentinel)
    want = before.clone()
    for col, src in ((d["k_off"], k), (d["v_off"], v)):
        cache.window(want, case.q_pos0, d["klen"], col).copy_(src[:, case.q_pos0:].view(torch.int16))
    diff = (after != want).nonzero()
    assert not diff.numel(), (f"{case.name}: vj_kv_append left {diff.shape[0]} elements different from the expected "
                              f"cache; first at flat index {int(diff[0, 0]) - CGUARD} (stride {d['stride']}, "
                              f"ldkv {d['ldkv']})")
    stale = cache.window(after, d["klen"], case.rows, 0)
    assert bool((stale == SENT16).all()), "a row at or past klen lost its NaN"
    assert bool(torch.isnan(cache.window(after.view(BF16), d["klen"], case.rows, d["k_off"])).all())

    res = _attend_framed(case, cache, fq)
    assert bool((cache.snapshot() == after).all()), f"{case.name}: the attention wrote into the cache"
    fq.read(f"{case.name} new rows")  # guards of the inputs (its windows are inputs: whatever they hold is theirs)
    o = _values(res["o"], BF16)
    assert not bool(torch.isnan(o).any()), f"{case.name}: NaN in O (a stale row reached the output)"
    ex_o, E_o, ex_lse = _reference(case)
    ratio = ab.assert_within(o, ex_o, E_o, f"{case.name} o")  # every element, none skipped
    lse = _values(res["lse"], F32).reshape(H, -1) * ab.LN2  # stats hold log2 units
    err = (lse - ex_lse).abs()
    bad = ~(err <= 2e-3 + 1e-4 * ex_lse.abs())
    print(f"[attn-kv] {case.name}: o={ratio:.3f} of C={ab.C:.3f}, lse max |err| {float(err.max()):.2e}")
    assert not bool(bad.any()), f"{case.name} lse: {int(bad.sum())} outside atol 2e-3 rtol 1e-4; first at {bad.nonzero()[0]}"

    again = _attend_framed(case, cache, fq)
    _same_bits(res, again, f"{case.name} second run")
    nostats = _attend_framed(case, cache, fq, with_stats=False)
    _same_bits({"o": res["o"]}, {"o": nostats["o"]}, f"{case.name} stats = NULL")


@pytest.mark.parametrize("case", [c for c in CASES if c.name in ("fc6-p1-n2-hd32", "fc130-p2-n1-hd64", "dense-hd32")],
                         ids=_ids)
def test_ops_wrappers_match_the_framed_calls(case):
    """ops.kv_append / ops.attn_fwd_kv on packed tensors (K | V side by side, offsets 0 and D) give the framed
    calls' bits: strides and offsets only enter addresses."""
    from vjepa2_amd import ops

    cache, fq = Cache(case), _new_rows_frame(case)
    _append_framed(case, cache, fq)
    framed = _attend_framed(case, cache, fq)
    q, k, v = _inputs(case)
    D, klen, T = H * case.hd, case.q_pos0 + case.qlen, NSEQ * case.qlen
    qkv = torch.cat([q.reshape(T, D), k[:, case.q_pos0:].reshape(T, D), v[:, case.q_pos0:].reshape(T, D)], 1).to(DEV)
    kv = torch.full((NSEQ, case.rows, 2 * D), float("nan"), dtype=BF16, device=DEV)
    kv[:, :case.q_pos0] = torch.cat([k[:, :case.q_pos0], v[:, :case.q_pos0]], 2).to(DEV)
    ops.kv_append(qkv, kv, case.q_pos0, case.qlen, D, 2 * D)
    stats = torch.empty(H, T, dtype=F32, device=DEV)
    o = ops.attn_fwd_kv(qkv, kv, klen, H, case.hd, case.hd ** -0.5, q_pos0=case.q_pos0, fblk=case.fblk, stats=stats)
    torch.cuda.synchronize()
    assert torch.equal(kv[:, :klen].cpu(), torch.cat([k, v], 2)) and bool(torch.isnan(kv[:, klen:]).all())
    _same_bits(framed, {"o": o.view(torch.int16).cpu(), "lse": stats.reshape(1, -1).view(torch.int32).cpu()},
               f"{case.name} packed vs framed")


def test_refused_call_writes_nothing():
    """q_pos0 + qlen > klen returns an error and leaves O, stats and the cache untouched."""
    from vjepa2_amd import _lib

    case = next(c for c in CASES if c.name == "fc6-p2-n1-hd32")
    d = _dims(case)
    cache, fq = Cache(case), _new_rows_frame(case)
    before = cache.snapshot()
    T = NSEQ * case.qlen
    fo = Frame(T, d["ldo"], BF16, {"o": (8, d["D"])})
    fs = Frame(1, H * T + 16, F32, {"lse": (8, H * T)})
    rc = _lib.load().vj_attn_fwd_kv(NSEQ, case.qlen, d["klen"] - 1, H, case.hd, fq.ptr(), d["ldq"], d["q_off"],
                                    cache.ptr(), d["stride"], d["ldkv"], d["k_off"], d["v_off"], fo.ptr(8), d["ldo"],
                                    fs.ptr(8), case.hd ** -0.5, case.q_pos0, case.fblk, _stream())
    assert rc != 0 and "q_pos0 + qlen > klen" in _lib.last_error(), _lib.last_error()
    torch.cuda.synchronize()
    fo.read("o", untouched=("o",))
    fs.read("stats", untouched=("lse",))
    assert bool((cache.snapshot() == before).all())
