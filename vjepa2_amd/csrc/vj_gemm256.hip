// Large-tile bf16 GEMM for gfx950: 256 x BN x 64 tiles (BN = 256 or 128), 512 threads = 8 waves,
// one workgroup per CU (LDS 144 / 112 KB), v_mfma_f32_16x16x32_bf16, waves 2 (M) x 4 (N), wave tile
// 128 x 64. (A 32x32x16 form of the tile, waves 4 x 2, measured no faster per kernel and 3 % slower
// per train step in round 4 - profiles/r04_gemm_mf32_*.txt - and was removed.)
// Same operand/epilogue contract as vj_gemm.hip (K-major or MN-major A and B, fused epilogues);
// used for the forward and data-gradient GEMMs of the encoder / predictor blocks (M = tokens) and the
// split-K weight gradients.
//
// Persistent: one workgroup per CU walks a run of tiles. The next tile's first two K stages are
// DMA'd while this tile finishes (stage 0 during the last K-tile, stage 1 before or during the
// epilogue), so the prologue latency and the block launch hide behind the epilogue; per-kernel LDS
// tables (GELU, RoPE cos/sin) are loaded once per workgroup.
//
// Schedule (per wave, K-tile t in LDS slot (t + par) & 1): 4 phases per K-tile = (k-step, M-half),
// each 4 x NTN MFMAs on a 64x(BN/4) quarter of the wave tile; the next phase's fragments (16 + 16
// VGPRs, double-buffered) are read from LDS while the current phase's MFMAs run, so LDS latency hides
// under MFMA with 128 accumulator + 64 fragment registers (no spill at 2 waves / SIMD). ONE barrier per
// K-tile (before the last phase): it retires this wave's DMA of tile t+1 (issued one tile earlier)
// and its reads of tile t; tile t+2 is then DMA'd into the freed slot and stays in flight across it.
// Epilogue: stores straight from registers (K-major B, 256-wide tiles: B rows staged permuted) or
// through a padded LDS image in the freed slot, with bias / residual / GELU / GELU' / RoPE fused.
#include <stdlib.h>
#include <atomic>
#include <type_traits>
#include "vj_gemm_tile.h"

namespace {

#if VJ_GEMM_STAMPS  // diagnostic build: s_memtime per tile (start, main loop done, epilogue done) of wave 0
__device__ long vj_gemm_stamps[2048 * 16 * 4];
// S64: s_memtime after each of the 16 barriers of K steps 1-4 of the block's second tile, waves 0 and 4
__device__ long vj_gemm_istamps[2048 * 2 * 16];
#endif

// counted wait for this wave's vector-memory operations (LDS-DMA pieces included): at most N in flight
template <int N>
__device__ __forceinline__ void vm_wait() {
  static_assert(N >= 0 && N <= 24 && N % 4 == 0, "vm_wait: add the count");
  if constexpr (N == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  else if constexpr (N == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  else if constexpr (N == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
  else if constexpr (N == 12) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
  else if constexpr (N == 16) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
  else if constexpr (N == 20) asm volatile("s_waitcnt vmcnt(20)" ::: "memory");
  else asm volatile("s_waitcnt vmcnt(24)" ::: "memory");
}

// Geometry, schedule switches, LDS layout and the supported parameter combinations: Cfg256 (vj_gemm_tile.h)
template <bool AK, bool BKM, int EPI, int BN, bool F8 = false, int NWV = 8, int BMT = 256, int STG = 0>
__global__ __launch_bounds__(NWV * 64, 2) void k_gemm256(G256 g) {
  using Cfg = Cfg256<AK, BKM, EPI, BN, F8, NWV, BMT, STG>;
  static_assert(Cfg::supported, "k_gemm256: unsupported (layout, epilogue, tile) combination");
  constexpr bool PART = Cfg::PART, RS = Cfg::RS, DIRECT = Cfg::DIRECT, AUX = Cfg::AUX, F32OUT = Cfg::F32OUT;
  constexpr bool EARLY1 = Cfg::EARLY1, GTAB = Cfg::GTAB, S64 = Cfg::S64, ASYNC = Cfg::ASYNC;
  constexpr int BM = Cfg::BM, MH = Cfg::MH, BK = Cfg::BK, NT = Cfg::NT, WNX = Cfg::WNX, WM = Cfg::WM, WN = Cfg::WN;
  constexpr int PB = Cfg::PB, NTN = Cfg::NTN, A_BYTES = Cfg::A_BYTES, STAGE = Cfg::STAGE, DMAW = Cfg::DMAW;
  constexpr int NSL = Cfg::NSL, DIST = Cfg::DIST, USZ = Cfg::USZ, GSZ = Cfg::GSZ, SA = Cfg::SA, SB = Cfg::SB;
  constexpr int EA = Cfg::EA, EB = Cfg::EB, WRS = Cfg::WRS;
  static_assert(EA >= 2 && EB >= 3, "S64 waits assume at least one interval of DMA lead");
  static_assert(Cfg::SLOT_END <= Cfg::LDS_BYTES && Cfg::GTAB_END <= Cfg::LDS_BYTES && Cfg::RING_END <= Cfg::LDS_BYTES &&
                    Cfg::S64_END <= Cfg::RING_END && Cfg::TAB_END <= Cfg::LDS_BYTES && Cfg::RTAB_END <= Cfg::LDS_BYTES &&
                    Cfg::IMG_END <= Cfg::SLOT_END,
                "an LDS region ends past the array");
  static_assert(Cfg::lds_disjoint, "LDS regions overlap");
  static_assert(Cfg::LDS_BYTES * Cfg::BLOCKS_PER_CU <= LDS_PER_CU, "the CU's workgroups exceed its LDS");
  // first row of virtual m-tile i relative to the wave's first row (S64: two 64-row bands)
  auto rowoff = [](int i) { return S64 ? (i >> 2) * 128 + (i & 3) * 16 : i * 16; };
  __shared__ __attribute__((aligned(16))) char smem_raw[Cfg::LDS_BYTES];
  LDS_AS char* smem = (LDS_AS char*)smem_raw;
  [[maybe_unused]] LDS_AS char* ring = smem + Cfg::RING0;

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wr = wave / WNX, wc = wave % WNX;

  // Persistent walk. The logical tiles (K slice outermost, then the tile order) are cut into 8
  // contiguous runs, one per XCD (blocks b and b + 8 share an XCD); the P blocks of an XCD walk its
  // run with stride P, so the tiles an XCD has in flight are consecutive and share A / B panels in
  // its L2. Every block leaves after its last tile: no inter-block dependency.
  const int ntile = g.tiles_m * g.tiles_n;
  const int nb = ntile * g.nsplit;
  const int P = gridDim.x >> 3;
  const int xcd = blockIdx.x & 7, jb = blockIdx.x >> 3;
  const int q = nb >> 3, rmd = nb & 7;
  const int run0 = xcd < rmd ? xcd * (q + 1) : rmd * (q + 1) + (xcd - rmd) * q;
  const int runend = run0 + q + (xcd < rmd ? 1 : 0);
  if (run0 + jb >= runend) return;

  auto make_tile = [&](int wg) {
    Tile T;
    const int z = wg / ntile, w = wg - z * ntile;
    int tm, tn;
    if (g.group > 0) {  // runs of `group` tile rows walked column by column
      const int per = g.group * g.tiles_n, grp = w / per, first = grp * g.group;
      const int gm = min(g.tiles_m - first, g.group), loc = w - grp * per;
      tm = first + loc % gm;
      tn = loc / gm;
    } else {
      tm = w / g.tiles_n;
      tn = w - tm * g.tiles_n;
    }
    // wave-uniform by construction; readfirstlane keeps them in SGPRs (the divisions above run on
    // the VALU, and VGPRs are all taken by the accumulators and fragments)
    T.m0 = __builtin_amdgcn_readfirstlane(tm * BM);
    T.n0 = __builtin_amdgcn_readfirstlane(tn * BN);
    T.z = __builtin_amdgcn_readfirstlane(z);
    const int kb = T.z * g.kslice;
    T.Keff = min(g.K, kb + g.kslice) - kb;
    T.nk = (T.Keff + BK - 1) / BK;
    return T;
  };
  // buffer descriptors of a tile's A and B panels (from its K slice on; the range check zero-fills
  // ragged M / N / K)
  auto rsrc_a = [&](const Tile& T) {
    const int kb = T.z * g.kslice;
    const bf16_t* abase = AK ? g.A + (long)T.m0 * g.lda + kb : g.A + (long)kb * g.lda + T.m0;
    return make_rsrc(abase, AK ? clampb((long)(g.M - T.m0) * g.lda * 2 - kb * 2L)
                               : clampb(((long)(g.K - kb) * g.lda - T.m0) * 2));
  };
  auto rsrc_b = [&](const Tile& T) {
    const int kb = T.z * g.kslice;
    const bf16_t* bbase = BKM ? g.B + (long)T.n0 * g.ldb + kb : g.B + (long)kb * g.ldb + T.n0;
    return make_rsrc(bbase, BKM ? clampb((long)(g.N - T.n0) * g.ldb * 2 - kb * 2L)
                                : clampb(((long)(g.K - kb) * g.ldb - T.n0) * 2));
  };
  const bool iss = DMAW == 8 || wave < DMAW;  // this wave issues main-loop LDS-DMA pieces
  auto load_k = [&](__amdgpu_buffer_rsrc_t ra, __amdgpu_buffer_rsrc_t rb, const Tile& T, int t, int slot,
                    int lane) {
    LDS_AS char* s = smem + slot * STAGE;
    if (iss) {
      stage<AK, BM, false, DMAW, BK, WNX, PB>(ra, g.lda, g.M - T.m0, t * BK, T.Keff, s, wave, lane);
      stage<BKM, BN, DIRECT, DMAW, BK, WNX, PB>(rb, g.ldb, g.N - T.n0, t * BK, T.Keff, s + A_BYTES, wave, lane);
    }
  };
  auto load_tile = [&](const Tile& T, int t, int slot, int lane) {
    load_k(rsrc_a(T), rsrc_b(T), T, t, slot, lane);
  };
  // the next tile's stage 1, issued around the epilogue (no MFMAs to keep fed): all 8 waves
  auto load_tile8 = [&](const Tile& T, int t, int slot, int lane) {
    LDS_AS char* s = smem + slot * STAGE;
    stage<AK, BM, false, NWV, BK, WNX, PB>(rsrc_a(T), g.lda, g.M - T.m0, t * BK, T.Keff, s, wave, lane);
    stage<BKM, BN, DIRECT, NWV, BK, WNX, PB>(rsrc_b(T), g.ldb, g.N - T.n0, t * BK, T.Keff, s + A_BYTES, wave, lane);
  };

  // per-kernel tables (RoPE): global loads issued before the first DMA (so their waits do not queue
  // behind it), written to the table area after it; the first barrier of the tile loop publishes them
  constexpr int RTR = EPI == EPI_ROPE ? (ROPE_TAB_MAX + NT - 1) / NT : 0;
  [[maybe_unused]] f32x2 rpf[RTR > 0 ? RTR : 1];
  [[maybe_unused]] const int ntab = EPI == EPI_ROPE ? g.rope.npos * g.rope.half : 0;  // <= ROPE_TAB_MAX (host)
  if constexpr (EPI == EPI_ROPE) {
#pragma unroll
    for (int i = 0; i < RTR; ++i) {
      const int e = threadIdx.x + NT * i;
      rpf[i] = e < ntab ? f32x2{g.rope.cos_t[e], g.rope.sin_t[e]} : f32x2{0.f, 0.f};
    }
  }
  // tile-row positions (frame | row << 10 | col << 20) and the interleaved cos/sin table (RoPE)
  [[maybe_unused]] LDS_AS int* rpos = (LDS_AS int*)(smem + Cfg::RPOS_OFF);
  [[maybe_unused]] LDS_AS f32x2* rtab = (LDS_AS f32x2*)(smem + Cfg::RTAB_OFF);

  int wg = run0 + jb;
  Tile cur = make_tile(wg);
  int par = 0;  // LDS slot of K-tile t of the current tile: (t + par) & 1

  // ---- STG: staggered main loop (GEMM). 32-deep K units in a ring of 4 LDS slots (A
  // 256 x 32 then B 256 x 32, 16 KB each); the block's tiles form ONE stream of units (position q =
  // unit q % nku of the block's tile q / nku), and position q + 2 is DMA'd while q is computed, so the
  // next tile's first units arrive under this tile's last ones and its epilogue. Each wave issues 4
  // of the 32 1-KB pieces of every unit (waves 0-3: A, 4-7: B; their lane offsets are fixed per
  // tile, the unit's K offset rides in soffset), 2 per load interval; past the stream end the pieces
  // zero-fill an unread slot, so the per-wave vmcnt count stays 4.
  [[maybe_unused]] const int nku = STG ? (g.K + 31) / 32 : 0;
  // The ring position is a running wave-uniform byte offset (ring_step: one add and one wrap per
  // use): du = the DMA stream's unit slot; the unit to read lies DIST slots behind it. dku = the DMA
  // stream's unit within its tile (S64: its 64-deep step), whose K offset is the soffset of its pieces.
  [[maybe_unused]] int dwg = wg, du = 0, dku = 0;
  [[maybe_unused]] __amdgpu_buffer_rsrc_t drs;
  [[maybe_unused]] uint32_t dvo[4];
  const bool isA = wave < 4;
  auto dma_setup = [&]() {  // lane offsets / descriptor of this wave's operand of DMA tile dwg
    if (dwg < runend) {
      const Tile T = make_tile(dwg);
      const int left = isA ? g.M - T.m0 : g.N - T.n0;
      const long ld = isA ? g.lda : g.ldb;
      if (isA) drs = make_rsrc(g.A + (long)T.m0 * g.lda, clampb((long)left * g.lda * 2));
      else drs = make_rsrc(g.B + (long)T.n0 * g.ldb, clampb((long)left * g.ldb * 2));
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = (4 * (wave & 3) + j) * 16 + (lane >> 2);  // LDS row of the lane's 16-B chunk
        const int c = (lane & 3) ^ kswz32(r);                   // its logical chunk (64-B row swizzle)
        int gr = r;
        if (!isA) {  // PERM (stage()): LDS row r of a 64-row group holds group row 4 (r % 16) + r / 16
          const int rl = r & 63;
          gr = (r - rl) + 4 * (rl & 15) + (rl >> 4);
        }
        dvo[j] = gr < left ? (uint32_t)(gr * ld * 2 + c * 16) : VJ_OOB;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) dvo[j] = VJ_OOB;
    }
  };
  // this wave's pieces 2h, 2h + 1 of the DMA stream's unit (into the slot at du)
  auto dma_half = [&](auto h_c) {
    constexpr int h = decltype(h_c)::value;
    LDS_AS char* dst = ring + du + (isA ? 0 : 16384) + (4 * (wave & 3) + 2 * h) * 1024;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(drs, dst, 16, dvo[2 * h], dku * 64, 0, 0);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(drs, dst + 1024, 16, dvo[2 * h + 1], dku * 64, 0, 0);
    if constexpr (h == 1) {
      du = ring_step<NSL, USZ>(du);
      if (++dku == nku) {
        dku = 0;
        dwg += P;
        dma_setup();
      }
    }
  };
  // ---- S64 stream: this wave group's operand (A: waves 0-3, B: waves 4-7) as granules; position d of
  // the group's stream = (tile, step, half h), into slot d % SA (A) / SA + d % SB (B).
  // Each wave DMAs rows 32 (wave & 3) .. + 31 of every granule (4 pieces of 8 rows); its lane offsets
  // are fixed for the launch (rows relative to the granule's first row), the descriptor's range check
  // (from that row to the operand's end) zero-fills rows past M / N and, past the stream end (byte count 0),
  // whole granules, so the per-wave vmcnt counts never change.
  // Both descriptors of a tile (granule halves h = 0 / 1: rows 0-127 / 128-255 of the operand's tile
  // rows, each with its own clamped byte count) are built once, when the DMA stream enters the tile, and
  // kept as their six varying words (dlo, dhi, dcnt: two whole descriptors cost two SGPRs more, which
  // the kernels spill); a granule only picks its half and lines the words up. The position is a
  // running wave-uniform byte offset (ring_step): dd = the DMA stream's slot within the group's ring.
  // The two rings have the same size and DMA lead, so in either group the step's A0 and Blo lie EA
  // slots behind dd of their rings (one add and one wrap each). dku = the DMA stream's step within
  // its tile, whose K offset is the soffset of the granule's pieces.
  // A tile has an even number of granules, so the stream alternates h = 0, 1 without exception: the
  // half is a compile-time argument, and the tile switch can only follow an h = 1 granule.
  [[maybe_unused]] const int nks = S64 ? g.K >> 6 : 0;
  [[maybe_unused]] uint32_t dlo[2] = {0, 0}, dhi[2] = {0, 0}, dcnt[2] = {0, 0};
  [[maybe_unused]] int dd = 0;
  static_assert(SA == SB && EA == EB, "S64 reads both rings at one offset derived from the DMA slot");
  [[maybe_unused]] LDS_AS char* const dring = ring + (isA ? 0 : SA * GSZ) + (wave & 3) * 4096;
  auto dma_setup64 = [&]() {
    if (dwg < runend) {
      const Tile T = make_tile(dwg);
      const bf16_t* base = isA ? g.A + (long)T.m0 * g.lda : g.B + (long)T.n0 * g.ldb;
      const int left = isA ? g.M - T.m0 : g.N - T.n0;
      const long dld = isA ? g.lda : g.ldb;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const unsigned long long a = (unsigned long long)(base + h * 128 * dld);
        dlo[h] = __builtin_amdgcn_readfirstlane((int)(unsigned)a);
        dhi[h] = __builtin_amdgcn_readfirstlane((int)(unsigned)(a >> 32)) & 0xffff;
        dcnt[h] = __builtin_amdgcn_readfirstlane((int)clampb((long)(left - 128 * h) * dld * 2));
      }
    } else {  // past the stream end: empty ranges, every piece zero-fills
      dcnt[0] = dcnt[1] = 0;
    }
  };
  auto dma_gran = [&](auto h_c) {
    constexpr int h = decltype(h_c)::value;
    LDS_AS char* dst = dring + dd;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(dlo[h] | ((unsigned long long)dhi[h] << 32)), (short)0, (int)dcnt[h], 0x00020000);  // as make_rsrc
#pragma unroll
    for (int k = 0; k < 4; ++k)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, dst + k * 1024, 16, dvo[k], dku * 128, 0, 0);
    dd = ring_step<SA, GSZ>(dd);
    if constexpr (h == 1) {
      if (++dku == nks) {
        dku = 0;
        dwg += P;
        dma_setup64();
      }
    }
  };
  if constexpr (S64) {
    const long dld = isA ? g.lda : g.ldb;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int r = 32 * (wave & 3) + 8 * k + (lane >> 3);  // granule row of the lane's 16-B chunk
      const int c = (lane & 7) ^ ((r >> 1) & 7);            // its logical chunk (128-B row swizzle)
      const int rl = r & 63;                                 // B: PERM within 64-row groups (stage())
      const int gr = isA ? r : (r - rl) + 4 * (rl & 15) + (rl >> 4);
      dvo[k] = (uint32_t)(gr * dld * 2 + c * 16);
    }
    dma_setup64();
#pragma unroll
    for (int i = 0; i < cmax(EA, EB); ++i)
      if (i < (isA ? EA : EB)) {
        if (i & 1) dma_gran(std::integral_constant<int, 1>{});
        else dma_gran(std::integral_constant<int, 0>{});
      }
  } else if constexpr (STG) {
    dma_setup();
#pragma unroll
    for (int i = 0; i < DIST; ++i) {
      dma_half(std::integral_constant<int, 0>{});
      dma_half(std::integral_constant<int, 1>{});
    }
  } else {
    load_tile(cur, 0, 0, lane);
    if (cur.nk > 1) load_tile(cur, 1, 1, lane);
  }
  if constexpr (EPI == EPI_ROPE) {
#pragma unroll
    for (int i = 0; i < RTR; ++i) {
      const int e = threadIdx.x + NT * i;
      if (e < ntab) rtab[e] = rpf[i];
    }
  }
  // GELU table: computed once per (persistent) workgroup under the first units' DMA; read only in the
  // epilogues, after the first tile's barriers
  if constexpr (GTAB) gelu_tab_fill((LDS_AS f32x2*)(smem + Cfg::GTAB_OFF), threadIdx.x, NT);

  // Accumulators: acc[i][j] = m-tile i (16 rows), n block j; the epilogue walks the 2 * MH m-tiles,
  // 4 rows per lane (rows rowoff(i) + 4 (lane >> 4) + r of the wave tile).
  f32x4 acc[2 * MH][NTN];
  auto accv = [&](int i, int j, int r) -> float { return acc[i][j][r]; };
  auto accs = [&](int i, int j, int r, float v) { acc[i][j][r] = v; };
  bf16x8 Aa[MH], Ab[MH], Ba[NTN], Bb[NTN];
  // A fragments of M-half mh (4 m-tiles), k-step ks; B fragments of all NTN n-tiles, k-step ks
  auto rdA = [&](bf16x8 (&X)[MH], int slot, int mh, int ks) {
    const LDS_AS char* s = smem + slot * STAGE;
#pragma unroll
    for (int i = 0; i < MH; ++i) X[i] = frag<AK, BM, BK>(s, wr * WM + (mh * MH + i) * 16, ks, lane);
  };
  auto rdB = [&](bf16x8 (&Y)[NTN], int slot, int ks) {
    const LDS_AS char* s = smem + slot * STAGE + A_BYTES;
#pragma unroll
    for (int j = 0; j < NTN; ++j) Y[j] = frag<BKM, BN, BK>(s, wc * WN + j * 16, ks, lane);
  };
  // ---- fp8 (F8): one K-tile row is 128 B = 128 e4m3 values = ONE v_mfma_scale_f32_16x16x128_f8f6f4
  // per 16x16 output tile. Its 32-B lane operand is the two 16-B fragments the bf16 path reads for
  // k-steps 0 and 1 (chunks g and 4 + g of the row). A and B take the same byte -> k assignment, so
  // the product sums the same 128 terms. Fragments are read straight into 8-VGPR operand tuples (as
  // many VGPRs as the bf16 path's): Xa / Xb = the two m-tiles of an m-quarter q, alternating, and
  // Y8 = the n-tiles. The per-row scales are the same for every k of a row, so they ride in the
  // MFMA's per-lane E8M0 scale operands whatever the lane's k assignment: lane l of m-tile i scales
  // A row (i * 16 + (l & 15)) by 2^ea, of n-tile j B row (j * 16 + (l & 15)) by 2^eb (loaded per tile).
  [[maybe_unused]] int f8sa[8], f8sb[NTN];
  [[maybe_unused]] i32x8 Xa[2], Xb[2], Y8[NTN];
  auto cat = [](bf16x8 lo, bf16x8 hi) {
    const i32x4 l = __builtin_bit_cast(i32x4, lo), h = __builtin_bit_cast(i32x4, hi);
    return __builtin_shufflevector(l, h, 0, 1, 2, 3, 4, 5, 6, 7);
  };
  auto rdA8 = [&](i32x8 (&X)[2], int slot, int qq) {
    const LDS_AS char* s = smem + slot * STAGE;
#pragma unroll
    for (int i = 0; i < 2; ++i)
      X[i] = cat(frag<AK, BM>(s, wr * 128 + (2 * qq + i) * 16, 0, lane),
                 frag<AK, BM>(s, wr * 128 + (2 * qq + i) * 16, 1, lane));
  };
  auto rdB8 = [&](int j0, int j1, int slot) {
    const LDS_AS char* s = smem + slot * STAGE + A_BYTES;
#pragma unroll
    for (int j = j0; j < j1; ++j)
      Y8[j] = cat(frag<BKM, BN>(s, wc * WN + j * 16, 0, lane), frag<BKM, BN>(s, wc * WN + j * 16, 1, lane));
  };
  auto mm8 = [&](const i32x8 (&X)[2], int qq, int j0, int j1) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = j0; j < j1; ++j)
        acc[2 * qq + i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(X[i], Y8[j], acc[2 * qq + i][j], 0, 0,
                                                                              0, f8sa[2 * qq + i], 0, f8sb[j]);
  };
  // Fused bias gradient (EPI_PARTIAL_RS, tiles of column tile 0): row sums of the A
  // fragments the MFMAs already hold. Wave (wr, wc) sums m-tiles 2 wc and 2 wc + 1 of its 128-row
  // band (so the 4 waves of a band cover its 8 m-tiles once), in M-half wc / 2, with v_dot2 against
  // bf16 ones: 4 VALU per m-tile and k-step beside 16 MFMAs, two f32 registers per lane (lane l:
  // row l & 15, k = 8 (l >> 4) .. + 7; the 4 lane groups are summed in the epilogue).
  [[maybe_unused]] float rsa = 0.f, rsb = 0.f;
  [[maybe_unused]] bool rs_on = false;
  auto rsum8 = [](const bf16x8& x, float s) {
    typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
    const bf16x2_t one = {(__bf16)1.0f, (__bf16)1.0f};
    s = __builtin_amdgcn_fdot2_f32_bf16(__builtin_shufflevector(x, x, 0, 1), one, s, false);
    s = __builtin_amdgcn_fdot2_f32_bf16(__builtin_shufflevector(x, x, 2, 3), one, s, false);
    s = __builtin_amdgcn_fdot2_f32_bf16(__builtin_shufflevector(x, x, 4, 5), one, s, false);
    return __builtin_amdgcn_fdot2_f32_bf16(__builtin_shufflevector(x, x, 6, 7), one, s, false);
  };
  auto rs_phase = [&](const bf16x8 (&X)[MH], int mh) {
    if constexpr (RS && MH == 4) {
      if (rs_on && (wc >> 1) == mh) {  // wave-uniform
        if (wc & 1) {
          rsa = rsum8(X[2], rsa);
          rsb = rsum8(X[3], rsb);
        } else {
          rsa = rsum8(X[0], rsa);
          rsb = rsum8(X[1], rsb);
        }
      }
    }
  };
  auto mm = [&](const bf16x8 (&X)[MH], int mh, const bf16x8 (&Y)[NTN]) {
#pragma unroll
    for (int i = 0; i < MH; ++i)
#pragma unroll
      for (int j = 0; j < NTN; ++j)
        acc[mh * MH + i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(X[i], Y[j], acc[mh * MH + i][j], 0, 0, 0);
    rs_phase(X, mh);
  };
  // m-tiles i0 .. i1 - 1 of one phase (the last phase is split around the B DMA pieces)
  auto mm_rows = [&](const bf16x8 (&X)[MH], int mh, const bf16x8 (&Y)[NTN], int i0, int i1) {
#pragma unroll
    for (int i = 0; i < MH; ++i)
      if (i >= i0 && i < i1)
#pragma unroll
        for (int j = 0; j < NTN; ++j)
          acc[mh * MH + i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(X[i], Y[j], acc[mh * MH + i][j], 0, 0, 0);
    if (i1 == MH) rs_phase(X, mh);
  };
  // MN-major operands are read with asm transposed reads (ds_read_tr16_async): each phase first
  // waits for the fragments it consumes (read in the previous phase), then issues the next reads.
  auto release = [&](bf16x8 (&X)[MH], bf16x8 (&Y)[NTN]) {
    if constexpr (ASYNC) {
      lds_wait();
      tie(X);
      tie(Y);
    }
  };

#if VJ_GEMM_STAMPS
  int stamp_it = 0;
#endif
  // One tile per iteration, in this order (the vmcnt counts of the main loops depend on it):
  //  1. bookkeeping and prefetches (RoPE token ids, row-sum switch, fp8 scales, STG bias columns);
  //  2. the main loop of the kernel's form (S64 | 32-deep staggered | one tile), whose tail DMAs the next
  //     tile's stage 0, and its stage 1 where the epilogue neither needs the slot nor loads aux rows;
  //  3. the epilogue (direct | staged), with the next tile's stage 1 behind its last aux fetch;
  //  4. staged epilogue: the next tile's stage 1 into the image's slot;
  //  5. barrier bookkeeping and the step to the next tile.
  for (;;) {
#if VJ_GEMM_STAMPS
    const long st0 = __builtin_amdgcn_s_memtime();
    long st_k1 = 0;  // staggered loops: after the tile's first 64-deep K step
#endif
    // ---- 1. bookkeeping and prefetches
    const int wgn = wg + P;
    const bool has_next = wgn < runend;
    // the next tile's descriptors are rebuilt where they are used (SGPR pressure: 106 is the cap)
    const int nk = cur.nk;
    const int parn = (nk + par) & 1;     // the next tile's stage 0 reuses the slot this tile frees first
    const int sle = (nk - 1 + par) & 1;  // slot of the last K-tile: free once the loop ends
    [[maybe_unused]] int pf_id = 0;  // RoPE: token id of tile row threadIdx.x, read under the main loop
    if constexpr (EPI == EPI_ROPE) {
      const int t = threadIdx.x;
      if (t < BM && cur.m0 + t < g.M) pf_id = g.rope.ids ? g.rope.ids[cur.m0 + t] : (cur.m0 + t) % g.rope.mod;
    }
#pragma unroll
    for (int i = 0; i < 2 * MH; ++i)
#pragma unroll
      for (int j = 0; j < NTN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (RS) {
      rs_on = g.rsum && cur.n0 == 0;
      rsa = rsb = 0.f;
    }
    if constexpr (F8) {  // this tile's per-row scale exponents (retired by the wait below)
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int m = cur.m0 + wr * 128 + i * 16 + (lane & 15);
        f8sa[i] = 127 + (m < g.M ? g.ea[m] : 0);
      }
#pragma unroll
      for (int j = 0; j < NTN; ++j) {
        int r = wc * WN + j * 16 + (lane & 15);
        if constexpr (DIRECT) {  // permuted B staging: LDS row r holds global row NTN*(r%16) + r/16 of its group
          const int rl = r % WN;
          r = (r - rl) + NTN * (rl & 15) + (rl >> 4);
        }
        const int n = cur.n0 + r;
        f8sb[j] = 127 + (n < g.N ? g.eb[n] : 0);
      }
    }
    // STG: the bias columns are loaded before the main loop (in the epilogue the load would wait for
    // the next tile's DMA pieces issued after it: vmcnt counts in order)
    // (loads issued between the DMA pieces only ever make the main loop's counted vmcnt waits wait
    // longer, never shorter: its counts assume the DMA pieces alone)
    [[maybe_unused]] float biasp[NTN];
    if constexpr (STG) {
      const int nbp = cur.n0 + wc * WN + NTN * (lane & 15);
#pragma unroll
      for (int j = 0; j < NTN; ++j) biasp[j] = 0.f;
      if (EPI != EPI_GELU_BWD && g.bias && nbp < g.N) {
        const float4 bv = *(const float4*)(g.bias + nbp);
        biasp[0] = bv.x; biasp[1] = bv.y; biasp[2] = bv.z; biasp[3] = bv.w;
      }
    }
    // STG with a residual / saved-derivative epilogue: the first m-tile of aux rows is fetched one
    // unit before the tile ends (after that unit's DMA wait), so the epilogue's first reads do not
    // wait behind the next tile's DMA pieces
    [[maybe_unused]] f32x4 auxr[AUX && STG ? 4 : 1];
    auto stg_aux = [&] {
      if constexpr (AUX && STG) {
        const int m = cur.m0 + wr * WRS + 4 * (lane >> 4);
        const int n = cur.n0 + wc * WN + NTN * (lane & 15);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool ok = m + r < g.M && n < g.N;
          const long off = ok ? (long)(m + r) * g.ldaux + n : 0;
          if constexpr (EPI == EPI_F32_RESID) {
            auxr[r] = *(const f32x4*)((const float*)g.aux + off);
          } else {
            const uint2 x = *(const uint2*)((const bf16_t*)g.aux + off);
            auxr[r] = f32x4{__builtin_bit_cast(float, x.x), __builtin_bit_cast(float, x.y), 0.f, 0.f};
          }
        }
      }
    };
    // ---- 2. main loop
    if constexpr (S64) {
      // S64 main loop (above). Waits, with j = the group's load-interval index (A position j / B
      // position j are DMA'd EA / EB intervals ahead): waves 0-3 end every L with A position j + 1
      // landed (vmcnt(4 (EA - 1))); waves 4-7 end each L1 with the next step's Blo / Bhi (B positions
      // up to j + 2) landed (vmcnt(4 (EB - 2))); the barrier after an L publishes them to every wave.
      // The aux rows of a residual / saved-derivative epilogue (4 loads per lane) are fetched in the last
      // step's L0, after its DMA pieces: the L1 waits after them count 4 more.
      if (wg == run0 + jb) {  // first tile: A position 0 and B positions 0, 1 landed, RoPE table published
        if (isA) vm_wait<4 * (EA - 1)>();
        else vm_wait<4 * (EB - 2)>();
        __builtin_amdgcn_s_barrier();
        if (wr == 1) __builtin_amdgcn_s_barrier();
      }
      auto bar = [] {
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
      };
      // Aa / Ab: A fragments (m-tiles 0-3 of the wave's band) at k-steps 0 / 1; Ba / Bb: B fragments
      auto mm64 = [&](auto h_c) {
        constexpr int h = decltype(h_c)::value;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[4 * h + i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Aa[i], Ba[j], acc[4 * h + i][j], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[4 * h + i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ab[i], Bb[j], acc[4 * h + i][j], 0, 0, 0);
      };
#if VJ_GEMM_STAMPS
      long* ist = (stamp_it == 1 && (wave & 3) == 0 && lane == 0 && blockIdx.x < 2048)
                      ? vj_gemm_istamps + ((long)blockIdx.x * 2 + (wave >> 2)) * 16 : nullptr;
      auto istamp = [&](int s, int k) {
        if (ist && s >= 1 && s <= 4) ist[(s - 1) * 4 + k] = __builtin_amdgcn_s_memtime();
      };
#else
      auto istamp = [](int, int) {};
#endif
      for (int s = 0; s < nks; ++s) {
        const LDS_AS char* sA0 = ring + ring_step<SA, GSZ>(dd, SA - EA);
        const LDS_AS char* sA1 = ring + ring_step<SA, GSZ>(dd, SA - EA + 1);
        const LDS_AS char* sB = ring + SA * GSZ + ring_step<SB, GSZ>(dd, SB - EB + (wc >> 1));
        const bool last = s + 1 == nks;
        // L0
#pragma unroll
        for (int i = 0; i < 4; ++i) Aa[i] = frag<true, 128, 64>(sA0, wr * 64 + i * 16, 0, lane);
#pragma unroll
        for (int j = 0; j < 4; ++j) Ba[j] = frag<true, 128, 64>(sB, (wc & 1) * 64 + j * 16, 0, lane);
#pragma unroll
        for (int i = 0; i < 4; ++i) Ab[i] = frag<true, 128, 64>(sA0, wr * 64 + i * 16, 1, lane);
#pragma unroll
        for (int j = 0; j < 4; ++j) Bb[j] = frag<true, 128, 64>(sB, (wc & 1) * 64 + j * 16, 1, lane);
        dma_gran(std::integral_constant<int, EA & 1>{});
        if (isA) vm_wait<4 * (EA - 1)>();
        if (AUX && last) stg_aux();
        bar();
        istamp(s, 0);
        mm64(std::integral_constant<int, 0>{});
        bar();
        istamp(s, 1);
        // L1
#pragma unroll
        for (int i = 0; i < 4; ++i) Aa[i] = frag<true, 128, 64>(sA1, wr * 64 + i * 16, 0, lane);
#pragma unroll
        for (int i = 0; i < 4; ++i) Ab[i] = frag<true, 128, 64>(sA1, wr * 64 + i * 16, 1, lane);
        dma_gran(std::integral_constant<int, (EA & 1) ^ 1>{});
        // counts: pieces issued after the awaited granule (+ 4 aux loads in the last step)
        constexpr int WA = 4 * (EA - 1), WB = 4 * (EB - 2);
        if (AUX && last) {
          if (isA) vm_wait<WA + 4>();
          else vm_wait<WB + 4>();
        } else {
          if (isA) vm_wait<WA>();
          else vm_wait<WB>();
        }
        bar();
        istamp(s, 2);
        mm64(std::integral_constant<int, 1>{});
#if VJ_GEMM_STAMPS
        if (s == 0) st_k1 = __builtin_amdgcn_s_memtime();
#endif
        if (!last || wr == 0) bar();
        istamp(s, 3);
      }
    } else if constexpr (STG) {
      // Staggered main loop. Per unit, each wave runs L | M (intervals between workgroup
      // barriers): L = the unit's fragment reads (A m-tiles 0-7, B n-tiles 0-3: 12 ds_read_b128) + its
      // 4 DMA pieces of unit q + 2, M = the unit's 32 MFMAs. Waves 4-7 run one interval behind waves
      // 0-3 (one extra barrier before their first tile), so while one wave of a SIMD pair issues
      // MFMAs the other reads LDS / issues DMA. Every wave waits for its own pieces of unit q + 1 at
      // the end of L of unit q (vmcnt(4): the 4 pieces of unit q + 2 stay in flight); the barrier
      // after it orders them before any wave's reads of q + 1.
      // Tile boundary: waves 0-3 go from the last M1's barrier into the epilogue and on to the next
      // tile's L0; waves 4-7 skip that barrier (their epilogue starts right after the last MFMAs)
      // and take it after the epilogue, before the next tile's L0 - the pairing (and the
      // half-interval stagger) is unchanged and the two epilogues overlap.
      if (wg == run0 + jb) {  // first tile: unit 0 landed everywhere, RoPE table published
        if constexpr (DIST == 3) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (wr == 1) __builtin_amdgcn_s_barrier();
      }
      auto bar = [] {
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
      };
      for (int u = 0; u < nku; ++u) {
        const LDS_AS char* sA = ring + ring_step<NSL, USZ>(du, NSL - DIST);  // DIST slots behind the DMA
        const LDS_AS char* sB = sA + 16384;
#pragma unroll
        for (int i = 0; i < 4; ++i) Aa[i] = frag<true, 256, 32>(sA, wr * 128 + i * 16, 0, lane);
#pragma unroll
        for (int j = 0; j < NTN; ++j) Ba[j] = frag<true, 256, 32>(sB, wc * WN + j * 16, 0, lane);
#pragma unroll
        for (int i = 0; i < 4; ++i) Ab[i] = frag<true, 256, 32>(sA, wr * 128 + 64 + i * 16, 0, lane);
        dma_half(std::integral_constant<int, 0>{});
        dma_half(std::integral_constant<int, 1>{});
        // unit q + 1 landed: the pieces of units q + 2 .. q + DIST (4 each) stay in flight, and the aux
        // rows fetched one unit ago
        // rows fetched one unit ago (exactly 4 loads per lane: one per row). Any other load issued
        // after unit q + 1's pieces (the tile's bias / RoPE ids) only lengthens the wait.
        if (AUX && u == nku - 1 && nku > 1) {
          if constexpr (DIST == 3) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
          else asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        } else {
          if constexpr (DIST == 3) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
          else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        }
        if (AUX && u == nku - 2) stg_aux();
        if (AUX && nku == 1) stg_aux();
        bar();
        mm(Aa, 0, Ba);
        mm(Ab, 1, Ba);
#if VJ_GEMM_STAMPS
        if (u == 1) st_k1 = __builtin_amdgcn_s_memtime();
#endif
        if (u + 1 < nku || wr == 0) bar();
      }
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if constexpr (F8) {
        rdA8(Xa, par, 0);
        rdB8(0, NTN / 2, par);
      } else {
        rdA(Aa, par, 0, 0);
        rdB(Ba, par, 0);
      }

      // Per K-tile t: 4 phases, each with the fragments of the NEXT phase read while the current
      // phase's MFMAs run: (k-step, M-half) = (0,0) (0,1) (1,0) (1,1), 4*NTN MFMAs each. One barrier
      // per tile, before phase 3 (whose prefetch reads
      // tile t+1): it retires this wave's DMA of tile t+1 (issued one tile earlier) and its reads of
      // tile t; then slot (t + par) & 1 is free for the DMA of tile t+2, or of the next tile's stages
      // once this tile has none left.
      const __amdgpu_buffer_rsrc_t ra = rsrc_a(cur), rb = rsrc_b(cur);
      // 8-wave bf16 main loop: only the A pieces of K-tile t + 2 go out after the barrier; the B pieces
      // are issued inside the last phase's MFMAs (SPLIT: m-tiles / MFMAs before them)
      constexpr bool SPREAD = NWV == 8 && !F8 && BK == 64;
      constexpr int SPLIT = MH == 4 ? SPLIT_AT : MH - 1;
      // one K-tile; TAIL (the last two K-tiles) DMAs the next tile's stages instead of this tile's
      auto ktile = [&](const int t, auto tail_c) {
        constexpr bool TAIL = decltype(tail_c)::value;
        const int sl = (t + par) & 1;
        if constexpr (F8) {
          // m-quarters q0..q2 (A: Aa, Ab alternate); B's upper n-tiles of this K-tile arrive under
          // q0's lower-half MFMAs
          rdB8(NTN / 2, NTN, sl);
          rdA8(Xb, sl, 1);
          __builtin_amdgcn_sched_barrier(0);
          mm8(Xa, 0, 0, NTN / 2);
          mm8(Xa, 0, NTN / 2, NTN);
          __builtin_amdgcn_sched_barrier(0);
          rdA8(Xa, sl, 2);
          __builtin_amdgcn_sched_barrier(0);
          mm8(Xb, 1, 0, NTN);
          __builtin_amdgcn_sched_barrier(0);
          rdA8(Xb, sl, 3);
          __builtin_amdgcn_sched_barrier(0);
          mm8(Xa, 2, 0, NTN);
          __builtin_amdgcn_sched_barrier(0);
        } else if constexpr (BK == 32) {
          // one k-step: phase 0 = (M-half 0) under the read of M-half 1's A fragments; phase 1 after
          // the barrier, the next K-tile's fragments read under its MFMAs
          rdA(Ab, sl, 1, 0);
          __builtin_amdgcn_sched_barrier(0);
          mm(Aa, 0, Ba);
          __builtin_amdgcn_sched_barrier(0);
        } else {
          release(Aa, Ba);
          rdA(Ab, sl, 1, 0);
          __builtin_amdgcn_sched_barrier(0);
          mm(Aa, 0, Ba);
          __builtin_amdgcn_sched_barrier(0);
          release(Ab, Ba);
          rdA(Aa, sl, 0, 1);
          rdB(Bb, sl, 1);
          __builtin_amdgcn_sched_barrier(0);
          mm(Ab, 1, Ba);
          __builtin_amdgcn_sched_barrier(0);
          release(Aa, Bb);
          rdA(Ab, sl, 1, 1);
          __builtin_amdgcn_sched_barrier(0);
          mm(Aa, 0, Bb);
          __builtin_amdgcn_sched_barrier(0);
        }
        if (t + 1 < nk) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        else asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the next tile's stage 0 stays in flight
        if constexpr (ASYNC) {
          tie(Ab);
          tie(Bb);
        }
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (!TAIL) {
          if constexpr (SPREAD) {
            if (iss)
              stage<AK, BM, false, DMAW, BK, WNX, PB>(ra, g.lda, g.M - cur.m0, (t + 2) * BK, cur.Keff,
                                                       smem + sl * STAGE, wave, lane);
          } else {
            load_k(ra, rb, cur, t + 2, sl, lane);
          }
        } else if (has_next) {
          // slot sl is free: the next tile's stage 0 (t == nk-2) or stage 1 (t == nk-1; stage 0 goes
          // to the other, unused slot when nk == 1); stage 1 waits for the epilogue unless EARLY1
          int lt = lane;
          asm volatile("" : "+v"(lt));  // tail-only addressing: not hoisted across the main loop
          const Tile nx = make_tile(wgn);
          if (t + 2 == nk) {
            load_tile(nx, 0, sl, lt);
          } else {
            if (nk == 1) load_tile(nx, 0, sl ^ 1, lt);
            if (EARLY1 && nx.nk > 1) load_tile8(nx, 1, sl, lt);
          }
        }
        auto b_pieces = [&] {
          if (iss)
            stage<BKM, BN, DIRECT, DMAW, BK, WNX, PB>(rb, g.ldb, g.N - cur.n0, (t + 2) * BK, cur.Keff,
                                                       smem + sl * STAGE + A_BYTES, wave, lane);
        };
        if constexpr (F8) {
          // q3; the next K-tile's q0 A fragments and lower B n-tiles are read under it
          if (t + 1 < nk) rdA8(Xa, sl ^ 1, 0);
          __builtin_amdgcn_sched_barrier(0);
          mm8(Xb, 3, 0, NTN / 2);
          __builtin_amdgcn_sched_barrier(0);
          if (t + 1 < nk) rdB8(0, NTN / 2, sl ^ 1);
          __builtin_amdgcn_sched_barrier(0);
          mm8(Xb, 3, NTN / 2, NTN);
          __builtin_amdgcn_sched_barrier(0);
        } else if constexpr (BK == 32) {
          mm(Ab, 1, Ba);
          __builtin_amdgcn_sched_barrier(0);
          if (t + 1 < nk) {  // overwrite Aa / Ba once phase 1's MFMAs have been issued
            rdA(Aa, sl ^ 1, 0, 0);
            rdB(Ba, sl ^ 1, 0);
          }
          __builtin_amdgcn_sched_barrier(0);
        } else {
          if (t + 1 < nk) {
            rdA(Aa, sl ^ 1, 0, 0);
            rdB(Ba, sl ^ 1, 0);
          }
          __builtin_amdgcn_sched_barrier(0);
          if constexpr (SPREAD && !TAIL) {
            mm_rows(Ab, 1, Bb, 0, SPLIT);
            __builtin_amdgcn_sched_barrier(0);
            b_pieces();
            __builtin_amdgcn_sched_barrier(0);
            mm_rows(Ab, 1, Bb, SPLIT, MH);
          } else {
            mm(Ab, 1, Bb);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      };
      int t = 0;
      for (; t + 2 < nk; ++t) ktile(t, std::false_type{});
      for (; t < nk; ++t) ktile(t, std::true_type{});
    }

    // ---- 3. epilogue. Its lane-derived addressing is recomputed per tile (an opaque copy of the lane id
    // keeps the compiler from hoisting it out of the tile loop, where it would hold VGPRs across the
    // main loop)
#if VJ_GEMM_STAMPS
    const long st1 = __builtin_amdgcn_s_memtime();
#endif
    int lane_e = lane;
    asm volatile("" : "+v"(lane_e));
    if constexpr (DIRECT) {
      const int lane = lane_e;
      const int lrow = 4 * (lane >> 4);  // the lane's row offset in an m-tile
      // ---- direct epilogue (K-major B staged with PERM): lane (c = lane&15, g = lane>>4) owns rows
      // rowoff(i) + 4g + r of m-tile i and the NTN
      // consecutive columns nb .. nb+NTN-1, so every row goes out of registers as one 8/16-B store;
      // no LDS round trip.
      const int nb = cur.n0 + wc * WN + NTN * (lane & 15);
      const bool nok = nb < g.N;
      const int mb = cur.m0 + wr * WRS + lrow;
      float bias[NTN];
#pragma unroll
      for (int j = 0; j < NTN; ++j) bias[j] = STG ? biasp[j] : 0.f;
      if (!STG && EPI != EPI_GELU_BWD && !PART && g.bias && nok)
#pragma unroll
        for (int j = 0; j < NTN; ++j) bias[j] = g.bias[nb + j];
      // RoPE (modules.py:26-50, 343-365): tile rows' (frame, row, col) positions + interleaved
      // cos/sin table in LDS; this lane's NTN/2 column pairs fix slice/axis/frequency once.
      [[maybe_unused]] bool ract[NTN / 2];
      [[maybe_unused]] int rsh[NTN / 2], rf0[NTN / 2], rf1[NTN / 2];
      if constexpr (EPI == EPI_ROPE) {
        const RopeP& r = g.rope;
        const int t = threadIdx.x;
        if (t < BM) {  // the previous tile's readers are past this tile's main-loop barriers
          const int fr = pf_id / r.tpf, rem = pf_id - r.tpf * fr, hr = rem / r.tpr;
          rpos[t] = fr | (hr << 10) | ((rem - r.tpr * hr) << 20);
        }
        const int sw = 2 * r.half, e0 = (nb % r.D) % r.hd;
#pragma unroll
        for (int p = 0; p < NTN / 2; ++p) {
          const int e = e0 + 2 * p, ax = e / sw, js = e - ax * sw;
          ract[p] = nok && nb < 2 * r.D && e < 3 * sw;
          rsh[p] = 10 * ax;
          rf0[p] = js % r.half;
          rf1[p] = (js + 1) % r.half;
        }
        __syncthreads();
      }
      // residual (f32) / pre-activation (bf16 bits) rows: m-tile i+1's fetched while m-tile i is stored
      // AUX_PF m-tiles of rows in flight. Stamped (tools/gemm_stamps.py): the residual epilogue takes
      // ~36k cycles per tile vs ~10k without the reads, but deeper prefetch (3, 5, 7) measured no
      // faster: the 64 MB of residual every CU reads at once is the bound, not the latency chain
      [[maybe_unused]] float aux[AUX_PF + 1][4][NTN];
      // per-tile lane offsets (elements): row r of virtual m-tile i is then + (rowoff(i) + r) * ld, a
      // wave-uniform (scalar) product, instead of a 64-bit multiply per row
      [[maybe_unused]] const long off_aux = AUX ? (long)mb * g.ldaux + nb : 0;
      auto fetch = [&](int i, float (&dst)[4][NTN]) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int m = mb + rowoff(i) + r;
          const bool ok = m < g.M && nok;
          const long off = ok ? off_aux + (long)(rowoff(i) + r) * g.ldaux : 0;
          if constexpr (EPI == EPI_F32_RESID) {
            if constexpr (NTN == 4) {
              const float4 x = *(const float4*)((const float*)g.aux + off);
              dst[r][0] = x.x; dst[r][1] = x.y; dst[r][2] = x.z; dst[r][3] = x.w;
            } else {
              const float2 x = *(const float2*)((const float*)g.aux + off);
              dst[r][0] = x.x; dst[r][1] = x.y;
            }
          } else {
            if constexpr (NTN == 4) {  // saved GELU derivative
              const uint2 x = *(const uint2*)((const bf16_t*)g.aux + off);
              dst[r][0] = bf_lo(x.x); dst[r][1] = bf_hi(x.x);
              dst[r][2] = bf_lo(x.y); dst[r][3] = bf_hi(x.y);
            } else {
              const uint32_t x = *(const uint32_t*)((const bf16_t*)g.aux + off);
              dst[r][0] = bf_lo(x); dst[r][1] = bf_hi(x);
            }
          }
        }
      };
      // bf16 rows widened to 16-B stores: lanes c (even) and c + 1 swap row halves, so the even lane
      // stores rows 0, 1 and the odd lane rows 2, 3 of the 8 columns 4 (c & ~1) .. + 7 (N % 8 == 0)
      const bool odd = lane & 1;
      const int nb8 = nb - (odd ? 4 : 0);
      const bool nok8 = nb8 < g.N;
      const int mrow = mb + (odd ? 2 : 0);  // first row this lane stores of a virtual m-tile
      // every register index below is a compile-time constant (a lane-dependent row index into pk
      // compiled to a compare / select chain over all 8 words per store)
      auto store_wide = [&](bf16_t* base, long ld, long off, int i, const uint32_t (&pk)[4][2]) {
        uint32_t snd[4], keep[4], rcv[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          snd[k] = odd ? pk[k >> 1][k & 1] : pk[2 + (k >> 1)][k & 1];
          keep[k] = odd ? pk[2 + (k >> 1)][k & 1] : pk[k >> 1][k & 1];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) rcv[k] = dpp_u<DPP_XOR1>(snd[k]);  // lane pair exchange on the VALU
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          if (mrow + rowoff(i) + h < g.M && nok8) {
            const uint32_t a = 2 * h, b = 2 * h + 1;
            const uint4 v = make_uint4(odd ? rcv[a] : keep[a], odd ? rcv[b] : keep[b], odd ? keep[a] : rcv[a],
                                       odd ? keep[b] : rcv[b]);
            *(uint4*)(base + off + (long)(rowoff(i) + h) * ld) = v;
          }
        }
      };
      // per-tile lane offsets of the bf16 outputs (C, C2) and the f32 output rows
      [[maybe_unused]] const long off_c = (long)mrow * g.ldc + nb8;
      [[maybe_unused]] const long off_c2 = EPI == EPI_GELU ? (long)mrow * g.ldc2 + nb8 : 0;
      [[maybe_unused]] const long off_f = PART ? ((long)cur.z * g.M + mb) * g.N + nb
                                                             : (long)mb * g.ldc + nb;
      [[maybe_unused]] const long ld_f = PART ? (long)g.N : g.ldc;
      [[maybe_unused]] float* const base_f = PART ? g.ws : (float*)g.C;
      if constexpr (AUX)
#pragma unroll
        for (int i = 0; i < AUX_PF; ++i) {
          if constexpr (STG) {  // m-tile 0, fetched under the last unit
            static_assert(AUX_PF == 1, "STG prefetches one m-tile of aux rows");
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              if constexpr (EPI == EPI_F32_RESID) {
#pragma unroll
                for (int j = 0; j < NTN; ++j) aux[0][r][j] = auxr[r][j];
              } else {
                aux[0][r][0] = bf_lo(auxr[r][0]); aux[0][r][1] = bf_hi(auxr[r][0]);
                aux[0][r][2] = bf_lo(auxr[r][1]); aux[0][r][3] = bf_hi(auxr[r][1]);
              }
            }
          } else {
            fetch(i, aux[i]);
          }
        }
      // GELU: the derivative pass is compiled separately, for callers that save it (g.C)
      auto rows = [&](auto save_c) {
      constexpr bool SAVE_D = decltype(save_c)::value;
#pragma unroll
      for (int i = 0; i < 2 * MH; ++i) {
        if constexpr (AUX) {
          if (i + AUX_PF < 2 * MH) fetch(i + AUX_PF, aux[(i + AUX_PF) % (AUX_PF + 1)]);
          if (!STG && i == 2 * MH - 1 - AUX_PF && has_next) {  // behind the last aux fetch
            const Tile nxt = make_tile(wgn);
            if (nxt.nk > 1) load_tile8(nxt, 1, sle, lane);
          }
        }
        if constexpr (F32OUT && NTN == 4) {
          // f32 rows stored from the accumulators themselves: a 4x4 in-place transpose (tied swaps)
          // turns accv(i, r, 0..3) into row r's 4 columns, bias / residual are added in place (tied
          // adds). Stores read their data registers after issue, so staging copies recycled from row
          // to row cost one memory latency per 16-B store; the accumulators are not reused before the
          // next tile.
#pragma unroll
          for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = a + 1; b < 4; ++b) {
              float x = accv(i, a, b), y = accv(i, b, a);
              asm volatile("v_swap_b32 %0, %1" : "+v"(x), "+v"(y));
              accs(i, a, b, x);
              accs(i, b, a, y);
            }
#pragma unroll
          for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              float x = accv(i, r, e);
              asm volatile("v_add_f32 %0, %0, %1" : "+v"(x) : "v"(bias[e]));
              if constexpr (EPI == EPI_F32_RESID) asm volatile("v_add_f32 %0, %0, %1" : "+v"(x) : "v"(aux[i % (AUX_PF + 1)][r][e]));
              accs(i, r, e, x);
            }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int m = mb + rowoff(i) + r;
            if (m < g.M && nok) {
              float* dst = base_f + off_f + (long)(rowoff(i) + r) * ld_f;
              *(f32x4*)dst = acc[i][r];
            }
          }
          continue;
        }
        [[maybe_unused]] uint32_t pk[4][2], ga[4][2];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int m = mb + rowoff(i) + r;
          float v[NTN];
#pragma unroll
          for (int j = 0; j < NTN; ++j) v[j] = accv(i, j, r) + bias[j];
          if constexpr (EPI == EPI_ROPE) {
            const int rp = rpos[wr * WRS + rowoff(i) + lrow + r];
#pragma unroll
            for (int p = 0; p < NTN / 2; ++p) {
              if (!ract[p]) continue;
              const int pos = min((rp >> rsh[p]) & 1023, g.rope.npos - 1) * g.rope.half;
              const f32x2 a = rtab[pos + rf0[p]], b = rtab[pos + rf1[p]];
              const float x0 = v[2 * p], x1 = v[2 * p + 1];
              v[2 * p] = x0 * a[0] - x1 * a[1];
              v[2 * p + 1] = x1 * b[0] + x0 * b[1];
            }
          }
          if constexpr (EPI == EPI_F32_RESID || EPI == EPI_BF16_RESID) {
#pragma unroll
            for (int j = 0; j < NTN; ++j) v[j] += aux[i % (AUX_PF + 1)][r][j];
          }
          if constexpr (F32OUT) {
            if (m < g.M && nok) {
              float* dst = base_f + off_f + (long)(rowoff(i) + r) * ld_f;
              *(float4*)dst = make_float4(v[0], v[1], v[2], v[3]);
            }
          } else {
#pragma unroll
            for (int q2 = 0; q2 < 2; ++q2) {
              if constexpr (EPI == EPI_GELU_BWD)
                pk[r][q2] = pack_bf2(v[2 * q2] * aux[i % (AUX_PF + 1)][r][2 * q2],
                                     v[2 * q2 + 1] * aux[i % (AUX_PF + 1)][r][2 * q2 + 1]);
              else
                pk[r][q2] = pack_bf2(v[2 * q2], v[2 * q2 + 1]);
              if constexpr (EPI == EPI_GELU) {  // pk: the bf16 pre-activation -> GELU, derivative (if saved)
                if constexpr (GTAB) ga[r][q2] = gelu_pair_tab<SAVE_D>(pk[r][q2], smem + Cfg::GTAB_OFF, &pk[r][q2]);
                else ga[r][q2] = gelu_pair(pk[r][q2], SAVE_D ? &pk[r][q2] : nullptr);
              }
            }
          }
        }
        if constexpr (!F32OUT) {
          if (EPI != EPI_GELU || SAVE_D) store_wide((bf16_t*)g.C, g.ldc, off_c, i, pk);
          if constexpr (EPI == EPI_GELU) store_wide((bf16_t*)g.C2, g.ldc2, off_c2, i, ga);
        }
      }
      };
      if (EPI == EPI_GELU && g.C) rows(std::true_type{});
      else rows(std::false_type{});
    } else {
      const int lane = lane_e;
      // ---- staged epilogue: passes of MTP m-tiles (16*MTP rows) per wave through a padded image in
      // the last K-tile's slot (free now; the next tile's stage 1 is DMA'd there afterwards): 2 m-tiles
      // per pass where the image fits the slot (BN = 128), else 1
      constexpr int STR = Cfg::STR, LPR = Cfg::LPR, RPI = Cfg::RPI, MTP = Cfg::MTP, PR = Cfg::PR, IT = Cfg::IT;
      LDS_AS float* wl = (LDS_AS float*)(smem + sle * STAGE + wave * PR * STR * 4);
      if constexpr (RS && MH == 4) {
        if (rs_on) {  // the row sums: lane groups (k sub-ranges) added, rows 32 wc + 16 (lane >> 4) + (lane & 15)
          float sa = rsa + __shfl_xor(rsa, 16), sb = rsb + __shfl_xor(rsb, 16);
          sa += __shfl_xor(sa, 32);
          sb += __shfl_xor(sb, 32);
          const int m = cur.m0 + wr * 128 + 32 * wc + (lane & 31);
          if (lane < 32 && m < g.M) g.rsum[(long)cur.z * g.M + m] = lane < 16 ? sa : sb;
        }
      }
      bool ract[2] = {false, false};
      int rsh[2] = {0, 0}, rf0[2] = {0, 0}, rf1[2] = {0, 0};
      const int col = (lane % LPR) * 4;  // this thread's 4 columns, fixed for every row it stores
      const int ncol = cur.n0 + wc * WN + col;
      if constexpr (EPI == EPI_ROPE) {
        const RopeP& r = g.rope;
        const int t = threadIdx.x;
        if (t < BM) {
          const int fr = pf_id / r.tpf, rem = pf_id - r.tpf * fr, hr = rem / r.tpr;
          rpos[t] = fr | (hr << 10) | ((rem - r.tpr * hr) << 20);
        }
        const int sw = 2 * r.half, e0 = (ncol % r.D) % r.hd;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
          const int e = e0 + 2 * p, ax = e / sw, js = e - ax * sw;
          ract[p] = ncol < 2 * r.D && e < 3 * sw;
          rsh[p] = 10 * ax;
          rf0[p] = js % r.half;
          rf1[p] = (js + 1) % r.half;
        }
        __syncthreads();
      }
      float4 bias4 = make_float4(0.f, 0.f, 0.f, 0.f);
      if (EPI != EPI_GELU_BWD && !PART && g.bias && ncol < g.N) bias4 = *(const float4*)(g.bias + ncol);
#pragma unroll
      for (int pass = 0; pass < 8 / MTP; ++pass) {
#pragma unroll
        for (int ii = 0; ii < MTP; ++ii)
#pragma unroll
          for (int j = 0; j < NTN; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
              wl[(ii * 16 + (lane >> 4) * 4 + r) * STR + j * 16 + (lane & 15)] = acc[pass * MTP + ii][j][r];
        __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): own writes visible to own reads (wave-private)
        // residual / GELU pre-activation rows of this pass fetched up front: one memory latency per
        // pass instead of one per row
        [[maybe_unused]] float4 rres[EPI == EPI_F32_RESID ? IT : 1];
        [[maybe_unused]] uint2 rpre[EPI == EPI_GELU_BWD || EPI == EPI_BF16_RESID ? IT : 1];
        if constexpr (AUX) {
#pragma unroll
          for (int it = 0; it < IT; ++it) {
            const int m = cur.m0 + wr * 128 + pass * PR + it * RPI + lane / LPR;
            const bool ok = m < g.M && ncol < g.N;
            const long mm2 = ok ? m : 0;
            const int nn = ok ? ncol : 0;
            if constexpr (EPI == EPI_F32_RESID) rres[it] = *(const float4*)((const float*)g.aux + mm2 * g.ldaux + nn);
            else rpre[it] = *(const uint2*)((const bf16_t*)g.aux + mm2 * g.ldaux + nn);
          }
        }
#pragma unroll
        for (int it = 0; it < IT; ++it) {
          const int row = it * RPI + lane / LPR;
          const f32x4 v4 = *(const LDS_AS f32x4*)(wl + row * STR + col);
          const int m = cur.m0 + wr * 128 + pass * PR + row;
          const int n = ncol;
          if (m >= g.M || n >= g.N) continue;
          float v[4] = {v4[0] + bias4.x, v4[1] + bias4.y, v4[2] + bias4.z, v4[3] + bias4.w};
          if constexpr (EPI == EPI_BF16 || EPI == EPI_ROPE) {
            if constexpr (EPI == EPI_ROPE) {
              const int rp = rpos[wr * 128 + pass * PR + row];
#pragma unroll
              for (int p = 0; p < 2; ++p) {
                if (!ract[p]) continue;
                const int pos = min((rp >> rsh[p]) & 1023, g.rope.npos - 1) * g.rope.half;
                const f32x2 a = rtab[pos + rf0[p]], b = rtab[pos + rf1[p]];
                const float x0 = v[2 * p], x1 = v[2 * p + 1];
                v[2 * p] = x0 * a[0] - x1 * a[1];
                v[2 * p + 1] = x1 * b[0] + x0 * b[1];
              }
            }
            *(uint2*)((bf16_t*)g.C + (long)m * g.ldc + n) = make_uint2(pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]));
          } else if constexpr (EPI == EPI_F32) {
            *(float4*)((float*)g.C + (long)m * g.ldc + n) = make_float4(v[0], v[1], v[2], v[3]);
          } else if constexpr (PART) {
            *(float4*)(g.ws + ((long)cur.z * g.M + m) * g.N + n) = make_float4(v[0], v[1], v[2], v[3]);
          } else if constexpr (EPI == EPI_F32_RESID) {
            const float4 rr = rres[it];
            *(float4*)((float*)g.C + (long)m * g.ldc + n) = make_float4(rr.x + v[0], rr.y + v[1], rr.z + v[2], rr.w + v[3]);
          } else if constexpr (EPI == EPI_GELU) {
            uint32_t d0, d1;
            const uint32_t a0 = gelu_pair(pack_bf2(v[0], v[1]), &d0), a1 = gelu_pair(pack_bf2(v[2], v[3]), &d1);
            if (g.C) *(uint2*)((bf16_t*)g.C + (long)m * g.ldc + n) = make_uint2(d0, d1);
            *(uint2*)((bf16_t*)g.C2 + (long)m * g.ldc2 + n) = make_uint2(a0, a1);
          } else if constexpr (EPI == EPI_BF16_RESID) {
            const uint2 pu = rpre[it];  // bf16 residual
            *(uint2*)((bf16_t*)g.C + (long)m * g.ldc + n) =
                make_uint2(pack_bf2(bf_lo(pu.x) + v[0], bf_hi(pu.x) + v[1]), pack_bf2(bf_lo(pu.y) + v[2], bf_hi(pu.y) + v[3]));
          } else {  // EPI_GELU_BWD
            const uint2 pu = rpre[it];  // saved GELU derivative (bf16)
            *(uint2*)((bf16_t*)g.C + (long)m * g.ldc + n) =
                make_uint2(pack_bf2(v[0] * bf_lo(pu.x), v[1] * bf_hi(pu.x)), pack_bf2(v[2] * bf_lo(pu.y), v[3] * bf_hi(pu.y)));
          }
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);
      }
      // ---- 4. the next tile's stage 1
      __syncthreads();  // every wave is done with its image before the slot is DMA'd
      if (has_next) {
        const Tile nxt = make_tile(wgn);
        if (nxt.nk > 1) load_tile8(nxt, 1, sle, lane);
      }
    }

#if VJ_GEMM_STAMPS
    {
      if constexpr (!STG) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // STG: the DMA stream runs on
      const long st2 = __builtin_amdgcn_s_memtime();
      if (threadIdx.x == 0 && blockIdx.x < 2048 && stamp_it < 16) {
        long* d = vj_gemm_stamps + ((long)blockIdx.x * 16 + stamp_it) * 4;
        d[0] = st0; d[1] = st1; d[2] = st2; d[3] = st_k1;
      }
      ++stamp_it;
    }
#endif
    // ---- 5. barrier bookkeeping, next tile
    if constexpr (STG) {
      // waves 4-7: the barrier skipped after their last MFMAs (see the main loop); waves 0-3: the
      // matching one after the block's last tile, so both halves end with equal barrier counts
      if (wr == 1 || !has_next) __builtin_amdgcn_s_barrier();
    }
    if (!has_next) break;
    wg = wgn;
    cur = make_tile(wgn);
    par = parn;
  }
}

int num_cus() {
  static int cus[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
  if (cus[dev] <= 0) {
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256;
    cus[dev] = v;
  }
  return cus[dev];
}

// The environment knobs of the kernel choice, read per call (the tests change them between launches).
// Switches: -1 = unset, else 0 / 1 (any other value counts as unset).
struct Knobs {
  int stg, stg64, bm192, w2, w2_192;
  int group;  // VJ_GEMM_GROUP: -1 = unset, 0 = row-major, n = tile rows per group
  int pxcd;   // VJ_GEMM_PXCD: blocks per XCD (0 = unset)
};
Knobs read_knobs() {
  auto sw = [](const char* name) {
    const char* e = getenv(name);
    return e && (e[0] == '0' || e[0] == '1') ? e[0] - '0' : -1;
  };
  const char* grp = getenv("VJ_GEMM_GROUP");
  const char* px = getenv("VJ_GEMM_PXCD");
  return Knobs{sw("VJ_GEMM_STG"),   sw("VJ_GEMM_STG64"), sw("VJ_GEMM_BM192"),
               sw("VJ_GEMM_2W"),    sw("VJ_GEMM_2W192"), grp ? (atoi(grp) > 0 ? atoi(grp) : 0) : -1,
               px && atoi(px) > 0 ? atoi(px) : 0};
}

// Persistent grid: one block per CU (capped by the tile count), a multiple of 8 so every XCD gets
// the same number of blocks. VJ_GEMM_PXCD caps the blocks per XCD (tests: many tiles per block).
// (A phase offset between the blocks of an XCD, so odd blocks' epilogues fall under the even
// blocks' main loops, measured no gain in round 3 and was removed.)
// CUs the persistent grids leave free (vj_set_reserved_cus): while a data-parallel rank's gradient
// buckets are all-reduced, RCCL's channel kernels hold CUs; a persistent GEMM block that cannot be
// placed on one of them only starts when it frees, and its statically assigned tiles then run after
// every other block's (measured on one GPU with a 16-CU proxy copy: step -11.6 %,
// profiles/r06_rccl_proxy_ab.txt). Set by distributed.GradReducer around its bucket window.
std::atomic<int> g_reserved_cus{0};

int grid256(long nb, int per_cu, const Knobs& kn) {
  int per_xcd = per_cu * (num_cus() - g_reserved_cus.load(std::memory_order_relaxed)) / 8;
  if (kn.pxcd > 0) per_xcd = kn.pxcd;
  if (per_xcd < 1) per_xcd = 1;
  const long need = (nb + 7) / 8;
  return 8 * (int)(need < per_xcd ? need : per_xcd);
}

// Grouped tile order (tile rows per group): a square-ish set of the ~32 tiles an XCD has in flight
// shares fewer A / B panels in its L2. Measured (tools/bench_kernels.py, MI355X): groups of 8 rows
// pay on tall problems (target fc1 M = 49152: -7 %, predictor fc1 / fc2 / dgrad M = 71232: -3..-10 %)
// and cost 2-5 % on the ~46-row-tile context problems (round 3). With the round-4 kernels and the
// concurrent streams, groups of 4 rows on every problem measured best per step: +0.4 % / +0.25 % over
// 8-or-row-major, +0.1 % over 8 on the tall ones with 4 on the rest (profiles/r04_gemm_group_ab.txt;
// in isolation 8 is still ~1 % ahead on the target fc1 / QKV, 4 ahead on context QKV / dgrad).
// VJ_GEMM_GROUP overrides (0 = row-major; tests: grouped order at small sizes).
int tile_group(const Knobs& kn) { return kn.group >= 0 ? kn.group : 4; }

// 256-wide column tiles unless the last one would waste more than 15 % of the work (measured,
// tools/bench_kernels.py: predictor QKV N = 1152 -17 % with 256-wide tiles; N = 384 +14 %; 256-wide
// tiles for every N > 256: DESIGN.md). The split-K weight gradients take the same rule: ViT-g's
// N = 1408 runs 6 tiles of 256 instead of 11 of 128 (twice the work per operand byte).
bool wide_tile_ok(int N) { return N % 256 == 0 || (N > 256 && vj_cdiv(N, 256) * 256L * 100 <= 115L * N); }

// Which kernel a GEMM gets: tile rows (256 / 192) x columns (256 / 128), waves (8 / 4), main loop
// (stg: 0 = one tile, 1 = staggered 32-deep units, 2 = S64), workgroups per CU and the tile group.
struct Plan256 {
  bool ok;  // false: the 256-row kernel declines the problem
  int bm, bn, waves, stg, per_cu, group;
};

// The choice, a pure function of the problem, the CU count and the knobs.
//  * 4 waves, two workgroups per CU (NWV = 4), for K-major GEMMs whose N needs 128-wide tiles: the
//    direct-store epilogue overlaps the other workgroup's MFMAs. Measured (tools/bench_kernels.py):
//    predictor fc2 N = 384 (f32 residual epilogue) -14 %, N = 384 bf16 even; on 256-wide shapes the
//    32-deep main loop loses 10-20 %, so they stay on the 8-wave kernel. VJ_GEMM_2W: 0 = never, 1 = every
//    K-major GEMM, unset = the 128-wide shapes. Its tiles are 192 x 128, 64 deep: each 1-KB DMA piece is
//    8 whole 128-B rows, where 256 x 128 tiles' 32-deep pieces fetch 16 half lines (twice the L1 -> L2
//    requests, which bound that kernel: profiles/r05_gemm_dma_diag.txt). Bitwise the same outputs;
//    predictor fc2 132 -> 115 us, QKV / proj data gradients -8..-11 %, step +0.4 %
//    (profiles/r05_gemm_2w192_ab.txt). VJ_GEMM_2W192=0 restores the 256 x 128 form; RoPE keeps it (no
//    room for its table at 2 x 80 KB).
//  * staggered main loops for the K-major 256 x 256-tile GEMMs: form 1 = 32-deep units (K % 32 == 0),
//    form 2 = S64, 64-deep whole-line granules (K % 64 == 0). Measured, round 4
//    (profiles/r04_gemm_staggered_step.txt): form 1 pays on the GELU / RoPE / bf16 / f32 epilogues
//    (-1.6..-1.8 % in the step) and not on the residual / saved-derivative ones. Round 6
//    (profiles/r06_gemm_s64.txt): isolated, S64 runs a K step 3-4 % faster where the operand panels
//    stream from beyond L2 (K = 4096: target fc2 -2.4..-4 %) and takes the residual epilogues below the
//    one-tile kernel (target proj / fc2, bf16 or f32 residual, -1..-4 %), but is 4-12 % slower per K step
//    on the L2-resident K = 1024 panels of the QKV / GELU / RoPE / data-gradient GEMMs; in the train step,
//    where the side streams' GEMMs share the chip (and its L2), S64 on every shape beats both the round-5
//    choice (+0.8 %) and S64 only on K >= 2048 and the residual epilogues (+0.55 %), two interleaved runs
//    each in one call. Default: S64 wherever K % 64 == 0, else form 1 on the epilogues without aux rows.
//    VJ_GEMM_STG: 0 = never, 1 = every epilogue (form 1 where S64 cannot run); VJ_GEMM_STG64: 0 / 1
//    forces form 1 / 2 wherever a staggered loop runs.
//  * 192-row tiles (one-tile main loop) for a K-major 256-wide GEMM whose rounds of tiles over the CUs
//    cost clearly less than with 256 rows: rounds x rows, 192-row tiles charged 8 % for their lower
//    MFMA : fragment-read ratio (measured 6-9 % on full-round shapes), and at least 15 % predicted gain
//    (a predictor step whose M made the 8 % rule pick 192 ran its fc1 / dgrad slower). Where S64 can run
//    instead, the 256-row S64 tiles measured +0.2 % per step over the cost model's 192-row picks (the
//    context GEMMs, M ~ 11.7k; VJ_GEMM_BM192=0 vs default, two same-call runs each,
//    profiles/r06_gemm_s64.txt). VJ_GEMM_BM192: 0 = never, 1 = always, unset = the cost model.
Plan256 plan256(int M, int N, int K, bool a_kmajor, bool b_kmajor, int epi, int cus, const Knobs& kn) {
  if (epi < EPI_BF16 || (epi > EPI_ROPE && epi != EPI_BF16_RESID) || N % 8) return Plan256{false};
  Plan256 p{true, 256, wide_tile_ok(N) ? 256 : 128, 8, 0, 1, tile_group(kn)};
  if (!a_kmajor || !b_kmajor) return p;
  if (kn.w2 >= 0 ? kn.w2 : p.bn == 128) {
    p.bn = 128;
    p.waves = 4;
    p.per_cu = 2;
    if (kn.w2_192 != 0 && epi != EPI_ROPE) p.bm = 192;
    return p;
  }
  if (p.bn == 128) return p;
  if (K % 32 == 0 && kn.stg != 0) {
    const bool aux = epi == EPI_F32_RESID || epi == EPI_BF16_RESID || epi == EPI_GELU_BWD;
    p.stg = (kn.stg64 == 0 || K % 64) ? 1 : 2;
    if (aux && p.stg == 1 && kn.stg != 1) p.stg = 0;
  }
  if (p.stg == 2 && kn.bm192 != 1) return p;
  const long tn = vj_cdiv(N, 256);
  const long r256 = (vj_cdiv(M, 256) * tn + cus - 1) / cus, r192 = (vj_cdiv(M, 192) * tn + cus - 1) / cus;
  if (kn.bm192 >= 0 ? kn.bm192 : r192 * 192 * 108 < r256 * 256 * 85) {
    p.bm = 192;
    p.stg = 0;
  }
  return p;
}

// The runtime epilogue -> kernel instantiation, for one set of the other template parameters: the one
// list of epilogues, instantiated where Cfg256 supports the combination.
template <int... E>
struct EpiList {};
using Epilogues = EpiList<EPI_BF16, EPI_F32, EPI_F32_RESID, EPI_GELU, EPI_GELU_BWD, EPI_ROPE, EPI_PARTIAL, EPI_BF16_RESID,
                          EPI_PARTIAL_RS>;

template <bool AK, bool BKM, int EPI, int BN, bool F8, int NWV, int BMT, int STG>
int launch_epi256(const G256& g, hipStream_t st, const Knobs& kn) {
  using Cfg = Cfg256<AK, BKM, EPI, BN, F8, NWV, BMT, STG>;
  if constexpr (Cfg::supported) {
    const dim3 grid(grid256((long)g.tiles_m * g.tiles_n * g.nsplit, Cfg::BLOCKS_PER_CU, kn));
    hipLaunchKernelGGL((k_gemm256<AK, BKM, EPI, BN, F8, NWV, BMT, STG>), grid, dim3(Cfg::THREADS), 0, st, g);
    VJ_LAUNCH_CHECK("vj_gemm256");
    return VJ_OK;
  } else {
    return VJ_ERR_UNSUPPORTED;
  }
}

template <bool AK, bool BKM, int BN, bool F8, int NWV, int BMT, int STG, int... E>
int launch_list256(int epi, const G256& g, hipStream_t st, const Knobs& kn, EpiList<E...>) {
  int rc = -1;
  (void)((epi == E && ((rc = launch_epi256<AK, BKM, E, BN, F8, NWV, BMT, STG>(g, st, kn)), true)) || ...);
  if (rc >= 0) return rc;
  vj_set_error("vj_gemm256: bad epilogue %d", epi);
  return VJ_ERR_ARG;
}
template <bool AK, bool BKM, int BN, bool F8 = false, int NWV = 8, int BMT = 256, int STG = 0>
int launch256(int epi, const G256& g, hipStream_t st, const Knobs& kn) {
  return launch_list256<AK, BKM, BN, F8, NWV, BMT, STG>(epi, g, st, kn, Epilogues{});
}

// the planned kernel on g (tiles_m, tiles_n and group are set from the plan)
int launch_plan(const Plan256& p, bool ak, bool bkm, int epi, G256& g, hipStream_t st, const Knobs& kn) {
  g.tiles_m = vj_cdiv(g.M, p.bm);
  g.tiles_n = vj_cdiv(g.N, p.bn);
  g.group = p.group;
  if (p.waves == 4)
    return p.bm == 192 ? launch256<true, true, 128, false, 4, 192>(epi, g, st, kn)
                       : launch256<true, true, 128, false, 4, 256>(epi, g, st, kn);
  if (p.bm == 192) return launch256<true, true, 256, false, 8, 192>(epi, g, st, kn);
  if (p.stg == 2) return launch256<true, true, 256, false, 8, 256, 2>(epi, g, st, kn);
  if (p.stg == 1) return launch256<true, true, 256, false, 8, 256, 1>(epi, g, st, kn);
  if (p.bn == 256) {
    if (ak) return bkm ? launch256<true, true, 256>(epi, g, st, kn) : launch256<true, false, 256>(epi, g, st, kn);
    return bkm ? launch256<false, true, 256>(epi, g, st, kn) : launch256<false, false, 256>(epi, g, st, kn);
  }
  if (ak) return bkm ? launch256<true, true, 128>(epi, g, st, kn) : launch256<true, false, 128>(epi, g, st, kn);
  return bkm ? launch256<false, true, 128>(epi, g, st, kn) : launch256<false, false, 128>(epi, g, st, kn);
}

}  // namespace

extern "C" int vj_set_reserved_cus(int n) {
  VJ_CHECK_ARG(n >= 0 && n <= num_cus() - 8, "vj_set_reserved_cus: %d of %d CUs", n, num_cus());
  g_reserved_cus.store(n, std::memory_order_relaxed);
  return VJ_OK;
}

// The kernel vj_gemm_bf16 / vj_qkv_rope_gemm would run for a problem under the current VJ_GEMM_* knobs
// (no device work; cus == 0: the current device's CU count). out6 = tile rows, tile columns, waves,
// main-loop form (0 one tile / 1 staggered / 2 S64), workgroups per CU, tile group. Returns
// VJ_ERR_UNSUPPORTED (out6 untouched) where the 256-row kernel declines.
extern "C" int vj_gemm256_plan(int M, int N, int K, int a_kmajor, int b_kmajor, int epi, int cus, int* out6) {
  VJ_CHECK_ARG(M > 0 && N > 0 && K > 0 && cus >= 0 && out6, "vj_gemm256_plan: bad arguments");
  const Plan256 p = plan256(M, N, K, a_kmajor, b_kmajor, epi, cus ? cus : num_cus(), read_knobs());
  if (!p.ok) return VJ_ERR_UNSUPPORTED;
  const int v[6] = {p.bm, p.bn, p.waves, p.stg, p.per_cu, p.group};
  memcpy(out6, v, sizeof(v));
  return VJ_OK;
}

// Called by vj_gemm_bf16_splitk (splitk == 1) when the problem suits a 256-row tile; arguments
// already validated there. Returns VJ_ERR_UNSUPPORTED when it declines.
int vj_gemm256_dispatch(int M, int N, int K, const void* A, long lda, int a_kmajor, const void* B, long ldb,
                        int b_kmajor, int epi, const float* bias, const void* aux, long ldaux, void* C, long ldc,
                        void* C2, long ldc2, hipStream_t st, const void* rope) {
  if (ldc % 4 || ldc2 % 4 || ldaux % 4) return VJ_ERR_UNSUPPORTED;
  if (((uintptr_t)C & 15) || ((uintptr_t)C2 & 15) || ((uintptr_t)aux & 15) || ((uintptr_t)bias & 15))
    return VJ_ERR_UNSUPPORTED;
  const Knobs kn = read_knobs();
  const Plan256 p = plan256(M, N, K, a_kmajor, b_kmajor, epi, num_cus(), kn);
  if (!p.ok) return VJ_ERR_UNSUPPORTED;
  G256 g{(const bf16_t*)A, (const bf16_t*)B, M, N, K, lda, ldb, C, ldc, C2, ldc2, bias, aux, ldaux,
         0, 0, RopeP{}, K, 1, nullptr, 0};
  if (epi == EPI_ROPE) {
    if (!rope) return VJ_ERR_UNSUPPORTED;
    g.rope = *(const RopeP*)rope;
    if (g.rope.hd % 4 || g.rope.D % 4 || g.rope.npos < 1 || g.rope.npos > 1024) return VJ_ERR_UNSUPPORTED;
    if ((long)g.rope.npos * g.rope.half > ROPE_TAB_MAX) return VJ_ERR_UNSUPPORTED;
  }
  return launch_plan(p, a_kmajor, b_kmajor, epi, g, st, kn);
}

// Split-K partial products ws[z] = A[:, z-th K slice] B[z-th K slice, :]^T (f32, [splitk][M][N]) with
// 256-row tiles; the caller reduces the slabs. rsum (or null): the row sums of A per K slice,
// [splitk][M] (fused bias gradient). Returns VJ_ERR_UNSUPPORTED when it declines.
int vj_gemm256_partial(int M, int N, int K, const void* A, long lda, int a_kmajor, const void* B, long ldb,
                       int b_kmajor, int kslice, int splitk, float* ws, hipStream_t st, float* rsum) {
  if (a_kmajor || b_kmajor || N % 8 || M < 256 || N < 128) return VJ_ERR_UNSUPPORTED;
  const Knobs kn = read_knobs();
  const Plan256 p{true, 256, wide_tile_ok(N) ? 256 : 128, 8, 0, 1, tile_group(kn)};
  if ((long)vj_cdiv(M, p.bm) * vj_cdiv(N, p.bn) * splitk > 0x7fffffffL) return VJ_ERR_UNSUPPORTED;
  G256 g{(const bf16_t*)A, (const bf16_t*)B, M, N, K, lda, ldb, nullptr, 0, nullptr, 0, nullptr, nullptr, 0,
         0, 0, RopeP{}, kslice, splitk, ws, 0};
  g.rsum = rsum;
  return launch_plan(p, false, false, rsum ? EPI_PARTIAL_RS : EPI_PARTIAL, g, st, kn);
}

extern "C" int vj_gemm_bf16(int M, int N, int K, const void* A, long lda, int a_kmajor, const void* B, long ldb,
                            int b_kmajor, int epi, const float* bias, const void* aux, long ldaux, void* C, long ldc,
                            void* C2, long ldc2, void* stream);

extern "C" int vj_rope(int T, int H, int hd, void* qkv, long ld, int q_off, int k_off, const int* ids, int ids_mod,
                       int tokens_per_frame, int tokens_per_row, const float* cos_tab, const float* sin_tab, int half,
                       int inverse, void* stream);

// Fused QKV projection + 3-axis RoPE of q and k (modules.py:330 + 343-365): one launch whose epilogue
// rotates the f32 accumulator rows before the bf16 store; falls back to GEMM + vj_rope for shapes
// the 256-row kernel declines.
extern "C" int vj_qkv_rope_gemm(int M, int K, const void* A, long lda, const void* B, long ldb, const float* bias,
                                void* C, long ldc, int H, int hd, const int* ids, int ids_mod, int tpf, int tpr,
                                const float* cos_t, const float* sin_t, int npos, void* stream) {
  if (M == 0) return VJ_OK;
  const int N = 3 * H * hd;
  VJ_CHECK_ARG(hd % 8 == 0 && cos_t && sin_t && (ids || ids_mod > 0), "vj_qkv_rope_gemm: bad rope arguments");
  VJ_CHECK_ARG(tpf > 0 && tpr > 0 && npos > 0, "vj_qkv_rope_gemm: tokens_per_frame/row and npos must be > 0");
  const int half = (hd / 3) / 2;
  if (M >= 1024) {
    RopeP rp{ids, ids_mod, tpf, tpr, half, hd, H * hd, cos_t, sin_t, npos};
    const int rc = vj_gemm256_dispatch(M, N, K, A, lda, 1, B, ldb, 1, EPI_ROPE, bias, nullptr, 0, C, ldc, nullptr, 0,
                                       (hipStream_t)stream, &rp);
    if (rc != VJ_ERR_UNSUPPORTED) return rc;
  }
  int rc = vj_gemm_bf16(M, N, K, A, lda, 1, B, ldb, 1, EPI_BF16, bias, nullptr, 0, C, ldc, nullptr, 0, stream);
  if (rc) return rc;
  return vj_rope(M, H, hd, C, ldc, 0, H * hd, ids, ids_mod, tpf, tpr, cos_t, sin_t, half, 0, stream);
}

// ---- fp8 forward GEMMs (opt-in fp8 target-encoder path, BASELINE configs[4]) -----------------------
// A [M, K] and B [N, K] are OCP e4m3 bytes, both K-major (X W^T), with per-row power-of-two scales:
// A(m, k) = A8[m, k] * 2^ea[m], B(n, k) = B8[n, k] * 2^eb[n] (ea / eb device int32; vj_quant_rows_fp8
// or vj_layernorm_fwd_fp8 produce them). The 256-row kernel reads the bytes as bf16 pairs: K, lda and
// ldb must be multiples of 16 bytes. Epilogues as vj_gemm_bf16 (BF16, F32, F32_RESID, GELU) / RoPE.
static int gemm256_f8(int M, int N, int K, const void* A, long lda, const int* ea, const void* B, long ldb,
                      const int* eb, int epi, const float* bias, const void* aux, long ldaux, void* C, long ldc,
                      void* C2, long ldc2, hipStream_t st, const RopeP* rope) {
  if (M == 0 || N == 0) return VJ_OK;
  VJ_CHECK_ARG(M > 0 && N > 0 && K > 0 && K % 16 == 0 && lda % 16 == 0 && ldb % 16 == 0 && lda >= K && ldb >= K,
               "vj_gemm_fp8: K, lda, ldb must be multiples of 16 (M=%d N=%d K=%d lda=%ld ldb=%ld)", M, N, K, lda, ldb);
  VJ_CHECK_ARG(N % 8 == 0 && ldc % 4 == 0 && ldc2 % 4 == 0 && ldaux % 4 == 0, "vj_gemm_fp8: N %% 8, ld %% 4");
  VJ_CHECK_ARG(!(((uintptr_t)A | (uintptr_t)B | (uintptr_t)C | (uintptr_t)C2 | (uintptr_t)aux | (uintptr_t)bias) & 15),
               "vj_gemm_fp8: operands must be 16-B aligned");
  VJ_CHECK_ARG(A && B && ea && eb, "vj_gemm_fp8: null operand or scale exponents");
  VJ_CHECK_ARG(epi == EPI_BF16 || epi == EPI_F32 || epi == EPI_F32_RESID || epi == EPI_GELU || epi == EPI_ROPE,
               "vj_gemm_fp8: epilogue %d unsupported (forward only)", epi);
  VJ_CHECK_ARG(epi != EPI_F32_RESID || aux, "vj_gemm_fp8: EPI_F32_RESID needs the residual");
  VJ_CHECK_ARG(epi != EPI_GELU || C2, "vj_gemm_fp8: EPI_GELU needs the activation output C2");
  VJ_CHECK_ARG(epi == EPI_GELU || C, "vj_gemm_fp8: output C is required");
  VJ_CHECK_ARG((long)M * lda < 0x7fffffffL && (long)N * ldb < 0x7fffffffL, "vj_gemm_fp8: operand too large");
  // 256 x 128 tiles: the 256-wide fp8 tile needs ~20 VGPRs more than the bf16 one and spills
  const Knobs kn = read_knobs();
  G256 g{(const bf16_t*)A, (const bf16_t*)B, M, N, K / 2, lda / 2, ldb / 2, C, ldc, C2, ldc2, bias, aux, ldaux,
         vj_cdiv(M, 256), vj_cdiv(N, 128), RopeP{}, K / 2, 1, nullptr, tile_group(kn), ea, eb};
  if (epi == EPI_ROPE) {
    VJ_CHECK_ARG(rope != nullptr, "vj_gemm_fp8: EPI_ROPE needs the rope tables");
    g.rope = *rope;
    VJ_CHECK_ARG(g.rope.hd % 4 == 0 && g.rope.D % 4 == 0 && g.rope.npos >= 1 && g.rope.npos <= 1024 &&
                     (long)g.rope.npos * g.rope.half <= ROPE_TAB_MAX,
                 "vj_gemm_fp8: rope table too large (npos=%d)", g.rope.npos);
  }
  return launch256<true, true, 128, true>(epi, g, st, kn);
}

extern "C" int vj_gemm_fp8(int M, int N, int K, const void* A, long lda, const int* ea, const void* B, long ldb,
                           const int* eb, int epi, const float* bias, const void* aux, long ldaux, void* C, long ldc,
                           void* C2, long ldc2, void* stream) {
  VJ_CHECK_ARG(epi != EPI_ROPE, "vj_gemm_fp8: use vj_qkv_rope_gemm_fp8 for the RoPE epilogue");
  return gemm256_f8(M, N, K, A, lda, ea, B, ldb, eb, epi, bias, aux, ldaux, C, ldc, C2, ldc2, (hipStream_t)stream,
                    nullptr);
}

// vj_qkv_rope_gemm on fp8 operands (no unfused fallback: an fp8 request the kernel declines fails)
extern "C" int vj_qkv_rope_gemm_fp8(int M, int K, const void* A, long lda, const int* ea, const void* B, long ldb,
                                    const int* eb, const float* bias, void* C, long ldc, int H, int hd,
                                    const int* ids, int ids_mod, int tpf, int tpr, const float* cos_t,
                                    const float* sin_t, int npos, void* stream) {
  if (M == 0) return VJ_OK;
  VJ_CHECK_ARG(hd % 8 == 0 && cos_t && sin_t && (ids || ids_mod > 0), "vj_qkv_rope_gemm_fp8: bad rope arguments");
  VJ_CHECK_ARG(tpf > 0 && tpr > 0 && npos > 0, "vj_qkv_rope_gemm_fp8: tokens_per_frame/row and npos must be > 0");
  const RopeP rp{ids, ids_mod, tpf, tpr, (hd / 3) / 2, hd, H * hd, cos_t, sin_t, npos};
  return gemm256_f8(M, 3 * H * hd, K, A, lda, ea, B, ldb, eb, EPI_ROPE, bias, nullptr, 0, C, ldc, nullptr, 0,
                    (hipStream_t)stream, &rp);
}

#if VJ_GEMM_STAMPS
extern "C" int vj_debug_gemm_stamps(void* dst, long nbytes) {
  hipMemset(dst, 0, 0);
  return hipMemcpyFromSymbol(dst, HIP_SYMBOL(vj_gemm_stamps), nbytes, 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : 1;
}
extern "C" int vj_debug_gemm_istamps(void* dst, long nbytes) {
  return hipMemcpyFromSymbol(dst, HIP_SYMBOL(vj_gemm_istamps), nbytes, 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : 1;
}
extern "C" int vj_debug_gemm_stamps_clear() {
  static long z[2048 * 16 * 4];
  return hipMemcpyToSymbol(HIP_SYMBOL(vj_gemm_stamps), z, sizeof(z), 0, hipMemcpyHostToDevice) == hipSuccess ? 0 : 1;
}
#endif
