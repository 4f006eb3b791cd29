// Device helpers of the 256-row bf16 / fp8 GEMM kernel (vj_gemm256.hip): the kernel argument block, LDS-DMA
// staging of K-major / MN-major operand tiles with the XOR swizzles, MFMA fragment reads, the
// GELU epilogue pair and Cfg256, the kernel's compile-time configuration (geometry, LDS layout). Everything sits in an anonymous namespace: each translation unit compiles
// its own copy (no cross-TU codegen coupling of the kernels).
#pragma once
#include "vj_common.h"

namespace {

// epilogue numbering: vj_common.h (EPI_BF16_RESID: the no-grad target encoder's residual stream in the
// reference's own autocast precision, x = x + proj(...) in bf16, half the epilogue bytes of F32_RESID)

using RopeP = VjRope;

struct G256 {
  const bf16_t* A;
  const bf16_t* B;
  int M, N, K;
  long lda, ldb;
  void* C;
  long ldc;
  void* C2;
  long ldc2;
  const float* bias;
  const void* aux;
  long ldaux;
  int tiles_m, tiles_n;
  RopeP rope;
  int kslice;  // K range of one K slice (= K unless EPI_PARTIAL)
  int nsplit;  // K slices: slice z covers [z*kslice, min(K, (z+1)*kslice)) (EPI_PARTIAL only; else 1)
  float* ws;   // EPI_PARTIAL: f32 partial products [nsplit][M][N]
  int group;   // tile rows per group of the grouped tile order (0: row-major, n fastest)
  // F8 kernels: A / B are fp8 e4m3 (OCP) viewed as bf16 pairs (K, lda, ldb above in 2-byte units);
  // ea[m] / eb[n] = power-of-two exponents of the per-row (A: token) / per-row (B: output channel)
  // scales: A(m, k) = a8 * 2^ea[m], B(n, k) = b8 * 2^eb[n] (E8M0 scale operands of the MFMA)
  const int* ea = nullptr;
  const int* eb = nullptr;
  // EPI_PARTIAL: f32 row sums of A over each K slice, [nsplit][M] (the bias gradient fused into a
  // weight-gradient GEMM: A = dY^T, so row m of A summed over the tokens is db[m]); null: none
  float* rsum = nullptr;
};

constexpr int BK = 64;
// LDS behind the two operand stages for the per-kernel tables: the GELU tables (f32 derivative:
// 13 KB) or the RoPE tile positions (1 KB) + interleaved cos/sin table (npos * half * 8 B).
constexpr int TAB_BYTES = 16384;
constexpr int ROPE_TAB_MAX = (TAB_BYTES - 256 * 4) / 8;  // cos/sin pairs that fit behind the positions

__device__ __forceinline__ uint32_t clampb(long b) {
  if (b < 0) return 0;
  return b > 0x7fffffffL ? 0x7fffffffu : (uint32_t)b;
}

// Byte offset of a slot in a ring of S slots of SZ bytes, n <= S slots after the slot at byte offset x:
// one add and one wrap (a mask where the ring's byte size is a power of two, else a compare-select).
// The staggered main loops keep their LDS positions as such running wave-uniform offsets.
template <int S, int SZ>
__device__ __forceinline__ int ring_step(int x, int n = 1) {
  constexpr int R = S * SZ;
  if constexpr ((R & (R - 1)) == 0) return (x + n * SZ) & (R - 1);
  x += n * SZ;
  return x >= R ? x - R : x;
}

__device__ __forceinline__ int mn_swz(int k) { return 2 * (k & 3) + 8 * ((k >> 3) & 1); }

// 64-B K-major rows (32-deep K tiles): the 16-B chunk swizzle. A 16x16x32 fragment read (row rb + (l &
// 15), chunk l >> 4) is serviced in the lane groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, {32-35,
// 44-47, 52-59}, {36-43, 48-51, 60-63} (MI355X_MICROARCH.md, LDS), each of which holds rows j, j+4,
// j+8, j+12 at chunks (g, g^1, g^1, g) for some g: conflict-free iff swz over the row quarters
// q = (r >> 2) & 3 makes {swz(0), swz(1)^1, swz(2)^1, swz(3)} distinct. swz = 3 * (q >> 1) does;
// (r >> 2) & 3 (used until round 5) gave {0, 0, 3, 3}: every group 2-way conflicted (PMC: bank-conflict
// cycles = half the LDS cycles of the staggered GEMM).
__device__ __forceinline__ int kswz32(int r) { return 3 * ((r >> 3) & 1); }

// K-major image: [ROWS][64] bf16, 128-B rows, chunk ^= (row>>1)&7 ([ROWS][32]: 64-B rows, kswz32).
// MN-major image: [64][ROWS] bf16, ROWS*2-B rows, chunk ^= mn_swz(k).
// PERM (K-major B only): LDS row r of each WN-row group holds global row NTN*(r%PB) + r/PB of the
// group (PB = the MFMA output block width, 16 or 32; NTN = WN / PB), so n block j of the MFMA
// accumulators covers the group's columns {NTN*c + j}: each lane then owns NTN CONSECUTIVE output
// columns and the epilogue stores straight from registers.
// NW waves issue the tile's 1-KB pieces (waves 0 .. NW-1).
template <bool KMAJ, int ROWS, bool PERM = false, int NW = 8, int BKT = 64, int WNX = 4, int PB = 16>
__device__ __forceinline__ void stage(__amdgpu_buffer_rsrc_t rs, long ld, int rows_left, int k0, int K,
                                      LDS_AS char* lds, int wave, int lane) {
  constexpr int PIECES = ROWS * BKT * 2 / 1024;  // 1-KB DMA pieces per operand tile
  constexpr int PPW = PIECES / NW;
  static_assert(KMAJ || BKT == 64, "MN-major staging is written for 64-deep K tiles");
#pragma unroll
  for (int i = 0; i < PPW; ++i) {
    const int p = wave * PPW + i;
    uint32_t voff;
    if constexpr (KMAJ) {
      // 128-B rows (BK 64): chunk ^= (row>>1)&7; 64-B rows (BK 32): chunk ^= kswz32(row)
      constexpr int CPR = BKT / 8, RPP = 64 / CPR;  // 16-B chunks per row, rows per piece
      const int r = p * RPP + lane / CPR;
      const int c = (lane % CPR) ^ (BKT == 64 ? ((r >> 1) & 7) : kswz32(r));
      const int kk = k0 + c * 8;
      int gr = r;
      if constexpr (PERM) {
        constexpr int WN = ROWS / WNX, NTN = WN / PB;
        const int rl = r % WN;
        gr = (r - rl) + NTN * (rl % PB) + (rl / PB);
      }
      voff = (gr < rows_left && kk < K) ? (uint32_t)(((long)gr * ld + kk) * 2) : VJ_OOB;
    } else {
      constexpr int CPR = ROWS / 8;     // chunks per LDS row
      constexpr int RPP = 64 / CPR;     // k-rows per piece
      const int kr = p * RPP + lane / CPR;
      const int c = (lane % CPR) ^ mn_swz(kr);
      const int col = c * 8;
      voff = (k0 + kr < K && col < rows_left) ? (uint32_t)(((long)(k0 + kr) * ld + col) * 2) : VJ_OOB;
    }
    dma16(rs, lds + p * 1024, voff);
  }
}

// 16x16x32 operand fragment: lane l holds X(rb + (l&15), 32s + 8(l>>4) + j), j = 0..7.
template <bool KMAJ, int ROWS, int BKT = 64>
__device__ __forceinline__ bf16x8 frag(const LDS_AS char* lds, int rb, int s, int lane) {
  if constexpr (KMAJ) {
    const int r = rb + (lane & 15);
    if constexpr (BKT == 32) {  // 64-B rows, one k-step
      const int c = (lane >> 4) ^ kswz32(r);
      return *(const LDS_AS bf16x8*)(lds + r * 64 + c * 16);
    }
    const int c = (4 * s + (lane >> 4)) ^ ((r >> 1) & 7);
    return *(const LDS_AS bf16x8*)(lds + r * 128 + c * 16);
  } else {
    const int gi = lane & 15;
    const int k0 = 32 * s + 8 * (lane >> 4) + (gi >> 2);
    const int col = rb + 4 * (gi & 3);
    const int within = (col & 7) * 2;
    const int c = col >> 3;
    const s16x4 lo = ds_read_tr16_async(lds + k0 * (ROWS * 2) + ((c ^ mn_swz(k0)) * 16) + within);
    const s16x4 hi = ds_read_tr16_async(lds + (k0 + 4) * (ROWS * 2) + ((c ^ mn_swz(k0 + 4)) * 16) + within);
    s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, v);
  }
}

// GELU (nn.GELU(), vision_transformer.py:100) in the epilogues: the forward evaluates it on the bf16
// pre-activation (the reference's autocast order) and, when the caller saves for the backward, the
// derivative gelu'(pre) in the same pass (its erf and Gaussian terms are already computed); the
// backward epilogue then multiplies by the saved derivative (one VALU op per element).
__device__ __forceinline__ uint32_t gelu_pair(uint32_t pk, uint32_t* dpk) {
  float y0, d0, y1, d1;
  gelu_fwd_grad(__builtin_bit_cast(float, pk << 16), y0, d0);
  gelu_fwd_grad(__builtin_bit_cast(float, pk & 0xffff0000u), y1, d1);
  if (dpk) *dpk = pack_bf2(d0, d1);
  return pack_bf2(y0, y1);
}

// ---- GELU by table (the staggered fc1 kernel's epilogue). The pre-activation is a bf16 value (the
// reference's autocast rounding point), so GELU(pre) and GELU'(pre) are functions of its 16 bits.
// Entry (i, s) of the LDS table (interleaved: byte 16 i + 8 s) holds {cdf, dy} = gelu_cdf_grad(x) for
// x = (-1)^s * bf16(GT_LO - 1 + i) (i >= 1), x = (-1)^s * 0 (i = 0); the epilogue forms y = x * cdf,
// the same f32 product gelu_fwd_grad takes, and dy as stored. Magnitudes outside [2^-10, 16) share
// one entry per side because their bf16 outputs are the same:
//  * |x| < 2^-10 -> the +-0 entry: cdf(x) = 0.5 +- 0.4|x| stays within 2^-10.3 of 0.5 (relative),
//    inside half a bf16 ulp of x / 2 for y and of 0.5 for dy; below 2^-24 cdf(x) IS cdf(+-0) (rcp(1 +
//    0.27 a) = 1, exp2(-zs^2) = 1), which keeps the f32-denormal products (round-half-even ties of
//    x / 2 in bf16) those of the exact evaluation;
//  * |x| >= 16 -> the largest entry below 16: exp2(-zs^2) underflows to 0, so cdf = 1 (x > 0) or
//    0 (x < 0) and dy = 1 or 0 exactly, as for every larger |x|;
//  * inf / NaN: y = x * cdf gives what the exact evaluation gives; dy = fma(x, 0, dy_tab) is NaN for
//    them (x * 0) and dy_tab otherwise (dy is never -0).
// ~9 VALU + one LDS read per element instead of ~17 VALU + rcp + exp2; bitwise equal to gelu_fwd_grad
// on all 65536 bf16 inputs (tests/test_gpu_kernels.py::test_gelu_epilogues_bitwise_all_bf16).
constexpr uint32_t GT_LO = 0x3A80;       // bf16 bits of 2^-10
constexpr uint32_t GT_HI = 0x417F;       // largest bf16 below 16
constexpr int GT_N = GT_HI - GT_LO + 2;  // entries per sign (index 0: |x| < 2^-10, zero, denormals)
constexpr int GT_BYTES = 2 * GT_N * 8;   // 28.7 KB

__device__ __forceinline__ void gelu_tab_fill(LDS_AS f32x2* tab, int tid, int nthreads) {
  for (int e = tid; e < 2 * GT_N; e += nthreads) {
    const uint32_t i = (uint32_t)e >> 1, sg = (uint32_t)e & 1;
    const uint32_t bits = (i == 0 ? 0u : GT_LO - 1 + i) | (sg << 15);
    float cdf, dy;
    gelu_cdf_grad(__builtin_bit_cast(float, bits << 16), cdf, dy);
    tab[e] = f32x2{cdf, dy};
  }
}

// GELU (and GELU' into *dpk when SAVE_D) of the two bf16 pre-activations packed in pk, by table
template <bool SAVE_D>
__device__ __forceinline__ uint32_t gelu_pair_tab(uint32_t pk, const LDS_AS char* tab, uint32_t* dpk) {
  typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
  const u16x2 b = __builtin_bit_cast(u16x2, pk);
  u16x2 i = __builtin_elementwise_sub_sat(b & (u16x2)0x7fff, (u16x2)(GT_LO - 1));
  i = __builtin_elementwise_min(i, (u16x2)(GT_N - 1));
  const uint32_t a = __builtin_bit_cast(uint32_t, (u16x2)((i << 4) | ((b >> 12) & (u16x2)8)));
  const float x0 = __builtin_bit_cast(float, pk << 16), x1 = __builtin_bit_cast(float, pk & 0xffff0000u);
  if constexpr (SAVE_D) {
    const f32x2 t0 = *(const LDS_AS f32x2*)(tab + (a & 0xffffu));
    const f32x2 t1 = *(const LDS_AS f32x2*)(tab + (a >> 16));
    *dpk = pack_bf2(fmaf(x0, 0.f, t0[1]), fmaf(x1, 0.f, t1[1]));
    return pack_bf2(x0 * t0[0], x1 * t1[0]);
  } else {
    const float c0 = *(const LDS_AS float*)(tab + (a & 0xffffu));
    const float c1 = *(const LDS_AS float*)(tab + (a >> 16));
    return pack_bf2(x0 * c0, x1 * c1);
  }
}

struct Tile {
  int m0, n0, z, Keff, nk;  // buffer descriptors are rebuilt per DMA: SGPRs are the scarce resource
};

// bf16 -> f32 of the low / high half of a packed pair (exact)
__device__ __forceinline__ float bf_lo(uint32_t u) { return __builtin_bit_cast(float, u << 16); }
__device__ __forceinline__ float bf_hi(uint32_t u) { return __builtin_bit_cast(float, u & 0xffff0000u); }
// the same on a pair held in a float register (the bit pattern of a 4-byte load)
__device__ __forceinline__ float bf_lo(float u) { return __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, u) << 16); }
__device__ __forceinline__ float bf_hi(float u) {
  return __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, u) & 0xffff0000u);
}

// Schedule choices fixed by round-3 measurements (the variants were removed from the source; the
// numbers are in DESIGN.md and profiles/r03_gemm_*):
//  * 8-wave main loop: only the A pieces of K-tile t + 2 go out after the barrier; the B pieces are
//    issued after 3 of the last phase's 4 m-tiles (SPLIT_AT): -2..-7 % and a further 0..-5 % on the
//    ViT-L shapes (r03_gemm_spread_kernels.txt,
//    r03_gemm_split_kernels.txt). Also the A pieces after the first m-tile: slower.
//  * on 256-wide bf16 tiles without a VALU-heavy epilogue only waves 0-3 issue the main-loop LDS-DMA
//    (DMA_WAVES; their SIMD partners keep issuing MFMAs); the next tile's stage 1, issued around the
//    epilogue, goes out from all 8 waves (r03_gemm_dmaw4_kernels.txt, r03_gemm_s1all_step_ab.txt).
//    Slower and removed: the RoPE / GELU tiles on 4 DMA waves, A / B pieces split over waves 0-3 /
//    4-7, the DMA from waves 4-7, s_setprio around the MFMA clusters or for waves 4-7.
//  * one m-tile of residual / saved-derivative rows prefetched ahead in the direct epilogue (deeper:
//    no faster, r03 stamps).
constexpr int SPLIT_AT = 3;
constexpr int DMA_WAVES = 4;
constexpr int AUX_PF = 1;

constexpr int LDS_PER_CU = 163840;
constexpr int cmax(int a, int b) { return a > b ? a : b; }

// Everything k_gemm256<AK, BKM, EPI, BN, F8, NWV, BMT, STG> derives from its template parameters: which
// combinations exist (`supported`: the kernel asserts it, the launcher instantiates nothing else), the
// tile / wave geometry, the schedule switches, the launch shape and the LDS layout. LDS_BYTES is the
// end of the furthest region, so a region cannot outgrow the array unnoticed.
//
// NWV = 8: 8 waves (2 x 4), 64-deep K tiles, one workgroup per CU. NWV = 4 ("2W"): 4 waves (2 x 2),
// TWO workgroups per CU, so one workgroup's epilogue (HBM / VALU) runs under the other's main loop
// (MFMA); K-major operands only; 192 x 128 tiles 64 deep (80 KB, the default) or 256 x 128 tiles 32
// deep (64 KB with the RoPE table area).
// BMT = 192 (K-major bf16 direct-store tiles only): 96-row wave tiles (3 m-tiles per M-half) for
// problems whose 256-row tile count leaves a round of CUs under-filled (context GEMMs, M ~ 11.7k:
// 184 tiles of 256 x 256 on 256 CUs -> 244 tiles of 192 x 256).
// STG: the staggered main loops (vj_gemm256.hip), 1 = 32-deep units, 2 = S64.
template <bool AK, bool BKM, int EPI, int BN, bool F8, int NWV, int BMT, int STG>
struct Cfg256 {
  static constexpr bool PART = EPI == EPI_PARTIAL || EPI == EPI_PARTIAL_RS;  // split-K partial slabs (RS: + row sums)
  static constexpr bool RS = EPI == EPI_PARTIAL_RS;
  static constexpr int BM = BMT;
  static constexpr int MH = BM / 64;  // virtual 16-row m-tiles per half of the wave's rows (4 / 3)
  // 2-workgroup kernels: 256 x 128 tiles 32 deep (64-B LDS rows), or 192 x 128 tiles 64 deep (128-B
  // rows: whole cache lines per DMA piece, half the L1 -> L2 requests; 80 KB, no table: RoPE excluded)
  static constexpr int BK = (NWV == 8 || BMT == 192) ? 64 : 32;
  static constexpr int NT = NWV * 64;
  static constexpr int WNX = NWV / 2;    // waves across N (4 / 2)
  static constexpr int WMX = NWV / WNX;  // waves across M (2)
  static constexpr int WM = BM / WMX;    // wave tile rows (128 / 96)
  static constexpr int WN = BN / WNX;    // wave tile columns (64 / 32)
  static constexpr int PB = 16;          // MFMA output block width
  static constexpr int NTN = WN / PB;    // n blocks per wave (4 / 2)
  static constexpr int A_BYTES = BM * BK * 2;
  static constexpr int B_BYTES = BN * BK * 2;
  static constexpr int STAGE = A_BYTES + B_BYTES;
  // LDS-DMA issuers: DMA_WAVES = 4 -> waves 0-3 only on 256-wide tiles (their SIMD partners 4-7 keep
  // issuing MFMAs meanwhile), except the RoPE / GELU / GELU-backward tiles, whose next-tile stage 1
  // goes out right before (or in) their VALU-heavy epilogue, where waves 0-3 would start it 16
  // pieces late; 128-wide tiles (the predictor's N = 384) measured slower with it.
  static constexpr bool VALU_EPI = EPI == EPI_ROPE || EPI == EPI_GELU || EPI == EPI_GELU_BWD;
  static constexpr int DMAW = NWV != 8 ? NWV : (VALU_EPI || BN != 256 || F8) ? 8 : DMA_WAVES;
  // K-major B with 4 n blocks per wave: permuted B staging + stores straight from registers (16-B
  // f32 / 8-B bf16 per row); 128-wide tiles would store 4-8 B per lane, so they keep the LDS path
  static constexpr bool DIRECT = BKM && NTN == 4;
  static constexpr bool AUX = EPI == EPI_F32_RESID || EPI == EPI_GELU_BWD || EPI == EPI_BF16_RESID;
  static constexpr bool F32OUT = EPI == EPI_F32 || EPI == EPI_F32_RESID || PART;
  // MN-major operands are read with asm transposed reads (ds_read_tr16_async)
  static constexpr bool ASYNC = !AK || !BKM;
  // The next tile's stage 0 is DMA'd during this tile's last K-tile. Its stage 1 goes out right
  // after the last barrier, unless the epilogue still needs that LDS slot (staged epilogue: after
  // it) or issues global loads that would queue behind the DMA in vmcnt order (AUX: once the last
  // aux rows are fetched).
  static constexpr bool EARLY1 = DIRECT && !AUX;

  static constexpr bool supported =
      // staggered main loops: 8-wave K-major bf16 256 x 256 tiles
      (!STG || (AK && BKM && !F8 && NWV == 8 && BMT == 256 && BN == 256 && !PART)) &&
      // fp8: the forward epilogues only
      (!F8 || (AK && BKM && (EPI == EPI_BF16 || EPI == EPI_F32 || EPI == EPI_F32_RESID || EPI == EPI_GELU ||
                             EPI == EPI_ROPE))) &&
      // 2-workgroup GEMM: K-major bf16 operands only
      (NWV == 8 || (NWV == 4 && AK && BKM && !F8)) &&
      // 192-row tiles: direct K-major bf16 (the 4-wave kernel without the RoPE table)
      (BMT == 256 || (BMT == 192 && !F8 && AK && DIRECT && (NWV == 8 || EPI != EPI_ROPE))) &&
      // bf16 residual: forward GEMMs (both K-major); split-K slabs: weight gradients (both MN-major)
      (EPI != EPI_BF16_RESID || (AK && BKM)) && (!PART || (!AK && !BKM));

  // STG: ring of NSL 32-KB unit slots, DMA distance NSL - 2 units; 5 slots (all 160 KB of the CU's
  // LDS, distance 3) unless the RoPE epilogue needs the table area (4 slots + table, distance 2)
  // (GTAB: the GELU epilogue by table, 4 slots behind the 28.7-KB table at LDS offset 0, whose byte
  // offsets then fit the 16-bit lanes the lookup computes them in). More slots than 4 (distance 2,
  // the depth of the RoPE / GELU kernels) measured the same on every target shape: DESIGN.md.
  static constexpr bool GTAB = STG && EPI == EPI_GELU;
  static constexpr int USZ = 32768;
  static constexpr int NSL = STG ? ((EPI == EPI_ROPE || GTAB) ? 4 : 5) : 1;
  static constexpr int DIST = NSL - 2;
  // S64 (STG == 2): the same ring area as 16-KB granules, SA A slots then SB B slots (DMA distance
  // SA - 1 / SB - 1 granules). 4 + 4 granules = the 4-slot ring's 128 KB, beside the GELU / RoPE tables.
  // Deeper B rings (5 / 6 on the kernels without an LDS table) removed the DMA stalls of a tile's
  // first K steps (interval stamps) but slowed every later step: qkv tgt 260 -> 274 us, step -0.6 %
  // (profiles/r06_gemm_s64.txt); 4 kept.
  static constexpr bool S64 = STG == 2;
  static constexpr int GSZ = 16384;
  static constexpr int SA = 4, SB = 4;
  static constexpr int EA = SA - 1, EB = SB - 1;
  // first row of the wave's rows (S64: the wave's 64-row band in each 128-row half)
  static constexpr int WRS = S64 ? 64 : WM;

  // staged epilogue (!DIRECT): passes of MTP m-tiles (16 * MTP rows) per wave through a padded image in
  // the last K-tile's operand slot: 2 m-tiles per pass where the image fits the slot (BN = 128), else 1
  static constexpr int STR = WN + 4;    // floats per staged row (conflict-free ds_write_b32)
  static constexpr int LPR = WN / 4;    // lanes per staged row (16-B each)
  static constexpr int RPI = 64 / LPR;  // rows per wave-instruction
  static constexpr int MTP = (NWV * 32 * STR * 4 <= STAGE) ? 2 : 1;
  static constexpr int PR = 16 * MTP;   // rows per pass
  static constexpr int IT = PR / RPI;   // row-instructions per pass

  // ---- LDS regions (byte offset, size). One-tile kernels: two operand slots, then the table area
  // (every epilogue reserves it; 2 x 80 KB of the 4-wave 192-row kernel leave no room: RoPE excluded).
  // Staggered kernels: [GELU table] ring [RoPE table area].
  static constexpr int SLOT_OFF = 0, SLOT_END = STG ? 0 : 2 * STAGE;
  static constexpr int GTAB_OFF = 0, GTAB_END = GTAB ? GT_BYTES : 0;
  static constexpr int RING0 = GTAB ? 32768 : 0, RING_END = STG ? RING0 + NSL * USZ : 0;
  static constexpr int S64_END = S64 ? RING0 + (SA + SB) * GSZ : 0;  // the granule rings, inside the ring area
  static constexpr int TABB = (STG ? EPI != EPI_ROPE : (NWV == 4 && BMT == 192)) ? 0 : TAB_BYTES;
  static constexpr int TAB_OFF = 2 * STAGE, TAB_END = TABB ? TAB_OFF + TABB : 0;
  // RoPE: tile-row positions (frame | row << 10 | col << 20), then the interleaved cos/sin table
  static constexpr int RPOS_OFF = TAB_OFF, RTAB_OFF = RPOS_OFF + BM * 4;
  static constexpr int RTAB_END = EPI == EPI_ROPE ? RTAB_OFF + ROPE_TAB_MAX * 8 : 0;
  static constexpr int IMG_END = DIRECT ? 0 : STAGE + NWV * PR * STR * 4;  // image in the second slot
  static constexpr int LDS_BYTES = cmax(cmax(SLOT_END, RING_END), TAB_END);
  static constexpr int THREADS = NT;
  static constexpr int BLOCKS_PER_CU = NWV == 4 ? 2 : 1;
  // regions that must not overlap: table | ring | table area, operand slots | table area
  static constexpr bool lds_disjoint = GTAB_END <= RING0 && (TABB == 0 || cmax(SLOT_END, RING_END) <= TAB_OFF) &&
                                       (EPI != EPI_ROPE || RTAB_END <= TAB_END);
};

}  // namespace
