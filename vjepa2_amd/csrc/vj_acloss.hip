// V-JEPA 2-AC post-training, the loss side of one step (app/vjepa_droid/train.py: forward_predictions' layer_norm,
// loss_fn's mean(|z - h| ** p) / p, and their autograd) as two row kernels and a fixed-order reduce over f32
// [B, R, D] rows. z may be a frame slice of a longer predictor output and h the target sequence shifted by one
// frame: both come with a sample stride and a row stride, nothing is copied first.
//   vj_ac_loss_fwd     zn = layer_norm(z) (or z), per-row (mean, rstd), per-row sum_d |zn - h| ** p
//   vj_ac_loss_bwd     g = scale sign(zn - h) |zn - h| ** (p - 1) + gzn, dz = the LayerNorm backward of g; zn is
//                      recomputed from z and the stats by the forward's own expression (the same bits)
//   vj_ac_loss_reduce  loss = scale * the row sums added in f64 in a fixed order
// One row per wave, a lane holds float4 chunks lane + 64 j of its row (as k_plan_frame, whose normalisation
// arithmetic this repeats operation for operation). No float atomics: two runs are bitwise equal.
#include <math.h>

#include "vj_common.h"

// as vj_plan.hip: the normalisation is the same sequence of separate IEEE operations there and here
#pragma clang fp contract(off)

namespace {

constexpr int ACL_THREADS = 256;    // 4 waves, one row each
constexpr int ACL_WAVES = ACL_THREADS / 64;
constexpr int ACL_MAX_D = 2048;     // a lane holds 8 float4 of a row
constexpr int ACL_CHUNKS = ACL_MAX_D / 256;
constexpr int RED_THREADS = 1024;   // vj_ac_loss_reduce: one workgroup

__device__ __forceinline__ double wave_sum_f64(double v) {  // fixed xor tree, every lane gets the same total
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
  return v;
}

__device__ __forceinline__ float sum4(const f32x4 a) { return (a[0] + a[1]) + (a[2] + a[3]); }

// |d| ** p: p == 1 and p == 2 without powf (PMODE 1 / 2), anything else through powf (PMODE 0)
template <int PMODE>
__device__ __forceinline__ float abs_pow(float d, float p) {
  if (PMODE == 1) return fabsf(d);
  if (PMODE == 2) return d * d;
  return powf(fabsf(d), p);
}

// sign(d) |d| ** (p - 1), sign(0) = 0 (torch)
template <int PMODE>
__device__ __forceinline__ float sign_pow(float d, float pm1) {
  if (PMODE == 2) return d;
  const float s = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
  if (PMODE == 1) return s;
  return d == 0.f ? 0.f : s * powf(fabsf(d), pm1);  // p < 1: 0 ** (p - 1) is inf, and sign(0) inf a NaN
}

template <int PMODE>
__global__ __launch_bounds__(ACL_THREADS) void k_ac_loss_fwd(long rows, int R, int D, const float* __restrict__ z,
                                                             long zss, long zrs, const float* __restrict__ h, long hss,
                                                             long hrs, int normalize, float eps, float p,
                                                             float* __restrict__ zn, float* __restrict__ stats,
                                                             float* __restrict__ rowsum) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * ACL_WAVES + (threadIdx.x >> 6);
  if (row >= rows) return;  // wave-uniform
  const long b = row / R;
  const long r = row - b * R;
  const int nchunk = D >> 2;
  const float invD = 1.f / (float)D;
  const f32x4* zrow = (const f32x4*)(z + b * zss + r * zrs);
  f32x4 v[ACL_CHUNKS];
#pragma unroll
  for (int j = 0; j < ACL_CHUNKS; ++j) {
    const int c = lane + 64 * j;
    v[j] = c < nchunk ? zrow[c] : (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  if (normalize) {
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < ACL_CHUNKS; ++j) sum += sum4(v[j]);
    const float mean = wave_sum(sum) * invD;
    float sq = 0.f;
#pragma unroll
    for (int j = 0; j < ACL_CHUNKS; ++j) {
      if (lane + 64 * j < nchunk) {
        const f32x4 d = v[j] - mean;
        sq += sum4(d * d);
      }
    }
    const float var = wave_sum(sq) * invD;
    const float rstd = 1.f / sqrtf(var + eps);
#pragma unroll
    for (int j = 0; j < ACL_CHUNKS; ++j) v[j] = (v[j] - mean) * rstd;
    if (lane == 0) *(f32x2*)(stats + row * 2) = (f32x2){mean, rstd};
  }
  if (zn) {
    f32x4* orow = (f32x4*)(zn + row * D);
#pragma unroll
    for (int j = 0; j < ACL_CHUNKS; ++j) {
      const int c = lane + 64 * j;
      if (c < nchunk) orow[c] = v[j];
    }
  }
  if (rowsum) {
    const f32x4* hrow = (const f32x4*)(h + b * hss + r * hrs);
    float e = 0.f;
#pragma unroll
    for (int j = 0; j < ACL_CHUNKS; ++j) {
      const int c = lane + 64 * j;
      if (c < nchunk) {
        const f32x4 d = v[j] - hrow[c];
        e += (abs_pow<PMODE>(d[0], p) + abs_pow<PMODE>(d[1], p)) + (abs_pow<PMODE>(d[2], p) + abs_pow<PMODE>(d[3], p));
      }
    }
    e = wave_sum(e);
    if (lane == 0) rowsum[row] = e;
  }
}

template <int PMODE>
__global__ __launch_bounds__(ACL_THREADS) void k_ac_loss_bwd(long rows, int R, int D, const float* __restrict__ z,
                                                             long zss, long zrs, const float* __restrict__ stats,
                                                             const float* __restrict__ h, long hss, long hrs,
                                                             int normalize, float p, float scale,
                                                             const float* __restrict__ gscale,
                                                             const float* __restrict__ gzn, float* __restrict__ dz) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * ACL_WAVES + (threadIdx.x >> 6);
  if (row >= rows) return;  // wave-uniform
  const long b = row / R;
  const long r = row - b * R;
  const int nchunk = D >> 2;
  const float invD = 1.f / (float)D;
  const f32x4* zrow = (const f32x4*)(z + b * zss + r * zrs);
  f32x4 v[ACL_CHUNKS], g[ACL_CHUNKS];
#pragma unroll
  for (int j = 0; j < ACL_CHUNKS; ++j) {
    const int c = lane + 64 * j;
    v[j] = c < nchunk ? zrow[c] : (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  float rstd = 1.f;
  if (normalize) {
    const f32x2 st = *(const f32x2*)(stats + row * 2);
    rstd = st[1];
#pragma unroll
    for (int j = 0; j < ACL_CHUNKS; ++j) v[j] = (v[j] - st[0]) * rstd;  // the forward's zn, bit for bit
  }
  const float sc = gscale ? scale * gscale[0] : scale;
  const float pm1 = p - 1.f;
#pragma unroll
  for (int j = 0; j < ACL_CHUNKS; ++j) {
    const int c = lane + 64 * j;
    g[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (c < nchunk) {
      if (h) {
        const f32x4 d = v[j] - ((const f32x4*)(h + b * hss + r * hrs))[c];
#pragma unroll
        for (int e = 0; e < 4; ++e) g[j][e] = sc * sign_pow<PMODE>(d[e], pm1);
      }
      if (gzn) g[j] = g[j] + ((const f32x4*)(gzn + row * D))[c];
    }
  }
  if (normalize) {
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < ACL_CHUNKS; ++j) {  // lanes past the row hold zeros in g
      s1 += sum4(g[j]);
      s2 += sum4(g[j] * v[j]);
    }
    const float m1 = wave_sum(s1) * invD;
    const float m2 = wave_sum(s2) * invD;
#pragma unroll
    for (int j = 0; j < ACL_CHUNKS; ++j) g[j] = ((g[j] - m1) - v[j] * m2) * rstd;
  }
  f32x4* orow = (f32x4*)(dz + row * D);
#pragma unroll
  for (int j = 0; j < ACL_CHUNKS; ++j) {
    const int c = lane + 64 * j;
    if (c < nchunk) orow[c] = g[j];
  }
}

// thread t adds rows t, t + 1024, ... in f64, the xor tree per wave, then the 16 waves in wave order
__global__ __launch_bounds__(RED_THREADS) void k_ac_loss_reduce(long n, const float* __restrict__ rowsum, double scale,
                                                                float* __restrict__ loss) {
  __shared__ double part[RED_THREADS / 64];
  double acc = 0.0;
  for (long i = threadIdx.x; i < n; i += RED_THREADS) acc += (double)rowsum[i];
  acc = wave_sum_f64(acc);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int w = 0; w < RED_THREADS / 64; ++w) t += part[w];
    loss[0] = (float)(t * scale);
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// the checks both entry points share; `who` names the entry point in the message
int check_rows(const char* who, int B, int R, int D, long zss, long zrs, const void* h, long hss, long hrs) {
  VJ_CHECK_ARG(B >= 1 && R >= 1, "%s: B and R must be >= 1 (got %d, %d)", who, B, R);
  VJ_CHECK_ARG((long)B * R <= (1L << 30), "%s: B * R = %ld exceeds 2^30", who, (long)B * R);
  VJ_CHECK_ARG(D >= 4 && D % 4 == 0, "%s: D must be a positive multiple of 4 (got %d)", who, D);
  VJ_CHECK_ARG(D <= ACL_MAX_D, "%s: D %d > %d", who, D, ACL_MAX_D);
  VJ_CHECK_ARG(zrs >= D, "%s: z row stride %ld < D %d", who, zrs, D);
  VJ_CHECK_ARG(zss >= (long)(R - 1) * zrs + D, "%s: z sample stride %ld < the %d rows of a sample", who, zss, R);
  VJ_CHECK_ARG(!h || hrs >= D, "%s: h row stride %ld < D %d", who, hrs, D);
  VJ_CHECK_ARG(!h || hss >= (long)(R - 1) * hrs + D, "%s: h sample stride %ld < the %d rows of a sample", who, hss, R);
  VJ_CHECK_ARG(zrs % 4 == 0 && zss % 4 == 0 && (!h || (hrs % 4 == 0 && hss % 4 == 0)),
               "%s: strides must be multiples of 4 floats", who);
  return VJ_OK;
}

}  // namespace

extern "C" int vj_ac_loss_fwd(int B, int R, int D, const float* z, long z_sample_stride, long z_row_stride,
                              const float* h, long h_sample_stride, long h_row_stride, int normalize, float eps,
                              float p, float* zn, float* stats, float* rowsum, void* stream) {
  VJ_CHECK_ARG(z, "vj_ac_loss_fwd: null operand (z)");
  VJ_CHECK_ARG(zn || rowsum, "vj_ac_loss_fwd: nothing to do (neither zn nor rowsum)");
  VJ_CHECK_ARG(!rowsum || h, "vj_ac_loss_fwd: null operand (rowsum without h)");
  VJ_CHECK_ARG(!normalize || stats, "vj_ac_loss_fwd: normalize without stats");
  if (const int rc = check_rows("vj_ac_loss_fwd", B, R, D, z_sample_stride, z_row_stride, rowsum ? h : nullptr,
                                h_sample_stride, h_row_stride))
    return rc;
  VJ_CHECK_ARG(!rowsum || p > 0.f, "vj_ac_loss_fwd: loss exponent must be > 0 (got %g)", (double)p);
  VJ_CHECK_ARG(aligned16(z) && (!rowsum || aligned16(h)) && aligned16(zn),
               "vj_ac_loss_fwd: z, h and zn must be 16-byte aligned");
  VJ_CHECK_ARG(((uintptr_t)stats & 7u) == 0, "vj_ac_loss_fwd: stats must be 8-byte aligned");
  const long rows = (long)B * R;
  const dim3 grid(vj_cdiv(rows, ACL_WAVES)), block(ACL_THREADS);
  const int nrm = normalize ? 1 : 0;
  if (!rowsum) h = nullptr;
#define ACL_FWD(PM)                                                                                              \
  hipLaunchKernelGGL(k_ac_loss_fwd<PM>, grid, block, 0, (hipStream_t)stream, rows, R, D, z, z_sample_stride,     \
                     z_row_stride, h, h_sample_stride, h_row_stride, nrm, eps, p, zn, stats, rowsum)
  if (p == 1.f) ACL_FWD(1);
  else if (p == 2.f) ACL_FWD(2);
  else ACL_FWD(0);
#undef ACL_FWD
  VJ_LAUNCH_CHECK("vj_ac_loss_fwd");
  return VJ_OK;
}

extern "C" int vj_ac_loss_bwd(int B, int R, int D, const float* z, long z_sample_stride, long z_row_stride,
                              const float* stats, const float* h, long h_sample_stride, long h_row_stride,
                              int normalize, float p, float scale, const float* gscale, const float* gzn, float* dz,
                              void* stream) {
  VJ_CHECK_ARG(z && dz, "vj_ac_loss_bwd: null operand (z or dz)");
  VJ_CHECK_ARG(h || gzn, "vj_ac_loss_bwd: nothing to do (neither h nor gzn)");
  VJ_CHECK_ARG(!normalize || stats, "vj_ac_loss_bwd: normalize without stats");
  if (const int rc = check_rows("vj_ac_loss_bwd", B, R, D, z_sample_stride, z_row_stride, h, h_sample_stride,
                                h_row_stride))
    return rc;
  VJ_CHECK_ARG(!h || p > 0.f, "vj_ac_loss_bwd: loss exponent must be > 0 (got %g)", (double)p);
  VJ_CHECK_ARG(aligned16(z) && aligned16(h) && aligned16(gzn) && aligned16(dz),
               "vj_ac_loss_bwd: z, h, gzn and dz must be 16-byte aligned");
  VJ_CHECK_ARG(((uintptr_t)stats & 7u) == 0, "vj_ac_loss_bwd: stats must be 8-byte aligned");
  const long rows = (long)B * R;
  const dim3 grid(vj_cdiv(rows, ACL_WAVES)), block(ACL_THREADS);
  const int nrm = normalize ? 1 : 0;
#define ACL_BWD(PM)                                                                                              \
  hipLaunchKernelGGL(k_ac_loss_bwd<PM>, grid, block, 0, (hipStream_t)stream, rows, R, D, z, z_sample_stride,     \
                     z_row_stride, stats, h, h_sample_stride, h_row_stride, nrm, p, scale, gscale, gzn, dz)
  if (p == 1.f) ACL_BWD(1);
  else if (p == 2.f) ACL_BWD(2);
  else ACL_BWD(0);
#undef ACL_BWD
  VJ_LAUNCH_CHECK("vj_ac_loss_bwd");
  return VJ_OK;
}

extern "C" int vj_ac_loss_reduce(long n, const float* rowsum, double scale, float* loss, void* stream) {
  VJ_CHECK_ARG(rowsum && loss, "vj_ac_loss_reduce: null operand");
  VJ_CHECK_ARG(n >= 1, "vj_ac_loss_reduce: n must be >= 1 (got %ld)", n);
  hipLaunchKernelGGL(k_ac_loss_reduce, dim3(1), dim3(RED_THREADS), 0, (hipStream_t)stream, n, rowsum, scale, loss);
  VJ_LAUNCH_CHECK("vj_ac_loss_reduce");
  return VJ_OK;
}
