// Goal-image planning with the action-conditioned predictor: the stages of the cross-entropy-method loop
// (notebooks/utils/mpc_utils.py, world_model_wrapper.py) that sit between two predictor forwards. Latency
// kernels, like vj_xent / vj_focal: a few hundred samples of 7-wide actions and poses, and one pass over the
// newest predicted frame. Their point is that nothing is read back and nothing is concatenated between two
// forwards, not FLOPs.
//   vj_cem_sample  actions[s][h] = clip(noise[h][s] * std[h] + mean[h]) with the axis overrides, the zeroed
//                  rotation delta and the closed gripper (mpc_utils.py:93-107): every rollout step in one launch.
//   vj_pose_step   compute_new_pose (mpc_utils.py:166-190): xyz and gripper in f32, the Euler angles of
//                  R(action) R(pose) in f64, rounded once.
//   vj_plan_frame  F.layer_norm(frame, (D,)) -> next slot of the frame trajectory, and the L1 energy to the goal.
//   vj_cem_update  top-k selection by rank count + mean / unbiased std of the elites + the momentum update.
// No float atomics: every sum is a fixed tree or a fixed loop, two runs are bitwise equal.
#include <math.h>

#include "vj_common.h"

// The reference's f32 expressions are separate IEEE operations (torch: one kernel per op): no fma here.
#pragma clang fp contract(off)

namespace {

constexpr int PLAN_THREADS = 256;     // vj_plan_frame: 4 waves, one row each in flight
constexpr int PLAN_MAX_D = 2048;      // as vj_layernorm_fwd: a lane holds 8 float4 of a row
constexpr int UPD_THREADS = 1024;     // vj_cem_update: one workgroup
constexpr int UPD_MAX_S = 4096;       // energies + elite list in LDS
constexpr int UPD_PER_THREAD = UPD_MAX_S / UPD_THREADS;

__device__ __forceinline__ float clipf(float x, float lo, float hi) {  // torch.clip: a NaN stays a NaN
  return x < lo ? lo : (x > hi ? hi : x);
}

// fixed xor tree over the 64 lanes on doubles (every lane gets the same total)
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
  return v;
}

struct CemAxis {
  float val[4];
  int on[4];
};

__global__ __launch_bounds__(256) void k_cem_sample(int S, int rollout, const float* __restrict__ noise,
                                                    const float* __restrict__ mean, const float* __restrict__ std,
                                                    float maxnorm, float gclip, CemAxis ax, int close_from,
                                                    float* __restrict__ actions) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;  // = h * S + s: the noise's own order
  if (i >= (long)S * rollout) return;
  const int h = (int)(i / S);
  const int s = (int)(i - (long)h * S);
  const f32x4 n = *(const f32x4*)(noise + i * 4);
  const f32x4 sd = *(const f32x4*)(std + h * 4);
  const f32x4 mu = *(const f32x4*)(mean + h * 4);
  float a[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const float p = n[c] * sd[c];
    a[c] = p + mu[c];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) a[c] = clipf(a[c], -maxnorm, maxnorm);
  a[3] = clipf(a[3], -gclip, gclip);
#pragma unroll
  for (int c = 0; c < 4; ++c)
    if (ax.on[c]) a[c] = ax.val[c];
  if (close_from >= 0 && h >= close_from) a[3] = 1.f;
  float* o = actions + ((long)s * rollout + h) * 7;  // rows of 7 floats: 4-byte aligned only
  o[0] = a[0];
  o[1] = a[1];
  o[2] = a[2];
  o[3] = 0.f;
  o[4] = 0.f;
  o[5] = 0.f;
  o[6] = a[3];
}

// R = Rz(c) Ry(b) Rx(a): scipy's from_euler("xyz", [a, b, c]) (extrinsic rotations about x, then y, then z)
__device__ __forceinline__ void euler_xyz_matrix(double a, double b, double c, double R[3][3]) {
  const double sa = sin(a), ca = cos(a), sb = sin(b), cb = cos(b), sc = sin(c), cc = cos(c);
  R[0][0] = cc * cb;
  R[0][1] = cc * sb * sa - sc * ca;
  R[0][2] = cc * sb * ca + sc * sa;
  R[1][0] = sc * cb;
  R[1][1] = sc * sb * sa + cc * ca;
  R[1][2] = sc * sb * ca - cc * sa;
  R[2][0] = -sb;
  R[2][1] = cb * sa;
  R[2][2] = cb * ca;
}

__global__ __launch_bounds__(256) void k_pose_step(int S, const float* __restrict__ pose, long ldp,
                                                   const float* __restrict__ action, long lda, float* __restrict__ out,
                                                   long ldo) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  const float* p = pose + (long)s * ldp;
  const float* a = action + (long)s * lda;
  float pv[7], av[7];
#pragma unroll
  for (int c = 0; c < 7; ++c) {
    pv[c] = p[c];
    av[c] = a[c];
  }
  double P[3][3], A[3][3], M[3][3];
  euler_xyz_matrix((double)pv[3], (double)pv[4], (double)pv[5], P);
  euler_xyz_matrix((double)av[3], (double)av[4], (double)av[5], A);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) M[i][j] = A[i][0] * P[0][j] + A[i][1] * P[1][j] + A[i][2] * P[2][j];
  // M = Rz(yaw) Ry(pitch) Rx(roll): M20 = -sin(pitch), (M21, M22) = cos(pitch) (sin, cos)(roll),
  // (M10, M00) = cos(pitch) (sin, cos)(yaw). pitch in [-pi/2, pi/2], roll and yaw from atan2.
  const double cp = hypot(M[0][0], M[1][0]);
  double roll, pitch, yaw;
  pitch = atan2(-M[2][0], cp);
  if (cp > 1e-7) {
    roll = atan2(M[2][1], M[2][2]);
    yaw = atan2(M[1][0], M[0][0]);
  } else {  // gimbal lock: scipy's convention, the third angle is zero and the first carries the rest
    yaw = 0.0;
    roll = M[2][0] < 0.0 ? atan2(M[0][1], M[1][1]) : atan2(-M[0][1], M[1][1]);
  }
  float* o = out + (long)s * ldo;
  o[0] = pv[0] + av[0];
  o[1] = pv[1] + av[1];
  o[2] = pv[2] + av[2];
  o[3] = (float)roll;
  o[4] = (float)pitch;
  o[5] = (float)yaw;
  o[6] = clipf(pv[6] + av[6], 0.f, 1.f);
}

// One workgroup per sample, one wave per row (rows wave, wave + 4, ...). A lane holds chunks lane + 64 j of its
// row (float4 each). Energy: |y - goal| summed per lane in f32 (<= 32 terms), the DPP tree over the wave, then
// f64 over the wave's rows and over the 4 waves in wave order.
__global__ __launch_bounds__(PLAN_THREADS) void k_plan_frame(int R, int D, const float* __restrict__ src, long ss,
                                                             long sr, int normalize, float eps, float* __restrict__ dst,
                                                             long ds, const float* __restrict__ goal,
                                                             float* __restrict__ energy) {
  __shared__ double part[PLAN_THREADS / 64];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const long s = blockIdx.x;
  const int nchunk = D >> 2;
  const float invD = 1.f / (float)D;
  double acc = 0.0;
  for (int r = wave; r < R; r += PLAN_THREADS / 64) {
    const f32x4* row = (const f32x4*)(src + s * ss + (long)r * sr);
    f32x4 v[PLAN_MAX_D / 256];
#pragma unroll
    for (int j = 0; j < PLAN_MAX_D / 256; ++j) {
      const int c = lane + 64 * j;
      v[j] = c < nchunk ? row[c] : (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    if (normalize) {
      float sum = 0.f;
#pragma unroll
      for (int j = 0; j < PLAN_MAX_D / 256; ++j) sum += (v[j][0] + v[j][1]) + (v[j][2] + v[j][3]);
      const float mean = wave_sum(sum) * invD;
      float sq = 0.f;
#pragma unroll
      for (int j = 0; j < PLAN_MAX_D / 256; ++j) {
        if (lane + 64 * j < nchunk) {
          const f32x4 d = v[j] - mean;
          sq += (d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3]);
        }
      }
      const float var = wave_sum(sq) * invD;
      const float rstd = 1.f / sqrtf(var + eps);
#pragma unroll
      for (int j = 0; j < PLAN_MAX_D / 256; ++j) v[j] = (v[j] - mean) * rstd;
    }
    if (dst) {
      f32x4* drow = (f32x4*)(dst + s * ds + (long)r * D);
#pragma unroll
      for (int j = 0; j < PLAN_MAX_D / 256; ++j) {
        const int c = lane + 64 * j;
        if (c < nchunk) drow[c] = v[j];
      }
    }
    if (energy) {
      const f32x4* grow = (const f32x4*)(goal + (long)r * D);
      float e = 0.f;
#pragma unroll
      for (int j = 0; j < PLAN_MAX_D / 256; ++j) {
        const int c = lane + 64 * j;
        if (c < nchunk) {
          const f32x4 d = v[j] - grow[c];
          e += (fabsf(d[0]) + fabsf(d[1])) + (fabsf(d[2]) + fabsf(d[3]));
        }
      }
      acc += (double)wave_sum(e);
    }
  }
  if (energy) {
    if (lane == 0) part[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
      double t = 0.0;
      for (int w = 0; w < PLAN_THREADS / 64; ++w) t += part[w];
      energy[s] = (float)(t / ((double)R * (double)D));
    }
  }
}

// does sample j rank ahead of sample i? Smaller energy first, ties to the lower index, a NaN after every number.
__device__ __forceinline__ bool ahead_of(float ej, int j, float ei, int i) {
  const bool nj = ej != ej, ni = ei != ei;
  if (ni) return !nj || j < i;
  return !nj && (ej < ei || (ej == ei && j < i));
}

struct CemMomenta {  // (1 - m) and m as the reference's f32 scalars: xyz mean, xyz std, gripper mean, gripper std
  float keep[4];
  float take[4];
};

__global__ __launch_bounds__(UPD_THREADS) void k_cem_update(int S, int rollout, int k, const float* __restrict__ energy,
                                                            const float* __restrict__ actions, CemMomenta mom,
                                                            float* __restrict__ mean, float* __restrict__ std,
                                                            int* __restrict__ elite_idx) {
  __shared__ float e_s[UPD_MAX_S];
  __shared__ int elite_s[UPD_MAX_S];  // ascending by index
  __shared__ int byrank_s[UPD_MAX_S];  // ascending by energy: the order of the reference's topk(largest=False)
  __shared__ int chunk_cnt[UPD_MAX_S / 64];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  for (int i = tid; i < S; i += UPD_THREADS) e_s[i] = energy[i];
  __syncthreads();
  // ---- rank count; index q * 1024 + tid, so a wave's ballot covers 64 consecutive samples (chunk q * 16 + wave)
  unsigned long long mask[UPD_PER_THREAD];
#pragma unroll
  for (int q = 0; q < UPD_PER_THREAD; ++q) {
    const int i = q * UPD_THREADS + tid;
    bool sel = false;
    if (i < S) {
      const float ei = e_s[i];
      int rank = 0;
      for (int j = 0; j < S; ++j) rank += ahead_of(e_s[j], j, ei, i) ? 1 : 0;
      sel = rank < k;
      if (sel) byrank_s[rank] = i;
    }
    mask[q] = __ballot(sel);
    if (lane == 0) chunk_cnt[q * (UPD_THREADS / 64) + wave] = __popcll(mask[q]);
  }
  __syncthreads();
  // ---- the elites' indices, ascending: position = elites in earlier chunks + elites at lower lanes of this one
#pragma unroll
  for (int q = 0; q < UPD_PER_THREAD; ++q) {
    const int i = q * UPD_THREADS + tid;
    if (i < S && ((mask[q] >> lane) & 1ull)) {
      const int chunk = q * (UPD_THREADS / 64) + wave;
      int pos = 0;
      for (int c = 0; c < chunk; ++c) pos += chunk_cnt[c];
      pos += __popcll(mask[q] & ((1ull << lane) - 1ull));
      elite_s[pos] = i;
      if (elite_idx) elite_idx[pos] = i;
    }
  }
  __syncthreads();
  // ---- one wave per (rollout step, column). The mean is the reference's own f32 arithmetic: the elites summed
  // one after the other in rank order, then divided by k (torch's mean over the gathered top-k rows, so equal
  // inputs give the reference's bits). The unbiased std is two-pass in f64 around the f64 mean, rounded once
  // (torch accumulates it in f64 as well). Then the momentum update in f32 (mpc_utils.py:136-150).
  for (int p = wave; p < rollout * 4; p += UPD_THREADS / 64) {
    const int h = p >> 2;
    const int c4 = p & 3;
    const int col = c4 == 3 ? 6 : c4;
    const float* base = actions + (long)h * 7 + col;
    float fsum = 0.f;
    double sum = 0.0;
    for (int e0 = 0; e0 < k; e0 += 64) {  // wave-uniform trip count
      const int e = e0 + lane;
      const float v = e < k ? base[(long)byrank_s[e] * rollout * 7] : 0.f;
      sum += (double)v;
      const int n = k - e0 < 64 ? k - e0 : 64;
      for (int j = 0; j < n; ++j) fsum += __shfl(v, j, 64);  // every lane adds the same values in the same order
    }
    const double mu = wave_sum_f64(sum) / (double)k;
    double sq = 0.0;
    for (int e = lane; e < k; e += 64) {
      const double d = (double)base[(long)elite_s[e] * rollout * 7] - mu;
      sq += d * d;
    }
    const double var = wave_sum_f64(sq) / (double)(k - 1);
    if (lane == 0) {
      const int gm = c4 == 3 ? 2 : 0;  // momenta: xyz (mean 0, std 1), gripper (mean 2, std 3)
      const float m_new = fsum / (float)k;
      const float s_new = (float)sqrt(var);
      const float a0 = m_new * mom.keep[gm];
      const float a1 = mean[p] * mom.take[gm];
      const float b0 = s_new * mom.keep[gm + 1];
      const float b1 = std[p] * mom.take[gm + 1];
      mean[p] = a0 + a1;
      std[p] = b0 + b1;
    }
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace

extern "C" int vj_cem_sample(int S, int rollout, const float* noise, const float* mean, const float* std,
                             float maxnorm, float gripper_clip, const int* axis_on, const float* axis_val,
                             int close_from, float* actions, void* stream) {
  VJ_CHECK_ARG(noise && mean && std && actions, "vj_cem_sample: null operand");
  VJ_CHECK_ARG(S >= 1 && rollout >= 1, "vj_cem_sample: S and rollout must be >= 1 (got %d, %d)", S, rollout);
  VJ_CHECK_ARG((long)S * rollout <= (1L << 26), "vj_cem_sample: S * rollout = %ld exceeds 2^26", (long)S * rollout);
  VJ_CHECK_ARG(aligned16(noise) && aligned16(mean) && aligned16(std),
               "vj_cem_sample: noise, mean and std must be 16-byte aligned");
  VJ_CHECK_ARG(maxnorm >= 0.f && gripper_clip >= 0.f, "vj_cem_sample: maxnorm and gripper_clip must be >= 0");
  VJ_CHECK_ARG(close_from >= -1, "vj_cem_sample: close_from must be -1 (never) or a rollout step (got %d)", close_from);
  VJ_CHECK_ARG(!axis_on || axis_val, "vj_cem_sample: axis_on without axis_val");
  CemAxis ax;
  for (int c = 0; c < 4; ++c) {
    ax.on[c] = axis_on ? (axis_on[c] != 0) : 0;
    ax.val[c] = ax.on[c] ? axis_val[c] : 0.f;
  }
  const long n = (long)S * rollout;
  hipLaunchKernelGGL(k_cem_sample, dim3(vj_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, S, rollout, noise, mean,
                     std, maxnorm, gripper_clip, ax, close_from, actions);
  VJ_LAUNCH_CHECK("vj_cem_sample");
  return VJ_OK;
}

extern "C" int vj_pose_step(int S, const float* pose, long ldp, const float* action, long lda, float* out, long ldo,
                            void* stream) {
  VJ_CHECK_ARG(pose && action && out, "vj_pose_step: null operand");
  VJ_CHECK_ARG(S >= 1, "vj_pose_step: S must be >= 1 (got %d)", S);
  VJ_CHECK_ARG(ldp >= 7 && lda >= 7 && ldo >= 7, "vj_pose_step: row strides %ld / %ld / %ld < 7", ldp, lda, ldo);
  hipLaunchKernelGGL(k_pose_step, dim3(vj_cdiv(S, 256)), dim3(256), 0, (hipStream_t)stream, S, pose, ldp, action, lda,
                     out, ldo);
  VJ_LAUNCH_CHECK("vj_pose_step");
  return VJ_OK;
}

extern "C" int vj_plan_frame(int S, int R, int D, const float* src, long src_sample_stride, long src_row_stride,
                             int normalize, float eps, float* dst, long dst_sample_stride, const float* goal,
                             float* energy, void* stream) {
  VJ_CHECK_ARG(src, "vj_plan_frame: null operand (src)");
  VJ_CHECK_ARG(dst || energy, "vj_plan_frame: nothing to do (neither dst nor energy)");
  VJ_CHECK_ARG(!energy || goal, "vj_plan_frame: null operand (energy without goal)");
  VJ_CHECK_ARG(S >= 1 && R >= 1, "vj_plan_frame: S and R must be >= 1 (got %d, %d)", S, R);
  VJ_CHECK_ARG(D >= 4 && D % 4 == 0, "vj_plan_frame: D must be a positive multiple of 4 (got %d)", D);
  VJ_CHECK_ARG(D <= PLAN_MAX_D, "vj_plan_frame: D %d > %d", D, PLAN_MAX_D);
  VJ_CHECK_ARG(src_row_stride >= D, "vj_plan_frame: src row stride %ld < D %d", src_row_stride, D);
  VJ_CHECK_ARG(src_sample_stride >= (long)(R - 1) * src_row_stride + D,
               "vj_plan_frame: src sample stride %ld < the %d rows of a sample", src_sample_stride, R);
  VJ_CHECK_ARG(!dst || dst_sample_stride >= (long)R * D, "vj_plan_frame: dst sample stride %ld < R * D = %ld",
               dst_sample_stride, (long)R * D);
  VJ_CHECK_ARG(src_row_stride % 4 == 0 && src_sample_stride % 4 == 0 && (!dst || dst_sample_stride % 4 == 0),
               "vj_plan_frame: strides must be multiples of 4 floats");
  VJ_CHECK_ARG(aligned16(src) && aligned16(dst) && aligned16(goal),
               "vj_plan_frame: src, dst and goal must be 16-byte aligned");
  hipLaunchKernelGGL(k_plan_frame, dim3(S), dim3(PLAN_THREADS), 0, (hipStream_t)stream, R, D, src, src_sample_stride,
                     src_row_stride, normalize ? 1 : 0, eps, dst, dst ? dst_sample_stride : 0L, goal, energy);
  VJ_LAUNCH_CHECK("vj_plan_frame");
  return VJ_OK;
}

extern "C" int vj_cem_update(int S, int rollout, int k, const float* energy, const float* actions,
                             double momentum_mean, double momentum_std, double momentum_mean_gripper,
                             double momentum_std_gripper, float* mean, float* std, int* elite_idx, void* stream) {
  VJ_CHECK_ARG(energy && actions && mean && std, "vj_cem_update: null operand");
  VJ_CHECK_ARG(S >= 1 && rollout >= 1, "vj_cem_update: S and rollout must be >= 1 (got %d, %d)", S, rollout);
  VJ_CHECK_ARG(rollout <= 4096, "vj_cem_update: rollout %d > 4096", rollout);
  VJ_CHECK_ARG(S <= UPD_MAX_S, "vj_cem_update: S %d > %d", S, UPD_MAX_S);
  VJ_CHECK_ARG(k >= 2, "vj_cem_update: k must be >= 2 (the unbiased std of one elite is undefined), got %d", k);
  VJ_CHECK_ARG(k <= S, "vj_cem_update: k %d > S %d", k, S);
  const double m[4] = {momentum_mean, momentum_std, momentum_mean_gripper, momentum_std_gripper};
  CemMomenta mom;
  for (int i = 0; i < 4; ++i) {
    mom.keep[i] = (float)(1.0 - m[i]);  // the reference's Python float (1.0 - m), then an f32 scalar
    mom.take[i] = (float)m[i];
  }
  hipLaunchKernelGGL(k_cem_update, dim3(1), dim3(UPD_THREADS), 0, (hipStream_t)stream, S, rollout, k, energy, actions,
                     mom, mean, std, elite_idx);
  VJ_LAUNCH_CHECK("vj_cem_update");
  return VJ_OK;
}
