// Fused multi-view softmax cross-entropy of the frozen-encoder probe
// (evals/video_classification_frozen/eval.py:299, 325-328): per-view CrossEntropyLoss, its gradient, the
// view-averaged softmax's argmax and the top-1 count, one head per call.
//
// A latency kernel (the eval shapes are a dozen rows of a few hundred classes), so the layout minimises
// dependent steps, not bytes: one wave owns one sample b and walks its V rows (row v*B + b) twice.
//   pass A  per row, one online max / sum-of-exponentials sweep (lane-strided, then a DPP wave combine):
//           M_v, S_v, the row loss log S_v + (M_v - x[label]);
//   pass B  per class (lane-strided), every view's p = exp(x - M_v) / S_v: the gradient store and the
//           view sum whose argmax is the prediction (ascending classes per lane + a (value, index)
//           wave reduction: the lowest index wins an exact tie).
// The statistics of view v stay in lane v's registers (v_readlane by the uniform loop counter): no LDS
// and no barrier inside a sample. More than 64 views keep log S + M in row_loss[] until the row's
// loss replaces it (same wave writes and reads it; the exponent then carries the rounding of that sum).
// Small problems run as ONE workgroup that also reduces loss[V] and `correct`; larger ones run one
// sample per wave over several workgroups and a second single-workgroup launch does that reduction.
// Every sum is fixed-order (lanes, then b ascending): bitwise reproducible, no atomics.
#include <limits.h>
#include <math.h>

#include "vj_common.h"

namespace {

constexpr int XENT_WAVES = 16;                 // waves (= samples in flight) per workgroup
constexpr int XENT_THREADS = XENT_WAVES * 64;
constexpr long XENT_ONE_BLOCK_ELEMS = 65536;   // V*B*C up to here: one workgroup, one launch

__device__ __forceinline__ long load_label(const void* labels, int i64, int b) {
  return i64 ? ((const long*)labels)[b] : (long)((const int*)labels)[b];
}

__device__ __forceinline__ float lane_bcast(float v, int lane) {  // lane: wave-uniform
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// loss[v] = mean_b row_loss[v*B + b]; correct = #{b : pred[b] == label[b]} (one workgroup)
__device__ void xent_finish(int V, int B, const void* labels, int i64, const float* row_loss, const int* pred,
                            float* loss, int* correct, int* lds_cnt) {
  const int tid = threadIdx.x;
  const float invB = 1.f / (float)B;
  for (int v = tid; v < V; v += blockDim.x) {
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += row_loss[(long)v * B + b];
    loss[v] = s * invB;
  }
  int cnt = 0;
  for (int b = tid; b < B; b += blockDim.x) cnt += (long)pred[b] == load_label(labels, i64, b) ? 1 : 0;
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
  if ((tid & 63) == 0) lds_cnt[tid >> 6] = cnt;
  __syncthreads();
  if (tid == 0) {
    int c = 0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) c += lds_cnt[w];
    *correct = c;
  }
}

__global__ __launch_bounds__(XENT_THREADS) void k_xent(int V, int B, int C, const float* __restrict__ logits, long ld,
                                                       const void* __restrict__ labels, int i64,
                                                       float* __restrict__ loss, float* row_loss,
                                                       float* __restrict__ dlogits, long lddl, int* pred,
                                                       int* __restrict__ correct) {
  __shared__ int lds_cnt[XENT_WAVES];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const float invB = 1.f / (float)B;
  const bool regs = V <= 64;  // wave-uniform
  for (int b = blockIdx.x * XENT_WAVES + wave; b < B; b += gridDim.x * XENT_WAVES) {
    const long lb = load_label(labels, i64, b);
    const bool has = lb >= 0 && lb < (long)C;  // an out-of-range label matches no class (and indexes nothing)
    float my_m = 0.f, my_is = 0.f;             // lane v: M_v and 1 / S_v
    // ---- pass A
    for (int v = 0; v < V; ++v) {
      const long r = (long)v * B + b;
      const float* row = logits + r * ld;
      float m = -INFINITY, s = 0.f;
      for (int c = lane; c < C; c += 64) {
        const float x = row[c];
        if (x > m) {
          s = s * expf(m - x) + 1.f;  // m = -inf at the first element: s = 0 * 0 + 1
          m = x;
        } else {
          s += expf(x - m);
        }
      }
      const float M = wave_max(m);
      s = m == -INFINITY ? 0.f : s * expf(m - M);  // a lane past the row's end holds nothing
      const float S = wave_sum(s);
      const float lse_m = logf(S);
      const float xl = has ? row[lb] : 0.f;  // no class matches: the loss is the log-sum-exp
      if (regs) {
        if (lane == v) {
          my_m = M;
          my_is = 1.f / S;
        }
        if (lane == 0) row_loss[r] = lse_m + (M - xl);
      } else if (lane == 0) {
        row_loss[r] = lse_m + M;  // until pass B is done
      }
    }
    if (!regs) __threadfence_block();
    // ---- pass B
    float best = -INFINITY;
    int best_c = INT_MAX;
    for (int c = lane; c < C; c += 64) {
      float acc = 0.f;
      for (int v = 0; v < V; ++v) {
        const long r = (long)v * B + b;
        const float x = logits[r * ld + c];
        float p;
        if (regs) {
          p = expf(x - lane_bcast(my_m, v)) * lane_bcast(my_is, v);
        } else {
          p = expf(x - row_loss[r]);
        }
        acc += p;
        if (dlogits) dlogits[r * lddl + c] = (p - ((long)c == lb ? 1.f : 0.f)) * invB;
      }
      if (acc > best) {
        best = acc;
        best_c = c;
      }
    }
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(best, o);
      const int oc = __shfl_xor(best_c, o);
      if (ov > best || (ov == best && oc < best_c)) {
        best = ov;
        best_c = oc;
      }
    }
    if (lane == 0) pred[b] = best_c == INT_MAX ? 0 : best_c;  // every sum NaN: class 0
    if (!regs) {
      __threadfence_block();
      if (lane == 0) {
        for (int v = 0; v < V; ++v) {
          const long r = (long)v * B + b;
          row_loss[r] = has ? row_loss[r] - logits[r * ld + lb] : row_loss[r];
        }
      }
    }
  }
  if (gridDim.x == 1) {
    __threadfence_block();
    __syncthreads();
    xent_finish(V, B, labels, i64, row_loss, pred, loss, correct, lds_cnt);
  }
}

__global__ __launch_bounds__(XENT_THREADS) void k_xent_finish(int V, int B, const void* __restrict__ labels, int i64,
                                                              const float* __restrict__ row_loss,
                                                              const int* __restrict__ pred, float* __restrict__ loss,
                                                              int* __restrict__ correct) {
  __shared__ int lds_cnt[XENT_WAVES];
  xent_finish(V, B, labels, i64, row_loss, pred, loss, correct, lds_cnt);
}

}  // namespace

extern "C" int vj_xent(int V, int B, int C, const float* logits, long ld, const void* labels, int labels_i64,
                       float* loss, float* row_loss, float* dlogits, long lddl, int* pred, int* correct,
                       void* stream) {
  VJ_CHECK_ARG(logits && labels && loss && row_loss && pred && correct, "vj_xent: null operand");
  VJ_CHECK_ARG(V >= 1 && B >= 1 && C >= 1, "vj_xent: V, B and C must be >= 1 (got %d, %d, %d)", V, B, C);
  VJ_CHECK_ARG((long)V * B <= INT_MAX, "vj_xent: V * B = %ld rows exceed int range", (long)V * B);
  VJ_CHECK_ARG(ld >= C, "vj_xent: ld %ld < C %d", ld, C);
  VJ_CHECK_ARG(!dlogits || lddl >= C, "vj_xent: dlogits stride %ld < C %d", lddl, C);
  const long elems = (long)V * B * C;
  const int blocks = elems <= XENT_ONE_BLOCK_ELEMS ? 1 : vj_cdiv(B, XENT_WAVES);
  hipLaunchKernelGGL(k_xent, dim3(blocks), dim3(XENT_THREADS), 0, (hipStream_t)stream, V, B, C, logits, ld, labels,
                     labels_i64, loss, row_loss, dlogits, lddl, pred, correct);
  VJ_LAUNCH_CHECK("vj_xent");
  if (blocks > 1) {
    hipLaunchKernelGGL(k_xent_finish, dim3(1), dim3(XENT_THREADS), 0, (hipStream_t)stream, V, B, labels, labels_i64,
                       (const float*)row_loss, (const int*)pred, loss, correct);
    VJ_LAUNCH_CHECK("vj_xent (finish)");
  }
  return VJ_OK;
}
