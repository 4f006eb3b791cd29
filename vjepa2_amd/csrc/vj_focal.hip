// Fused sigmoid focal loss, its gradient and the top-k class-recall bookkeeping of the frozen
// action-anticipation probe (evals/action_anticipation_frozen/losses.py:9-49 with reduction="sum",
// metrics.py:19-42), up to three heads (verb, noun, action) of one classifier per launch.
//
// A latency kernel like vj_xent (a dozen rows of 97 / 300 / ~3.8 k classes): one wave owns one row of
// one segment and makes two lane-strided sweeps over it (the second finds the row in cache).
//   loss   with s = -x for the label's class and +x for every other one, BCEWithLogits = softplus(s),
//          1 - p_t = sigmoid(s) and (1 - p_t)^gamma = exp(-gamma * softplus(-s)) (sigmoid(s)^2 when gamma
//          is 2): everything comes from e = exp(-|s|) and log1p(e), no log(1 - p), finite for |x| far
//          beyond 80. d loss / dx = +-alpha_t * (1 - p_t)^gamma * (sigmoid(s) + gamma * softplus(s) * p_t).
//   recall the row is a hit iff the label is among the row's top k once the invalid classes are pushed
//          below every valid one. No top-k list is built; the label's RANK is counted instead:
//            rank = #{valid c : x_c > x_label} + #{valid c < label : x_c == x_label},  hit = rank < k.
//          If the label's own class is invalid, every valid class counts as greater and the invalid
//          classes of a lower index as ties. A NaN compares as not greater. TIE RULE: among equal
//          values the lower class index ranks first. (torch.topk leaves the order of ties unspecified;
//          wherever the reference's top k is tie-free the two agree.)
//          hit: tp[label] += 1, miss: fn[label] += 1 (integer atomics: exact in any order).
// A label outside [0, C) matches no class, indexes nothing and updates no counter (its hit flag is 0).
// Each lane sums its elements in f64, the wave combine is the fixed DPP tree, loss[s] is the f64 sum of the
// row sums in ascending b: bitwise reproducible, no float atomics. Small problems run as ONE workgroup
// that also writes loss[]; larger ones run 4 rows per workgroup and a second single-workgroup launch
// sums the rows.
#include <limits.h>
#include <math.h>

#include "vj_common.h"

namespace {

constexpr int FOCAL_WAVES = 16;                // one workgroup: rows in flight
constexpr int FOCAL_WAVES_MULTI = 4;           // several workgroups: rows per workgroup
constexpr long FOCAL_ONE_BLOCK_ELEMS = 16384;  // B * sum(C_s) up to here: one workgroup, one launch
constexpr int FOCAL_MAX_SEG = 3;

struct FocalSeg {
  const float* x;
  const void* labels;
  const unsigned char* valid;
  float* dx;
  int* tp;
  int* fn;
  long ld;
  long lddx;
  int C;
  int pad_;
};
struct FocalArgs {
  FocalSeg s[FOCAL_MAX_SEG];
};

__device__ __forceinline__ long focal_label(const void* labels, int i64, int b) {
  return i64 ? ((const long*)labels)[b] : (long)((const int*)labels)[b];
}

__device__ __forceinline__ int wave_sum_int(int v) {  // wave_sum's DPP / permlane tree on integers
  uint32_t u = (uint32_t)v;
  u += dpp_u<DPP_XOR1>(u);
  u += dpp_u<DPP_XOR2>(u);
  u += dpp_u<DPP_HALF_MIRROR>(u);
  u += dpp_u<DPP_MIRROR>(u);
  auto r = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  u = r[0] + r[1];
  r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  return (int)(r[0] + r[1]);
}

// One element: its loss and d loss / dx. t: this is the label's class. G2: gamma == 2.
template <bool G2>
__device__ __forceinline__ void focal_elem(float x, bool t, float alpha, float gamma, float& l, float& g) {
  const float s = t ? -x : x;
  const float e = expf(-fabsf(s));
  const float l1p = log1pf(e);
  const float inv = 1.f / (1.f + e);
  const float sig = s >= 0.f ? inv : e * inv;  // sigmoid(s) = 1 - p_t
  const float pt = s >= 0.f ? e * inv : inv;   // p_t
  const float sp = fmaxf(s, 0.f) + l1p;        // softplus(s) = BCEWithLogits(x, t)
  const float mod = G2 ? sig * sig : expf(-gamma * (fmaxf(-s, 0.f) + l1p));
  const float a = alpha >= 0.f ? (t ? alpha : 1.f - alpha) : 1.f;
  l = a * sp * mod;
  const float d = a * mod * (sig + gamma * sp * pt);
  g = t ? -d : d;
}

template <bool G2>
__device__ __forceinline__ float focal_sweep(const float* __restrict__ row, float* __restrict__ drow, int C, long lb,
                                             float alpha, float gamma, int lane) {
  double acc = 0.0;
  for (int c = lane; c < C; c += 64) {
    float l, g;
    focal_elem<G2>(row[c], (long)c == lb, alpha, gamma, l, g);
    acc += (double)l;
    if (drow) drow[c] = g;
  }
  return wave_sum((float)acc);
}

// loss[s] = sum_b row_loss[s * B + b] (threads 0 .. nseg-1 of one workgroup)
__device__ void focal_finish(int nseg, int B, const float* row_loss, float* loss) {
  const int s = threadIdx.x;
  if (s < nseg) {
    double a = 0.0;
    for (int b = 0; b < B; ++b) a += (double)row_loss[(long)s * B + b];
    loss[s] = (float)a;
  }
}

__global__ __launch_bounds__(FOCAL_WAVES * 64) void k_focal(FocalArgs A, int nseg, int B, int i64, float alpha,
                                                            float gamma, int k, int loss_kind, float* __restrict__ loss,
                                                            float* row_loss, int* __restrict__ hit) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int waves = blockDim.x >> 6;
  const int rows = nseg * B;
  for (int r = blockIdx.x * waves + wave; r < rows; r += gridDim.x * waves) {
    const int si = r / B;  // wave-uniform
    const int b = r - si * B;
    const FocalSeg S = si == 0 ? A.s[0] : si == 1 ? A.s[1] : A.s[2];
    const int C = S.C;
    const float* row = S.x + (long)b * S.ld;
    const long lb = focal_label(S.labels, i64, b);
    const bool has = lb >= 0 && lb < (long)C;  // an out-of-range label matches no class (and indexes nothing)
    if (loss_kind) {
      float* drow = S.dx ? S.dx + (long)b * S.lddx : nullptr;
      const float sum = gamma == 2.f ? focal_sweep<true>(row, drow, C, lb, alpha, gamma, lane)
                                     : focal_sweep<false>(row, drow, C, lb, alpha, gamma, lane);
      if (lane == 0) row_loss[r] = sum;
    }
    // ---- the label's rank among the valid classes
    int h = 0;
    if (has) {
      const unsigned char* valid = S.valid;
      const float xl = row[lb];
      const bool lvalid = valid ? valid[lb] != 0 : true;
      int cnt = 0;
      for (int c = lane; c < C; c += 64) {
        const bool v = valid ? valid[c] != 0 : true;
        const float x = row[c];
        bool ahead;
        if (lvalid) {
          ahead = v && (x > xl || (x == xl && (long)c < lb));
        } else {
          ahead = v || (long)c < lb;
        }
        cnt += ahead ? 1 : 0;
      }
      cnt = wave_sum_int(cnt);
      h = cnt < k ? 1 : 0;
      if (lane == 0) atomicAdd(h ? S.tp + lb : S.fn + lb, 1);
    }
    if (lane == 0) hit[r] = h;
  }
  if (gridDim.x == 1 && loss_kind) {
    __threadfence_block();
    __syncthreads();
    focal_finish(nseg, B, row_loss, loss);
  }
}

__global__ __launch_bounds__(64) void k_focal_finish(int nseg, int B, const float* __restrict__ row_loss,
                                                     float* __restrict__ loss) {
  focal_finish(nseg, B, row_loss, loss);
}

}  // namespace

extern "C" int vj_focal(int B, int nseg, const float* const* logits, const long* ld, const int* C,
                        const void* const* labels, int labels_i64, const unsigned char* const* valid,
                        float* const* dlogits, const long* lddl, int* const* tp, int* const* fn, float alpha,
                        float gamma, int k, int loss_kind, float* loss, float* row_loss, int* hit, void* stream) {
  VJ_CHECK_ARG(nseg >= 1 && nseg <= FOCAL_MAX_SEG, "vj_focal: nseg must be 1..3 (got %d)", nseg);
  VJ_CHECK_ARG(loss_kind == 0 || loss_kind == 1, "vj_focal: loss_kind must be 0 (metrics only) or 1 (focal), got %d",
               loss_kind);
  VJ_CHECK_ARG(logits && ld && C && labels && tp && fn && hit, "vj_focal: null operand");
  VJ_CHECK_ARG(!loss_kind || (loss && row_loss), "vj_focal: null loss operand (loss and row_loss with loss_kind 1)");
  VJ_CHECK_ARG(B >= 1 && k >= 1, "vj_focal: B and k must be >= 1 (got %d, %d)", B, k);
  VJ_CHECK_ARG((long)B * nseg <= INT_MAX, "vj_focal: B * nseg = %ld rows exceed int range", (long)B * nseg);
  FocalArgs A;
  memset(&A, 0, sizeof(A));
  long elems = 0;
  for (int s = 0; s < nseg; ++s) {
    VJ_CHECK_ARG(logits[s] && labels[s] && tp[s] && fn[s], "vj_focal: null operand in segment %d", s);
    VJ_CHECK_ARG(C[s] >= 1, "vj_focal: C must be >= 1 (segment %d has %d)", s, C[s]);
    VJ_CHECK_ARG(ld[s] >= C[s], "vj_focal: segment %d ld %ld < C %d", s, ld[s], C[s]);
    float* dx = loss_kind && dlogits ? dlogits[s] : nullptr;
    VJ_CHECK_ARG(!dx || (lddl && lddl[s] >= C[s]), "vj_focal: segment %d dlogits stride %ld < C %d", s,
                 lddl ? lddl[s] : 0L, C[s]);
    A.s[s].x = logits[s];
    A.s[s].labels = labels[s];
    A.s[s].valid = valid ? valid[s] : nullptr;
    A.s[s].dx = dx;
    A.s[s].tp = tp[s];
    A.s[s].fn = fn[s];
    A.s[s].ld = ld[s];
    A.s[s].lddx = dx ? lddl[s] : 0;
    A.s[s].C = C[s];
    elems += (long)B * C[s];
  }
  const int rows = B * nseg;
  const bool one = elems <= FOCAL_ONE_BLOCK_ELEMS;
  const int blocks = one ? 1 : vj_cdiv(rows, FOCAL_WAVES_MULTI);
  const int threads = (one ? FOCAL_WAVES : FOCAL_WAVES_MULTI) * 64;
  hipLaunchKernelGGL(k_focal, dim3(blocks), dim3(threads), 0, (hipStream_t)stream, A, nseg, B, labels_i64, alpha, gamma,
                     k, loss_kind, loss, row_loss, hit);
  VJ_LAUNCH_CHECK("vj_focal");
  if (blocks > 1 && loss_kind) {
    hipLaunchKernelGGL(k_focal_finish, dim3(1), dim3(64), 0, (hipStream_t)stream, nseg, B, (const float*)row_loss,
                       loss);
    VJ_LAUNCH_CHECK("vj_focal (finish)");
  }
  return VJ_OK;
}
