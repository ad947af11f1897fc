// Scoring a visit sweep against its anchor: the second half of mcts_analysis.py:run_analysis (:1150-1400), on the device.
// azmi_search_run_to leaves the snapshots of every (tree, checkpoint) in one block (SbSweepArrays); these kernels score every
// row against the anchor row of the same tree and reduce the scores per checkpoint, so that nothing but [N, J] figures leaves
// the device.  The six policy figures are policy_metrics.py's; azmi_policy_divergences runs the same row function over any
// [rows, M] pair of policies (the batch_* functions network_pareto.py calls).
//
// Arithmetic: float64 throughout, the float32 snapshot values converted exactly (as net_vs_search does).  The reference computes
// in float32 numpy, whose pairwise sums nothing can be matched bit for bit against; the yardstick of these kernels is the same
// expressions in float64.  The sums run lane-strided and are folded across the lanes by an xor butterfly, which gives every
// lane the same bits: not numpy's order, a few ulp of a sum of at most 2 M terms.
//
// top_k(x) is THE PROJECT'S DEFINITION: the last k indices of x ordered ascending by (value, index), which is
// np.argsort(x, kind="stable")[-k:] - among equal values the higher index ranks higher.  The reference calls np.argsort with its
// default kind, which is not stable for every M and numpy build, so its choice among equal values is not a definition.  With
// M < k every index is in both sets and the divisor stays k (identical Connect4 policies: top9 = 7 / 9, as the reference's
// formula gives).  k rounds of a wave arg-max on the (value, index) key: round r takes the largest key below round r - 1's
// winner, which removes the winners without storing anything; no sort, no atomics.
//
// Same grid-to-tree mapping as search_batch_kernels.h: the small game's 8-lane groups, one wavefront per tree for the wide games;
// a tree's lanes walk its J checkpoints.  These kernels read the snapshot blocks and write only their own output block.
#pragma once
#include "search_batch_kernels.h"

namespace azmi {

// (the columns of a row: SweepCol, kSweepCols, kPolicyCols in search_batch_types.h)
constexpr uint32_t kSwNone = 0xFFFFFFFFu;

__device__ __forceinline__ double sw_nan() { return __longlong_as_double(0x7FF8000000000000LL); }

template <int L>
__device__ __forceinline__ double sw_fold(double x) {
  for (int off = L / 2; off > 0; off >>= 1) x += __shfl_xor(x, off, L);
  return x;
}

// top[r] = the index of the r-th largest (value, index) key of x[0 .. M), kSwNone from r = M on; the same on every lane
template <int L>
__device__ __forceinline__ void sw_top9(uint32_t lane, uint32_t M, const float* x, uint32_t (&top)[9]) {
  float last_v = 0.0f;
  uint32_t last_i = kSwNone;
#pragma unroll
  for (int r = 0; r < 9; ++r) {
    float best_v = 0.0f;
    uint32_t best_i = kSwNone;
    for (uint32_t m = lane; m < M; m += L) {
      const float v = x[m];
      if (last_i != kSwNone && !(v < last_v || (v == last_v && m < last_i))) continue;      // an earlier round's winner
      if (best_i == kSwNone || v > best_v || (v == best_v && m > best_i)) { best_v = v; best_i = m; }
    }
    for (int off = L / 2; off > 0; off >>= 1) {
      const float ov = __shfl_xor(best_v, off, L);
      const uint32_t oi = __shfl_xor(best_i, off, L);
      if (oi != kSwNone && (best_i == kSwNone || ov > best_v || (ov == best_v && oi > best_i))) { best_v = ov; best_i = oi; }
    }
    top[r] = best_i;
    if (best_i != kSwNone) { last_v = best_v; last_i = best_i; }
  }
}

// |top_k(p) & top_k(q)| for the nested k = 1, 3, 9 (an index occurs once in a list, so matching pairs count the intersection)
__device__ __forceinline__ uint32_t sw_common(const uint32_t (&a)[9], const uint32_t (&b)[9], int k) {
  uint32_t c = 0;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
#pragma unroll
    for (int j = 0; j < 9; ++j) {
      if (i < k && j < k && a[i] != kSwNone && a[i] == b[j]) ++c;
    }
  }
  return c;
}

// policy_metrics.py, expression for expression, of one pair of rows by its L lanes; every lane returns the same out[0 .. 6):
//   jsd        m = 0.5 (p + q);  0.5 sum over p > 0 of p ln(p / m)  +  0.5 sum over q > 0 of q ln(q / m)
//   tv         0.5 sum |p - q|
//   hellinger  sqrt(0.5 sum (sqrt p - sqrt q)^2)
//   top1 / top3 / top9   |top_k(p) & top_k(q)| / k
template <int L>
__device__ __forceinline__ void sw_policy_row(uint32_t lane, uint32_t M, const float* p, const float* q, double (&out)[kPolicyCols]) {
  double sp = 0.0, sq = 0.0, tv = 0.0, h = 0.0;
  for (uint32_t m = lane; m < M; m += L) {
    const double pm = static_cast<double>(p[m]), qm = static_cast<double>(q[m]);
    const double mid = 0.5 * (pm + qm);
    if (pm > 0.0) sp += pm * log(pm / mid);
    if (qm > 0.0) sq += qm * log(qm / mid);
    tv += fabs(pm - qm);
    const double d = sqrt(pm) - sqrt(qm);
    h += d * d;
  }
  sp = sw_fold<L>(sp); sq = sw_fold<L>(sq); tv = sw_fold<L>(tv); h = sw_fold<L>(h);
  uint32_t tp[9], tq[9];
  sw_top9<L>(lane, M, p, tp);
  sw_top9<L>(lane, M, q, tq);
  out[kSwJsd] = 0.5 * sp + 0.5 * sq;
  out[kSwTv] = 0.5 * tv;
  out[kSwHellinger] = sqrt(0.5 * h);
  out[kSwTop1] = static_cast<double>(sw_common(tp, tq, 1));
  out[kSwTop3] = static_cast<double>(sw_common(tp, tq, 3)) / 3.0;
  out[kSwTop9] = static_cast<double>(sw_common(tp, tq, 9)) / 9.0;
}

// sum x[m] * y[m]: the expected reward of policy x under the Q values y (mcts_analysis.py:1213)
template <int L>
__device__ __forceinline__ double sw_dot(uint32_t lane, uint32_t M, const float* x, const float* y) {
  double s = 0.0;
  for (uint32_t m = lane; m < M; m += L) s += static_cast<double>(x[m]) * static_cast<double>(y[m]);
  return sw_fold<L>(s);
}

// kl_divergence(x, y): sum over x > 0 of x ln(x / (y + 1e-10))
template <int L>
__device__ __forceinline__ double sw_kl(uint32_t lane, uint32_t M, const float* x, const float* y) {
  double s = 0.0;
  for (uint32_t m = lane; m < M; m += L) {
    const double xm = static_cast<double>(x[m]);
    if (xm > 0.0) s += xm * log(xm / (static_cast<double>(y[m]) + 1e-10));
  }
  return sw_fold<L>(s);
}

// policy_entropy(x): -sum over x > 0 of x ln x
template <int L>
__device__ __forceinline__ double sw_entropy(uint32_t lane, uint32_t M, const float* x) {
  double s = 0.0;
  for (uint32_t m = lane; m < M; m += L) {
    const double xm = static_cast<double>(x[m]);
    if (xm > 0.0) s += xm * log(xm);
  }
  return -sw_fold<L>(s);
}

// ======================= the rows of one tree ===========================================================================================
//   sw        the swept batch's snapshot set, rf the reference batch's (the same block when the sweep is scored against itself)
//   anchor    checkpoint of rf: p = rf.probs[i, anchor], the Q values rf.root_q[i, anchor], v_a = rf.root_values[i, anchor, 0]
//   raw       checkpoint of rf holding the one-visit policy r, or < 0
//   outcomes  [N] game outcomes, or null
//   rows      [N, J, kSweepCols]; ceiling [N]; valid [N, J]
// Row (i, j) is valid when snapshot j of tree i and the anchor snapshot of tree i were both taken; an invalid row is NaN in every
// column.  pressure, benefit, closer_than_raw and the tree's ceiling need the raw snapshot and are NaN without it; abs_err and
// the two closer_than flags need the outcome.  The flags are 1.0 / 0.0.
template <int L>
__device__ __forceinline__ void sw_score_tree(uint32_t lane, uint32_t M, uint32_t i, const SbSweepArrays& sw, const SbSweepArrays& rf, uint32_t anchor,
                                              int32_t raw, const double* outcomes, double* rows, double* ceiling, uint8_t* valid) {
  const double nan = sw_nan();
  const uint32_t J = sw.n_cp, Jr = rf.n_cp;
  const uint32_t taken = sw.taken[i], taken_ref = rf.taken[i];
  const bool a_ok = ((taken_ref >> anchor) & 1u) != 0u;
  const bool r_ok = a_ok && raw >= 0 && ((taken_ref >> static_cast<uint32_t>(raw)) & 1u) != 0u;
  const size_t row_a = static_cast<size_t>(i) * Jr + anchor;
  const size_t row_r = static_cast<size_t>(i) * Jr + (r_ok ? static_cast<uint32_t>(raw) : anchor);
  const float* p = rf.probs + row_a * M;
  const float* qv = rf.root_q + row_a * M;
  const float* r = rf.probs + row_r * M;
  const bool have_o = outcomes != nullptr;
  const double o = have_o ? outcomes[i] : nan;
  double reward_a = nan, reward_r = nan, v_a = nan, v_r = nan, ceil_i = nan;
  if (a_ok) { reward_a = sw_dot<L>(lane, M, p, qv); v_a = static_cast<double>(rf.root_values[row_a * 3]); }
  if (r_ok) {
    reward_r = sw_dot<L>(lane, M, r, qv);
    v_r = static_cast<double>(rf.root_values[row_r * 3]);
    ceil_i = sw_kl<L>(lane, M, p, r);
  }
  if (lane == 0) ceiling[i] = ceil_i;
  for (uint32_t j = 0; j < J; ++j) {
    const size_t row = static_cast<size_t>(i) * J + j;
    double* out = rows + row * kSweepCols;
    const bool ok = a_ok && ((taken >> j) & 1u) != 0u;
    if (lane == 0) valid[row] = ok ? 1 : 0;
    if (!ok) {
      for (uint32_t c = lane; c < kSweepCols; c += L) out[c] = nan;
      continue;
    }
    const float* q = sw.probs + row * M;
    double six[kPolicyCols];
    sw_policy_row<L>(lane, M, p, q, six);
    const double reward = sw_dot<L>(lane, M, q, qv);
    const double entropy = sw_entropy<L>(lane, M, q);
    const double pressure = r_ok ? sw_kl<L>(lane, M, q, r) : nan;
    if (lane != 0) continue;
    const double v_j = static_cast<double>(sw.root_values[row * 3]);
#pragma unroll
    for (uint32_t c = 0; c < kPolicyCols; ++c) out[c] = six[c];
    out[kSwReward] = reward;
    out[kSwRegret] = reward_a - reward;
    out[kSwPressure] = pressure;
    out[kSwBenefit] = r_ok ? reward - reward_r : nan;
    out[kSwEntropy] = entropy;
    out[kSwValueGap] = fabs(v_j - v_a);
    const double err = fabs(v_j - o);
    out[kSwAbsErr] = have_o ? err : nan;
    out[kSwCloserAnchor] = have_o ? (err < fabs(v_a - o) ? 1.0 : 0.0) : nan;
    out[kSwCloserRaw] = have_o && r_ok ? (err < fabs(v_r - o) ? 1.0 : 0.0) : nan;
  }
}

template <class GM>
__global__ __launch_bounds__(256) void k_sb_sweep_metrics(SbSweepArrays sw, SbSweepArrays rf, uint32_t n, uint32_t anchor, int32_t raw,
                                                          const double* outcomes, double* rows, double* ceiling, uint8_t* valid) {
  constexpr int G = GM::GROUP;
  static_assert(G == 8, "lane-group shuffles of width 8");
  const uint32_t gtid = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t slot = gtid / G, lane = gtid % G;
  if (slot >= n) return;
  sw_score_tree<G>(lane, GM::M, slot, sw, rf, anchor, raw, outcomes, rows, ceiling, valid);
}

template <class GM>
__global__ __launch_bounds__(64) void k_sb_big_sweep_metrics(SbSweepArrays sw, SbSweepArrays rf, uint32_t n, uint32_t anchor, int32_t raw,
                                                             const double* outcomes, double* rows, double* ceiling, uint8_t* valid) {
  const uint32_t slot = blockIdx.x, lane = threadIdx.x;
  if (slot >= n) return;
  sw_score_tree<64>(lane, GM::M, slot, sw, rf, anchor, raw, outcomes, rows, ceiling, valid);
}

// ======================= the means of a checkpoint ======================================================================================
// One workgroup per checkpoint j; for every column, mean[j, c] over the trees whose row (i, j) is not NaN there and count[j, c]
// of them (NaN mean for a count of 0).  Lane t adds trees t, t + 256, ... in ascending order, then a fixed-shape LDS tree folds
// the 256 partial sums (kSweepMeanThreads): the result depends on n alone, never on scheduling.  No floating-point atomics.
__global__ __launch_bounds__(256) void k_sb_sweep_mean(const double* rows, uint32_t n, uint32_t J, double* mean, uint32_t* count) {
  __shared__ double s_sum[kSweepMeanThreads];
  __shared__ uint32_t s_cnt[kSweepMeanThreads];
  const uint32_t j = blockIdx.x, t = threadIdx.x;
  if (j >= J) return;
  for (uint32_t c = 0; c < kSweepCols; ++c) {
    double sum = 0.0;
    uint32_t cnt = 0;
    for (uint32_t i = t; i < n; i += kSweepMeanThreads) {
      const double x = rows[(static_cast<size_t>(i) * J + j) * kSweepCols + c];
      if (x == x) { sum += x; ++cnt; }
    }
    s_sum[t] = sum; s_cnt[t] = cnt;
    __syncthreads();
    for (uint32_t w = kSweepMeanThreads / 2; w > 0; w >>= 1) {
      if (t < w) { s_sum[t] += s_sum[t + w]; s_cnt[t] += s_cnt[t + w]; }
      __syncthreads();
    }
    if (t == 0) {
      mean[j * kSweepCols + c] = s_cnt[0] ? s_sum[0] / static_cast<double>(s_cnt[0]) : sw_nan();
      count[j * kSweepCols + c] = s_cnt[0];
    }
    __syncthreads();
  }
}

// ======================= any [rows, M] pair of policies =================================================================================
// out[row, 0 .. 6) = sw_policy_row of (p[row], q[row]): L = 8 lanes a row for M <= 8, one wavefront a row above
template <int L>
__global__ __launch_bounds__(256) void k_policy_divergences(const float* p, const float* q, uint32_t rows, uint32_t M, double* out) {
  const size_t gtid = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  const size_t row = gtid / L;
  const uint32_t lane = static_cast<uint32_t>(gtid % L);
  if (row >= rows) return;
  double six[kPolicyCols];
  sw_policy_row<L>(lane, M, p + row * M, q + row * M, six);
  if (lane != 0) return;
#pragma unroll
  for (uint32_t c = 0; c < kPolicyCols; ++c) out[row * kPolicyCols + c] = six[c];
}

}  // namespace azmi
