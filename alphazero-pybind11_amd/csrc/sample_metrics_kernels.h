// Per-row policy and value diagnostics of a net against the samples, and their bucketed sums, on the device: the held-out metric
// set of network_pareto.eval_loss (network_pareto.py:652-738) and the per-sample arrays of _analyze_iteration_variants
// (game_runner.py:2509-2627), one read of every row where the reference makes a dozen torch passes over [B, M].
//
// Conventions of samples_kernels.h: float64 arithmetic on the float32 inputs, one row per lane group, every floating-point sum in
// an order fixed by the problem size alone, no floating-point atomics, no kernel that waits for another workgroup.  `p` holds
// PROBABILITIES (what the leaf net writes), where the reference holds log-probabilities.
//
// Tie rule of every argmax and top-3 in this file: the LOWER index wins (np.argmax; the first three of a stable argsort of -x;
// what pib.max(dim=1) gives on the reference's CPU path - real targets are full of tied zeros).  policy_divergences and
// sweep_metrics resolve ties towards the HIGHER index, as policy_metrics.py does; the two rules are not interchangeable.
#pragma once
#include "samples_kernels.h"

namespace azmi {

// the float64 columns k_sample_metrics writes, column-contiguous ([kSampleMetricColumns][n]); alphazero.samples.Metric mirrors it
enum SampleMetric : uint32_t {
  kSmPiLoss = 0,          // -sum over t > 0 of t * log(max(p, FLT_MIN)): k_sample_loss at scale 1, bit for bit
  kSmVLoss = 1,           // the same on the value rows at scale cv: k_sample_loss at scale cv, bit for bit
  kSmTargetEntropy = 2,   // -sum over t > 0 of t * log(t)                          (network_pareto.py:716)
  kSmEntropy = 3,         // -sum over all m of t * log(t + 1e-9)                   (game_runner.py:2562)
  kSmKl = 4,              // sum over t > 0 of t * log(t / (p + 1e-10))             (network_pareto.py:713)
  kSmTop1 = 5,            // max_m t
  kSmNetTop1 = 6,         // max_m p
  kSmNetAtMcts = 7,       // p[argmax t]
  kSmTop1Gap = 8,         // top1 - net_at_mcts
  kSmTop1Agree = 9,       // 1.0 when argmax p == argmax t, else 0.0
  kSmTop3Overlap = 10,    // |top3(p) & top3(t)|, 0..3 (M < 3: the sets have M members)
  kSmVPred = 11,          // p_v[i, 0]
  kSmVActual = 12,        // target_v[i, 0]
};
constexpr uint32_t kSampleMetricColumns = 13;
constexpr uint32_t kSampleMetricChecked = 5;      // the columns 0..4 (the sums) are the ones the reduction checks for NaN / inf
constexpr uint32_t kMetricMaxBuckets = 8;
constexpr uint32_t kMetricThreads = kLossThreads;

// ---- k_sample_metrics -------------------------------------------------------------------------------------------------------
// The three largest entries of a row under the order "larger value first, lower index first among equals".  A NaN sorts as -inf
// (its index stays valid: the index columns of such a row are unspecified but in range); an empty place is (-inf, kTopNone) and
// sorts behind every real entry.
constexpr uint32_t kTopNone = 0xFFFFFFFFu;

struct Top3 {
  float v[3];
  uint32_t i[3];
};

__device__ __forceinline__ bool top_before(float va, uint32_t ia, float vb, uint32_t ib) { return va > vb || (va == vb && ia < ib); }

__device__ __forceinline__ void top3_clear(Top3& a) {
  for (int k = 0; k < 3; ++k) { a.v[k] = -INFINITY; a.i[k] = kTopNone; }
}

// -> true when (v, i) became the first entry
__device__ __forceinline__ bool top3_insert(Top3& a, float v, uint32_t i) {
  if (top_before(v, i, a.v[0], a.i[0])) {
    a.v[2] = a.v[1]; a.i[2] = a.i[1];
    a.v[1] = a.v[0]; a.i[1] = a.i[0];
    a.v[0] = v; a.i[0] = i;
    return true;
  }
  if (top_before(v, i, a.v[1], a.i[1])) {
    a.v[2] = a.v[1]; a.i[2] = a.i[1];
    a.v[1] = v; a.i[1] = i;
  } else if (top_before(v, i, a.v[2], a.i[2])) {
    a.v[2] = v; a.i[2] = i;
  }
  return false;
}

// one butterfly step: the lane's three merged with those of lane ^ off (inside groups of `width` lanes); `carry` travels with the
// first entry.  The order is total over distinct indices, so both partners end with the same three.
__device__ __forceinline__ void top3_merge(Top3& a, float& carry, int off, int width) {
  Top3 b;
  for (int k = 0; k < 3; ++k) { b.v[k] = __shfl_xor(a.v[k], off, width); b.i[k] = __shfl_xor(a.i[k], off, width); }
  const float other = __shfl_xor(carry, off, width);
  if (top3_insert(a, b.v[0], b.i[0])) carry = other;
  top3_insert(a, b.v[1], b.i[1]);
  top3_insert(a, b.v[2], b.i[2]);
}

__device__ __forceinline__ double smp_fold_w(double x, int width) {      // smp_fold<width> with the width at run time: the same adds
  for (int off = width / 2; off > 0; off >>= 1) x += __shfl_xor(x, off, width);
  return x;
}

__device__ __forceinline__ double smp_nan() { return __longlong_as_double(0x7FF8000000000000LL); }

// One row per group of G lanes, G = the larger of the lane groups k_sample_loss gives M and V (lm, lv: 8, 16, 32 or 64).  The
// policy row is read by the first lm lanes of the group exactly as k_sample_loss<lm> reads it (lane l takes m = l, l + lm, ... in
// ascending order, the partial sums fold by an xor butterfly of width lm), the value row by the first lv lanes likewise: a row's
// bits depend on (M, V) only, and pi_loss / v_loss are k_sample_loss's.  Every input element is read once; the top-3 sets and the
// probability at the target's argmax travel through the same butterfly.
// Special values: a negative target makes the sums of its row NaN (policy: pi_loss, target_entropy, entropy, kl; value: v_loss);
// a NaN probability makes pi_loss and kl NaN where its target is positive, net_top1 NaN (the maximum of a row with a NaN is NaN,
// as np.max), net_at_mcts and top1_gap NaN where it sits at the target's argmax; a NaN target makes top1 NaN as well.
template <int G>
__global__ void __launch_bounds__(kMetricThreads) k_sample_metrics(const float* __restrict__ target_pi, const float* __restrict__ p_pi,
                                                                   const float* __restrict__ target_v, const float* __restrict__ p_v,
                                                                   uint32_t n, uint32_t M, uint32_t V, int lm, int lv, double cv,
                                                                   double* __restrict__ cols, uint64_t col_stride,
                                                                   uint32_t* __restrict__ mcts_argmax, uint32_t* __restrict__ net_argmax) {
  constexpr uint32_t kRows = kMetricThreads / G;
  const uint64_t row = uint64_t(blockIdx.x) * kRows + threadIdx.x / G;
  const uint32_t lane = threadIdx.x % G;
  if (row >= n) return;      // (whole groups leave: G divides the wavefront, the shuffles below stay inside a group)

  double s_pi = 0.0, s_te = 0.0, s_en = 0.0, s_kl = 0.0;
  Top3 tt, tp;
  top3_clear(tt);
  top3_clear(tp);
  float p_at = 0.0f;      // p at the lane's best target
  bool t_nan = false, p_nan = false;
  if (lane < static_cast<uint32_t>(lm)) {
    const float* t = target_pi + row * M;
    const float* q = p_pi + row * M;
    for (uint32_t m = lane; m < M; m += lm) {
      const float tf = t[m], pf = q[m];
      const double tm = static_cast<double>(tf), pm = static_cast<double>(pf);
      if (tm > 0.0) {
        s_pi += tm * log(pm < static_cast<double>(FLT_MIN) ? static_cast<double>(FLT_MIN) : pm);
        s_te += tm * log(tm);
        s_kl += tm * log(tm / (pm + 1e-10));
        s_en += tm * log(tm + 1e-9);      // (a zero target's term is 0 * log(1e-9) = -0.0, and x + -0.0 is x: left out, the same bits)
      } else if (tm < 0.0) {
        s_pi += smp_nan();
        s_te += smp_nan();
        s_en += smp_nan();
        s_kl += smp_nan();
      } else if (tm != tm) {
        s_en += smp_nan();                // (the one sum that runs over all m; the others skip a NaN target as k_sample_loss does)
      }
      t_nan |= tf != tf;
      p_nan |= pf != pf;
      // m ascends, so an entry equal to the lane's third never displaces it: most entries leave after one comparison
      const float tk = tf != tf ? -INFINITY : tf, pk = pf != pf ? -INFINITY : pf;
      if (tk > tt.v[2] || tt.i[2] == kTopNone) {
        if (top3_insert(tt, tk, m)) p_at = pf;
      }
      if (pk > tp.v[2] || tp.i[2] == kTopNone) top3_insert(tp, pk, m);
    }
  }
  s_pi = smp_fold_w(s_pi, lm);
  s_te = smp_fold_w(s_te, lm);
  s_en = smp_fold_w(s_en, lm);
  s_kl = smp_fold_w(s_kl, lm);
  float unused = 0.0f;
  uint32_t nan_bits = (t_nan ? 1u : 0u) | (p_nan ? 2u : 0u);
  for (int off = lm / 2; off > 0; off >>= 1) {
    top3_merge(tt, p_at, off, lm);
    top3_merge(tp, unused, off, lm);
    nan_bits |= __shfl_xor(nan_bits, off, lm);
  }

  double s_v = 0.0;
  float v_pred = 0.0f, v_actual = 0.0f;
  if (lane < static_cast<uint32_t>(lv)) {
    const float* t = target_v + row * V;
    const float* q = p_v + row * V;
    for (uint32_t k = lane; k < V; k += lv) {
      const float tf = t[k], pf = q[k];
      const double tm = static_cast<double>(tf);
      if (tm > 0.0) {
        const double pm = static_cast<double>(pf);
        s_v += tm * log(pm < static_cast<double>(FLT_MIN) ? static_cast<double>(FLT_MIN) : pm);
      } else if (tm < 0.0) {
        s_v += smp_nan();
      }
      if (k == 0) { v_pred = pf; v_actual = tf; }
    }
  }
  s_v = smp_fold_w(s_v, lv);

  if (lane != 0) return;
  uint32_t overlap = 0;
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) overlap += (tt.i[a] != kTopNone && tt.i[a] == tp.i[b]) ? 1u : 0u;
  const double top1 = (nan_bits & 1u) ? smp_nan() : static_cast<double>(tt.v[0]);
  const double net_top1 = (nan_bits & 2u) ? smp_nan() : static_cast<double>(tp.v[0]);
  const double at = static_cast<double>(p_at);
  double* c = cols + row;
  c[kSmPiLoss * col_stride] = 0.0 - 1.0 * s_pi;      // (0 - x: an all-zero row is +0.0, as in k_sample_loss)
  c[kSmVLoss * col_stride] = 0.0 - cv * s_v;
  c[kSmTargetEntropy * col_stride] = 0.0 - s_te;
  c[kSmEntropy * col_stride] = 0.0 - s_en;
  c[kSmKl * col_stride] = s_kl;
  c[kSmTop1 * col_stride] = top1;
  c[kSmNetTop1 * col_stride] = net_top1;
  c[kSmNetAtMcts * col_stride] = at;
  c[kSmTop1Gap * col_stride] = top1 - at;
  c[kSmTop1Agree * col_stride] = tt.i[0] == tp.i[0] ? 1.0 : 0.0;
  c[kSmTop3Overlap * col_stride] = static_cast<double>(overlap);
  c[kSmVPred * col_stride] = static_cast<double>(v_pred);
  c[kSmVActual * col_stride] = static_cast<double>(v_actual);
  mcts_argmax[row] = tt.i[0];      // (M >= 1: lane 0 holds entry 0, so the first place is never empty)
  net_argmax[row] = tp.i[0];
}

// ---- k_sample_plane_argmax --------------------------------------------------------------------------------------------------
// out[i] = the lower-index argmax over the P planes first .. first + P - 1 of canonical [n, C, H, W] at one cell: the variant id
// of the unified StarGambit encoding (c[:, 32:36, 6, 6].argmax(1), game_runner.py:2535).  One thread per row.
__global__ void __launch_bounds__(kMetricThreads) k_sample_plane_argmax(const float* __restrict__ canonical, uint32_t n, uint64_t row_elems,
                                                                        uint64_t plane_elems, uint64_t first_offset, uint32_t P,
                                                                        uint8_t* __restrict__ out) {
  const uint64_t i = uint64_t(blockIdx.x) * kMetricThreads + threadIdx.x;
  if (i >= n) return;
  const float* x = canonical + i * row_elems + first_offset;
  float best = x[0];
  uint32_t at = 0;
  for (uint32_t k = 1; k < P; ++k) {
    const float v = x[k * plane_elems];
    if (v > best) { best = v; at = k; }
  }
  out[i] = static_cast<uint8_t>(at);
}

// ---- the bucketed reduction -------------------------------------------------------------------------------------------------
// sum[b][c] = the float64 sum of column c over the rows of bucket b, through the tile tree of k_plan_sum: tiles of kPlanBlock, one
// workgroup per tile (blockIdx.x) and per (bucket, column) pair (blockIdx.y = b * kSampleMetricColumns + c), one launch per level.
// A row outside the bucket enters as +0.0, so the bits of a sum depend on n and on which rows belong, on nothing else.  With a
// bucket array there is one more pseudo-bucket, b == n_buckets: every row ("overall"), whose sums go to total[].
struct SampleMetricsRecord {      // azmi_sample_metrics_record
  double sum[kMetricMaxBuckets][kSampleMetricColumns];
  double total[kSampleMetricColumns];
  uint32_t count[kMetricMaxBuckets];
  uint32_t nonfinite;            // rows with a NaN or +-inf in one of the first kSampleMetricChecked columns
  uint32_t first_nonfinite;      // the smallest such row, kPlanNone for none
  uint32_t invalid;              // rows whose bucket id is >= n_buckets: they belong to no bucket
  uint32_t reserved;
};

// where the top of the tree puts pair `bc`: the record's sum[b][c], the pseudo-bucket in total[c]
__device__ __forceinline__ double* metrics_slot(SampleMetricsRecord* rec, uint32_t bc, uint32_t n_buckets, bool has_all) {
  const uint32_t b = bc / kSampleMetricColumns, c = bc % kSampleMetricColumns;
  return has_all && b == n_buckets ? &rec->total[c] : &rec->sum[b][c];
}

// level 0, on the columns themselves.  bucket == nullptr: one bucket, every row.  The workgroups of column 0 count their bucket's
// rows; those of pair 0 also check every row of the tile (non-finite sums, invalid bucket ids), by integer atomics on the record.
__global__ void __launch_bounds__(kPlanBlock) k_metrics_sum(const double* __restrict__ cols, uint64_t col_stride, uint32_t n,
                                                            const uint8_t* __restrict__ bucket, uint32_t n_buckets, double* __restrict__ out,
                                                            SampleMetricsRecord* __restrict__ rec) {
  const uint32_t i = blockIdx.x * kPlanBlock + threadIdx.x;
  const uint32_t bc = blockIdx.y, b = bc / kSampleMetricColumns, c = bc % kSampleMetricColumns;
  const bool has_all = bucket != nullptr;
  const uint32_t id = i < n ? (bucket ? bucket[i] : 0u) : kPlanNone;
  const bool mine = i < n && (id == b || (has_all && b == n_buckets));
  const double x = mine ? cols[c * col_stride + i] : 0.0;
  if (bc == 0 && i < n) {
    bool bad = false;
    for (uint32_t k = 0; k < kSampleMetricChecked; ++k) bad |= !isfinite(cols[k * col_stride + i]);
    if (bad) {
      atomicAdd(&rec->nonfinite, 1u);
      atomicMin(&rec->first_nonfinite, i);
    }
    if (id >= n_buckets) atomicAdd(&rec->invalid, 1u);
  }
  if (c == 0 && b < n_buckets) {      // (uniform over the workgroup)
    const uint32_t rows = __syncthreads_count(mine);
    if (threadIdx.x == 0 && rows) atomicAdd(&rec->count[b], rows);
  }
  const double s = plan_block_sum(x);
  if (threadIdx.x == 0) {
    if (gridDim.x == 1) *metrics_slot(rec, bc, n_buckets, has_all) = s;
    else out[uint64_t(bc) * gridDim.x + blockIdx.x] = s;
  }
}

// the levels above: out[bc][tile] = the sum of in[bc][tile * kPlanBlock ...) (elements past n_in count as +0.0)
__global__ void __launch_bounds__(kPlanBlock) k_metrics_sum_up(const double* __restrict__ in, uint32_t n_in, uint32_t n_buckets, bool has_all,
                                                               double* __restrict__ out, SampleMetricsRecord* __restrict__ rec) {
  const uint32_t i = blockIdx.x * kPlanBlock + threadIdx.x;
  const uint32_t bc = blockIdx.y;
  const double x = i < n_in ? in[uint64_t(bc) * n_in + i] : 0.0;
  const double s = plan_block_sum(x);
  if (threadIdx.x == 0) {
    if (gridDim.x == 1) *metrics_slot(rec, bc, n_buckets, has_all) = s;
    else out[uint64_t(bc) * gridDim.x + blockIdx.x] = s;
  }
}

}  // namespace azmi
