// The participation ratio of a feature matrix on the device: NNWrapper.effective_rank (neural_net.py:826-873) behind the pooled
// trunk features of the fp32 leaf net (azmi_net_trunk_features).  With Fc the column-centred [n][C] features and G = Fc^T Fc,
// sum s^2 = tr G and sum s^4 = |G|_F^2 for the singular values s of Fc, so the reference's figure (sum s^2)^2 / sum s^4 is
// (tr G)^2 / |G|_F^2: no singular values are computed.
//
// Arithmetic: float64 on the float32 features (the reference: a float32 SVD).  Two passes over the features: the
// column means first, then the products of the centred values; S2 - S1 S1^T / n cancels when a column's mean is large against its
// spread.  Every product is one fma into its accumulator.
//
// Determinism: every sum has an order fixed by (n, C) alone (rank_plan below).  A column's sum and an entry of G are added row by
// row inside a slab of rows by ONE thread, the slabs in ascending order by one thread, the trace and the norm by a butterfly
// inside a workgroup and the workgroups' sums in ascending order.  No floating-point atomics, and no kernel waits for another
// workgroup: every level is a launch of its own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace azmi {

constexpr uint32_t kRankTile = 64;            // a workgroup owns a 64 x 64 tile of G (a wavefront 32 x 32, a lane 4 x 4)
constexpr uint32_t kRankRows = 32;            // rows of the features staged in LDS per step
constexpr uint32_t kRankThreads = 256;
constexpr uint32_t kRankLd = kRankTile + 2;   // LDS row of doubles: 16-byte aligned, off the power of two
constexpr uint32_t kRankTileCells = kRankTile * kRankTile;
constexpr uint32_t kRankMaxChannels = 2048;
constexpr uint32_t kRankMaxSlabs = 256;       // row slabs of the Gram pass (grid.y)
constexpr uint32_t kRankWantGroups = 1024;    // workgroups the Gram pass aims at: four a CU
constexpr uint32_t kRankSumRows = 128;        // the column sums: a slab holds at least this many rows ...
constexpr uint32_t kRankMaxSumSlabs = 256;    // ... and there are at most this many slabs

struct FeatureRankRecord {      // azmi_feature_rank_record
  double trace, frob2, rank;
  uint32_t n, channels;
};

// how (n, C) is cut: tiles of kRankTile columns, the pairs (ti <= tj) of them, slabs of rows for the Gram pass (a multiple of
// kRankRows each) and for the column sums.  A function of (n, C) alone: two calls add in the same order.
struct RankPlan {
  uint32_t tiles, pairs, slabs, slab_rows, sum_slabs, sum_slab_rows;
};
inline RankPlan rank_plan(uint32_t n, uint32_t C) {
  RankPlan p;
  p.tiles = (C + kRankTile - 1) / kRankTile;
  p.pairs = p.tiles * (p.tiles + 1) / 2;
  uint32_t want = (kRankWantGroups + p.pairs - 1) / p.pairs;
  want = want > kRankMaxSlabs ? kRankMaxSlabs : want;
  const uint64_t per = (uint64_t(n) + want - 1) / want;
  p.slab_rows = static_cast<uint32_t>((per + kRankRows - 1) / kRankRows * kRankRows);
  p.slabs = static_cast<uint32_t>((uint64_t(n) + p.slab_rows - 1) / p.slab_rows);
  uint32_t sw = (n + kRankSumRows - 1) / kRankSumRows;
  sw = sw > kRankMaxSumSlabs ? kRankMaxSumSlabs : sw;
  p.sum_slab_rows = (n + sw - 1) / sw;
  p.sum_slabs = (n + p.sum_slab_rows - 1) / p.sum_slab_rows;
  return p;
}

// pair index -> (ti, tj), ti <= tj: row ti of the upper triangle holds tiles - ti pairs
__device__ __forceinline__ void rank_pair(uint32_t pair, uint32_t tiles, uint32_t& ti, uint32_t& tj) {
  ti = 0;
  while (pair >= tiles - ti) { pair -= tiles - ti; ++ti; }
  tj = ti + pair;
}

__device__ __forceinline__ double rank_fold64(double x) {
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
  return x;
}

// part[slab][c] = the float64 sum of column c over the rows of the slab, in ascending row order.  One wavefront per (64 columns,
// slab): lane = column, so a row's 64 floats are one 256-byte read.
__global__ void __launch_bounds__(64) k_rank_colsum(const float* __restrict__ f, uint32_t n, uint32_t C, uint32_t slab_rows,
                                                    double* __restrict__ part) {
  const uint32_t c = blockIdx.x * 64 + threadIdx.x;
  if (c >= C) return;
  const uint64_t lo = uint64_t(blockIdx.y) * slab_rows;
  const uint64_t hi = lo + slab_rows < n ? lo + slab_rows : n;
  double s = 0.0;
#pragma unroll 4
  for (uint64_t r = lo; r < hi; ++r) s += static_cast<double>(f[r * C + c]);
  part[uint64_t(blockIdx.y) * C + c] = s;
}

// mean[c] = (the slab sums in ascending order) / n; mean_out (may be NULL) receives a copy
__global__ void __launch_bounds__(kRankThreads) k_rank_mean(const double* __restrict__ part, uint32_t slabs, uint32_t C, uint32_t n,
                                                            double* __restrict__ mean, double* __restrict__ mean_out) {
  const uint32_t c = blockIdx.x * kRankThreads + threadIdx.x;
  if (c >= C) return;
  double s = 0.0;
  for (uint32_t k = 0; k < slabs; ++k) s += part[uint64_t(k) * C + c];
  s /= static_cast<double>(n);
  mean[c] = s;
  if (mean_out) mean_out[c] = s;
}

// part[slab][pair][x][y] = sum over the rows r of the slab, ascending, of (f[r][64 ti + x] - mean) * (f[r][64 tj + y] - mean).
// A step stages kRankRows rows of the two column tiles in LDS, centred, as float64 (one tile for a pair on the diagonal); a lane
// then reads 4 + 4 values per row for its 16 fmas.  Columns past C and rows past the slab enter as 0.0 and add nothing.
__global__ void __launch_bounds__(kRankThreads) k_rank_gram(const float* __restrict__ f, uint32_t n, uint32_t C, const double* __restrict__ mean,
                                                            uint32_t tiles, uint32_t slab_rows, double* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) double sa[kRankRows][kRankLd];
  __shared__ __attribute__((aligned(16))) double sb[kRankRows][kRankLd];
  uint32_t ti, tj;
  rank_pair(blockIdx.x, tiles, ti, tj);
  const bool diag = ti == tj;      // (the same in every thread of the workgroup)
  const uint32_t lc = threadIdx.x % kRankTile, lr = threadIdx.x / kRankTile;      // the loader's column and first row: 4 rows a pass
  const uint32_t ca = ti * kRankTile + lc, cb = tj * kRankTile + lc;
  const double ma = ca < C ? mean[ca] : 0.0, mb = cb < C ? mean[cb] : 0.0;
  const uint32_t wave = threadIdx.x / 64, lane = threadIdx.x % 64;
  const uint32_t x0 = (wave / 2) * 32 + (lane / 8) * 4, y0 = (wave % 2) * 32 + (lane % 8) * 4;
  double acc[4][4];
#pragma unroll
  for (int x = 0; x < 4; ++x)
#pragma unroll
    for (int y = 0; y < 4; ++y) acc[x][y] = 0.0;
  const uint64_t lo = uint64_t(blockIdx.y) * slab_rows;
  const uint64_t hi = lo + slab_rows < n ? lo + slab_rows : n;
  for (uint64_t r0 = lo; r0 < hi; r0 += kRankRows) {
#pragma unroll
    for (uint32_t k = 0; k < kRankRows / 4; ++k) {
      const uint32_t row = lr + 4 * k;
      const uint64_t r = r0 + row;
      sa[row][lc] = (r < hi && ca < C) ? static_cast<double>(f[r * C + ca]) - ma : 0.0;
      if (!diag) sb[row][lc] = (r < hi && cb < C) ? static_cast<double>(f[r * C + cb]) - mb : 0.0;
    }
    __syncthreads();
    const double (*pb)[kRankLd] = diag ? sa : sb;
#pragma unroll 4
    for (uint32_t row = 0; row < kRankRows; ++row) {
      const double2 a01 = *reinterpret_cast<const double2*>(&sa[row][x0]), a23 = *reinterpret_cast<const double2*>(&sa[row][x0 + 2]);
      const double2 b01 = *reinterpret_cast<const double2*>(&pb[row][y0]), b23 = *reinterpret_cast<const double2*>(&pb[row][y0 + 2]);
      const double a[4] = {a01.x, a01.y, a23.x, a23.y}, b[4] = {b01.x, b01.y, b23.x, b23.y};
#pragma unroll
      for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < 4; ++y) acc[x][y] = fma(a[x], b[y], acc[x][y]);
    }
    __syncthreads();
  }
  double* out = part + (uint64_t(blockIdx.y) * gridDim.x + blockIdx.x) * kRankTileCells;
#pragma unroll
  for (int x = 0; x < 4; ++x) {
    *reinterpret_cast<double2*>(&out[(x0 + x) * kRankTile + y0]) = double2{acc[x][0], acc[x][1]};
    *reinterpret_cast<double2*>(&out[(x0 + x) * kRankTile + y0 + 2]) = double2{acc[x][2], acc[x][3]};
  }
}

// G[i][j] = the slabs' parts in ascending order, written to gram (may be NULL) on both sides of the diagonal, and the
// workgroup's share of tr G and |G|_F^2 (an entry of a pair off the diagonal stands for two) to block_trace / block_frob2
// [pairs * 16].  grid (kRankTileCells / kRankThreads, pairs).
__global__ void __launch_bounds__(kRankThreads) k_rank_reduce(const double* __restrict__ part, uint32_t slabs, uint32_t C, uint32_t tiles,
                                                              double* __restrict__ gram, double* __restrict__ block_trace,
                                                              double* __restrict__ block_frob2) {
  __shared__ double s_tr[kRankThreads / 64], s_fr[kRankThreads / 64];
  uint32_t ti, tj;
  rank_pair(blockIdx.y, tiles, ti, tj);
  const bool diag = ti == tj;
  const uint32_t e = blockIdx.x * kRankThreads + threadIdx.x, x = e / kRankTile, y = e % kRankTile;
  const uint64_t pairs = gridDim.y;
  double g = 0.0;
  for (uint32_t k = 0; k < slabs; ++k) g += part[(uint64_t(k) * pairs + blockIdx.y) * kRankTileCells + e];
  const uint32_t i = ti * kRankTile + x, j = tj * kRankTile + y;
  if (gram && i < C && j < C) {
    gram[uint64_t(i) * C + j] = g;
    if (!diag) gram[uint64_t(j) * C + i] = g;
  }
  double tr = rank_fold64(diag && x == y ? g : 0.0);
  double fr = rank_fold64(diag ? g * g : 2.0 * (g * g));
  if (threadIdx.x % 64 == 0) { s_tr[threadIdx.x / 64] = tr; s_fr[threadIdx.x / 64] = fr; }
  __syncthreads();
  if (threadIdx.x == 0) {
    tr = s_tr[0]; fr = s_fr[0];
    for (uint32_t w = 1; w < kRankThreads / 64; ++w) { tr += s_tr[w]; fr += s_fr[w]; }
    const uint32_t b = blockIdx.y * gridDim.x + blockIdx.x;
    block_trace[b] = tr; block_frob2[b] = fr;
  }
}

// the record: the workgroups' sums, thread t adding those at t, t + 256, ... in ascending order, then the butterfly.
// frob2 == 0 exactly (one row, equal rows) gives rank 1.0, as the reference returns; no epsilon.
__global__ void __launch_bounds__(kRankThreads) k_rank_final(const double* __restrict__ block_trace, const double* __restrict__ block_frob2,
                                                             uint32_t blocks, uint32_t n, uint32_t C, FeatureRankRecord* __restrict__ rec) {
  __shared__ double s_tr[kRankThreads / 64], s_fr[kRankThreads / 64];
  double tr = 0.0, fr = 0.0;
  for (uint32_t b = threadIdx.x; b < blocks; b += kRankThreads) { tr += block_trace[b]; fr += block_frob2[b]; }
  tr = rank_fold64(tr); fr = rank_fold64(fr);
  if (threadIdx.x % 64 == 0) { s_tr[threadIdx.x / 64] = tr; s_fr[threadIdx.x / 64] = fr; }
  __syncthreads();
  if (threadIdx.x == 0) {
    tr = s_tr[0]; fr = s_fr[0];
    for (uint32_t w = 1; w < kRankThreads / 64; ++w) { tr += s_tr[w]; fr += s_fr[w]; }
    rec->trace = tr; rec->frob2 = fr;
    rec->rank = fr == 0.0 ? 1.0 : tr * tr / fr;
    rec->n = n; rec->channels = C;
  }
}

}  // namespace azmi
