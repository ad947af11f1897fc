// The sample path between self-play and training, on the device: the per-row surprise loss of the current net against every
// sample's target, a copy count per sample from its share of the total loss, and the rows repeated that many times
// (resample_by_surprise, game_runner.py:1148-1255; sample_loss / sample_loss_pi / sample_loss_v, neural_net.py:664-676, 875-879).
//
// Arithmetic: float64 on the float32 inputs, as in sweep_metrics and net_vs_search.  Two departures from the reference, both
// stated in DESIGN.md §8.5: the total is a float64 tree sum (the reference: numpy's float32 np.sum), and the draw that rounds a
// fractional weight is ours (the reference: np.random.random from the global numpy state, which nothing can reproduce).
//
// Determinism: every sum below has an order fixed by the problem size alone.  A row's loss is folded inside its lane group;
// the total is a tree over tiles of kPlanBlock elements whose shape depends on n only (one workgroup per tile, no grid-stride
// loop, so the number of workgroups IS the number of tiles); the offsets are integer sums.  No floating-point atomics, and no
// kernel waits for another workgroup: the reduction and the scan are separate launches per level.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cfloat>

#include "dev_rng.h"

namespace azmi {

// ---- k_sample_loss ----------------------------------------------------------------------------------------------------------
constexpr uint32_t kLossThreads = 256;

template <int L>
__device__ __forceinline__ double smp_fold(double x) {
  for (int off = L / 2; off > 0; off >>= 1) x += __shfl_xor(x, off, L);
  return x;
}

// loss[i] = -scale * sum over t[i,m] > 0 of t[i,m] * log(max(p[i,m], FLT_MIN)).  A row belongs to a group of L lanes (8, 16, 32 or
// 64: the power of two that covers M, one wavefront striding m beyond 64); lane l adds its m = l, l + L, ... in ascending order
// and the group folds the L partial sums by an xor butterfly: the bits of a row depend on (M, L) only, not on n or on the grid.
// A zero target contributes exactly 0 whatever p is; a NaN probability stays NaN; a NEGATIVE target makes the row NaN, so that
// the plan's non-finite check names it (the host checks of the staged path never let one get here).
template <int L>
__global__ void __launch_bounds__(kLossThreads) k_sample_loss(const float* __restrict__ target, const float* __restrict__ p, uint32_t n,
                                                              uint32_t M, double scale, double* __restrict__ loss) {
  constexpr uint32_t kRows = kLossThreads / L;
  const uint64_t row = uint64_t(blockIdx.x) * kRows + threadIdx.x / L;
  const uint32_t lane = threadIdx.x % L;
  if (row >= n) return;      // (whole groups leave: L divides the wavefront, the shuffles below stay inside a group)
  const float* t = target + row * M;
  const float* q = p + row * M;
  double s = 0.0;
  for (uint32_t m = lane; m < M; m += L) {
    const double tm = static_cast<double>(t[m]);
    if (tm > 0.0) {
      const double pm = static_cast<double>(q[m]);
      s += tm * log(pm < static_cast<double>(FLT_MIN) ? static_cast<double>(FLT_MIN) : pm);
    } else if (tm < 0.0) {
      s += __longlong_as_double(0x7FF8000000000000LL);
    }
  }
  s = smp_fold<L>(s);
  if (lane == 0) loss[row] = 0.0 - scale * s;      // (0 - x: an all-zero row is +0.0)
}

// ---- k_resample_plan --------------------------------------------------------------------------------------------------------
// One tile = kPlanBlock elements = one workgroup.  Levels of the reduction and of the scan, by n:
//   n <= kPlanBlock (1024)               one level:    the tile's sum is the total
//   n <= kPlanBlock^2 (2^20)             two levels:   up to 1024 tile sums, reduced / scanned by one more workgroup
//   n <= kPlanBlock^3 (2^30, the limit)  three levels: up to 2^20 tile sums, 1024 sums of those, one workgroup on top
constexpr uint32_t kPlanBlock = 1024;
constexpr uint32_t kPlanMaxRows = 1u << 30;
constexpr uint32_t kPlanNone = 0xFFFFFFFFu;

struct ResampleRecord {      // azmi_resample_record
  double total_loss;
  uint64_t rows_out;
  uint32_t nonfinite;
  uint32_t first_nonfinite;
};

// the sum of the workgroup's kPlanBlock values, on thread 0: xor butterfly inside a wavefront, then the 16 wavefront sums in
// ascending order
__device__ __forceinline__ double plan_block_sum(double x) {
  __shared__ double s_wave[kPlanBlock / 64];
  x = smp_fold<64>(x);
  if (threadIdx.x % 64 == 0) s_wave[threadIdx.x / 64] = x;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0) {
    for (uint32_t w = 0; w < kPlanBlock / 64; ++w) s += s_wave[w];
  }
  return s;
}

// out[tile] = the sum of in[tile * kPlanBlock ...) (elements past n_in count as +0.0).  kCheck (level 0, the losses themselves):
// also counts the rows that are NaN or +-inf and keeps the smallest such row, by integer atomics on the record.
template <bool kCheck>
__global__ void __launch_bounds__(kPlanBlock) k_plan_sum(const double* __restrict__ in, uint32_t n_in, double* __restrict__ out,
                                                         ResampleRecord* __restrict__ rec) {
  const uint32_t i = blockIdx.x * kPlanBlock + threadIdx.x;
  const double x = i < n_in ? in[i] : 0.0;
  if (kCheck && i < n_in && !isfinite(x)) {
    atomicAdd(&rec->nonfinite, 1u);
    atomicMin(&rec->first_nonfinite, i);
  }
  const double s = plan_block_sum(x);
  if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// u_i of DESIGN.md §8.5: 53 bits of mix64(seed + 0x9E3779B97F4A7C15 * (i + 1)), in [0, 1)
__host__ __device__ __forceinline__ double plan_uniform(uint64_t seed, uint32_t i) {
  return static_cast<double>(slot_seed(seed, i) >> 11) * (1.0 / 9007199254740992.0);
}

// the exclusive prefix sum of the workgroup's kPlanBlock values; *total (valid on every thread) = their sum
__device__ __forceinline__ uint64_t plan_block_scan(uint64_t x, uint64_t* total) {
  __shared__ uint64_t s_wave[kPlanBlock / 64];
  const uint32_t lane = threadIdx.x % 64, wave = threadIdx.x / 64;
  uint64_t inc = x;
  for (int off = 1; off < 64; off <<= 1) {
    const uint64_t up = __shfl_up(inc, off, 64);
    if (lane >= static_cast<uint32_t>(off)) inc += up;
  }
  if (lane == 63) s_wave[wave] = inc;
  __syncthreads();
  uint64_t base = 0, all = 0;
  for (uint32_t w = 0; w < kPlanBlock / 64; ++w) {
    const uint64_t sw = s_wave[w];
    if (w < wave) base += sw;
    all += sw;
  }
  *total = all;
  return base + inc - x;
}

// copies[i] from the weights and the rounding rule of game_runner.py:1189-1193, every operation in float64 in this order:
//   w = 0.5 + (loss[i] / total) * 0.5 * n,  k = floor(w),  copies[i] = k + (u_i < w - k);   total <= 0: every count is 1.
// A weight that is not a finite number in [0, 2^32) (a non-finite loss: the caller raises on the record) gives 0 copies.
// offsets[i] = the exclusive prefix sum INSIDE the tile; tile_total[tile] = the tile's sum (k_plan_scan / k_plan_add finish it).
__global__ void __launch_bounds__(kPlanBlock) k_plan_copies(const double* __restrict__ loss, uint32_t n, uint64_t seed,
                                                            const double* __restrict__ total_loss, uint32_t* __restrict__ copies,
                                                            uint64_t* __restrict__ offsets, uint64_t* __restrict__ tile_total) {
  const uint32_t i = blockIdx.x * kPlanBlock + threadIdx.x;
  const double total = *total_loss;
  uint32_t c = 0;
  if (i < n) {
    if (total <= 0.0) {
      c = 1;
    } else {
      const double w = 0.5 + (loss[i] / total) * 0.5 * static_cast<double>(n);
      if (w >= 0.0 && w < 4294967295.0) {
        const double k = floor(w);
        c = static_cast<uint32_t>(k) + (plan_uniform(seed, i) < w - k ? 1u : 0u);
      }
    }
    copies[i] = c;
  }
  uint64_t all;
  const uint64_t ex = plan_block_scan(c, &all);
  if (i < n) offsets[i] = ex;
  if (threadIdx.x == 0) tile_total[blockIdx.x] = all;
}

// in place: data[tile * kPlanBlock ...) becomes its exclusive prefix sum, tile_total[tile] = the tile's sum
__global__ void __launch_bounds__(kPlanBlock) k_plan_scan(uint64_t* __restrict__ data, uint32_t n, uint64_t* __restrict__ tile_total) {
  const uint32_t i = blockIdx.x * kPlanBlock + threadIdx.x;
  const uint64_t x = i < n ? data[i] : 0;
  uint64_t all;
  const uint64_t ex = plan_block_scan(x, &all);
  if (i < n) data[i] = ex;
  if (threadIdx.x == 0) tile_total[blockIdx.x] = all;
}

// data[i] += tile_base[i / kPlanBlock]: the scanned level above, handed down
__global__ void __launch_bounds__(kPlanBlock) k_plan_add(uint64_t* __restrict__ data, uint32_t n, const uint64_t* __restrict__ tile_base) {
  const uint32_t i = blockIdx.x * kPlanBlock + threadIdx.x;
  if (i < n) data[i] += tile_base[blockIdx.x];
}

// ---- k_resample_gather ------------------------------------------------------------------------------------------------------
// out[offsets[i] + c] = in[i] for c < copies[i]  (x[np.repeat(np.arange(n), copies)]), source-driven, for up to kGatherMaxArrays row
// arrays in one launch (blockIdx.y = the array).  A row moves in units of 16 bytes when its size and both base addresses are
// multiples of 16 (the host decides per array), in dwords otherwise.  A row belongs to a group of G lanes, G = the power of two
// that covers its units, at most 64; a unit is loaded once and stored once per copy.
//
// Skew: a group stores the first kGatherOwn copies of its row by itself.  Where a row has more, the rest is spread over ALL
// groups of the workgroup (256 threads, four wavefronts: group g takes the copies kGatherOwn + g, + groups, ...), each re-reading
// the row's units from the cache: a row with thousands of copies runs at a workgroup's store rate, not at one wavefront's.
constexpr uint32_t kGatherThreads = 256;
constexpr uint32_t kGatherMaxArrays = 8;
constexpr uint32_t kGatherOwn = 4;

struct GatherArrays {
  const void* in[kGatherMaxArrays];
  void* out[kGatherMaxArrays];
  uint32_t units[kGatherMaxArrays];      // per row: 16-byte units (vec) or dwords
  uint32_t lanes[kGatherMaxArrays];      // G
  uint8_t vec[kGatherMaxArrays];
};

template <typename T>
__device__ __forceinline__ void gather_rows(const T* __restrict__ in, T* __restrict__ out, uint32_t U, uint32_t G, uint32_t n,
                                            const uint32_t* __restrict__ copies, const uint64_t* __restrict__ offsets) {
  __shared__ uint32_t s_copies[kGatherThreads];
  __shared__ uint64_t s_offset[kGatherThreads];
  const uint32_t groups = kGatherThreads / G, g = threadIdx.x / G, lane = threadIdx.x % G;
  const uint64_t row0 = uint64_t(blockIdx.x) * groups, row = row0 + g;
  uint32_t cnt = 0;
  uint64_t off = 0;
  if (row < n) { cnt = copies[row]; off = offsets[row]; }
  if (lane == 0) { s_copies[g] = cnt; s_offset[g] = off; }
  const uint32_t own = cnt < kGatherOwn ? cnt : kGatherOwn;
  if (own) {
    const T* src = in + row * U;
    T* dst = out + off * U;
    for (uint32_t u = lane; u < U; u += G) {
      const T x = src[u];
      for (uint32_t c = 0; c < own; ++c) dst[uint64_t(c) * U + u] = x;
    }
  }
  if (!__syncthreads_or(cnt > kGatherOwn)) return;
  for (uint32_t r = 0; r < groups; ++r) {      // (uniform over the workgroup)
    const uint32_t rc = s_copies[r];
    if (rc <= kGatherOwn) continue;
    const T* src = in + (row0 + r) * U;
    T* dst = out + s_offset[r] * U;
    for (uint32_t u = lane; u < U; u += G) {
      const T x = src[u];
      for (uint32_t c = kGatherOwn + g; c < rc; c += groups) dst[uint64_t(c) * U + u] = x;
    }
  }
}

__global__ void __launch_bounds__(kGatherThreads) k_resample_gather(GatherArrays a, uint32_t n, const uint32_t* __restrict__ copies,
                                                                    const uint64_t* __restrict__ offsets) {
  const uint32_t k = blockIdx.y;
  const uint32_t G = a.lanes[k];
  if (uint64_t(blockIdx.x) * (kGatherThreads / G) >= n) return;      // (arrays with wider groups need more workgroups than this one)
  if (a.vec[k]) gather_rows<uint4>(static_cast<const uint4*>(a.in[k]), static_cast<uint4*>(a.out[k]), a.units[k], G, n, copies, offsets);
  else gather_rows<uint32_t>(static_cast<const uint32_t*>(a.in[k]), static_cast<uint32_t*>(a.out[k]), a.units[k], G, n, copies, offsets);
}

}  // namespace azmi
