// The history window and the recency-weighted reservoir on the device (game_runner.py:955-1008 calc_hist_size, :1701-1869
// update_reservoir, :1289-1345 and :1923-2009 train / StreamingCompressedDataset): the keys of a weighted sample without
// replacement, the selection of the k largest of them, and the row gather that cuts training batches from a list of segments.
// DESIGN.md §8.5.2 states the formulas.
//
// Determinism: the keys are a function of (seed, row id, age) alone; the selection counts with integer atomics, whose sums do not
// depend on their order, and writes the chosen rows by an exclusive scan over tiles (the tile tree of k_plan_scan); the
// permutation of the gather is computed per row from (seed, pass, position).  No floating-point atomic, no kernel that waits for
// another workgroup, no sort.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dev_rng.h"
#include "samples_kernels.h"

namespace azmi {

// ---- k_reservoir_keys -------------------------------------------------------------------------------------------------------
constexpr uint32_t kKeyThreads = 256;

// m_i: the 52 high bits of mix64(seed + 0x9E3779B97F4A7C15 * (id + 1)) with a one appended, an odd integer in [1, 2^53 - 1];
// u_i = m_i * 2^-53 is exact in float64 and lies strictly inside (0, 1), so log(u_i) is finite and negative
__host__ __device__ __forceinline__ uint64_t key_uniform_bits(uint64_t seed, uint64_t id) {
  return ((mix64(seed + 0x9E3779B97F4A7C15ULL * (id + 1)) >> 12) << 1) | 1ULL;
}

// key_i = log(u_i) / w_i,  w_i = decay ** max(0, iteration - iters[i]): the k LARGEST keys are a weighted sample without
// replacement (Efraimidis and Spirakis, in the logarithm).  w_i == 0 (underflow) gives -inf; decay == 1 gives log(u_i) itself.
__global__ void __launch_bounds__(kKeyThreads) k_reservoir_keys(const int32_t* __restrict__ iters, const uint64_t* __restrict__ row_ids,
                                                                uint32_t n, double iteration, double decay, uint64_t seed,
                                                                double* __restrict__ keys, uint64_t* __restrict__ bits_out) {
  const uint32_t i = blockIdx.x * kKeyThreads + threadIdx.x;
  if (i >= n) return;
  const uint64_t m = key_uniform_bits(seed, row_ids ? row_ids[i] : static_cast<uint64_t>(i));
  const double u = static_cast<double>(m) * (1.0 / 9007199254740992.0);
  double age = iteration - static_cast<double>(iters[i]);
  age = age > 0.0 ? age : 0.0;
  keys[i] = log(u) / pow(decay, age);
  if (bits_out) bits_out[i] = m;
}

// ---- k_select_* : the k largest of n keys, as the ascending list of their rows ---------------------------------------------------
// A radix select on the order-preserving 64-bit image of a key, eight passes of eight bits from the top: a pass counts the
// digit of every key that still matches the digits decided so far (k_select_hist), one workgroup walks the 256 counts from the
// top and decides the next digit (k_select_pick).  After the last pass the prefix IS the image of the threshold key T and k_rem
// says how many of the keys equal to T are taken: the lowest rows.  The compaction is the tile tree of the plan: per tile the
// packed count (keys above T << 32 | keys equal to T), an exclusive scan over the tiles, and row i lands at
// (keys above T before i) + min(keys equal to T before i, k_rem).
constexpr uint32_t kSelectThreads = 256;
constexpr uint32_t kSelectMaxBlocks = 2048;
constexpr uint32_t kSelectPasses = 8;

struct SelectState {      // the first 24 bytes are azmi_select_record
  double threshold_key;
  uint64_t selected;
  uint32_t nan_rows;
  uint32_t first_bad_row;
  uint64_t prefix;      // the digits decided so far
  uint32_t k_rem;       // how many of the keys under the prefix are still to be taken
  uint32_t reserved;
  uint32_t hist[kSelectPasses][256];
};

// the image: a < b as float64 <=> image(a) < image(b) as uint64, for everything but NaN; -0.0 is read as +0.0 (x + 0.0)
__device__ __forceinline__ uint64_t key_image(double x) {
  const uint64_t b = static_cast<uint64_t>(__double_as_longlong(x + 0.0));
  return (b >> 63) ? ~b : b | 0x8000000000000000ULL;
}
__device__ __forceinline__ double key_of_image(uint64_t img) {
  return __longlong_as_double(static_cast<long long>((img >> 63) ? img & 0x7FFFFFFFFFFFFFFFULL : ~img));
}

__global__ void __launch_bounds__(kSelectThreads) k_select_hist(const double* __restrict__ keys, uint32_t n, SelectState* __restrict__ st,
                                                                uint32_t pass) {
  __shared__ uint32_t s_h[256];
  s_h[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t shift = 56u - 8u * pass;
  const uint64_t prefix = st->prefix;
  for (uint32_t i = blockIdx.x * kSelectThreads + threadIdx.x; i < n; i += gridDim.x * kSelectThreads) {
    const double x = keys[i];
    const uint64_t img = key_image(x);
    if (pass == 0) {
      if (x != x) {
        atomicAdd(&st->nan_rows, 1u);
        atomicMin(&st->first_bad_row, i);
      }
      atomicAdd(&s_h[img >> 56], 1u);
    } else if ((img >> (shift + 8u)) == prefix) {
      atomicAdd(&s_h[(img >> shift) & 255u], 1u);
    }
  }
  __syncthreads();
  const uint32_t c = s_h[threadIdx.x];
  if (c) atomicAdd(&st->hist[pass][threadIdx.x], c);
}

// one workgroup of one wavefront's worth of work: thread 0 walks the counts from digit 255 down to the one that holds the
// k_rem-th largest key under the prefix
__global__ void __launch_bounds__(64) k_select_pick(SelectState* __restrict__ st, uint32_t pass, uint32_t k) {
  if (threadIdx.x != 0) return;
  uint32_t rem = pass == 0 ? k : st->k_rem;
  uint32_t d = 255;
  for (;;) {
    const uint32_t c = st->hist[pass][d];
    if (c >= rem || d == 0) break;
    rem -= c;
    --d;
  }
  const uint64_t prefix = (st->prefix << 8) | d;
  st->prefix = prefix;
  st->k_rem = rem;
  if (pass == kSelectPasses - 1) {
    st->threshold_key = key_of_image(prefix);
    st->selected = k;
  }
}

// (keys above T) << 32 | (keys equal to T) of one row
__device__ __forceinline__ uint64_t select_flags(const double* __restrict__ keys, uint32_t i, uint32_t n, uint64_t T) {
  if (i >= n) return 0;
  const uint64_t img = key_image(keys[i]);
  return img > T ? 1ULL << 32 : img == T ? 1ULL : 0ULL;
}

__global__ void __launch_bounds__(kPlanBlock) k_select_tiles(const double* __restrict__ keys, uint32_t n, const SelectState* __restrict__ st,
                                                             uint64_t* __restrict__ tile_total) {
  uint64_t all;
  (void)plan_block_scan(select_flags(keys, blockIdx.x * kPlanBlock + threadIdx.x, n, st->prefix), &all);
  if (threadIdx.x == 0) tile_total[blockIdx.x] = all;
}

// tile_base: the exclusive scan of k_select_tiles' totals (null: one tile)
__global__ void __launch_bounds__(kPlanBlock) k_select_write(const double* __restrict__ keys, uint32_t n, const SelectState* __restrict__ st,
                                                             const uint64_t* __restrict__ tile_base, uint32_t k, int64_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * kPlanBlock + threadIdx.x;
  const uint32_t rem = st->k_rem;
  const uint64_t x = select_flags(keys, i, n, st->prefix);
  uint64_t all;
  const uint64_t ex = plan_block_scan(x, &all) + (tile_base ? tile_base[blockIdx.x] : 0);
  const uint32_t above = static_cast<uint32_t>(ex >> 32), equal = static_cast<uint32_t>(ex);
  if ((x >> 32) || (x && equal < rem)) {
    const uint32_t pos = above + (equal < rem ? equal : rem);
    if (pos < k) out[pos] = static_cast<int64_t>(i);      // (always: pos counts the chosen rows before i)
  }
}

// ---- k_window_gather --------------------------------------------------------------------------------------------------------
// out[j] = row p of the window, p = perm(first + j) (or index[first + j]), the window a list of up to kWindowMaxSegments
// arrays addressed through the exclusive prefix of their row counts.  perm is a bijection of [0, total): a Feistel network of
// kFeistelRounds rounds over `bits` = max(2, ceil(log2 total)) bits - the halves are bits / 2 and bits - bits / 2 wide and swap
// every round, the round function is mix64(R + key[r]) - walked until the value is below total again.
constexpr uint32_t kWindowMaxSegments = 64;
constexpr uint32_t kWindowThreads = 256;
constexpr uint32_t kFeistelRounds = 6;

struct WindowSegments {
  const void* base[kWindowMaxSegments];
  uint64_t start[kWindowMaxSegments];      // the first window row of the segment
  uint32_t count;
};

struct WindowPerm {
  uint64_t total;
  uint64_t key[kFeistelRounds];
  uint32_t bits;
};

__host__ __device__ __forceinline__ uint64_t window_perm(uint64_t x, const WindowPerm& pm) {
  do {
    uint32_t wl = pm.bits / 2, wr = pm.bits - wl;
    for (uint32_t r = 0; r < kFeistelRounds; ++r) {
      const uint64_t L = x >> wr, R = x & ((1ULL << wr) - 1);
      x = (R << wl) | (L ^ (mix64(R + pm.key[r]) & ((1ULL << wl) - 1)));
      const uint32_t w = wl; wl = wr; wr = w;
    }
  } while (x >= pm.total);
  return x;
}

// One workgroup moves kWindowThreads rows: thread t finds the source of row t (the permutation, then the segment), the
// workgroup then copies the rows' U units each as one flat range, so consecutive lanes store consecutive units of `out` and load
// consecutive units of a source row.  T: uint4 when the row size and every base address are multiples of 16, else dwords.
template <typename T>
__global__ void __launch_bounds__(kWindowThreads) k_window_gather(WindowSegments seg, WindowPerm pm, const int64_t* __restrict__ index,
                                                                  uint64_t first, uint32_t rows, uint32_t U, T* __restrict__ out) {
  __shared__ const T* s_src[kWindowThreads];
  const uint32_t row0 = blockIdx.x * kWindowThreads;
  const uint32_t here = rows - row0 < kWindowThreads ? rows - row0 : kWindowThreads;
  if (threadIdx.x < here) {
    uint64_t p = first + row0 + threadIdx.x;
    if (index) {
      p = static_cast<uint64_t>(index[p]);
      p = p < pm.total ? p : pm.total - 1;      // (an index outside the window reads its last row, never outside it)
    } else {
      p = window_perm(p, pm);
    }
    const void* base = seg.base[0];
    uint64_t start = 0;
    for (uint32_t s = 1; s < seg.count; ++s) {      // (uniform loads; an empty segment shares its start with the next and loses to it)
      if (seg.start[s] <= p) { base = seg.base[s]; start = seg.start[s]; }
    }
    s_src[threadIdx.x] = static_cast<const T*>(base) + (p - start) * U;
  }
  __syncthreads();
  const uint32_t units = here * U;
  T* dst = out + uint64_t(row0) * U;
#pragma unroll 4
  for (uint32_t e = threadIdx.x; e < units; e += kWindowThreads) {
    const uint32_t r = e / U;
    dst[e] = s_src[r][e - r * U];
  }
}

}  // namespace azmi
