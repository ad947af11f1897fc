// The device-pointer, stream-ordered surface of the stand-alone cache (azmi_cache_find_rows / azmi_cache_insert_rows, cache.hip):
// the probes and inserts of cache.hip's host-array entry points on rows that are already in HBM, with nothing read back.
//   k_cache_find_rows<WAVE>   per row exactly k_cache_find_wave<8> (WAVE, 64-entry shards) / k_cache_find_many (the generic tables):
//                             counters, frequency bump, ghost "reinsert" accounting, hash 0 a key; a hit's payload rows are written,
//                             a miss's rows are left as they were.
//   k_cache_miss_scan         the number of misses in front of every group of 64 rows, and their total, from hit[] (one workgroup)
//   k_cache_miss_scatter      miss_rows[0 .. total) = the rows with hit == 0, ascending
//   k_cache_insert_rows_wave  cache_apply_batch<true> over chunk `chunk` of the row list; the count is read on the device
//   k_cache_insert_rows       the generic tables: one lane per shard walks the list in list order
// Order of the compaction: row i of group g = i / 64 lands at offs[g] + (misses among the rows g * 64 .. i - 1).  offs[] is an
// exclusive prefix over per-group counts that one workgroup adds up in ascending group order, and the in-group term is the
// population count of the wavefront's ballot below the lane: both are functions of hit[] alone.  No position is drawn from an
// atomic counter, so miss_rows does not depend on which wavefront runs first.  The arithmetic is in the __host__ __device__
// helpers of cache_rows_index.h (tests/cache_rows_index_check.cpp runs them on the CPU against a plain loop).
#pragma once
#include "dev_cache.h"
#include "cache_rows_index.h"

namespace azmi {

template <bool WAVE>
__global__ __launch_bounds__(256) void k_cache_find_rows(CacheView c, const uint64_t* keys, uint32_t n, uint8_t* hit, float* policy, float* value) {
  const uint32_t gtid = blockIdx.x * blockDim.x + threadIdx.x;
  if constexpr (WAVE) {
    constexpr int G = 8;
    const uint32_t i = gtid / G, gl = gtid % G;
    if (i >= n) return;                 // (whole lane groups leave together: 256 is a multiple of 8)
    const uint64_t h = keys[i];
    uint32_t sh;
    const int slot = wave_shard_find<G>(c, h, gl, &sh);
    if (gl == 0) { wave_shard_find_account(c, h, sh, slot); hit[i] = slot >= 0; }
    if (slot < 0) return;
    const float* sp = c.policy + (static_cast<size_t>(sh) * kWaveCap + slot) * c.np;
    const float* sv = c.value + (static_cast<size_t>(sh) * kWaveCap + slot) * c.nv;
    for (uint32_t j = gl; j < c.np; j += G) policy[static_cast<size_t>(i) * c.np + j] = sp[j];
    for (uint32_t j = gl; j < c.nv; j += G) value[static_cast<size_t>(i) * c.nv + j] = sv[j];
  } else {
    const uint32_t i = gtid;
    if (i >= n) return;
    const uint64_t h = keys[i];
    uint32_t sh;
    const int slot = cache_find(c, h, &sh);
    cache_find_account(c, h, sh, slot);
    hit[i] = slot >= 0;
    if (slot < 0) return;
    const float* sp = c.policy + (static_cast<size_t>(sh) * c.cap + slot) * c.np;
    const float* sv = c.value + (static_cast<size_t>(sh) * c.cap + slot) * c.nv;
    for (uint32_t j = 0; j < c.np; ++j) policy[static_cast<size_t>(i) * c.np + j] = sp[j];
    for (uint32_t j = 0; j < c.nv; ++j) value[static_cast<size_t>(i) * c.nv + j] = sv[j];
  }
}

// offs[g] = misses among the rows in front of group g; *miss_count = all of them.  One workgroup of kRowsScanThreads: a thread
// counts its span of groups (leaving each group's count in offs), the counts are scanned (shuffles inside a wavefront, s_pref
// across the 16 wavefronts), and the thread turns its groups' counts into their prefixes
__global__ __launch_bounds__(kRowsScanThreads) void k_cache_miss_scan(const uint8_t* hit, uint32_t n, uint32_t* offs, uint32_t* miss_count) {
  __shared__ uint32_t s_pref[kRowsScanThreads / 64];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  uint32_t lo, hi;
  rows_scan_span(rows_groups(n), kRowsScanThreads, tid, &lo, &hi);
  uint32_t cnt = 0;
  for (uint32_t g = lo; g < hi; ++g) {
    uint32_t first, last, m = 0;
    rows_group_span(n, g, &first, &last);
    for (uint32_t i = first; i < last; ++i) m += hit[i] ? 0u : 1u;
    offs[g] = m;
    cnt += m;
  }
  uint32_t incl = cnt;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t up = __shfl_up(incl, d, 64);
    if (lane >= d) incl += up;
  }
  if (lane == 63u) s_pref[wave] = incl;
  __syncthreads();
  uint32_t before = 0, total = 0;
  for (uint32_t w = 0; w < kRowsScanThreads / 64; ++w) { const uint32_t t = s_pref[w]; if (w < wave) before += t; total += t; }
  uint32_t run = before + incl - cnt;
  for (uint32_t g = lo; g < hi; ++g) { const uint32_t m = offs[g]; offs[g] = run; run += m; }      // (the thread's own stores)
  if (tid == 0) *miss_count = total;
}

// one wavefront per group of 64 rows: the group's misses behind offs[group], in row order
__global__ __launch_bounds__(256) void k_cache_miss_scatter(const uint8_t* hit, uint32_t n, const uint32_t* offs, uint32_t* miss_rows) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;      // (n <= kRowsMax: no wrap)
  const uint32_t lane = threadIdx.x & 63u;
  const bool miss = i < n && hit[i] == 0;
  const unsigned long long mask = __ballot(miss);
  if (miss) miss_rows[offs[i / kRowsGroup] + rows_rank(mask, lane)] = i;
}

// chunk `chunk` of the list rows[0 .. min(*row_count, n_max)) (rows == nullptr: the rows 0 .. n_max - 1 themselves; row_count ==
// nullptr: n_max of them) through cache_apply_batch: the owner wavefront of a shard applies the shard's elements in list order.
// Launch <<<ceil(min(kApplyMax, n_max - chunk * kApplyMax) / 4), 256>>>; the chunks of one call run in order on one stream.
__global__ __launch_bounds__(256) void k_cache_insert_rows_wave(CacheView c, const uint64_t* keys, const float* policy, const float* value,
                                                                const uint32_t* rows, const uint32_t* row_count, uint32_t n_max, uint32_t chunk) {
  __shared__ uint32_t s_sid[kApplyMax];
  uint32_t off, m;
  if (!rows_chunk_cut(row_count ? *row_count : n_max, n_max, chunk, kApplyMax, &off, &m)) return;      // (uniform over the grid)
  if (rows) cache_apply_batch<true, true>(c, keys, policy, value, m, s_sid, nullptr, 0, rows + off);
  else cache_apply_batch<true>(c, keys + off, policy + static_cast<size_t>(off) * c.np, value + static_cast<size_t>(off) * c.nv, m, s_sid);
}

// the generic tables: k_cache_insert_many over the list (one lane per shard, list order kept inside a shard)
__global__ void k_cache_insert_rows(CacheView c, const uint64_t* keys, const float* policy, const float* value, const uint32_t* rows,
                                    const uint32_t* row_count, uint32_t n_max) {
  const uint32_t sh = blockIdx.x * blockDim.x + threadIdx.x;
  if (sh >= c.shards) return;
  const uint32_t limit = row_count ? *row_count : n_max;
  const uint32_t count = limit < n_max ? limit : n_max;
  ShardCtx ctx(c, sh);
  for (uint32_t j = 0; j < count; ++j) {
    const size_t i = rows ? rows[j] : j;
    const uint64_t h = keys[i];
    if (shard_of(c, h) != sh) continue;
    const int slot = ctx.insert(h);
    if (slot < 0) continue;
    float* dp = c.policy + (static_cast<size_t>(sh) * c.cap + slot) * c.np;
    float* dv = c.value + (static_cast<size_t>(sh) * c.cap + slot) * c.nv;
    for (uint32_t e = 0; e < c.np; ++e) dp[e] = policy[i * c.np + e];
    for (uint32_t e = 0; e < c.nv; ++e) dv[e] = value[i * c.nv + e];
  }
}

}  // namespace azmi
