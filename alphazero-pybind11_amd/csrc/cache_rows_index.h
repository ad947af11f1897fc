// The index arithmetic of the cache's device-pointer entries (cache_rows_kernels.h), apart from the kernels so that the host can run
// it: which groups of 64 rows a scan thread adds up, which rows a group holds, where a miss lands inside its group, and which
// elements of an insert list a launch applies.  No HIP header: tests/cache_rows_index_check.cpp compiles this file with a plain
// C++ compiler under the address and undefined-behaviour sanitizers and compares every function with a loop.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define AZMI_HD __host__ __device__
#else
#define AZMI_HD
#endif

namespace azmi {

constexpr uint32_t kRowsGroup = 64;          // rows per compaction group: one wavefront of k_cache_miss_scatter
constexpr uint32_t kRowsScanThreads = 1024;  // the one workgroup of k_cache_miss_scan
constexpr uint32_t kRowsMax = 1u << 30;      // rows per call (azmi_cache_find_rows / insert_rows refuse more)

// groups of 64 rows that n rows make (no n + 63: n may be anything up to 2^32 - 1 here)
AZMI_HD inline uint32_t rows_groups(uint32_t n) { return n / kRowsGroup + (n % kRowsGroup ? 1u : 0u); }
// the groups [lo, hi) that thread `tid` of `threads` adds up: consecutive, ascending with tid, all of [0, groups) together
AZMI_HD inline void rows_scan_span(uint32_t groups, uint32_t threads, uint32_t tid, uint32_t* lo, uint32_t* hi) {
  const uint32_t per = groups / threads + (groups % threads ? 1u : 0u);
  const uint64_t a = static_cast<uint64_t>(tid) * per;
  *lo = a < groups ? static_cast<uint32_t>(a) : groups;
  *hi = (a + per) < groups ? static_cast<uint32_t>(a + per) : groups;
}
// rows [first, last) of group g among n rows
AZMI_HD inline void rows_group_span(uint32_t n, uint32_t g, uint32_t* first, uint32_t* last) {
  const uint64_t a = static_cast<uint64_t>(g) * kRowsGroup;
  *first = a < n ? static_cast<uint32_t>(a) : n;
  *last = (a + kRowsGroup) < n ? static_cast<uint32_t>(a + kRowsGroup) : n;
}
// misses of the group in front of `lane`: the set bits of the group's miss mask below bit `lane` (lane < 64)
AZMI_HD inline uint32_t rows_rank(unsigned long long mask, uint32_t lane) {
  return static_cast<uint32_t>(__builtin_popcountll(mask & ((1ull << lane) - 1ull)));
}
// chunk `chunk` of an insert list: elements [*off, *off + *m) of the first min(row_count, n_max) ones, `chunk_max` per chunk;
// false: the chunk lies behind the count (the launch has nothing to do)
AZMI_HD inline bool rows_chunk_cut(uint32_t row_count, uint32_t n_max, uint32_t chunk, uint32_t chunk_max, uint32_t* off, uint32_t* m) {
  const uint32_t count = row_count < n_max ? row_count : n_max;
  const uint64_t a = static_cast<uint64_t>(chunk) * chunk_max;
  if (a >= count) { *off = count; *m = 0; return false; }
  *off = static_cast<uint32_t>(a);
  *m = (count - *off) < chunk_max ? count - *off : chunk_max;
  return true;
}
// launches an insert of up to n_max listed rows takes on the wave layout
AZMI_HD inline uint32_t rows_chunks(uint32_t n_max, uint32_t chunk_max) { return n_max / chunk_max + (n_max % chunk_max ? 1u : 0u); }

}  // namespace azmi
