// csrc/cache_rows_index.h on the CPU: the ordered compaction of the cache's miss list and the chunk / row_count cut of its row-list
// insert, run the way the kernels run them (k_cache_miss_scan's threads one after the other, k_cache_miss_scatter's wavefronts
// one after the other, one k_cache_insert_rows_wave launch per chunk) and compared with a plain loop.  Built with
// -fsanitize=address,undefined: every index the kernels would form is formed here against arrays of the exact size.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../alphazero-pybind11_amd/csrc/cache_rows_index.h"

using namespace azmi;

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s (n = %u)\n", __FILE__, __LINE__, #c, n); std::exit(1); } } while (0)

static uint64_t g_state = 0x243F6A8885A308D3ull;
static uint32_t rnd() { g_state = g_state * 6364136223846793005ull + 1442695040888963407ull; return static_cast<uint32_t>(g_state >> 33); }

// hit[] -> miss_rows / miss_count as the two kernels compute them
static void compact(const std::vector<uint8_t>& hit, uint32_t threads, std::vector<uint32_t>& rows, uint32_t& count) {
  const uint32_t n = static_cast<uint32_t>(hit.size());
  const uint32_t groups = rows_groups(n);
  std::vector<uint32_t> offs(groups);      // exactly the scratch the library allocates
  std::vector<uint32_t> cnt(threads);
  uint32_t covered = 0;
  for (uint32_t tid = 0; tid < threads; ++tid) {      // pass 1 of k_cache_miss_scan
    uint32_t lo, hi;
    rows_scan_span(groups, threads, tid, &lo, &hi);
    CHECK(lo == covered && hi >= lo && hi <= groups);      // consecutive, ascending, nothing twice
    covered = hi;
    for (uint32_t g = lo; g < hi; ++g) {
      uint32_t first, last, m = 0;
      rows_group_span(n, g, &first, &last);
      CHECK(first == g * kRowsGroup && last > first && last <= n && last - first <= kRowsGroup);
      for (uint32_t i = first; i < last; ++i) m += hit[i] ? 0u : 1u;
      offs[g] = m;
      cnt[tid] += m;
    }
  }
  CHECK(covered == groups);
  uint32_t before = 0;
  for (uint32_t tid = 0; tid < threads; ++tid) {      // the block scan, then pass 2
    uint32_t lo, hi, run = before;
    rows_scan_span(groups, threads, tid, &lo, &hi);
    for (uint32_t g = lo; g < hi; ++g) { const uint32_t m = offs[g]; offs[g] = run; run += m; }
    before += cnt[tid];
  }
  count = before;
  rows.assign(n, 0xFFFFFFFFu);
  const uint32_t lanes = rows_groups(n) * kRowsGroup;      // k_cache_miss_scatter: whole wavefronts
  for (uint32_t base = 0; base < lanes; base += kRowsGroup) {
    unsigned long long mask = 0;
    for (uint32_t lane = 0; lane < kRowsGroup; ++lane) if (base + lane < n && hit[base + lane] == 0) mask |= 1ull << lane;
    for (uint32_t lane = 0; lane < kRowsGroup; ++lane) {
      const uint32_t i = base + lane;
      if (!(i < n && hit[i] == 0)) continue;
      const uint32_t at = offs[i / kRowsGroup] + rows_rank(mask, lane);
      CHECK(at < count);
      rows.at(at) = i;
    }
  }
}

int main() {
  const uint32_t sizes[] = {0, 1, 63, 64, 65, 255, 257, 4001, 8192, 8193, 16385};
  const uint32_t kChunk = 8192;      // kApplyMax
  for (uint32_t n : sizes) {
    for (int pattern = 0; pattern < 5; ++pattern) {
      std::vector<uint8_t> hit(n);
      for (uint32_t i = 0; i < n; ++i)
        hit[i] = pattern == 0 ? 0 : pattern == 1 ? 1 : pattern == 2 ? (i % 3 == 0) : pattern == 3 ? (rnd() & 1u) : (rnd() % 17u != 0);
      std::vector<uint32_t> want;
      for (uint32_t i = 0; i < n; ++i) if (!hit[i]) want.push_back(i);
      for (uint32_t threads : {1024u, 64u, 1u}) {
        std::vector<uint32_t> rows;
        uint32_t count = 0;
        compact(hit, threads, rows, count);
        CHECK(count == want.size());
        for (uint32_t j = 0; j < count; ++j) CHECK(rows[j] == want[j]);
        for (uint32_t j = count; j < n; ++j) CHECK(rows[j] == 0xFFFFFFFFu);
      }
    }
    // the insert list: `launches` launches sized from n_max alone, each applying its cut of the first min(row_count, n_max) elements
    const uint32_t launches = rows_chunks(n, kChunk);
    CHECK(static_cast<uint64_t>(launches) * kChunk >= n && (launches == 0 || static_cast<uint64_t>(launches - 1) * kChunk < n));
    const uint32_t counts[] = {0, 1, n / 2, n ? n - 1 : 0, n, n + 1, 0xFFFFFFFFu};
    for (uint32_t row_count : counts) {
      std::vector<uint32_t> list(n), applied;
      for (uint32_t j = 0; j < n; ++j) list[j] = n - 1 - j;
      for (uint32_t k = 0; k < launches + 1; ++k) {      // (one launch more than the host enqueues: it must find nothing)
        uint32_t off, m;
        const bool work = rows_chunk_cut(row_count, n, k, kChunk, &off, &m);
        CHECK(work == (m != 0) && m <= kChunk && static_cast<uint64_t>(off) + m <= n);
        CHECK(!work || m <= (n - k * kChunk < kChunk ? n - k * kChunk : kChunk));      // inside the grid the host sized
        for (uint32_t j = 0; j < m; ++j) applied.push_back(list.at(off + j));
        if (k == launches) CHECK(!work);
      }
      const uint32_t expect = row_count < n ? row_count : n;
      CHECK(applied.size() == expect);
      for (uint32_t j = 0; j < expect; ++j) CHECK(applied[j] == list[j]);
    }
  }
  for (uint32_t lane = 0; lane < 64; ++lane) {
    const uint32_t n = lane;
    CHECK(rows_rank(~0ull, lane) == lane && rows_rank(0ull, lane) == 0 && rows_rank(1ull << lane, lane) == 0);
  }
  std::printf("cache_rows_index_check: ok (%zu sizes)\n", sizeof(sizes) / sizeof(sizes[0]));
  return 0;
}
