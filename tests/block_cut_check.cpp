// Stand-alone check of csrc/block_cut.h and of every layout written with it (search_batch_types.h, samples_layout.h); built and
// run by tests/test_block_cut.py with -fsanitize=address,undefined.  For every layout: the sizing pass (null base) equals the end
// offset of the cutting pass on a malloc of that size; every pointer is aligned to its element type; the arrays are disjoint, in
// order and inside the block, the last byte of each written to so that the sanitizer sees it.  The sizes are compared with the
// byte formulas the layouts replaced, written out below.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../alphazero-pybind11_amd/csrc/samples_layout.h"
#include "../alphazero-pybind11_amd/csrc/search_batch_types.h"
#include "../include/azmi.h"

using namespace azmi;

static int g_failed = 0;
#define CHECK(cond, ...)                                                    \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond);         \
      std::printf(__VA_ARGS__);                                             \
      std::printf("\n");                                                    \
      ++g_failed;                                                           \
    }                                                                       \
  } while (0)

struct Range {
  const char* name;
  const void* p;
  size_t count, elem, align;
};
#define R(ptr, count) Range{#ptr, ptr, static_cast<size_t>(count), sizeof(*(ptr)), alignof(decltype(*(ptr)))}

// `cut(c)` runs one layout on the cutter and returns its arrays in the order they are taken
template <class Cut>
size_t check_layout(const char* what, Cut&& cut) {
  BlockCut size;
  for (const Range& r : cut(size)) CHECK(r.p == nullptr, "%s: %s is not null in the sizing pass", what, r.name);
  const size_t bytes = size.off;
  unsigned char* block = static_cast<unsigned char*>(std::malloc(bytes ? bytes : 1));
  CHECK(block != nullptr, "%s: malloc(%zu)", what, bytes);
  if (!block) return bytes;
  BlockCut c(block);
  const std::vector<Range> ranges = cut(c);
  CHECK(c.off == bytes, "%s: the cutting pass ends at %zu, the sizing pass at %zu", what, c.off, bytes);
  const unsigned char* end_prev = block;
  for (const Range& r : ranges) {
    const unsigned char* p = static_cast<const unsigned char*>(r.p);
    CHECK(reinterpret_cast<uintptr_t>(p) % r.align == 0, "%s: %s is not aligned to %zu", what, r.name, r.align);
    CHECK(p >= end_prev, "%s: %s starts %td bytes before the end of the array in front of it", what, r.name, end_prev - p);
    CHECK(p + r.count * r.elem <= block + bytes, "%s: %s ends outside the block", what, r.name);
    if (p >= end_prev && p + r.count * r.elem <= block + bytes) {
      if (r.count) const_cast<unsigned char*>(p)[r.count * r.elem - 1] = 0xA5;
      end_prev = p + r.count * r.elem;
    }
  }
  std::free(block);
  return bytes;
}

// ---- the formulas of the parent ------------------------------------------------------------------------------------------------------
static size_t old_sweep_clear(size_t N, size_t M, size_t cap) { return N * (1 + cap * (1 + 3 * M + 3)) * 4; }
static size_t old_sweep(size_t N, size_t M, size_t cap) { return (N * (1 + cap * (1 + 3 * M + 3)) + N + kSbMaxCheckpoints) * 4; }
static size_t old_frontier_trees(size_t N, size_t M) { return 8 * (2 * N + 2 * N * M + N + 3 * N + N) + 4 * (N + (N + 1) + 1) + (N + N * M); }
static size_t old_frontier_records(size_t C, size_t V) { return C * (8 + 8 + 4 + 4 + 4 * V + 3); }
static size_t old_sweep_metrics(size_t N, size_t cap) { return 8 * (N * cap * kSweepCols + 2 * N + cap * kSweepCols) + 4 * cap * kSweepCols + N * cap; }
static size_t old_plan(size_t t0, size_t t1) { return (4 + 2 * (t0 + t1)) * 8; }
static size_t old_metrics(size_t pairs, size_t t0, size_t t1) { return sizeof(azmi_sample_metrics_record) + 8 * pairs * (t0 + t1); }

static size_t sweep_bytes(size_t N, size_t M, size_t cap, size_t* clear_bytes) {
  return check_layout("sweep snapshots", [&](BlockCut& c) {
    SbSweepArrays sw{};
    *clear_bytes = sb_cut_sweep(c, sw, N, M, cap);
    if (c.base) CHECK(reinterpret_cast<unsigned char*>(sw.target) == c.base + *clear_bytes, "sweep snapshots: target does not start at clear_bytes");
    return std::vector<Range>{R(sw.taken, N), R(sw.root_n, N * cap), R(sw.counts, N * cap * M), R(sw.probs, N * cap * M),
                              R(sw.root_values, N * cap * 3), R(sw.root_q, N * cap * M), R(sw.target, N), R(sw.cps, kSbMaxCheckpoints)};
  });
}

static size_t frontier_trees_bytes(size_t N, size_t M) {
  return check_layout("frontier per-tree", [&](BlockCut& c) {
    SbFrontierArrays fr{};
    sb_cut_frontier_trees(c, fr, N, M);
    if (c.base) CHECK(fr.temp == fr.reach + N, "frontier per-tree: reach | temp are not neighbours");
    return std::vector<Range>{R(fr.reach, N), R(fr.temp, N), R(fr.raw_pi, N * M), R(fr.samp_pi, N * M), R(fr.entropy, N), R(fr.value, 3 * N),
                              R(fr.key, N), R(fr.kept, N), R(fr.first_child, N + 1), R(fr.total, 1), R(fr.kind, N), R(fr.keep, N * M)};
  });
}

static size_t frontier_records_bytes(size_t cap, size_t V) {
  return check_layout("frontier records", [&](BlockCut& c) {
    SbFrontierArrays fr{};
    sb_cut_frontier_records(c, fr, cap, V);
    return std::vector<Range>{R(fr.child_reach, cap), R(fr.child_key, cap), R(fr.parent, cap), R(fr.action, cap), R(fr.child_scores, cap * V),
                              R(fr.child_player, cap), R(fr.child_variant, cap), R(fr.child_terminal, cap)};
  });
}

static size_t sweep_metrics_bytes(size_t N, size_t cap) {
  return check_layout("sweep-metrics output", [&](BlockCut& c) {
    SweepMetricsOut o{};
    sb_cut_sweep_metrics(c, o, N, cap);
    return std::vector<Range>{R(o.rows, N * cap * kSweepCols), R(o.ceiling, N), R(o.mean, cap * kSweepCols), R(o.outcomes, N),
                              R(o.count, cap * kSweepCols), R(o.valid, N * cap)};
  });
}

static size_t plan_bytes(size_t t0, size_t t1) {
  return check_layout("resample plan scratch", [&](BlockCut& c) {
    PlanScratch<azmi_resample_record> p{};
    cut_plan_scratch(c, p, t0, t1);
    return std::vector<Range>{R(p.rec, 1), R(p.sum0, t0), R(p.sum1, t1), R(p.tot0, t0), R(p.tot1, t1)};
  });
}

static size_t metrics_bytes(size_t pairs, size_t t0, size_t t1) {
  return check_layout("sample metrics scratch", [&](BlockCut& c) {
    MetricsScratch<azmi_sample_metrics_record> m{};
    cut_metrics_scratch(c, m, pairs, t0, t1);
    return std::vector<Range>{R(m.rec, 1), R(m.sum0, pairs * t0), R(m.sum1, pairs * t1)};
  });
}

static void search_blocks(size_t N, size_t M, size_t V, size_t sweep_cap, size_t record_cap, const size_t* expect) {
  size_t clear_bytes = 0;
  const size_t sw = sweep_bytes(N, M, sweep_cap, &clear_bytes);
  const size_t ft = frontier_trees_bytes(N, M), fr = frontier_records_bytes(record_cap, V), sm = sweep_metrics_bytes(N, sweep_cap);
  CHECK(sw == old_sweep(N, M, sweep_cap), "sweep snapshots: %zu bytes, the parent's formula gives %zu", sw, old_sweep(N, M, sweep_cap));
  CHECK(clear_bytes == old_sweep_clear(N, M, sweep_cap), "sweep snapshots: clear_bytes %zu, the parent's %zu", clear_bytes, old_sweep_clear(N, M, sweep_cap));
  CHECK(ft == old_frontier_trees(N, M), "frontier per-tree: %zu bytes, the parent's formula gives %zu", ft, old_frontier_trees(N, M));
  CHECK(fr == old_frontier_records(record_cap, V), "frontier records: %zu bytes, the parent's formula gives %zu", fr, old_frontier_records(record_cap, V));
  CHECK(sm == old_sweep_metrics(N, sweep_cap), "sweep-metrics output: %zu bytes, the parent's formula gives %zu", sm, old_sweep_metrics(N, sweep_cap));
  std::printf("N=%zu M=%zu V=%zu: sweep cap %zu: %zu bytes (clear %zu), frontier per-tree %zu, records cap %zu: %zu, sweep metrics %zu\n", N, M, V,
              sweep_cap, sw, clear_bytes, ft, record_cap, fr, sm);
  if (expect) {
    CHECK(sw == expect[0] && clear_bytes == expect[1] && ft == expect[2] && fr == expect[3] && sm == expect[4],
          "expected %zu (clear %zu), %zu, %zu, %zu bytes", expect[0], expect[1], expect[2], expect[3], expect[4]);
  }
}

int main() {
  // a cutter pads where a layout does not take its arrays in descending element size
  {
    alignas(8) unsigned char buf[24];
    BlockCut c(buf);
    uint8_t* a = c.take<uint8_t>(3);
    uint32_t* b = c.take<uint32_t>(1);
    double* d = c.take<double>(1);
    CHECK(a == buf && reinterpret_cast<unsigned char*>(b) == buf + 4 && reinterpret_cast<unsigned char*>(d) == buf + 8 && c.off == 16,
          "take does not align: offsets %td %td, end %zu", reinterpret_cast<unsigned char*>(b) - buf, reinterpret_cast<unsigned char*>(d) - buf, c.off);
    BlockCut n;
    CHECK(n.take<uint8_t>(3) == nullptr && n.take<uint32_t>(1) == nullptr && n.take<double>(1) == nullptr && n.off == 16, "the sizing pass ends at %zu", n.off);
  }
  static_assert(sizeof(azmi_resample_record) <= 32, "the parent kept 4 words for the plan's record");
  const size_t expect[5] = {752, 612, 560, 195, 1134};      // computed by hand from the parent's expressions
  search_blocks(3, 7, 3, 2, 5, expect);
  search_blocks(1, 7, 3, 1, 1, nullptr);
  search_blocks(1, 1, 1, 1, 1, nullptr);
  search_blocks(5, 81, 3, 32, 405, nullptr);
  // the two scratch blocks of samples.hip: not larger than the parent's formulas
  const size_t kTile = 1024, kColumns = AZMI_SAMPLE_METRIC_COLUMNS, kBuckets = AZMI_SAMPLE_METRIC_MAX_BUCKETS;
  for (size_t n : {size_t(1), size_t(1024), size_t(1025), (size_t(1) << 20) + 1}) {
    const size_t t0 = (n + kTile - 1) / kTile, t1 = (t0 + kTile - 1) / kTile;
    const size_t pb = plan_bytes(t0, t1);
    CHECK(pb <= old_plan(t0, t1), "resample plan scratch, n = %zu: %zu bytes, the parent's formula gives %zu", n, pb, old_plan(t0, t1));
    std::printf("n=%zu: plan scratch %zu bytes (parent %zu)", n, pb, old_plan(t0, t1));
    for (size_t pairs : {kColumns, (kBuckets + 1) * kColumns}) {      // without a bucket array (one bucket), with one (8 buckets + the total)
      const size_t mb = metrics_bytes(pairs, t0, t1);
      CHECK(mb <= old_metrics(pairs, t0, t1), "sample metrics scratch, n = %zu, %zu pairs: %zu bytes, the parent's formula gives %zu", n, pairs, mb,
            old_metrics(pairs, t0, t1));
      std::printf(", metrics scratch of %zu pairs %zu bytes (parent %zu)", pairs, mb, old_metrics(pairs, t0, t1));
    }
    std::printf("\n");
  }
  if (g_failed) { std::printf("%d checks failed\n", g_failed); return 1; }
  std::printf("block_cut_check: ok\n");
  return 0;
}
