// The scratch blocks of samples.hip, each cut from one allocation (block_cut.h).  The record types are template parameters so
// that this header stays plain C++: samples.hip cuts with the device records of samples_kernels.h / sample_metrics_kernels.h,
// whose sizes are those of the C records of include/azmi.h.
#pragma once
#include "block_cut.h"

namespace azmi {

// azmi_resample_plan: the record | the tile sums of the two lower levels (f64) | the tile totals of the scan's levels (u64);
// t0 tiles of rows, t1 tiles of tiles
template <class Rec>
struct PlanScratch {
  Rec* rec;
  double *sum0, *sum1;
  uint64_t *tot0, *tot1;
};
template <class Rec>
void cut_plan_scratch(BlockCut& c, PlanScratch<Rec>& p, size_t t0, size_t t1) {
  p.rec = c.take<Rec>(1);
  p.sum0 = c.take<double>(t0);
  p.sum1 = c.take<double>(t1);
  p.tot0 = c.take<uint64_t>(t0);
  p.tot1 = c.take<uint64_t>(t1);
}

// azmi_sample_metrics_reduce: the record | per (bucket, column) pair the tile sums of the first and of the second level
template <class Rec>
struct MetricsScratch {
  Rec* rec;
  double *sum0, *sum1;
};
template <class Rec>
void cut_metrics_scratch(BlockCut& c, MetricsScratch<Rec>& m, size_t pairs, size_t t0, size_t t1) {
  m.rec = c.take<Rec>(1);
  m.sum0 = c.take<double>(pairs * t0);
  m.sum1 = c.take<double>(pairs * t1);
}

// azmi_samples_select_top: the state (record, prefix, histograms) | the tile totals of the compaction's scan (u64): t0 tiles of
// rows, t1 tiles of tiles, one word for the total above them
template <class State>
struct SelectScratch {
  State* st;
  uint64_t *tot0, *tot1, *top;
};
template <class State>
void cut_select_scratch(BlockCut& c, SelectScratch<State>& s, size_t t0, size_t t1) {
  s.st = c.take<State>(1);
  s.tot0 = c.take<uint64_t>(t0);
  s.tot1 = c.take<uint64_t>(t1);
  s.top = c.take<uint64_t>(1);
}

// azmi_samples_feature_rank: the record (32 bytes) | the Gram parts per (slab, tile pair), which the kernel stores 16 bytes at a
// time and which therefore come first | the column means | the column sums per slab | the reduction's per-workgroup shares of the
// trace and of the squared norm
template <class Rec>
struct RankScratch {
  Rec* rec;
  double *gram_part, *mean, *col_part, *block_trace, *block_frob2;
};
template <class Rec>
void cut_rank_scratch(BlockCut& c, RankScratch<Rec>& r, size_t channels, size_t sum_slabs, size_t gram_cells, size_t blocks) {
  static_assert(sizeof(Rec) % 16 == 0, "the Gram parts behind the record are 16-byte aligned");
  r.rec = c.take<Rec>(1);
  r.gram_part = c.take<double>(gram_cells);
  r.mean = c.take<double>(channels);
  r.col_part = c.take<double>(sum_slabs * channels);
  r.block_trace = c.take<double>(blocks);
  r.block_frob2 = c.take<double>(blocks);
}

}  // namespace azmi
