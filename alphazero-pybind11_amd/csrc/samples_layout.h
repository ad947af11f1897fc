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

}  // namespace azmi
