// Batched position search, the step between two levels of opening_analysis.py's build_tree (csrc/search_frontier_kernels.h):
// azmi_search_expand computes the sampling distribution of every searched root, the moves kept by reach probability and the rules
// applied to every kept child, three launches whatever N is; azmi_search_frontier reads the result.  Host code only: the kernels
// and their launch functions are in search_batch.hip's device module (search_batch_host.h).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "search_batch_host.h"

using namespace azmi;

namespace {

// the per-tree block (first call) and room for `cap` records (first call, and whenever a call asks for more)
int frontier_reserve(azmi_search* s, uint32_t cap) {
  const size_t N = s->n, M = s->pm->gi.M, V = s->pm->gi.P + 1;
  if (!s->fr_trees) {
    void* q = nullptr;
    BlockCut size;
    SbFrontierArrays sized{};
    sb_cut_frontier_trees(size, sized, N, M);
    SB_TRY(hipHostMalloc(reinterpret_cast<void**>(&s->fr_host), 2 * N * sizeof(double), hipHostMallocDefault));
    SB_TRY(hipEventCreateWithFlags(&s->fr_uploaded, hipEventDisableTiming));
    SB_TRY(hipMalloc(&q, size.off));
    s->fr_trees = q;
    BlockCut cut(q);
    sb_cut_frontier_trees(cut, s->fr, N, M);
  }
  if (!s->fr_records.p || cap > s->fr_cap) {
    BlockCut size;
    SbFrontierArrays sized{};
    sb_cut_frontier_records(size, sized, cap, V);
    SB_TRY(s->fr_records.reserve(size.off));
    s->fr_cap = cap;
    BlockCut cut(s->fr_records.p);
    sb_cut_frontier_records(cut, s->fr, cap, V);
  }
  return AZMI_OK;
}

}  // namespace

extern "C" {

int azmi_search_expand(azmi_search* s, const double* reach, const double* temp, double min_reach, uint32_t max_children, void* stream) {
  int rc = sb_begin_move(s, "expand_frontier"); if (rc) return rc;
  if (!reach || !temp) return SB_FAIL(AZMI_ERR_INVALID, "expand_frontier: null argument");
  if (!(min_reach > 0.0) || !std::isfinite(min_reach)) return SB_FAIL(AZMI_ERR_INVALID, "expand_frontier: min_reach must be positive and finite, got %g", min_reach);
  if (max_children == 0) return SB_FAIL(AZMI_ERR_INVALID, "expand_frontier: max_children must be > 0");
  for (uint32_t i = 0; i < s->n; ++i) {
    if (!(reach[i] >= 0.0) || !std::isfinite(reach[i]))
      return SB_FAIL(AZMI_ERR_INVALID, "expand_frontier: tree %u: reach must be finite and not negative, got %g", i, reach[i]);
    if (!(temp[i] >= 0.0) || !std::isfinite(temp[i]))
      return SB_FAIL(AZMI_ERR_INVALID, "expand_frontier: tree %u: temp must be finite and not negative, got %g", i, temp[i]);
  }
  azmi_pm* pm = s->pm;
  SB_TRY(hipSetDevice(pm->device));
  const bool first = s->fr_host == nullptr;
  rc = frontier_reserve(s, max_children); if (rc) return rc;
  hipStream_t st = pm->pick(stream);
  const size_t N = s->n;
  if (!first) SB_TRY(hipEventSynchronize(s->fr_uploaded));      // the previous call's upload may still read fr_host
  std::memcpy(s->fr_host, reach, N * sizeof(double));
  std::memcpy(s->fr_host + N, temp, N * sizeof(double));
  SB_TRY(hipMemcpyAsync(const_cast<double*>(s->fr.reach), s->fr_host, 2 * N * sizeof(double), hipMemcpyHostToDevice, st));      // (reach | temp are neighbours)
  SB_TRY(hipEventRecord(s->fr_uploaded, st));
  s->fr.max_children = max_children;
  s->fr_valid = true;
  sb_launch_frontier_policy(s, min_reach, st);
  sb_launch_frontier_scan(s, st);
  sb_launch_frontier_emit(s, st);
  SB_TRY(hipGetLastError());
  return AZMI_OK;
}

int azmi_search_frontier(azmi_search* s, uint8_t* kind, uint64_t* key, double* raw_pi, double* sampling_pi, double* entropy, double* value,
                         uint32_t* first_child, uint32_t* parent, uint32_t* action, double* child_reach, uint64_t* child_key, uint8_t* child_player,
                         int8_t* child_variant, uint8_t* child_terminal, float* child_scores) {
  int rc = sb_begin_read(s, "frontier"); if (rc) return rc;
  if (!s->fr_valid) return SB_FAIL(AZMI_ERR_STATE, "frontier: no expand_frontier call has been made on this batch");
  azmi_pm* pm = s->pm;
  SB_TRY(hipSetDevice(pm->device));
  hipStream_t st = pm->last;
  uint32_t total = 0;
  SB_TRY(hipMemcpyAsync(&total, s->fr.total, 4, hipMemcpyDeviceToHost, st));
  rc = sb_check_device(s, st); if (rc) return rc;      // the one synchronisation
  const size_t N = s->n, M = pm->gi.M, V = pm->gi.P + 1;
  if (kind) SB_TRY(hipMemcpy(kind, s->fr.kind, N, hipMemcpyDeviceToHost));
  if (key) SB_TRY(hipMemcpy(key, s->fr.key, N * 8, hipMemcpyDeviceToHost));
  if (raw_pi) SB_TRY(hipMemcpy(raw_pi, s->fr.raw_pi, N * M * 8, hipMemcpyDeviceToHost));
  if (sampling_pi) SB_TRY(hipMemcpy(sampling_pi, s->fr.samp_pi, N * M * 8, hipMemcpyDeviceToHost));
  if (entropy) SB_TRY(hipMemcpy(entropy, s->fr.entropy, N * 8, hipMemcpyDeviceToHost));
  if (value) SB_TRY(hipMemcpy(value, s->fr.value, N * 3 * 8, hipMemcpyDeviceToHost));
  if (first_child) SB_TRY(hipMemcpy(first_child, s->fr.first_child, (N + 1) * 4, hipMemcpyDeviceToHost));
  if (total > s->fr.max_children)
    return SB_FAIL(AZMI_ERR_OVERFLOW, "frontier: the trees keep %u children, max_children = %u: the first %u records were written; expand again "
                   "with room for all of them", total, s->fr.max_children, s->fr.max_children);
  const size_t T = total;
  if (!T) return AZMI_OK;
  if (parent) SB_TRY(hipMemcpy(parent, s->fr.parent, T * 4, hipMemcpyDeviceToHost));
  if (action) SB_TRY(hipMemcpy(action, s->fr.action, T * 4, hipMemcpyDeviceToHost));
  if (child_reach) SB_TRY(hipMemcpy(child_reach, s->fr.child_reach, T * 8, hipMemcpyDeviceToHost));
  if (child_key) SB_TRY(hipMemcpy(child_key, s->fr.child_key, T * 8, hipMemcpyDeviceToHost));
  if (child_player) SB_TRY(hipMemcpy(child_player, s->fr.child_player, T, hipMemcpyDeviceToHost));
  if (child_variant) SB_TRY(hipMemcpy(child_variant, s->fr.child_variant, T, hipMemcpyDeviceToHost));
  if (child_terminal) SB_TRY(hipMemcpy(child_terminal, s->fr.child_terminal, T, hipMemcpyDeviceToHost));
  if (child_scores) SB_TRY(hipMemcpy(child_scores, s->fr.child_scores, T * V * 4, hipMemcpyDeviceToHost));
  return AZMI_OK;
}

}  // extern "C"
