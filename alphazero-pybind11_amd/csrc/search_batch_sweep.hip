// Batched position search, the visit sweep: azmi_search_run_to searches every tree to its own root_n target and snapshots the
// read-outs at checkpoints on the way (mcts_analysis.py:884-972, 975-1063); azmi_search_sweep_metrics scores the snapshot set
// against its anchor checkpoint, the second half of mcts_analysis.py:run_analysis; azmi_policy_divergences is the same row
// function over any [rows, M] pair of HOST policies.  Host code only: the kernels and their launch functions are in
// search_batch.hip's device module (search_batch_host.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "search_batch_host.h"

using namespace azmi;

namespace {

// room for `j` checkpoints in the snapshot block (sb_cut_sweep); a block grown for more checkpoints serves fewer
int sweep_reserve(azmi_search* s, uint32_t j) {
  const size_t N = s->n, M = s->pm->gi.M;
  if (!s->sw_block.p || j > s->sw_cap) {
    const size_t cap = std::max<uint32_t>(j, 1u);
    BlockCut size;
    SbSweepArrays sized{};
    sb_cut_sweep(size, sized, N, M, cap);
    SB_TRY(s->sw_block.reserve(size.off));
    BlockCut cut(s->sw_block.p);
    s->sw_clear_bytes = sb_cut_sweep(cut, s->sw, N, M, cap);
    s->sw_cap = static_cast<uint32_t>(cap);
  }
  s->sw.n_cp = j;
  return AZMI_OK;
}

// the output block of azmi_search_sweep_metrics (sb_cut_sweep_metrics) with room for `j` checkpoints
int sweep_metrics_reserve(azmi_search* s, uint32_t j, SweepMetricsOut* o) {
  const size_t N = s->n;
  if (!s->sm_block.p || j > s->sm_cap) {
    const size_t cap = std::max<uint32_t>(j, 1u);
    BlockCut size;
    sb_cut_sweep_metrics(size, *o, N, cap);
    SB_TRY(s->sm_block.reserve(size.off));
    s->sm_cap = static_cast<uint32_t>(cap);
  }
  BlockCut cut(s->sm_block.p);
  sb_cut_sweep_metrics(cut, *o, N, s->sm_cap);
  return AZMI_OK;
}

}  // namespace

extern "C" {

int azmi_search_run_to(azmi_search* s, int eval_type, azmi_net* net, azmi_cache* cache, const uint32_t* targets, const uint32_t* checkpoints,
                       uint32_t n_checkpoints, float temp, int pruned, int root_noise_enabled, void* stream) {
  int rc = sb_begin_step(s, "search_to"); if (rc) return rc;
  if (s->step_pending) return SB_FAIL(AZMI_ERR_STATE, "search_to: a find_leaves step is pending; call process_results first");
  if (!targets || (n_checkpoints && !checkpoints)) return SB_FAIL(AZMI_ERR_INVALID, "null argument");
  if (s->dl_L > 1)
    return SB_FAIL(AZMI_ERR_INVALID, "search_to with descents_per_step = %u: the checkpoint launches are planned from one root_n read and one "
                   "descent of every tree per step; use search(visits), or descents_per_step = 1", s->dl_L);
  if (s->gumbel)
    return SB_FAIL(AZMI_ERR_INVALID, "search_to on a Gumbel batch: sequential halving plans a fixed budget at its first descent, and a "
                   "root_n target on a reused tree is not one; use search(visits)");
  if (n_checkpoints > kSbMaxCheckpoints) return SB_FAIL(AZMI_ERR_INVALID, "search_to: at most %u checkpoints, got %u", kSbMaxCheckpoints, n_checkpoints);
  for (uint32_t j = 0; j < n_checkpoints; ++j)
    if (checkpoints[j] == 0 || (j && checkpoints[j] <= checkpoints[j - 1]))
      return SB_FAIL(AZMI_ERR_INVALID, "search_to: checkpoints must be positive and strictly ascending (checkpoint %u is %u)", j, checkpoints[j]);
  SbSearchArgs a;
  rc = sb_search_args(s, "search_to", eval_type, net, cache, &a); if (rc) return rc;
  azmi_pm* pm = s->pm;
  SB_TRY(hipSetDevice(pm->device));
  hipStream_t prev = pm->last;
  hipStream_t st = pm->pick(stream);
  if (prev != st) SB_TRY(hipStreamSynchronize(prev));      // the previous call's upload may still read sw_upload
  const uint32_t n = s->n, K = s->k_leaves, J = n_checkpoints;
  // the one read of the call: root_n (kind-5 read-out, column 1) and the status of every tree.  `launches` counts what the call
  // enqueues behind it
  std::vector<uint32_t> r(n);
  std::vector<int32_t> status(n);
  sb_launch_query_scalars(s, st);
  s->launches -= 1;
  SB_TRY(hipGetLastError());
  SB_TRY(hipMemcpy2DAsync(r.data(), 4, s->d_qu + 1, static_cast<size_t>(s->vec_u) * 4, 4, n, hipMemcpyDeviceToHost, st));
  SB_TRY(hipMemcpyAsync(status.data(), s->sb.status, static_cast<size_t>(n) * 4, hipMemcpyDeviceToHost, st));
  SB_TRY(hipStreamSynchronize(st));
  // root_n rises by exactly one per backed-up simulation, so tree i holds r[i] + t * K after step t until it reaches its target,
  // at step ceil(rem / K): the steps at which a tree newly reaches a checkpoint or its target are known here
  uint32_t T = 0;
  for (uint32_t i = 0; i < n; ++i)
    if (status[i] == 0 && targets[i] > r[i]) T = std::max(T, (targets[i] - r[i] + K - 1) / K);
  rc = sb_check_budget(s, "search_to", static_cast<uint64_t>(T) * K); if (rc) return rc;
  std::vector<uint8_t> event(static_cast<size_t>(T) + 1, 0);
  for (uint32_t i = 0; i < n; ++i) {
    if (status[i] != 0) continue;
    const uint32_t ti = targets[i] > r[i] ? (targets[i] - r[i] + K - 1) / K : 0u;
    if (T) event[ti] = 1;      // the pause (with T == 0 no step follows that a pause could keep a tree out of)
    for (uint32_t j = 0; j < J; ++j) {
      const uint32_t tj = checkpoints[j] > r[i] ? (checkpoints[j] - r[i] + K - 1) / K : 0u;
      if (tj <= ti) event[tj] = 1;
    }
  }
  if (T) event[T] = 1;         // the resume
  rc = sweep_reserve(s, J); if (rc) return rc;
  s->sw_upload.assign(targets, targets + n);
  if (J) s->sw_upload.insert(s->sw_upload.end(), checkpoints, checkpoints + J);
  s->sw_upload.resize(static_cast<size_t>(n) + kSbMaxCheckpoints, 0u);
  SB_TRY(hipMemsetAsync(s->sw_block.p, 0, s->sw_clear_bytes, st));
  SB_TRY(hipMemcpyAsync(s->sw.target, s->sw_upload.data(), s->sw_upload.size() * 4, hipMemcpyHostToDevice, st));
  s->sw_valid = true;
  if (T == 0 && !event[0]) return AZMI_OK;
  const uint32_t rn = root_noise_enabled ? 1u : 0u, pr = pruned ? 1u : 0u;
  // from the first checkpoint launch on a tree may be paused: every way out goes through a launch that resumes
  rc = AZMI_OK;
  for (uint32_t t = 0; t < T && rc == AZMI_OK; ++t) {
    if (event[t]) sb_launch_checkpoint(s, temp, pr, 0u, st);
    rc = sb_enqueue_step(s, a, K, rn, st);
    if (rc == AZMI_OK) s->sims_done += K;
  }
  sb_launch_checkpoint(s, temp, pr, 1u, st);
  if (rc != AZMI_OK) return rc;
  SB_TRY(hipGetLastError());
  return AZMI_OK;
}

int azmi_search_checkpoints(azmi_search* s, uint32_t* taken_mask, uint32_t* root_n, uint32_t* counts, float* probs, float* root_values,
                            float* root_q) {
  int rc = sb_begin_read(s, "checkpoints"); if (rc) return rc;
  if (!s->sw_valid) return SB_FAIL(AZMI_ERR_STATE, "checkpoints: no search_to call has been made on this batch");
  azmi_pm* pm = s->pm;
  SB_TRY(hipSetDevice(pm->device));
  rc = sb_check_device(s, pm->last); if (rc) return rc;      // (synchronises)
  const size_t N = s->n, J = s->sw.n_cp, M = pm->gi.M;
  if (taken_mask) SB_TRY(hipMemcpy(taken_mask, s->sw.taken, N * 4, hipMemcpyDeviceToHost));
  if (!J) return AZMI_OK;
  if (root_n) SB_TRY(hipMemcpy(root_n, s->sw.root_n, N * J * 4, hipMemcpyDeviceToHost));
  if (counts) SB_TRY(hipMemcpy(counts, s->sw.counts, N * J * M * 4, hipMemcpyDeviceToHost));
  if (probs) SB_TRY(hipMemcpy(probs, s->sw.probs, N * J * M * 4, hipMemcpyDeviceToHost));
  if (root_values) SB_TRY(hipMemcpy(root_values, s->sw.root_values, N * J * 3 * 4, hipMemcpyDeviceToHost));
  if (root_q) SB_TRY(hipMemcpy(root_q, s->sw.root_q, N * J * M * 4, hipMemcpyDeviceToHost));
  return AZMI_OK;
}

int azmi_search_sweep_metrics(azmi_search* s, azmi_search* ref, uint32_t anchor, int32_t raw, const double* outcomes, double* out_rows,
                              double* out_tree, double* out_mean, uint32_t* out_count, uint8_t* valid, void* stream) {
  int rc = sb_begin_move(s, "sweep_metrics"); if (rc) return rc;
  if (!ref) ref = s;
  if (!s->sw_valid) return SB_FAIL(AZMI_ERR_STATE, "sweep_metrics: no search_to call has been made on this batch");
  if (!ref->sw_valid) return SB_FAIL(AZMI_ERR_STATE, "sweep_metrics: no search_to call has been made on the reference batch");
  if (ref->step_pending) return SB_FAIL(AZMI_ERR_STATE, "sweep_metrics: a find_leaves step is pending on the reference batch; call process_results first");
  if (ref->pm->game != s->pm->game || ref->n != s->n || ref->pm->device != s->pm->device)
    return SB_FAIL(AZMI_ERR_INVALID, "sweep_metrics: the reference batch must hold the same game, tree count and device (game %d, %u trees, "
                   "device %d against game %d, %u trees, device %d)", ref->pm->game, ref->n, ref->pm->device, s->pm->game, s->n, s->pm->device);
  const uint32_t J = s->sw.n_cp, Jr = ref->sw.n_cp;
  if (anchor >= Jr) return SB_FAIL(AZMI_ERR_INVALID, "sweep_metrics: anchor %u out of range: the reference set has %u checkpoints", anchor, Jr);
  if (raw < -1 || (raw >= 0 && static_cast<uint32_t>(raw) >= Jr))
    return SB_FAIL(AZMI_ERR_INVALID, "sweep_metrics: raw %d out of range: -1 for none, or one of the reference set's %u checkpoints", raw, Jr);
  azmi_pm* pm = s->pm;
  SB_TRY(hipSetDevice(pm->device));
  hipStream_t prev = pm->last;
  hipStream_t st = pm->pick(stream);
  if (prev != st) SB_TRY(hipStreamSynchronize(prev));                              // the snapshots may still be on their way
  if (ref != s && ref->pm->last != st) SB_TRY(hipStreamSynchronize(ref->pm->last));
  SweepMetricsOut o;
  rc = sweep_metrics_reserve(s, J, &o); if (rc) return rc;
  const size_t N = s->n;
  if (outcomes) SB_TRY(hipMemcpyAsync(o.outcomes, outcomes, N * 8, hipMemcpyHostToDevice, st));
  sb_launch_sweep_metrics(s, ref, anchor, raw, outcomes ? o.outcomes : nullptr, o, st);
  sb_launch_sweep_mean(s, J, o, st);
  SB_TRY(hipGetLastError());
  if (out_tree) SB_TRY(hipMemcpyAsync(out_tree, o.ceiling, N * 8, hipMemcpyDeviceToHost, st));
  if (J) {
    if (out_rows) SB_TRY(hipMemcpyAsync(out_rows, o.rows, N * J * kSweepCols * 8, hipMemcpyDeviceToHost, st));
    if (out_mean) SB_TRY(hipMemcpyAsync(out_mean, o.mean, static_cast<size_t>(J) * kSweepCols * 8, hipMemcpyDeviceToHost, st));
    if (out_count) SB_TRY(hipMemcpyAsync(out_count, o.count, static_cast<size_t>(J) * kSweepCols * 4, hipMemcpyDeviceToHost, st));
    if (valid) SB_TRY(hipMemcpyAsync(valid, o.valid, N * J, hipMemcpyDeviceToHost, st));
  }
  return sb_check_device(s, st);      // the one synchronisation
}

int azmi_policy_divergences(const float* p, const float* q, uint32_t rows, uint32_t M, double* out, int device, void* stream) {
  constexpr uint32_t kMaxRows = 1u << 30, kMaxMoves = 1u << 20;
  if (rows > kMaxRows || M == 0 || M > kMaxMoves)
    return SB_FAIL(AZMI_ERR_INVALID, "azmi_policy_divergences: rows = %u, M = %u: at most %u rows of 1 to %u moves", rows, M, kMaxRows, kMaxMoves);
  if (rows && (!p || !q || !out)) return SB_FAIL(AZMI_ERR_INVALID, "azmi_policy_divergences: null argument");
  if (rows == 0) return AZMI_OK;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return SB_FAIL(AZMI_ERR_NO_DEVICE, "no HIP device: libazmi has no CPU path");
  if (device < 0 || device >= ndev) return SB_FAIL(AZMI_ERR_INVALID, "device %d out of range", device);
  SB_TRY(hipSetDevice(device));
  hipStream_t st = stream == AZMI_STREAM_ENGINE ? nullptr : static_cast<hipStream_t>(stream);
  const size_t cells = static_cast<size_t>(rows) * M;
  DevTemps tmp;
  float *d_p = nullptr, *d_q = nullptr;
  double* d_out = nullptr;
  AZMI_HIP_TRY_NODEV(tmp.upload_async(d_p, p, cells, st));
  hipError_t e = tmp.upload_async(d_q, q, cells, st);
  if (e == hipSuccess) e = tmp.alloc(d_out, static_cast<size_t>(rows) * kPolicyCols);
  if (e == hipSuccess) {
    sb_launch_policy_divergences(d_p, d_q, rows, M, d_out, st);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, static_cast<size_t>(rows) * kPolicyCols * 8, hipMemcpyDeviceToHost, st);
  const hipError_t es = hipStreamSynchronize(st);      // always: what was queued reads the buffers tmp is about to free
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return SB_FAIL(e == hipErrorOutOfMemory ? AZMI_ERR_OOM : AZMI_ERR_NO_DEVICE, "azmi_policy_divergences: %s", hipGetErrorString(e));
  return AZMI_OK;
}

}  // extern "C"
