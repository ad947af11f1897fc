// The host-buffer compatibility path of one PlayManager engine (build_batch / update_inferences of the reference's callers): rounds
// until some leaf waits for a net, its planes handed out to host memory, the answers taken back row by row.  Host code only: the
// round is launched through engine.hip (engine_host.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <deque>
#include <mutex>
#include <vector>

#include "../../include/azmi.h"
#include "engine_host.h"

using namespace azmi;

extern "C" {

// ---- host-buffer compatibility path ------------------------------------------------------------------
int azmi_pm_build_batch(azmi_pm* pm, float* batch, uint32_t cap, uint32_t* indices, uint32_t* n) {
  return azmi_pm_build_batch_group(pm, 0xFFFFFFFFu, batch, cap, indices, n);
}

// group == 0xFFFFFFFF: leaves of any model group (single-evaluator callers)
int azmi_pm_build_batch_group(azmi_pm* pm, uint32_t group, float* batch, uint32_t cap, uint32_t* indices, uint32_t* n) {
  if (!pm || !indices || !n) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");   // batch == NULL: pop_games_upto (indices only)
  std::lock_guard<std::recursive_mutex> lock_(pm->mu);
  *n = 0;
  if (cap == 0 || pm->stopped.load(std::memory_order_relaxed)) return AZMI_OK;
  if (group != 0xFFFFFFFFu && group >= pm->ep.num_groups) return azmi_host_fail(AZMI_ERR_INVALID, "model group %u out of range", group);
  const uint32_t S = pm->ep.S, CANON = pm->gi.C * pm->gi.H * pm->gi.W;
  hipStream_t st = pm->pick(AZMI_STREAM_ENGINE);
  int guard = 0;
  auto any_pending = [&]() { for (auto& q : pm->pending_g) if (!q.empty()) return true; return false; };
  auto mine = [&]() -> std::deque<uint32_t>* {
    if (group != 0xFFFFFFFFu) return pm->pending_g[group].empty() ? nullptr : &pm->pending_g[group];
    for (auto& q : pm->pending_g) if (!q.empty()) return &q;
    return nullptr;
  };
  while (!any_pending()) {
    if (pm->outstanding != 0) return AZMI_OK;  // rows handed out, answers not back yet
    Control c;
    int rc = azmi_host_read_ctl(pm, st, &c, true); if (rc) return rc;
    if (c.stop) return AZMI_OK;
    rc = azmi_host_launch_round(pm, st); if (rc) return rc;
    // the round's eval lists name exactly the leaves that need a network answer, per model group (a slot whose
    // last leaf was a cache hit or terminal is not listed); sorted so the hand-out order is deterministic
    Control c2;
    rc = azmi_host_read_ctl(pm, st, &c2, false); if (rc) return rc;
    for (uint32_t g = 0; g < pm->ep.num_groups; ++g) {
      const uint32_t cnt = std::min<uint32_t>(c2.eval_count[g], S);
      if (cnt == 0) continue;
      std::vector<uint32_t> lst;
      rc = d2h(lst, pm->ar.eval_list + static_cast<size_t>(g) * S, cnt, st); if (rc) return rc;
      std::sort(lst.begin(), lst.end());
      for (uint32_t sidx : lst) pm->pending_g[g].push_back(sidx);
    }
    if (++guard > (1 << 20)) return azmi_host_fail(AZMI_ERR_STATE, "build_batch made no progress");
  }
  std::deque<uint32_t>* q = mine();
  if (!q) return AZMI_OK;   // other groups have pending leaves, this one has none right now
  const uint32_t take = std::min<uint32_t>(cap, static_cast<uint32_t>(q->size()));
  for (uint32_t r = 0; r < take; ++r) {
    const uint32_t s = q->front();
    q->pop_front();
    indices[r] = s;
    if (batch) AZMI_HIP_TRY(hipMemcpyAsync(batch + static_cast<size_t>(r) * CANON, pm->ar.canon + static_cast<size_t>(s) * CANON,
                           CANON * 4, hipMemcpyDeviceToHost, st));
  }
  AZMI_HIP_TRY(hipStreamSynchronize(st));
  pm->outstanding += take;
  *n = take;
  return AZMI_OK;
}

int azmi_pm_update_inferences(azmi_pm* pm, const uint32_t* indices, uint32_t n, const float* v, const float* pi) {
  if (!pm || (n && (!indices || !v || !pi))) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  std::lock_guard<std::recursive_mutex> lock_(pm->mu);
  const uint32_t S = pm->ep.S, V = pm->gi.P + 1, M = pm->gi.M;
  if (n > pm->outstanding) return azmi_host_fail(AZMI_ERR_STATE, "update_inferences: more rows than build_batch handed out");
  // rows go straight to the slot-indexed device buffers: rows of other slots (cache hits written by the round
  // kernel) must not be touched, so there is no whole-buffer mirror upload
  for (uint32_t r = 0; r < n; ++r) {
    if (indices[r] >= S) return azmi_host_fail(AZMI_ERR_INVALID, "slot index out of range");
    AZMI_HIP_TRY(hipMemcpyAsync(pm->ar.v + static_cast<size_t>(indices[r]) * V, v + static_cast<size_t>(r) * V, V * 4, hipMemcpyHostToDevice, pm->stream));
    AZMI_HIP_TRY(hipMemcpyAsync(pm->ar.pi + static_cast<size_t>(indices[r]) * M, pi + static_cast<size_t>(r) * M, M * 4, hipMemcpyHostToDevice, pm->stream));
  }
  AZMI_HIP_TRY(hipStreamSynchronize(pm->stream));
  pm->outstanding -= n;
  return AZMI_OK;
}

}  // extern "C"
