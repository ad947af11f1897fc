// The diagnostic entry points of the pipeline (azmi_debug_*): duplicate requests in the last epoch's insert log, the lane-group
// primitives of the descent and expand_node on their own, the net side draining a ring alone.  Host code only: their kernels
// (pipe_debug_kernels.h) and launch functions are in pipeline.hip's device module (pipeline_host.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <utility>
#include <vector>

#include "dev_games.h"
#include "pipeline_host.h"

using namespace azmi;

// ---- diagnostics: how many of the last epoch's answers were asked for more than once --------------------------------------------
// The insert log holds the key of every answer the tree side consumed in the last epoch of the last azmi_run_pipeline call.  A key that
// is there k times went to the net k times inside one epoch - k - 1 evaluations an insert at answer time (the reference's,
// play_manager.cc:631-640) or a table of requests in flight would have saved.  out[0] = entries, out[1] = entries beyond the first
// of their key, out[2] = of those, the ones whose twin sits within 4096 log entries (~ in flight together).
extern "C" int azmi_debug_pipe_log_dupes(azmi_pm* pm, uint64_t* out) {
  if (!pm || !out || !pm->pipe) return azmi_host_fail(AZMI_ERR_INVALID, "no pipeline on this engine");
  std::lock_guard<std::recursive_mutex> lock_(pm->mu);
  PipeState* ps = pm->pipe;
  AZMI_HIP_TRY(hipSetDevice(pm->device));
  AZMI_HIP_TRY(hipDeviceSynchronize());
  PipeEpoch he;
  AZMI_HIP_TRY(hipMemcpy(&he, ps->pa.ep, sizeof(he), hipMemcpyDeviceToHost));
  const uint32_t n = std::min(he.ins_count, ps->pa.ins_cap);
  std::vector<uint64_t> keys(n);
  if (n) AZMI_HIP_TRY(hipMemcpy(keys.data(), ps->pa.ins_key, sizeof(uint64_t) * n, hipMemcpyDeviceToHost));
  std::vector<std::pair<uint64_t, uint32_t>> kv(n);
  for (uint32_t i = 0; i < n; ++i) kv[i] = {keys[i], i};
  std::sort(kv.begin(), kv.end());
  uint64_t dup = 0, near = 0;
  for (uint32_t i = 1; i < n; ++i)
    if (kv[i].first == kv[i - 1].first) { ++dup; if (kv[i].second - kv[i - 1].second < 4096u) ++near; }
  out[0] = n; out[1] = dup; out[2] = near;
  return AZMI_OK;
}

extern "C" int azmi_debug_group_select(int device, uint32_t rows, const uint32_t* k8, const uint32_t* n64, const float* q64, const float* p64,
                                       const float* v_parent8, const uint32_t* n_parent8, const float* fpu8, const float* cpuct8, const uint64_t* pred,
                                       float* sum64, uint32_t* best64, uint32_t* all64) {
  using namespace azmi;
  if (!k8 || !n64 || !q64 || !p64 || !v_parent8 || !n_parent8 || !fpu8 || !cpuct8 || !pred || !sum64 || !best64 || !all64)
    return azmi_host_fail(AZMI_ERR_INVALID, "azmi_debug_group_select: null buffer");
  if (rows == 0u || rows > 65536u) return azmi_host_fail(AZMI_ERR_INVALID, "azmi_debug_group_select: rows must be 1 .. 65536");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return azmi_host_fail(AZMI_ERR_NO_DEVICE, "no HIP device: libazmi has no CPU path");
  AZMI_HIP_TRY(hipSetDevice(device));
  // one allocation: eight per-group / per-lane inputs, the predicate words, three per-lane outputs (4-byte words; the predicates 8)
  const size_t n8 = static_cast<size_t>(rows) * 8u, n64w = static_cast<size_t>(rows) * 64u;
  const size_t words = 5u * n8 + 3u * n64w + 2u * rows + 3u * n64w;
  uint32_t* d = nullptr;
  AZMI_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d), words * 4u));
  unsigned long long* const d_pred = reinterpret_cast<unsigned long long*>(d);      // (first: 8-byte aligned)
  uint32_t* const d_k = d + 2u * rows; uint32_t* const d_npar = d_k + n8;
  float* const d_vpar = reinterpret_cast<float*>(d_npar + n8); float* const d_fpu = d_vpar + n8; float* const d_cpuct = d_fpu + n8;
  uint32_t* const d_n = reinterpret_cast<uint32_t*>(d_cpuct + n8);
  float* const d_q = reinterpret_cast<float*>(d_n + n64w); float* const d_p = d_q + n64w;
  float* const d_sum = d_p + n64w; uint32_t* const d_best = reinterpret_cast<uint32_t*>(d_sum + n64w); uint32_t* const d_all = d_best + n64w;
  hipError_t e = hipMemcpy(d_pred, pred, rows * 8u, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_k, k8, n8 * 4u, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_npar, n_parent8, n8 * 4u, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_vpar, v_parent8, n8 * 4u, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_fpu, fpu8, n8 * 4u, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_cpuct, cpuct8, n8 * 4u, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_n, n64, n64w * 4u, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_q, q64, n64w * 4u, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_p, p64, n64w * 4u, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    pipe_launch_debug_group_select(rows, d_k, d_n, d_q, d_p, d_vpar, d_npar, d_fpu, d_cpuct, d_pred, d_sum, d_best, d_all);
    e = hipDeviceSynchronize();
  }
  if (e == hipSuccess) e = hipMemcpy(sum64, d_sum, n64w * 4u, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(best64, d_best, n64w * 4u, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(all64, d_all, n64w * 4u, hipMemcpyDeviceToHost);
  (void)hipFree(d);
  if (e != hipSuccess) return azmi_host_fail(AZMI_ERR_NO_DEVICE, "azmi_debug_group_select: %s", hipGetErrorString(e));
  return AZMI_OK;
}

extern "C" int azmi_debug_group_expand(int device, uint32_t lane_pack, uint32_t rows, uint32_t reps, uint32_t cap, const uint64_t* bb0, const uint64_t* bb1,
                                       const uint32_t* player, const uint64_t* rng_in, uint32_t* words, uint64_t* rng_out, void* nodes_out) {
  using namespace azmi;
  if (!bb0 || !bb1 || !player || !rng_in || !words || !rng_out || !nodes_out) return azmi_host_fail(AZMI_ERR_INVALID, "azmi_debug_group_expand: null buffer");
  if (rows == 0u || rows > 4096u || reps == 0u || reps > 64u) return azmi_host_fail(AZMI_ERR_INVALID, "azmi_debug_group_expand: rows must be 1 .. 4096, reps 1 .. 64");
  if (cap < reps + reps * 8u || cap > 65536u) return azmi_host_fail(AZMI_ERR_INVALID, "azmi_debug_group_expand: cap must hold the parents and eight children each (%u .. 65536)", reps + reps * 8u);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return azmi_host_fail(AZMI_ERR_NO_DEVICE, "no HIP device: libazmi has no CPU path");
  AZMI_HIP_TRY(hipSetDevice(device));
  const size_t slots = static_cast<size_t>(rows) * 8u, calls = slots * reps, lanes = calls * 8u;
  const size_t node_bytes = slots * Connect4::P * cap * sizeof(NodeRec);
  NodeRec* d_nodes = nullptr; Control* d_ctl = nullptr; uint64_t* d_in = nullptr; uint32_t* d_player = nullptr; uint64_t* d_rng_out = nullptr; uint32_t* d_words = nullptr;
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&d_nodes), node_bytes);
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d_ctl), sizeof(Control));
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d_in), calls * 8u * 3u);          // bb0, bb1, rng_in
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d_player), calls * 4u);
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d_rng_out), lanes * 8u);
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d_words), lanes * 16u);
  if (e == hipSuccess) e = hipMemset(d_nodes, 0xAB, node_bytes);        // (what expand_node does not write stays recognisable)
  if (e == hipSuccess) e = hipMemset(d_ctl, 0, sizeof(Control));
  if (e == hipSuccess) e = hipMemset(d_words, 0xFF, lanes * 16u);
  if (e == hipSuccess) e = hipMemset(d_rng_out, 0xFF, lanes * 8u);
  if (e == hipSuccess) e = hipMemcpy(d_in, bb0, calls * 8u, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_in + calls, bb1, calls * 8u, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_in + 2u * calls, rng_in, calls * 8u, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_player, player, calls * 4u, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    pipe_launch_debug_group_expand(lane_pack != 0u, rows, reps, cap, d_nodes, d_ctl, d_in, d_in + calls, d_player, d_in + 2u * calls, d_words, d_rng_out);
    e = hipDeviceSynchronize();
  }
  if (e == hipSuccess) e = hipMemcpy(words, d_words, lanes * 16u, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(rng_out, d_rng_out, lanes * 8u, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(nodes_out, d_nodes, node_bytes, hipMemcpyDeviceToHost);
  (void)hipFree(d_nodes); (void)hipFree(d_ctl); (void)hipFree(d_in); (void)hipFree(d_player); (void)hipFree(d_rng_out); (void)hipFree(d_words);
  if (e != hipSuccess) return azmi_host_fail(AZMI_ERR_NO_DEVICE, "azmi_debug_group_expand: %s", hipGetErrorString(e));
  return AZMI_OK;
}

// Fills the request ring with `n` synthetic positions (n <= the ring) and lets the persistent net kernel alone drain it, `reps`
// times; ms_out = average milliseconds per drain (HIP events).  mode: the tile selection of k_pipe_net (0 both, 1 six-board, 2
// three-board).  Timing only: the slots' result granules are overwritten.
extern "C" int azmi_debug_pipe_net_bench(azmi_pm* pm, azmi_net* net, uint32_t n, uint32_t reps, uint32_t net_wgs, int mode, float* ms_out) {
  if (!pm || !net || !ms_out) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  if (mode == 3) return pipe_no_conveyor();
  std::lock_guard<std::recursive_mutex> lock_(pm->mu);
  azmi_net* nets_[2] = {net, net};
  const PipePlan plan_ = pipe_plan(pm, nets_, 2);
  if (plan_.kind == 0 || plan_.tree_only) return azmi_host_fail(AZMI_ERR_STATE, "not a pipeline engine");
  const azmi_net_c4_view view = plan_.view[0];
  if (n > kPipeRing) return azmi_host_fail(AZMI_ERR_INVALID, "at most %u requests", kPipeRing);
  AZMI_HIP_TRY(hipSetDevice(pm->device));
  if (!pm->pipe) { const int rc = pipe_create(pm); if (rc != AZMI_OK) return rc; }
  PipeState* ps = pm->pipe;
  PipeArrays& pa = ps->pa;
  { const int rc = pipe_size_net(pm, ps, view); if (rc != AZMI_OK) return rc; }
  pa.cap_ticks = 25000000ull;
  hipStream_t st = pm->stream;
  hipEvent_t e0, e1;
  AZMI_HIP_TRY(hipEventCreate(&e0)); AZMI_HIP_TRY(hipEventCreate(&e1));
  float total = 0.0f;
  const uint32_t wgs = net_wgs ? net_wgs : ps->net_wgs;
  for (uint32_t r = 0; r < reps + 1; ++r) {
    AZMI_HIP_TRY(hipMemsetAsync(pa.ep, 0, sizeof(PipeEpoch), st));
    pipe_launch_fill(pa, n, pm->ep.S, 1234 + r, st);
    AZMI_HIP_TRY(hipEventRecord(e0, st));
    { const int rc = pipe_launch_net(ps, view, mode, wgs, st, pa); if (rc != AZMI_OK) return rc; }
    AZMI_HIP_TRY(hipEventRecord(e1, st));
    pipe_launch_head_reset(pa, st);                // (head = tail for the next drain; the READY tokens of the synthetic answers are dropped)
    AZMI_HIP_TRY(hipStreamSynchronize(st));
    float ms = 0.0f;
    AZMI_HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    if (r > 0) total += ms;
  }
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  // the synthetic answers carry sequence numbers a real request of the same slot could draw later: wipe the granules
  AZMI_HIP_TRY(hipMemsetAsync(pa.res, 0, sizeof(unsigned long long) * static_cast<size_t>(pm->ep.S) * kResStride, st));
  AZMI_HIP_TRY(hipStreamSynchronize(st));
  *ms_out = total / static_cast<float>(reps);
  PipeCtl hc;
  AZMI_HIP_TRY(hipMemcpy(&hc, pa.ctl, sizeof(hc), hipMemcpyDeviceToHost));
  if (hc.err) {
    (void)hipMemset(&pa.ctl->err, 0, sizeof(uint32_t));
    return azmi_host_fail(AZMI_ERR_STATE, "pipeline error mask 0x%x in the net drain", hc.err);
  }
  return AZMI_OK;
}
