// The lock-step round loop of one PlayManager engine: a round, the net on its leaf batch, the fused net + move-step launch of a
// split round, the hipGraph of azmi_run_rounds, play() for RANDOM seats, poll.  Host code only: every kernel is launched through
// engine.hip (engine_host.h).
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <mutex>

#include "../../include/azmi.h"
#include "engine_host.h"
#include "leafnet_c4_types.h"

using namespace azmi;

int azmi_host_read_ctl(azmi_pm* pm, hipStream_t st, Control* out, bool settle) {
  if (settle) azmi_host_launch_settle(pm, st);
  AZMI_HIP_TRY(hipMemcpyAsync(out, pm->ar.ctl, sizeof(Control), hipMemcpyDeviceToHost, st));
  AZMI_HIP_TRY(hipStreamSynchronize(st));
  if (out->overflow)
    return azmi_host_fail(AZMI_ERR_OVERFLOW, "device engine stopped: overflow mask 0x%x (1 tree arena, 2 history, 4 move log, "
                          "8 path/children, 16 pick_move, 32 unknown move, 64 illegal move)", out->overflow);
  return AZMI_OK;
}

extern "C" {

int azmi_pm_round(azmi_pm* pm, void* stream) {
  if (!pm) return azmi_host_fail(AZMI_ERR_INVALID, "null pm");
  std::lock_guard<std::recursive_mutex> lock_(pm->mu);
  return azmi_host_launch_round(pm, pm->pick(stream));
}

namespace {
constexpr uint32_t kGraphRounds = 16;
// the net on this engine's leaf batch: only the rows k_round listed (Connect4 engine), else the whole batch
int pm_net_forward(azmi_pm* pm, uint32_t group, azmi_net* net, hipStream_t st) {
  int rc;
  if (pm->game == AZMI_GAME_CONNECT4 || pm->ep.num_groups > 1 || pm->ep.cache_on)
    rc = azmi_net_forward_rows(net, pm->ar.canon, pm->ar.v, pm->ar.pi, pm->ar.eval_list + static_cast<size_t>(group) * pm->ep.S,
                               &pm->ar.ctl->eval_count[group], pm->ep.S, st);
  else
    rc = azmi_net_forward(net, pm->ar.canon, pm->ar.v, pm->ar.pi, pm->ep.S, st);
  if (rc != AZMI_OK) return azmi_host_fail(rc, "%s", azmi_net_last_error());
  return AZMI_OK;
}
// split round + a Connect4-family bf16 net + one model group: the move step rides in the net launch (k_net_move)
bool can_fuse(const azmi_pm* pm, const azmi_net* net, azmi_net_c4_view* view) {
  return pm->split_rounds && pm->ep.num_groups == 1 && !pm->all_random && getenv("AZMI_NO_FUSE") == nullptr && azmi_net_c4_view_get(net, view) != 0 && view->x3 == 0;
}
int one_round_with_net(azmi_pm* pm, azmi_net* net, hipStream_t st) {
  azmi_net_c4_view view;
  if (can_fuse(pm, net, &view)) {
    const int rc = azmi_host_launch_round(pm, st, true);
    return rc != AZMI_OK ? rc : azmi_host_launch_net_move(pm, view, st);
  }
  int rc = azmi_host_launch_round(pm, st);
  if (rc != AZMI_OK) return rc;
  for (uint32_t g = 0; g < pm->ep.num_groups; ++g) {   // one net given: it serves every model group
    rc = pm_net_forward(pm, g, net, st);
    if (rc != AZMI_OK) return rc;
  }
  return AZMI_OK;
}
int ensure_graph(azmi_pm* pm, azmi_net* net, hipStream_t st) {
  if (pm->graph_exec && pm->graph_stream == st && pm->graph_net == net) return AZMI_OK;
  if (pm->graph_exec) { (void)hipGraphExecDestroy(pm->graph_exec); pm->graph_exec = nullptr; }
  hipGraph_t graph = nullptr;
  if (azmi_net_reserve_stream(net, st, pm->ep.S) != AZMI_OK) return azmi_host_fail(AZMI_ERR_OOM, "%s", azmi_net_last_error());
  AZMI_HIP_TRY(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
  int rc = AZMI_OK;
  for (uint32_t r = 0; r < kGraphRounds && rc == AZMI_OK; ++r) rc = one_round_with_net(pm, net, st);
  const hipError_t e = hipStreamEndCapture(st, &graph);
  if (rc != AZMI_OK) { if (graph) (void)hipGraphDestroy(graph); return rc; }
  if (e != hipSuccess) return azmi_host_fail(AZMI_ERR_NO_DEVICE, "hipStreamEndCapture: %s", hipGetErrorString(e));
  const hipError_t e2 = hipGraphInstantiate(&pm->graph_exec, graph, nullptr, nullptr, 0);
  (void)hipGraphDestroy(graph);
  if (e2 != hipSuccess) { pm->graph_exec = nullptr; return azmi_host_fail(AZMI_ERR_NO_DEVICE, "hipGraphInstantiate: %s", hipGetErrorString(e2)); }
  pm->graph_stream = st;
  pm->graph_net = net;
  return AZMI_OK;
}
}  // namespace

int azmi_run_rounds(azmi_pm* const* pms, azmi_net* net, uint32_t k, uint32_t rounds, void* const* streams) {
  if (!pms || !net || !streams || k == 0) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  for (uint32_t i = 0; i < k; ++i)      // PlayManager::stop(): the workers leave their loop (play_manager.cc:272)
    if (pms[i] && pms[i]->stopped.load(std::memory_order_relaxed)) return AZMI_OK;
  if (const char* sg = getenv("AZMI_STAGGER_US")) {     // experiment: odd shards start half a cycle late
    const uint32_t us = static_cast<uint32_t>(atoi(sg));
    for (uint32_t i = 1; i < k && us; i += 2) azmi_host_launch_delay(us, pms[i]->pick(streams[i]));
  }
  // hipGraph replay of 16 rounds per launch is available (AZMI_GRAPH=1) but off by default: measured equal to plain
  // launches on this workload (2300 vs 2304 games/s — the host is ahead of the GPU either way), and capturing and
  // instantiating a graph per engine costs about a second at start-up
  const bool use_graph = getenv("AZMI_GRAPH") != nullptr && getenv("AZMI_NO_GRAPH") == nullptr;
  uint32_t done = 0;
  if (use_graph) {
    for (uint32_t i = 0; i < k; ++i) {
      const int rc = ensure_graph(pms[i], net, pms[i]->pick(streams[i]));
      if (rc != AZMI_OK) return rc;
    }
    for (; done + kGraphRounds <= rounds; done += kGraphRounds)
      for (uint32_t i = 0; i < k; ++i) AZMI_HIP_TRY(hipGraphLaunch(pms[i]->graph_exec, pms[i]->graph_stream));
  }
  for (; done < rounds; ++done)
    for (uint32_t i = 0; i < k; ++i) {
      const int rc = one_round_with_net(pms[i], net, pms[i]->pick(streams[i]));
      if (rc != AZMI_OK) return rc;
    }
  return AZMI_OK;
}

// The round loop with one net PER MODEL GROUP (gating / benchmark matches, game_runner.py:2184-2332: two models, seats
// swapped by the permutations): nets[g] evaluates the leaves of model group g; NULL = that group needs no net (RANDOM /
// PLAYOUT evaluator).
int azmi_run_rounds_groups(azmi_pm* const* pms, azmi_net* const* nets, uint32_t num_nets, uint32_t k, uint32_t rounds, void* const* streams) {
  if (!pms || !nets || !streams || k == 0) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  for (uint32_t i = 0; i < k; ++i)
    if (pms[i]->ep.num_groups > num_nets) return azmi_host_fail(AZMI_ERR_INVALID, "engine %u has %u model groups but %u nets were given", i, pms[i]->ep.num_groups, num_nets);
  for (uint32_t r = 0; r < rounds; ++r)
    for (uint32_t i = 0; i < k; ++i) {
      azmi_pm* pm = pms[i];
      hipStream_t st = pm->pick(streams[i]);
      int rc = azmi_host_launch_round(pm, st);
      if (rc != AZMI_OK) return rc;
      for (uint32_t g = 0; g < pm->ep.num_groups; ++g) {
        if (!nets[g]) continue;
        rc = pm_net_forward(pm, g, nets[g], st);
        if (rc != AZMI_OK) return rc;
      }
    }
  return AZMI_OK;
}

int azmi_pm_net_forward(azmi_pm* pm, azmi_net* net, void* stream) {
  if (!pm || !net) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  std::lock_guard<std::recursive_mutex> lock_(pm->mu);
  for (uint32_t g = 0; g < pm->ep.num_groups; ++g) {   // the same net for every model group
    const int rc = pm_net_forward(pm, g, net, pm->pick(stream));
    if (rc != AZMI_OK) return rc;
  }
  return AZMI_OK;
}

int azmi_pm_round_net(azmi_pm* pm, azmi_net* net, void* stream, uint32_t part) {
  if (!pm || !net) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  std::lock_guard<std::recursive_mutex> lock_(pm->mu);
  hipStream_t st = pm->pick(stream);
  azmi_net_c4_view view;
  const bool fused = can_fuse(pm, net, &view);
  if (part == 0 || part == 1) {          // the tree half of the round
    const int rc = azmi_host_launch_round(pm, st, fused);
    if (rc != AZMI_OK || part == 1) return rc;
  }
  if (fused) return azmi_host_launch_net_move(pm, view, st);
  for (uint32_t g = 0; g < pm->ep.num_groups; ++g) {
    const int rc = pm_net_forward(pm, g, net, st);
    if (rc != AZMI_OK) return rc;
  }
  return AZMI_OK;
}

int azmi_pm_net_forward_group(azmi_pm* pm, uint32_t group, azmi_net* net, void* stream) {
  if (!pm || !net) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  std::lock_guard<std::recursive_mutex> lock_(pm->mu);
  if (group >= pm->ep.num_groups) return azmi_host_fail(AZMI_ERR_INVALID, "model group %u out of range", group);
  return pm_net_forward(pm, group, net, pm->pick(stream));
}

int azmi_pm_poll(azmi_pm* pm, void* stream, uint32_t* games_completed, uint32_t* live_slots) {
  if (!pm) return azmi_host_fail(AZMI_ERR_INVALID, "null pm");
  std::lock_guard<std::recursive_mutex> lock_(pm->mu);
  Control c;
  const int rc = azmi_host_read_ctl(pm, pm->pick(stream), &c, true);
  if (rc != AZMI_OK) return rc;
  if (games_completed) *games_completed = c.games_completed;
  if (live_slots) *live_slots = c.stop ? 0u : c.live_slots;
  return AZMI_OK;
}

int azmi_pm_play(azmi_pm* pm, void* stream) {
  if (!pm) return azmi_host_fail(AZMI_ERR_INVALID, "null pm");
  if (!pm->all_random) return azmi_host_fail(AZMI_ERR_STATE, "azmi_pm_play needs EvalType::RANDOM on every seat; drive NN seats with azmi_pm_round");
  hipStream_t st = pm->pick(stream);
  for (;;) {
    if (pm->stopped.load(std::memory_order_relaxed)) return AZMI_OK;   // play_manager.cc:272
    // several threads may sit in play() at once (the reference starts mcts_workers of them): each takes the engine for a
    // chunk of rounds, all of them return when the games are done
    std::lock_guard<std::recursive_mutex> lock_(pm->mu);
    for (int r = 0; r < 32; ++r) {
      const int rc = azmi_host_launch_round(pm, st);
      if (rc != AZMI_OK) return rc;
    }
    Control c;
    const int rc = azmi_host_read_ctl(pm, st, &c, true);
    if (rc != AZMI_OK) return rc;
    if (c.stop) return AZMI_OK;
  }
}

}  // extern "C"
