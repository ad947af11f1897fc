// One call of the asynchronous tree / net pipeline (azmi_run_pipeline*): what comes before its first epoch, one epoch's launches
// and event edges, and what comes after its last.  Host code only: the kernels and their launch functions are in pipeline.hip's
// device module, the state and its set-up in pipeline_state.hip (pipeline_host.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <map>
#include <memory>
#include <mutex>
#include <vector>

#include "dev_games.h"
#include "pipe_knobs.h"
#include "pipeline_host.h"

using namespace azmi;

namespace {

// An epoch's workgroup counts assume the chip to itself (placement): two engines' epochs at once would each find half of
// their workgroups without a place.  Calls from different threads therefore take turns (they are synchronous anyway).
// (one mutex per DEVICE: two engines on two different GPUs of one process do not wait for each other - VERDICT r4)
std::mutex& pipeline_turn_of(int device) {
  static std::mutex table_mu;
  static std::map<int, std::unique_ptr<std::mutex>> table;
  std::lock_guard<std::mutex> l(table_mu);
  auto& m = table[device];
  if (!m) m.reset(new std::mutex());
  return *m;
}

// Everything of a call that comes before its first epoch: the pipeline state on first use, the net side sized and measured for this
// call's net, the insert log, the locks and the answer table, the epoch's limits, and the restarts the first epoch starts from.
int pipe_prepare_call(azmi_pm* pm, const PipePlan& plan, const PipeKnobs& k, uint32_t epochs, uint64_t sims_per_epoch, hipStream_t st) {
  const azmi_net_c4_view& view = plan.view[0];
  const bool tree_only = plan.tree_only;
  if (!pm->pipe) { const int rc = pipe_create(pm); if (rc != AZMI_OK) return rc; }
  PipeState* ps = pm->pipe;
  PipeArrays& pa = ps->pa;
  ps->kind = plan.kind;
  ps->np1_valid = (plan.net_groups & 2u) != 0u;
  ps->np1 = plan.view[1].np;
  pa.n_groups = pm->ep.num_groups;
  pa.net_groups = plan.net_groups;
  if (pa.n_groups > 1u && !pa.ring1) {
    const int rc = pipe_alloc(ps, pa.ring1, static_cast<size_t>(kPipeRing) * kReqGranules);
    if (rc != AZMI_OK) return rc;
  }
  if (!tree_only) { const int rc = pipe_pair_streams(ps, st); if (rc != AZMI_OK) return rc; }
  if (!tree_only) { const int rc = pipe_size_net(pm, ps, view); if (rc != AZMI_OK) return rc; }
  if (!tree_only) { const int rc = pipe_calibrate(pm, ps, st, view); if (rc != AZMI_OK) return rc; }
  // the insert log holds an epoch's answers: at most one per simulation, in practice a third of them
  // (the quota is checked between passes: an epoch overshoots it by what the passes under way still finish)
  const uint64_t want_log = pm->ep.cache_on ? std::min<uint64_t>(std::min<uint64_t>(sims_per_epoch, 1024ull * pm->ep.S) + 2ull * pm->ep.S + static_cast<uint64_t>(ps->tree_wgs) * 32u * (pa.max_inline + 1u), 1ull << 24) : 0ull;
  if (want_log > pa.ins_cap) {
    int rc = pipe_alloc(ps, pa.ins_key, want_log);
    if (rc == AZMI_OK) rc = pipe_alloc(ps, pa.ins_pi, want_log * Connect4::M);
    if (rc == AZMI_OK) rc = pipe_alloc(ps, pa.ins_v, want_log * (Connect4::P + 1));
    if (rc == AZMI_OK && pa.n_groups > 1u) rc = pipe_alloc(ps, pa.ins_grp, want_log);
    if (rc != AZMI_OK) return rc;
    pa.ins_cap = static_cast<uint32_t>(want_log);
  }
  if (pm->ep.cache_on && !pa.locks) {      // one insert lock per shard, group 0's cache first
    size_t total = 0;
    for (uint32_t g = 0; g < pm->ep.num_groups && g < pm->group_caches.size(); ++g) total += pm->group_caches[g].shards;
    total = std::max<size_t>(total, pm->ar.cache.shards);
    pa.lock_base1 = pm->group_caches.empty() ? 0u : pm->group_caches[0].shards;
    const int rc = pipe_alloc(ps, pa.locks, total);
    if (rc != AZMI_OK) return rc;
  }
  if (pm->ep.cache_on && !pa.l0 && !tree_only && plan.kind == 1 && !k.no_l0) {
    // the answer table: a power of two of 128-byte entries, an eighth of the S3-FIFO's entries, between 4 Ki and 4 Mi (512 MB: an
    // epoch of the headline brings ~200 k answers).  Measured and dropped: a table of half the S3-FIFO's entries (64 Mi = 8 GB at the
    // headline's cache) with shard hits copied into it - a table hit costs the probe one round trip instead of two, but 8 GB more of
    // randomly probed memory made every probe slower: 4968 games/s against 5667 (AZMI_PIPE_L0_LOG2 / AZMI_PIPE_L0_WB bring it back)
    uint64_t want = static_cast<uint64_t>(pm->ar.cache.shards) * kWaveCap / 8u;
    uint32_t sh = 12;
    while (sh < 22u && (1ull << sh) < want) ++sh;
    if (k.l0_log2 >= 0) sh = static_cast<uint32_t>(k.l0_log2);
    const int rc = pipe_alloc(ps, pa.l0, (static_cast<size_t>(1) << sh) * kResStride);
    if (rc != AZMI_OK) return rc;
    pa.l0_mask = (1u << sh) - 1u;
    pa.l0_wb = k.l0_wb;
  }
  if (pa.l0) {
    // the table's entries are answers of the nets the LAST call ran with: another net behind a group (or the groups' nets swapped)
    // would be served the old net's (v, pi) as hits - wipe it.  (It also outlives the S3-FIFO's evictions inside one
    // engine: by design, the table is a second, direct-mapped level of the position cache.)
    const void* n0 = (plan.net_groups & 1u) ? static_cast<const void*>(plan.view[0].np.blocks) : nullptr;
    const void* n1 = (plan.net_groups & 2u) ? static_cast<const void*>(plan.view[1].np.blocks) : nullptr;
    if (n0 != ps->l0_nets[0] || n1 != ps->l0_nets[1]) {
      if (ps->l0_nets[0] || ps->l0_nets[1]) AZMI_HIP_TRY(hipMemsetAsync(pa.l0, 0, (static_cast<size_t>(pa.l0_mask) + 1u) * kResStride * sizeof(unsigned long long), st));
      ps->l0_nets[0] = n0; ps->l0_nets[1] = n1;
    }
  }
  // an epoch must end long before the wall-clock cap (a stall detector, 250 ms): with the move step inside the epoch nothing else ends it,
  // so the quota is held to 1024 simulations per slot (~50 ms at the slowest per-slot rate measured)
  pa.quota = std::min<uint64_t>(sims_per_epoch, 1024ull * pm->ep.S);
  pa.net_needed = std::max<uint32_t>(8u, (pm->ep.S + 2u) / 3u + 8u);
  pa.idle_num = k.idle_num;
  pa.cap_ticks = k.cap_ticks;
  pa.test_drop = k.test_drop;
  pa.soft_ticks = k.soft_ticks;
  // A slot has at most one request out and a tile takes three: more than S / 3 net workgroups (+ 8 of slack) can never all have work.
  // A small engine therefore does not launch the ~500 the chip holds: idle persistent workgroups are not free - they poll - and
  // the rare seconds-long stalls of the tree side were only ever seen with hundreds of them idle.
  ps->net_launch = std::min<uint32_t>(ps->net_wgs, std::max<uint32_t>(8u, (pm->ep.S + 2u) / 3u + 8u));
  if (k.net_all) ps->net_launch = ps->net_wgs;
  while (ps->tev.size() < 4ull * epochs) {
    hipEvent_t ev;
    AZMI_HIP_TRY(hipEventCreate(&ev));
    ps->tev.push_back(ev);
  }
  // the lock-step kernels leave the key of a round's leaf in cache_keys for the next round's insert: none of that here
  if (pm->ep.cache_on) AZMI_HIP_TRY(hipMemsetAsync(pm->ar.cache_keys, 0, sizeof(uint64_t) * pm->ep.S, st));
  return azmi_host_launch_assign(pm, st, 1u);
}

// ONE epoch's launches and event edges, in the order each stream sees them.  `st` is the caller's stream (the tree side, and everything
// between epochs); net_stream runs the net kernel beside it, tree_stream (CU split only) the tree kernel.  The order is load-bearing
// (DESIGN 2.1): change nothing here without measuring.
int pipe_enqueue_epoch(azmi_pm* pm, const PipePlan& plan, const PipeKnobs& k, uint32_t e, hipStream_t st) {
  PipeState* ps = pm->pipe;
  const PipeArrays& pa = ps->pa;
  const bool tree_only = plan.tree_only;
  AZMI_HIP_TRY(hipMemsetAsync(pa.ep, 0, sizeof(PipeEpoch), st));
  pipe_launch_seed(pm, pa, st);
  AZMI_HIP_TRY(hipGetLastError());
  if (!tree_only) {
    AZMI_HIP_TRY(hipEventRecord(ps->ev_go, st));
    AZMI_HIP_TRY(hipStreamWaitEvent(ps->net_stream, ps->ev_go, 0));
  }
  // the tree kernel goes first: its workgroups take their places per shader engine, the net kernel is sized for what is left
  // (CU split: on its own stream, masked to the tree side's CUs; the caller's stream waits for it)
  hipStream_t ts = ps->tree_stream && !tree_only ? ps->tree_stream : st;
  if (ts != st) AZMI_HIP_TRY(hipStreamWaitEvent(ts, ps->ev_go, 0));
  AZMI_HIP_TRY(hipEventRecord(ps->tev[4 * e + 2], ts));
  pipe_launch_tree(pm, ps, pa, ts, k.prof);
  AZMI_HIP_TRY(hipGetLastError());
  AZMI_HIP_TRY(hipEventRecord(ps->tev[4 * e + 3], ts));
  if (ts != st) { AZMI_HIP_TRY(hipEventRecord(ps->ev_tree, ts)); AZMI_HIP_TRY(hipStreamWaitEvent(st, ps->ev_tree, 0)); }
  if (pm->ep.cache_on) {      // behind the tree kernel, beside the net side's last tiles
    pipe_launch_cache_insert(pm, pa, 2048u, 0u, st);
    AZMI_HIP_TRY(hipGetLastError());
  }
  if (!tree_only) {
    AZMI_HIP_TRY(hipEventRecord(ps->tev[4 * e + 0], ps->net_stream));
    const int rc = pipe_launch_net(ps, plan.view[0], k.tile, ps->net_launch, ps->net_stream, pa);
    if (rc != AZMI_OK) return rc;
    AZMI_HIP_TRY(hipEventRecord(ps->tev[4 * e + 1], ps->net_stream));
    AZMI_HIP_TRY(hipEventRecord(ps->ev_net, ps->net_stream));
    AZMI_HIP_TRY(hipStreamWaitEvent(st, ps->ev_net, 0));
  }
  pipe_launch_settle(pm, pa, st);
  AZMI_HIP_TRY(hipGetLastError());
  int rc = azmi_host_launch_move_step(pm, st);
  if (rc != AZMI_OK) return rc;
  rc = azmi_host_launch_assign(pm, st, 1u);
  if (rc != AZMI_OK) return rc;
  if (pm->ep.cache_on) {
    pipe_launch_cache_insert(pm, pa, 256u, 1u, st);
    AZMI_HIP_TRY(hipGetLastError());
  }
  return AZMI_OK;
}

// After the last epoch: the control blocks read back (the call is synchronous - a pipeline error must not go unseen), the balance
// rule for the next call, out_stats, and the error report - which leaves the engine whole.
int pipe_finish_call(azmi_pm* pm, const PipePlan& plan, const PipeKnobs& k, uint32_t epochs, uint64_t host_enqueue_us, hipStream_t st, uint64_t* out_stats) {
  PipeState* ps = pm->pipe;
  PipeArrays& pa = ps->pa;
  const bool tree_only = plan.tree_only;
  PipeCtl hc;
  PipeEpoch he;
  AZMI_HIP_TRY(hipMemcpyAsync(&hc, pa.ctl, sizeof(hc), hipMemcpyDeviceToHost, st));
  AZMI_HIP_TRY(hipMemcpyAsync(&he, pa.ep, sizeof(he), hipMemcpyDeviceToHost, st));
  AZMI_HIP_TRY(hipStreamSynchronize(st));
  if (hc.lost_total != ps->lost_seen) {
    fprintf(stderr, "azmi_run_pipeline: %u request(s) were given up by the net side and sent again (a net workgroup fell more than half a ring behind)\n", hc.lost_total - ps->lost_seen);
    ps->lost_seen = hc.lost_total;
  }
  if (!tree_only && !hc.err) pipe_balance(ps, hc, k.balance_a, k.balance_b);       // (takes effect with the next call's first epoch)
  if (out_stats) {
    out_stats[0] = hc.tiles; out_stats[1] = hc.tile_boards; out_stats[2] = he.sims; out_stats[3] = he.tree_arrived;
    out_stats[4] = he.net_arrived; out_stats[5] = he.ins_count; out_stats[6] = ps->net_launch; out_stats[7] = ps->tree_wgs;
    out_stats[8] = he.tree_late / 100u; out_stats[9] = he.net_late / 100u;
    double net_us = 0.0, tree_us = 0.0;
    for (uint32_t e = 0; e < epochs; ++e) {
      float ms = 0.0f;
      if (!tree_only && hipEventElapsedTime(&ms, ps->tev[4 * e + 0], ps->tev[4 * e + 1]) == hipSuccess) net_us += 1e3 * ms;
      if (hipEventElapsedTime(&ms, ps->tev[4 * e + 2], ps->tev[4 * e + 3]) == hipSuccess) tree_us += 1e3 * ms;
    }
    out_stats[10] = static_cast<uint64_t>(net_us); out_stats[11] = static_cast<uint64_t>(tree_us); out_stats[12] = epochs; out_stats[13] = host_enqueue_us;
    out_stats[14] = static_cast<uint64_t>(ps->calib_rounds & 0xFFu) | (static_cast<uint64_t>(std::min<unsigned long long>(hc.freezes, 0xFFFFFFull)) << 8) | (static_cast<uint64_t>(hc.lost_total) << 32);
    out_stats[15] = hc.l0_hits;
    if (k.prof) {
      fprintf(stderr, "pipe prof:");
      for (int i = 0; i < 16; ++i) fprintf(stderr, " %llu", hc.prof[i]);
      fprintf(stderr, "\n");
    }
    if (k.prof || k.hist) {
      fprintf(stderr, "pipe tile hist (tiles of 1 .. 6 boards since creation):");
      for (int i = 0; i < 6; ++i) fprintf(stderr, " %llu", hc.tile_hist[i]);
      fprintf(stderr, "\n");
    }
  }
  if (!hc.err) return AZMI_OK;
  fprintf(stderr, "pipeline dbg:");
  for (int i = 0; i < 18; ++i) fprintf(stderr, " %u", hc.dbg[i]);
  fprintf(stderr, "\n");
  if (plan.kind == 2) {      // the generic tree kernel: where each of its wavefronts was last (phase, 10 us units since its start)
    std::vector<PipeWg> hw(ps->tree_wgs);
    if (hipMemcpy(hw.data(), pa.wg, hw.size() * sizeof(PipeWg), hipMemcpyDeviceToHost) == hipSuccess) {
      fprintf(stderr, "pipeline generic tree kernel, workgroup: rhead rtail | phase@10us of its four wavefronts | their entry times, us after wavefront 0's:");
      for (uint32_t w = 0; w < ps->tree_wgs; ++w)
        fprintf(stderr, "  [%u: %u %u | %u@%u %u@%u %u@%u %u@%u | %d %d %d]", w, hw[w].rhead, hw[w].rtail, hw[w].pad[2] & 255u, hw[w].pad[2] >> 8, hw[w].pad[3] & 255u, hw[w].pad[3] >> 8,
                hw[w].pad[4] & 255u, hw[w].pad[4] >> 8, hw[w].pad[5] & 255u, hw[w].pad[5] >> 8,
                static_cast<int32_t>(hw[w].pad[7] - hw[w].pad[6]) / 100, static_cast<int32_t>(hw[w].pad[8] - hw[w].pad[6]) / 100, static_cast<int32_t>(hw[w].pad[9] - hw[w].pad[6]) / 100);
      fprintf(stderr, "\n  wavefront 0's longest interval between two looks: wall clock x10us | SQ clock >> 10 | 0 poll loop, 1 a pass | after polls | polls in all:");
      for (uint32_t w = 0; w < ps->tree_wgs; ++w) fprintf(stderr, "  [%u: %u | %u | %u | %u | %u]", w, hw[w].pad[10], hw[w].pad[11], hw[w].pad[12], hw[w].pad[13], hw[w].pad[14]);
      fprintf(stderr, "\n  longest phases of its passes (SQ clock >> 10): publication word | granules | log ticket + drain | steps + requests | tokens:");
      for (uint32_t w = 0; w < ps->tree_wgs; ++w) fprintf(stderr, "  [%u: %u | %u | %u | %u | %u]", w, hw[w].pad[18], hw[w].pad[19], hw[w].pad[20], hw[w].pad[21], hw[w].pad[22]);
      fprintf(stderr, "\n  its longest segments (SQ clock >> 10): token load | control words | between looks:");
      for (uint32_t w = 0; w < ps->tree_wgs; ++w) fprintf(stderr, "  [%u: %u | %u | %u]", w, hw[w].pad[15], hw[w].pad[16], hw[w].pad[17]);
      fprintf(stderr, "\n");
    }
  }
  // reported once: k_pipe_settle has put every slot whose request went unanswered back into the move step's kSlotQueued form, so
  // the engine is whole - the next call (either driver) carries on from here
  AZMI_HIP_TRY(hipMemsetAsync(&pa.ctl->err, 0, sizeof(uint32_t), st));
  AZMI_HIP_TRY(hipMemsetAsync(pa.ctl->dbg, 0, sizeof(pa.ctl->dbg), st));
  AZMI_HIP_TRY(hipStreamSynchronize(st));
  return azmi_host_fail(AZMI_ERR_STATE, "pipeline error mask 0x%x (1 a spin hit the epoch's time cap, 2 a ring entry never arrived, 4 a result tag "
                        "did not match, 8 insert log full, 16 cache lock, 32 slots, 64 the net side hit the time cap); census: %u of %u tree and %u of %u net workgroups started; "
                        "last epoch: head %u tail %u sims %llu ended %u dead %u stop %u tree_done %u tiles %llu boards %llu; latest tree / net workgroup start %u / %u us; "
                        "first time-out saw: slot %u seq %u / %u; net side: stop %u tree done %u of %u tail %u window at %u after %u0 us; "
                        "wavefronts that stood still > 2 ms (not one instruction between two looks at the clock) so far: %llu, the longest for %.1f ms",
                        hc.err, he.tree_arrived, ps->tree_wgs, he.net_arrived, ps->net_launch, hc.head, hc.tail, he.sims, he.ended, he.dead, he.stop,
                        he.tree_done, hc.tiles, hc.tile_boards, he.tree_late / 100u, he.net_late / 100u,
                        hc.dbg[1], hc.dbg[2], hc.dbg[3], hc.dbg[8], hc.dbg[9], hc.dbg[10], hc.dbg[11], hc.dbg[12], hc.dbg[13],
                        static_cast<unsigned long long>(hc.freezes), static_cast<double>(hc.freeze_max) * 1e-5);
}

int run_pipeline_impl(azmi_pm* pm, azmi_net* const* nets, uint32_t num_nets, uint32_t epochs, uint64_t sims_per_epoch, void* stream, uint64_t* out_stats) {
  if (!pm) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  const PipeKnobs k = pipe_read_knobs();
  std::lock_guard<std::recursive_mutex> lock_(pm->mu);
  std::lock_guard<std::mutex> turn_(pipeline_turn_of(pm->device));
  const PipePlan plan = pipe_plan(pm, nets, num_nets);
  if (plan.kind == 0)
    return azmi_host_fail(AZMI_ERR_STATE, "azmi_run_pipeline: the pipeline drives the Connect4 engine (no PLAYOUT seats, at most two model groups, at most %u "
                          "concurrent games) with a Connect4-family matrix-core net of one precision tier behind every model group that evaluates with a net "
                          "(or no net at all when every seat uses EvalType::RANDOM) - azmi_pipeline_supported; use azmi_run_rounds for everything else", kPipeRing / 2u);
  if (sims_per_epoch == 0) return azmi_host_fail(AZMI_ERR_INVALID, "azmi_run_pipeline: sims_per_epoch must be > 0");
  if (pm->stopped.load(std::memory_order_relaxed)) {     // PlayManager::stop(): the workers leave their loop (play_manager.cc:272)
    if (out_stats) for (int i = 0; i < 16; ++i) out_stats[i] = 0;
    return AZMI_OK;
  }
  if (k.net_conveyor && !plan.tree_only) return pipe_no_conveyor();      // (before any GPU work: the engine is as it was)
  AZMI_HIP_TRY(hipSetDevice(pm->device));
  hipStream_t st = pm->pick(stream);
  int rc = pipe_prepare_call(pm, plan, k, epochs, sims_per_epoch, st);
  if (rc != AZMI_OK) return rc;
  const auto host_t0 = std::chrono::steady_clock::now();       // what the host spends enqueueing the epochs (it runs ahead of the GPU)
  for (uint32_t e = 0; e < epochs; ++e) {
    rc = pipe_enqueue_epoch(pm, plan, k, e, st);
    if (rc != AZMI_OK) return rc;
    if (k.debug) {      // AZMI_PIPE_DEBUG: stop at the first epoch that raised an error, with that epoch's own counters
      PipeCtl dc; PipeEpoch de;
      AZMI_HIP_TRY(hipMemcpyAsync(&dc, pm->pipe->pa.ctl, sizeof(dc), hipMemcpyDeviceToHost, st));
      AZMI_HIP_TRY(hipMemcpyAsync(&de, pm->pipe->pa.ep, sizeof(de), hipMemcpyDeviceToHost, st));
      AZMI_HIP_TRY(hipStreamSynchronize(st));
      if (dc.err) {
        fprintf(stderr, "pipeline debug: epoch %u of this call: err 0x%x head %u tail %u sims %llu ended %u dead %u stop %u tree_done %u/%u arrived, net arrived %u, ins %u, late %u/%u\n",
                e, dc.err, dc.head, dc.tail, de.sims, de.ended, de.dead, de.stop, de.tree_done, de.tree_arrived, de.net_arrived, de.ins_count,
                de.tree_late / 100u, de.net_late / 100u);
        epochs = e + 1;
        break;
      }
    }
  }
  const uint64_t host_enqueue_us = static_cast<uint64_t>(std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - host_t0).count());
  return pipe_finish_call(pm, plan, k, epochs, host_enqueue_us, st, out_stats);
}

}  // namespace

extern "C" int azmi_run_pipeline(azmi_pm* pm, azmi_net* net, uint32_t epochs, uint64_t sims_per_epoch, void* stream, uint64_t* out_stats) {
  azmi_net* nets[2] = {net, net};            // the same net for every model group (azmi_pm_net_forward's rule)
  return run_pipeline_impl(pm, nets, 2, epochs, sims_per_epoch, stream, out_stats);
}
extern "C" int azmi_run_pipeline_groups(azmi_pm* pm, azmi_net* const* nets, uint32_t num_nets, uint32_t epochs, uint64_t sims_per_epoch, void* stream,
                                        uint64_t* out_stats) {
  return run_pipeline_impl(pm, nets, num_nets, epochs, sims_per_epoch, stream, out_stats);
}
