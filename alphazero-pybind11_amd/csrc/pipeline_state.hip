// The state of the asynchronous tree / net pipeline of one engine (pipeline_host.h): what a call can be driven with (pipe_plan,
// azmi_pipeline_supported*), creation on first use, the net side sized and measured beside the tree side (pipe_size_net,
// pipe_pair_streams, pipe_calibrate) and the balance between the two sides from call to call.  Host code only: the kernels and
// their launch functions are in pipeline.hip's device module.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "pipe_knobs.h"
#include "pipeline_host.h"

using namespace azmi;

void azmi::pipe_state_free(PipeState* p) {
  if (!p) return;
  for (void* q : p->allocs) (void)hipFree(q);
  if (p->net_stream) (void)hipStreamDestroy(p->net_stream);
  if (p->tree_stream) (void)hipStreamDestroy(p->tree_stream);
  if (p->ev_tree) (void)hipEventDestroy(p->ev_tree);
  for (hipStream_t q : p->parked) (void)hipStreamDestroy(q);
  if (p->ev_go) (void)hipEventDestroy(p->ev_go);
  if (p->ev_net) (void)hipEventDestroy(p->ev_net);
  for (hipEvent_t e : p->tev) (void)hipEventDestroy(e);
  delete p;
}

namespace {

// a stream for one side of the pipeline: plain, or - with the CU split on - masked to the side's CUs (bit i of the mask = CU i as the
// runtime numbers them; which physical CUs those are is nothing this code assumes: the two masks are disjoint, the census measures
// what fits)
int pipe_make_stream(PipeState* ps, hipStream_t* out, bool tree_side) {
  if (ps->cu_split == 0u) { AZMI_HIP_TRY(hipStreamCreateWithFlags(out, hipStreamNonBlocking)); return AZMI_OK; }
  std::vector<uint32_t> mask((ps->cu_total + 31u) / 32u, 0u);
  for (uint32_t cu = 0; cu < ps->cu_total; ++cu)
    if ((cu < ps->cu_split) == tree_side) mask[cu / 32u] |= 1u << (cu % 32u);
  AZMI_HIP_TRY(hipExtStreamCreateWithCUMask(out, static_cast<uint32_t>(mask.size()), mask.data()));
  return AZMI_OK;
}

uint32_t pipe_tree_wgs_for(uint32_t S, const PipeSetupKnobs& k) {
  // tree workgroups: a slot lives in ONE workgroup for an epoch (its home), so a workgroup's 32 lane-groups serve S / workgroups
  // slots; about a third of the slots is with the net or in a ring at any time.  Every tree workgroup takes a place from the net
  // side, and at 4096 slots both sides are full (tree wavefronts 94 % busy, net workgroups 87-91 %): measured, M simulations/s at 96 /
  // 112 / 128 / 144 / 160 workgroups: 89 / 101 / 102-105 / 100 / 88.  AZMI_PIPE_TREE_WGS sets another count.
  uint32_t t = std::min<uint32_t>(128u, std::max<uint32_t>(1u, (S + 31u) / 32u));
  if (k.tree_wgs) t = k.tree_wgs;
  return std::min<uint32_t>(t, std::max<uint32_t>(1u, S));
}

}  // namespace

int pipe_create(azmi_pm* pm) {
  const PipeSetupKnobs k = pipe_read_setup_knobs();
  auto ps = new PipeState();
  struct Guard { PipeState* p; ~Guard() { if (p) pipe_state_free(p); } } guard{ps};     // (a failed set-up leaves nothing half-built behind)
  PipeArrays& pa = ps->pa;
  const uint32_t S = pm->ep.S;
  ps->diag = k.diag;
  ps->whatif_depth = k.whatif_depth;
  ps->tree_wgs = ps->tree_wgs_default = pipe_tree_wgs_for(S, k);
  pa.n_tree_wgs = ps->tree_wgs;
  // the tree side may grow or shrink between calls with the share of leaves that reach the net (pipe_balance): unless the count was
  // fixed by hand, rings exist for 1.5 x the default and are sized for a third of it
  ps->balance = k.tree_wgs == 0u && !k.net_wgs_set && !k.no_balance && ps->tree_wgs >= 48u;
  ps->tree_wgs_alloc = ps->balance ? ps->tree_wgs + ps->tree_wgs / 2u : ps->tree_wgs;
  ps->tree_wgs_min = ps->balance ? ps->tree_wgs / 3u : ps->tree_wgs;
  {   // a workgroup's READY ring: at least twice its slots (every slot has at most one token out), a power of two
    const uint32_t per_wg = (S + ps->tree_wgs_min - 1u) / ps->tree_wgs_min;
    uint32_t sh = 6;
    while ((1u << sh) < 2u * per_wg + 2u * kTreeWindow) ++sh;
    pa.rshift = sh;
  }
  int rc = pipe_alloc(ps, pa.ctl, 1);
  if (rc == AZMI_OK) rc = pipe_alloc(ps, pa.wg, ps->tree_wgs_alloc);
  if (rc == AZMI_OK && k.pos0_set) {
    const uint32_t p0 = k.pos0;
    PipeCtl h{};
    h.head = h.tail = p0;
    if (hipMemcpy(pa.ctl, &h, sizeof(h), hipMemcpyHostToDevice) != hipSuccess) return azmi_host_fail(AZMI_ERR_NO_DEVICE, "pipeline: control block upload failed");
    std::vector<PipeWg> hw(ps->tree_wgs_alloc);
    for (auto& w : hw) { w = PipeWg{}; w.rhead = w.rtail = p0; }
    if (hipMemcpy(pa.wg, hw.data(), hw.size() * sizeof(PipeWg), hipMemcpyHostToDevice) != hipSuccess) return azmi_host_fail(AZMI_ERR_NO_DEVICE, "pipeline: control block upload failed");
  }
  if (rc == AZMI_OK) rc = pipe_alloc(ps, pa.ep, 1);
  if (rc == AZMI_OK) rc = pipe_alloc(ps, pa.ring, static_cast<size_t>(kPipeRing) * kReqGranules);
  if (rc == AZMI_OK) rc = pipe_alloc(ps, pa.rring, static_cast<size_t>(ps->tree_wgs_alloc) << pa.rshift);
  if (rc == AZMI_OK) rc = pipe_alloc(ps, pa.res, static_cast<size_t>(S) * kResStride);
  if (rc != AZMI_OK) return rc;
  // the pass and window rules (PipeSetupKnobs has the measurements behind the defaults)
  pa.max_inline = k.max_inline ? k.max_inline : (pm->max_inline_explicit ? pm->ep.max_inline : 8u);
  pa.min_active = k.min_active;
  pa.big_at = k.big_at;
  pa.take_wait = k.take_wait;
  if (k.cu_split >= 0) {
    hipDeviceProp_t prop;
    AZMI_HIP_TRY(hipGetDeviceProperties(&prop, pm->device));
    ps->cu_total = static_cast<uint32_t>(prop.multiProcessorCount);
    ps->cu_split = static_cast<uint32_t>(std::max(0, std::min(k.cu_split, static_cast<int>(ps->cu_total) - 1)));
    if (ps->cu_split) {
      { const int rc2 = pipe_make_stream(ps, &ps->tree_stream, true); if (rc2 != AZMI_OK) return rc2; }
      AZMI_HIP_TRY(hipEventCreateWithFlags(&ps->ev_tree, hipEventDisableTiming));
      // two tree workgroups per CU (256 registers x 4 wavefronts each)
      if (k.tree_wgs == 0u) { ps->tree_wgs = ps->tree_wgs_default = std::min(ps->tree_wgs_alloc, 2u * ps->cu_split); pa.n_tree_wgs = ps->tree_wgs; }
      ps->balance = false;
    }
  }
  { const int rc2 = pipe_make_stream(ps, &ps->net_stream, false); if (rc2 != AZMI_OK) return rc2; }
  AZMI_HIP_TRY(hipEventCreateWithFlags(&ps->ev_go, hipEventDisableTiming));
  AZMI_HIP_TRY(hipEventCreateWithFlags(&ps->ev_net, hipEventDisableTiming));
  guard.p = nullptr;
  pm->pipe = ps;       // owned by the engine from here on (freed with it)
  return AZMI_OK;
}

// The net side for THIS net: LDS per workgroup (bf16: the 6-board tile, two workgroups per CU; bf16x3: its 16-plane tile, one per CU)
// and the first guess of the workgroup count = the runtime's own occupancy answer x CUs - an UPPER bound; pipe_calibrate then measures
// what really runs beside the tree workgroups (a persistent kernel only works when every workgroup is resident, and how the dispatcher
// deals workgroups to shader engines is nothing this code may assume).  Called again when a call brings a net of the other tier.
int pipe_size_net(azmi_pm* pm, PipeState* ps, const azmi_net_c4_view& view) {
  const bool x3 = view.x3 != 0;
  if (ps->sized && ps->x3 == x3) return AZMI_OK;
  const PipeSetupKnobs k = pipe_read_setup_knobs();
  ps->x3 = x3;
  hipDeviceProp_t prop;
  AZMI_HIP_TRY(hipGetDeviceProperties(&prop, pm->device));
  int per_cu = 0;
  { const int rc = pipe_net_occupancy(x3, &ps->lds_bytes, &per_cu); if (rc != AZMI_OK) return rc; }
  uint32_t net = static_cast<uint32_t>(std::max(1, per_cu)) * (static_cast<uint32_t>(prop.multiProcessorCount) - ps->cu_split);
  if (k.net_wgs_set) net = k.net_wgs;
  ps->net_wgs = std::max<uint32_t>(1u, net);
  ps->calibrated = false;
  ps->places = 0;
  ps->sized = true;
  // the bf16x3 tiles cost three times the matrix work and get one workgroup per CU: the net side is what is short, and every tree
  // wavefront beside a tile slows it - half the tree workgroups (M simulations/s at 128 / 96 / 64: 27.7 / 33.4 / 36.2)
  if (ps->balance) {
    ps->tree_wgs = x3 ? std::max(ps->tree_wgs_min, ps->tree_wgs_default / 2u) : ps->tree_wgs_default;
    ps->pa.n_tree_wgs = ps->tree_wgs;
  }
  return AZMI_OK;
}

// net_stream must run beside `st` (see k_pair_wait): checked once per tree-side stream; a stream that shares st's hardware queue is
// parked and another one is tried.  Fails when no stream can be found (GPU_MAX_HW_QUEUES = 1): the caller drives the engine with
// azmi_run_rounds then.
int pipe_pair_streams(PipeState* ps, hipStream_t st) {
  if (ps->paired && ps->paired_with == st) return AZMI_OK;
  if (!ps->pair_flag) { const int rc = pipe_alloc(ps, ps->pair_flag, 4); if (rc != AZMI_OK) return rc; }
  for (int attempt = 0; attempt < 12; ++attempt) {
    AZMI_HIP_TRY(hipMemsetAsync(ps->pair_flag, 0, 4 * sizeof(uint32_t), st));
    AZMI_HIP_TRY(hipEventRecord(ps->ev_go, st));
    AZMI_HIP_TRY(hipStreamWaitEvent(ps->net_stream, ps->ev_go, 0));
    pipe_launch_pair_wait(ps->pair_flag, st);
    AZMI_HIP_TRY(hipGetLastError());
    pipe_launch_pair_set(ps->pair_flag, ps->net_stream);
    AZMI_HIP_TRY(hipGetLastError());
    uint32_t h[2] = {0, 0};
    AZMI_HIP_TRY(hipStreamSynchronize(ps->net_stream));
    AZMI_HIP_TRY(hipMemcpyAsync(h, ps->pair_flag, sizeof(h), hipMemcpyDeviceToHost, st));
    AZMI_HIP_TRY(hipStreamSynchronize(st));
    if (h[1] == 0u) { ps->paired = true; ps->paired_with = st; return AZMI_OK; }
    ps->parked.push_back(ps->net_stream);          // shares st's hardware queue
    ps->net_stream = nullptr;
    { const int rc2 = pipe_make_stream(ps, &ps->net_stream, false); if (rc2 != AZMI_OK) return rc2; }
  }
  return azmi_host_fail(AZMI_ERR_STATE, "azmi_run_pipeline: no second stream runs beside the caller's (one hardware queue? GPU_MAX_HW_QUEUES); "
                        "the pipeline needs its tree and net kernels on the chip together - use azmi_run_rounds");
}

// Measures how many net workgroups run BESIDE the tree workgroups: both persistent kernels are launched as they are in an epoch, with
// PipeArrays::census_hold set - every workgroup that gets a place holds it until 1 ms after the first one started (far longer than the
// two launches are apart) and leaves; one that the chip has no place for starts only then, finds itself late and is counted.  The net side gives up as many workgroups as came late (tree workgroups that came
// late count too: the net kernel had taken their places) until nobody is late.  No constant of the part's dealing order is involved;
// a second tenant on the chip, a CU mask or a new runtime change the answer, not the code.  (AZMI_PIPE_NO_CALIBRATE=1 skips it.)
int pipe_calibrate(azmi_pm* pm, PipeState* ps, hipStream_t st, const azmi_net_c4_view& view) {
  if (ps->calibrated || pipe_read_setup_knobs().no_calibrate) { ps->calibrated = true; return AZMI_OK; }
  PipeArrays pa = ps->pa;
  pa.census_hold = 100000u;
  for (int attempt = 0; attempt < 24; ++attempt) {
    AZMI_HIP_TRY(hipMemsetAsync(pa.ep, 0, sizeof(PipeEpoch), st));
    AZMI_HIP_TRY(hipEventRecord(ps->ev_go, st));
    AZMI_HIP_TRY(hipStreamWaitEvent(ps->net_stream, ps->ev_go, 0));
    if (ps->tree_stream) AZMI_HIP_TRY(hipStreamWaitEvent(ps->tree_stream, ps->ev_go, 0));
    pipe_launch_tree(pm, ps, pa, ps->tree_stream ? ps->tree_stream : st, false);
    AZMI_HIP_TRY(hipGetLastError());
    if (ps->tree_stream) { AZMI_HIP_TRY(hipEventRecord(ps->ev_tree, ps->tree_stream)); AZMI_HIP_TRY(hipStreamWaitEvent(st, ps->ev_tree, 0)); }
    { const int rc = pipe_launch_net(ps, view, 0, ps->net_wgs, ps->net_stream, pa); if (rc != AZMI_OK) return rc; }
    AZMI_HIP_TRY(hipEventRecord(ps->ev_net, ps->net_stream));
    AZMI_HIP_TRY(hipStreamWaitEvent(st, ps->ev_net, 0));
    PipeEpoch he;
    AZMI_HIP_TRY(hipMemcpyAsync(&he, pa.ep, sizeof(he), hipMemcpyDeviceToHost, st));
    AZMI_HIP_TRY(hipStreamSynchronize(st));
    ps->calib_rounds = static_cast<uint32_t>(attempt) + 1u;
    const uint32_t late = he.tree_late_n + he.net_late_n;
    if (late == 0u && he.tree_arrived == ps->tree_wgs && he.net_arrived == ps->net_wgs) {
      // (a workgroup serves ONE model group's ring for an epoch - its index's parity when both groups have a net: with one workgroup
      // group 1's ring would never be served and every epoch would run into the time cap - ADVICE r4)
      if (pa.net_groups == 3u && ps->net_wgs < 2u) break;
      ps->calibrated = true; ps->places = ps->x3 ? 0u : ps->tree_wgs + ps->net_wgs; return AZMI_OK;
    }
    if (ps->net_wgs <= 1u) break;
    ps->net_wgs = ps->net_wgs > late + 1u ? ps->net_wgs - std::max<uint32_t>(late, 1u) : 1u;
  }
  return azmi_host_fail(AZMI_ERR_STATE, "azmi_run_pipeline: the chip does not hold %u tree workgroups beside one net workgroup (another tenant on the GPU? "
                        "AZMI_PIPE_TREE_WGS too large?); use azmi_run_rounds", ps->tree_wgs);
}

// What azmi_run_pipeline(_groups) can drive: the Connect4 engine without PLAYOUT seats, at most two model groups, every group
// that evaluates with a net has a Connect4-family matrix-core net of ONE precision tier behind it.  nets[g] == NULL: group g needs
// no net (RANDOM seats: the reference's RandPlayer); no net at all: the tree side alone.
PipePlan pipe_plan(const azmi_pm* pm, azmi_net* const* nets, uint32_t num_nets) {
  PipePlan pl;
  const uint32_t G = pm->ep.num_groups;
  if (!(pm->game == AZMI_GAME_CONNECT4 && !pm->any_playout && G >= 1u && G <= 2u && pm->ep.S <= kPipeRing / 2u)) return pl;
  int x3 = -1;
  for (uint32_t g = 0; g < G; ++g) {
    if (!(pm->nn_groups >> g & 1u)) continue;                   // RANDOM seats: whatever stands in nets[g] is not asked
    azmi_net* n = (nets && g < num_nets) ? nets[g] : nullptr;
    if (!n) return pl;                                          // NN seats without a net
    if (azmi_net_c4_view_get(n, &pl.view[g]) == 0) return pl;
    if (x3 >= 0 && x3 != pl.view[g].x3) return pl;           // one precision tier per call (one net kernel)
    x3 = pl.view[g].x3;
    pl.net_groups |= 1u << g;
  }
  if (pl.net_groups == 0u) pl.tree_only = true;
  if (pl.net_groups == 2u) pl.view[0] = pl.view[1];             // (descriptor and LDS size of the one net there is)
  if (!(pl.net_groups & 2u)) pl.view[1] = pl.view[0];
  pl.kind = pipe_read_setup_knobs().generic ? 2 : 1;      // the fast tree kernel, unless the generic one is asked for
  return pl;
}
// The conveyor (round 5's weight-stationary net side: bit-identical to the tile kernel, slower) was an experiment build in round 6 and
// is gone: what asks for it is refused by name, never served by the tile kernel in silence.
int pipe_no_conveyor() {
  return azmi_host_fail(AZMI_ERR_STATE, "this library has no conveyor: the weight-stationary net side of round 5 measured slower than the tile kernel and was "
                        "removed (DESIGN.md 4.5b; git history, last present at commit 18a52a1); the tile kernel is the net side");
}
extern "C" int azmi_pipeline_supported(azmi_pm* pm, azmi_net* net) {
  if (!pm) return 0;
  azmi_net* nets[2] = {net, net};
  return pipe_plan(pm, nets, 2).kind != 0 ? 1 : 0;
}
extern "C" int azmi_pipeline_supported_groups(azmi_pm* pm, azmi_net* const* nets, uint32_t num_nets) {
  return pm && pipe_plan(pm, nets, num_nets).kind != 0 ? 1 : 0;
}

// The two sides share the chip's workgroup places, and how many each needs follows the share of leaves that reach the net.  Measured
// at 4096 slots on 512 places (M simulations/s by tree workgroups; m = evaluations per simulation):
//   m = 0.17 (128 M-entry cache, answer table on, the final tree pass):  128 / 144 / 160      -> 114 / 118 / 116
//   m = 0.19 (128 M entries, first half of the round):                    96 / 112 / 128 / 144 / 160 -> 88 / 96-101 / 96-105 / 100 / 88
//   m = 0.29 (32 M entries, first half):                                  80 /  96 / 112 / 128 -> 70 / 78 / 80 / 77
//   m = 0.55 (200 k entries, first half):                                 48 /  64 /  80 / 128 -> 43 / 51 / 52 / 39
// i.e. the best count falls about linearly with m: tree workgroups = places x (0.342 - 0.367 m), between a third and 1.5 x the
// default (ca = 0.342, cb = 0.367; AZMI_PIPE_BALANCE_A / _B set other coefficients).  m is taken over the PREVIOUS call; the count moves 8 workgroups per call,
// between epochs only (a slot's home is slot % tree workgroups for one epoch at a time; between epochs a slot is whole in HBM).  The
// games do not depend on it (a slot's game is a function of its seed alone).
void pipe_balance(PipeState* ps, const PipeCtl& hc, double ca, double cb) {
  if (!ps->balance || !ps->calibrated || ps->places == 0u) return;
  const unsigned long long ds = hc.sims_total - ps->bal_sims, db = hc.tile_boards - ps->bal_boards;
  ps->bal_sims = hc.sims_total; ps->bal_boards = hc.tile_boards;
  if (ds < 4096ull || db == 0ull) return;
  const double m = static_cast<double>(db) / static_cast<double>(ds);
  const double share = std::max(0.02, ca - cb * m);
  uint32_t want = static_cast<uint32_t>(static_cast<double>(ps->places) * share + 0.5);
  want = std::min(ps->tree_wgs_alloc, std::max(ps->tree_wgs_min, (want + 4u) / 8u * 8u));
  if (want + 8u <= ps->tree_wgs) ps->tree_wgs -= 8u;
  else if (want >= ps->tree_wgs + 8u) ps->tree_wgs += 8u;
  else return;
  ps->tree_wgs = std::min(ps->tree_wgs_alloc, std::max(ps->tree_wgs_min, ps->tree_wgs));
  ps->pa.n_tree_wgs = ps->tree_wgs;
  ps->net_wgs = ps->places > ps->tree_wgs ? ps->places - ps->tree_wgs : 1u;
}

// probes the S3-FIFO missed and the in-epoch answer table answered (azmi_pm_cache_stats moves them from misses to hits)
unsigned long long azmi_host_pipe_l0_hits(azmi_pm* pm, hipStream_t st) {
  if (!pm->pipe || !pm->pipe->pa.l0) return 0ull;
  unsigned long long v = 0;
  if (hipMemcpyAsync(&v, &pm->pipe->pa.ctl->l0_hits, sizeof(v), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return 0ull;
  return v;
}
