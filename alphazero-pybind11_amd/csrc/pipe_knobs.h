// Every environment knob of the pipeline (diagnostics and experiments; scripts/README.md lists them), in two structs with one reader
// each.  WHEN a variable is read is part of its meaning - tests and scripts set them between calls:
//   PipeKnobs       read once at the top of every azmi_run_pipeline* call (pipeline_run.hip)
//   PipeSetupKnobs  what shapes the pipeline state, read by pipeline_state.hip at the moment its user runs: pipe_plan (every call and
//                   every azmi_pipeline_supported*), pipe_create (the call that creates the state), pipe_size_net (a call that sizes
//                   the net side: the first one, and one that brings a net of the other precision tier), pipe_calibrate (every call
//                   until the census has succeeded).  Its last two fields are read once per process and kept in the state.
// Host code only: included by pipeline_state.hip and pipeline_run.hip.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>

namespace azmi {

// The environment knobs of ONE call, parsed once at its top (per call, not per process: tests and scripts set them between calls).
struct PipeKnobs {
  bool net_conveyor = false;                 // AZMI_PIPE_NET=conveyor: refused (pipe_no_conveyor)
  bool no_l0 = false;                        // AZMI_PIPE_NO_L0: no answer table
  int l0_log2 = -1;                          // AZMI_PIPE_L0_LOG2: log2 of the answer table's entries (-1: from the S3-FIFO's size)
  uint32_t l0_wb = 0;                        // AZMI_PIPE_L0_WB
  uint32_t idle_num = 0;                     // AZMI_PIPE_IDLE_FRAC (0.125), in 1024ths: an epoch ends when this share of the slots waits for the move step
  unsigned long long cap_ticks = 0;          // AZMI_PIPE_CAP_MS (250), in 100 MHz ticks: the wall-clock cap of an epoch, a stall detector
  unsigned long long soft_ticks = 0;         // AZMI_PIPE_SOFT_MS (a quarter of the cap): an epoch that runs long simply ends here
  uint32_t test_drop = 0;                    // AZMI_PIPE_TEST_DROP (the error-path test)
  // AZMI_PIPE_TILE, the net kernel's tile selection: 0 = by what a window brings within its patience (<= 3 requests: the 3-board tile), 1 = 6-board tiles only,
  // 2 = 3-board tiles only.  At 4096 slots 0 and 2 measure the same (the net side has places to spare); at 16384 slots the
  // 3-board tile's capacity (19.5 M evaluations/s on 416 workgroups) is the limit, so 0 it is.
  int tile = 0;
  bool net_all = false;                      // AZMI_PIPE_NET_ALL: launch every net workgroup the chip holds
  bool prof = false, hist = false;           // AZMI_PIPE_PROF, AZMI_PIPE_HIST
  bool debug = false;                        // AZMI_PIPE_DEBUG: read the error word back after every epoch
  double balance_a = 0.342, balance_b = 0.367;      // AZMI_PIPE_BALANCE_A / _B (pipe_balance)
};
inline PipeKnobs pipe_read_knobs() {
  PipeKnobs k;
  if (const char* e = getenv("AZMI_PIPE_NET")) k.net_conveyor = strcmp(e, "conveyor") == 0;
  k.no_l0 = getenv("AZMI_PIPE_NO_L0") != nullptr;
  if (const char* e = getenv("AZMI_PIPE_L0_LOG2")) k.l0_log2 = std::min(26, std::max(4, atoi(e)));
  if (const char* e = getenv("AZMI_PIPE_L0_WB")) k.l0_wb = static_cast<uint32_t>(atoi(e));
  double idle_frac = 0.125;
  if (const char* e = getenv("AZMI_PIPE_IDLE_FRAC")) idle_frac = atof(e);
  k.idle_num = std::max<uint32_t>(1u, std::min<uint32_t>(1024u, static_cast<uint32_t>(idle_frac * 1024.0)));
  double cap_ms = 250.0;
  if (const char* e = getenv("AZMI_PIPE_CAP_MS")) cap_ms = atof(e);
  k.cap_ticks = static_cast<unsigned long long>(cap_ms * 1e5);
  // (the error-path test asks for a soft limit beyond the cap)
  k.soft_ticks = k.cap_ticks / 4u;
  if (const char* e = getenv("AZMI_PIPE_SOFT_MS")) k.soft_ticks = static_cast<unsigned long long>(atof(e) * 1e5);
  if (const char* e = getenv("AZMI_PIPE_TEST_DROP")) k.test_drop = static_cast<uint32_t>(strtoul(e, nullptr, 0));
  if (const char* e = getenv("AZMI_PIPE_TILE")) k.tile = atoi(e);
  k.net_all = getenv("AZMI_PIPE_NET_ALL") != nullptr;
  k.prof = getenv("AZMI_PIPE_PROF") != nullptr;
  k.hist = getenv("AZMI_PIPE_HIST") != nullptr;
  k.debug = getenv("AZMI_PIPE_DEBUG") != nullptr;
  if (const char* e = getenv("AZMI_PIPE_BALANCE_A")) k.balance_a = atof(e);
  if (const char* e = getenv("AZMI_PIPE_BALANCE_B")) k.balance_b = atof(e);
  return k;
}

// The knobs that shape the pipeline state when it is planned, created, sized or measured.
struct PipeSetupKnobs {
  // ---- pipe_plan
  // the fast tree kernel (its plain, two-group and Gumbel builds) drives every supported engine; AZMI_PIPE_GENERIC=1 asks for the generic one (every
  // step through the lock-step engine's move-step function: an independent implementation kept as a cross-check, tests/test_gpu_pipeline.py)
  bool generic = false;
  // ---- pipe_create
  uint32_t tree_wgs = 0;                     // AZMI_PIPE_TREE_WGS: the tree workgroups, instead of pipe_tree_wgs_for's count (0: not set)
  bool net_wgs_set = false;                  // AZMI_PIPE_NET_WGS: the net workgroups, instead of the occupancy answer (pipe_size_net) ...
  uint32_t net_wgs = 0;
  bool no_balance = false;                   // AZMI_PIPE_NO_BALANCE; a count fixed by hand switches pipe_balance off as well
  bool pos0_set = false;                     // AZMI_PIPE_POS0, test hook: the rings' free-running 32-bit positions start here instead of at 0 (a long run
  uint32_t pos0 = 0;                         // wraps them after ~2 minutes: tests/test_gpu_pipeline.py starts just below 2^32)
  // inline budget of a pass: a group runs up to 8 simulations whose answers are at hand (cache hits, terminal leaves) before its slot
  // re-queues (M simulations/s at 3 / 5 / 6 / 8 / 16: 82 / 89-96 / 102 / 102-110 / 97-100); a pass may also end early once fewer than
  // min_active of its groups are still running (round 3: 3; with home workgroups 0 - the stragglers' slots would only queue for the
  // same four wavefronts).  An engine created with an explicit max_inline keeps it as its budget.
  uint32_t max_inline = 0;                   // AZMI_PIPE_INLINE (0: not set - the engine's explicit max_inline, else 8)
  uint32_t min_active = 0;                   // AZMI_PIPE_MIN_ACTIVE
  // net side: a workgroup draws a 6-request window (the 6-board tile: capacity) when at least big_at requests wait in the ring, else a
  // 3-request window (the 3-board tile: 39 us instead of 60 alone - with 4096 slots a slot's wait for its answer is what is short)
  // 1: the workgroup's own experience (round 5); round 4: 96      (same-box A/B at 4096 slots: 48 -> 100.0, 96 / 128 / 192 -> 102.4 M simulations/s; 16384 slots: no difference)
  uint32_t big_at = 1;                       // AZMI_PIPE_BIG_AT
  uint32_t take_wait = 0;                    // AZMI_PIPE_TAKE_WAIT (PipeArrays::take_wait)
  int cu_split = -1;                         // AZMI_PIPE_CU_SPLIT=T: the tree kernel on a stream masked to T CUs, the net kernel on the others (-1: not set)
  // ---- pipe_calibrate
  bool no_calibrate = false;                 // AZMI_PIPE_NO_CALIBRATE: take the occupancy answer as it is
  // ---- once per process (kept in PipeState by pipe_create)
  bool diag = false;                         // AZMI_PIPE_DIAG: the generic tree kernel's DIAG build (pipe_tree_kernels.h)
  // AZMI_WHATIF_NET_DEPTH=n (a measurement knob, never a result: the answers are another net's): the tiles run n residual blocks
  // instead of the net's - how much of the pipeline's rate is the tile's latency
  int whatif_depth = 0;
};
inline PipeSetupKnobs pipe_read_setup_knobs() {
  PipeSetupKnobs k;
  k.generic = getenv("AZMI_PIPE_GENERIC") != nullptr;
  if (const char* e = getenv("AZMI_PIPE_TREE_WGS")) k.tree_wgs = static_cast<uint32_t>(std::max(1, atoi(e)));
  if (const char* e = getenv("AZMI_PIPE_NET_WGS")) { k.net_wgs_set = true; k.net_wgs = static_cast<uint32_t>(atoi(e)); }
  k.no_balance = getenv("AZMI_PIPE_NO_BALANCE") != nullptr;
  if (const char* e = getenv("AZMI_PIPE_POS0")) { k.pos0_set = true; k.pos0 = static_cast<uint32_t>(strtoul(e, nullptr, 0)); }
  if (const char* e = getenv("AZMI_PIPE_INLINE")) k.max_inline = static_cast<uint32_t>(std::max(1, atoi(e)));
  if (const char* e = getenv("AZMI_PIPE_MIN_ACTIVE")) k.min_active = static_cast<uint32_t>(std::max(0, atoi(e)));
  if (const char* e = getenv("AZMI_PIPE_BIG_AT")) k.big_at = static_cast<uint32_t>(std::max(0, atoi(e)));
  if (const char* e = getenv("AZMI_PIPE_TAKE_WAIT")) k.take_wait = static_cast<uint32_t>(std::max(0, atoi(e)));
  if (const char* e = getenv("AZMI_PIPE_CU_SPLIT")) k.cu_split = std::max(0, atoi(e));
  k.no_calibrate = getenv("AZMI_PIPE_NO_CALIBRATE") != nullptr;
  static const bool diag = getenv("AZMI_PIPE_DIAG") != nullptr;
  static const int whatif_depth = [] { const char* e = getenv("AZMI_WHATIF_NET_DEPTH"); return e ? atoi(e) : 0; }();
  k.diag = diag;
  k.whatif_depth = whatif_depth;
  return k;
}

}  // namespace azmi
