// Host-side state of the asynchronous tree / net pipeline of one engine and what the translation units behind azmi_run_pipeline*
// share:
//   pipeline.hip        the ONE device module of pipe_tree_kernels.h, pipe_net_kernels.h and pipe_debug_kernels.h (a kernel's code
//                       depends on its module-mates and on the order they are instantiated in, DESIGN.md sections 1 and 8.3; and
//                       without relocatable device code a kernel is launched, and asked about, only where it is defined): the
//                       pipe_launch_* functions below and nothing else
//   pipeline_state.hip  the state: creation, net sizing, stream pairing, the workgroup census, the tree / net balance, the plan of
//                       a call, azmi_pipeline_supported*
//   pipeline_run.hip    a call: prepare, one epoch's launches and event edges, finish; azmi_run_pipeline*
//   pipeline_debug.hip  the host halves of the four azmi_debug_* entry points
// The last three are host code only: no kernel header, no launch of their own, no device code in their objects.  An edit to them
// cannot move a kernel.  The environment knobs are in pipe_knobs.h.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/azmi.h"
#include "engine_host.h"
#include "leafnet_c4_types.h"
#include "pipe_types.h"

namespace azmi {

struct PipeState {
  PipeArrays pa{};
  std::vector<void*> allocs;
  hipStream_t net_stream = nullptr;
  hipStream_t paired_with = nullptr;     // the tree-side stream net_stream was last seen running beside
  bool paired = false;
  std::vector<hipStream_t> parked;       // streams that shared a hardware queue with a tree-side stream (kept: destroying one frees its queue slot for the next try)
  uint32_t* pair_flag = nullptr;
  hipEvent_t ev_go = nullptr, ev_net = nullptr;
  uint32_t net_wgs = 0, tree_wgs = 0, tree_block = 256;
  uint32_t net_launch = 0;          // net workgroups an epoch really launches: net_wgs, held to what the engine's slots can keep busy
  std::vector<hipEvent_t> tev;      // timing events: four per epoch of a run (net kernel start / end, tree kernel start / end)
  size_t lds_bytes = 0;
  bool sized = false, x3 = false;   // pipe_size_net has run for a net of this precision tier
  bool np1_valid = false;           // this call has a second net (model group 1): its weights
  azmi_net_dev::NetPtrs np1{};
  int kind = 0;                     // PipePlan::kind of the current call (which tree kernel)
  bool calibrated = false;          // net_wgs has been measured beside the tree workgroups (pipe_calibrate)
  uint32_t calib_rounds = 0;
  // balance between the two sides (pipe_balance): rings are allocated for tree_wgs_alloc workgroups, `places` = tree + net workgroups
  // the chip was measured to hold, the cumulative counters are those of the previous call
  uint32_t tree_wgs_alloc = 0, tree_wgs_min = 1, tree_wgs_default = 1, places = 0;
  bool balance = false;
  unsigned long long bal_sims = 0, bal_boards = 0;
  uint32_t lost_seen = 0;           // PipeCtl::lost_total already reported
  const void* l0_nets[2] = {nullptr, nullptr};      // the weight images the answer table's entries were computed with (group 0, group 1)
  // CU split (AZMI_PIPE_CU_SPLIT=T): the tree kernel on a stream masked to T CUs, the net kernel on the others
  uint32_t cu_split = 0, cu_total = 0;
  hipStream_t tree_stream = nullptr;
  hipEvent_t ev_tree = nullptr;
  // the two once-per-process knobs (PipeSetupKnobs): the generic tree kernel's DIAG build, the what-if depth of the net kernel's tiles
  bool diag = false;
  int whatif_depth = 0;
};

// how a call is driven: which tree kernel, which model groups have a net behind their request ring
struct PipePlan {
  int kind = 0;                       // 0 = not supported, 1 = fast kernel (plain PUCT, one group), 2 = generic kernel (any search, <= 2 groups)
  bool tree_only = false;             // no net kernel at all (every seat RANDOM)
  uint32_t net_groups = 0;            // bit g: nets[g] serves group g's ring
  azmi_net_c4_view view[2]{};         // view[g] of group g's net (view[1] = view[0] when group 1 has none)
};

}  // namespace azmi

// a zeroed device array that lives as long as the state
template <class T>
int pipe_alloc(azmi::PipeState* ps, T*& p, size_t n) {
  void* q = nullptr;
  const size_t sz = std::max<size_t>(n, 1) * sizeof(T);
  AZMI_HIP_TRY(hipMalloc(&q, sz));
  ps->allocs.push_back(q);
  // hipMemset is asynchronous with respect to the host and runs on the null stream, which the (non-blocking) streams of the
  // pipeline do not wait for: without the synchronisation the zeroes can land while the first epoch is already running
  // (seen: the epoch block wiped under a running epoch of the second engine of a process)
  AZMI_HIP_TRY(hipMemset(q, 0, sz));
  AZMI_HIP_TRY(hipStreamSynchronize(nullptr));
  p = static_cast<T*>(q);
  return AZMI_OK;
}

// ---- defined in pipeline_state.hip ----------------------------------------------------------------------------------------------------
azmi::PipePlan pipe_plan(const azmi_pm* pm, azmi_net* const* nets, uint32_t num_nets);
int pipe_no_conveyor();
int pipe_create(azmi_pm* pm);
int pipe_size_net(azmi_pm* pm, azmi::PipeState* ps, const azmi_net_c4_view& view);
int pipe_pair_streams(azmi::PipeState* ps, hipStream_t st);
int pipe_calibrate(azmi_pm* pm, azmi::PipeState* ps, hipStream_t st, const azmi_net_c4_view& view);
void pipe_balance(azmi::PipeState* ps, const azmi::PipeCtl& hc, double ca, double cb);

// ---- defined in pipeline.hip: one launch function per kernel, on `st`, arguments as the kernels take them -------------------------------
// the LDS bytes of a net workgroup of this precision tier, set as the dynamic-LDS limit of its kernels, and the runtime's answer to
// how many such workgroups a CU holds
int pipe_net_occupancy(bool x3, size_t* lds_bytes, int* per_cu);
// ps->tree_wgs workgroups of the tree kernel of ps->kind (the fast one: its Gumbel, two-group, profiled or plain build)
void pipe_launch_tree(azmi_pm* pm, azmi::PipeState* ps, const azmi::PipeArrays& pa, hipStream_t st, bool prof);
// `wgs` workgroups of the net kernel of ps->x3 with tile selection `mode`
int pipe_launch_net(azmi::PipeState* ps, const azmi_net_c4_view& view, int mode, uint32_t wgs, hipStream_t st, const azmi::PipeArrays& pa);
void pipe_launch_pair_wait(uint32_t* flag, hipStream_t st);
void pipe_launch_pair_set(uint32_t* flag, hipStream_t st);
void pipe_launch_seed(azmi_pm* pm, const azmi::PipeArrays& pa, hipStream_t st);
void pipe_launch_settle(azmi_pm* pm, const azmi::PipeArrays& pa, hipStream_t st);
void pipe_launch_cache_insert(azmi_pm* pm, const azmi::PipeArrays& pa, uint32_t blocks, uint32_t late, hipStream_t st);
// diagnostics (null stream: the group primitives; `st`: the net drain's synthetic requests and its ring reset)
void pipe_launch_debug_group_select(uint32_t rows, const uint32_t* k8, const uint32_t* n64, const float* q64, const float* p64, const float* vpar8,
                                    const uint32_t* npar8, const float* fpu8, const float* cpuct8, const unsigned long long* pred, float* sum64,
                                    uint32_t* best64, uint32_t* all64);
void pipe_launch_debug_group_expand(bool lane_pack, uint32_t rows, uint32_t reps, uint32_t cap, azmi::NodeRec* nodes, azmi::Control* ctl, const uint64_t* bb0,
                                    const uint64_t* bb1, const uint32_t* player, const uint64_t* rng_in, uint32_t* words, uint64_t* rng_out);
void pipe_launch_fill(const azmi::PipeArrays& pa, uint32_t n, uint32_t S, uint64_t seed, hipStream_t st);
void pipe_launch_head_reset(const azmi::PipeArrays& pa, hipStream_t st);
