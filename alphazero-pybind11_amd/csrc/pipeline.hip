// The asynchronous tree / net pipeline of the Connect4 engine (see pipe_types.h for the structure and the hand-off
// protocol): persistent tree wavefronts, mover wavefronts and net workgroups for one EPOCH, then - at a kernel boundary - the
// position-cache inserts of everything the net answered in the epoch, game restarts (k_assign of the lock-step engine) and the
// move steps the mover wavefronts did not get to.
//
// Reference behaviour restated: the worker loop of PlayManager::play (play_manager.cc:258-600) with its queues
// (concurrent_queue.h:130-217) and GameRunner's batcher / gpu_loop / result_worker threads (game_runner.py:483-552, 651-726);
// the search itself is k_sim's (engine_kernels.h): MCTS::process_result (mcts.cc:500-555), MCTS::find_leaf (mcts.cc:462-498),
// Node::add_children (mcts.cc:93-101), S3FIFOCache::find / insert (s3fifo_cache.h:41-80).
// A slot's game is a function of its seed alone (the answer to a position does not depend on where or when the net evaluates
// it), so the games are the lock-step engine's games: tests/test_gpu_pipeline.py.
//
// This file is the ONE device module of the pipeline: the three kernel headers, in this order, and one thin launch function per
// kernel (pipeline_host.h), in the order the kernels were first launched from when all of this was one file - the order of first
// instantiation is part of a kernel's code (DESIGN.md sections 1 and 8.3).  Host logic lives in pipeline_state.hip,
// pipeline_run.hip and pipeline_debug.hip.
#include "pipeline_host.h"
#include "pipe_tree_kernels.h"
#include "pipe_net_kernels.h"
#include "pipe_debug_kernels.h"

using namespace azmi;

// the persistent net kernel's instantiations: tile selection x precision tier
using PipeNetFn = void (*)(azmi_net_dev::NetDesc, azmi_net_dev::NetPtrs, azmi_net_dev::NetPtrs, PipeArrays);
static PipeNetFn pipe_net_fn(int mode, bool x3) {
  if (x3) return mode == 1 ? &k_pipe_net<1, true> : mode == 2 ? &k_pipe_net<2, true> : &k_pipe_net<0, true>;
  return mode == 1 ? &k_pipe_net<1, false> : mode == 2 ? &k_pipe_net<2, false> : &k_pipe_net<0, false>;
}

int pipe_net_occupancy(bool x3, size_t* lds_bytes, int* per_cu) {
  *lds_bytes = (x3 ? azmi_net_dev::c4::TileBigX3::LDS_BYTES : azmi_net_dev::c4::TileBig::LDS_BYTES) + kPipeXs;
  for (int mode = 0; mode < 3; ++mode)
    AZMI_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(pipe_net_fn(mode, x3)), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(*lds_bytes)));
  AZMI_HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, reinterpret_cast<const void*>(pipe_net_fn(0, x3)), 256, *lds_bytes));
  return AZMI_OK;
}

int pipe_launch_net(PipeState* ps, const azmi_net_c4_view& view, int mode, uint32_t wgs, hipStream_t st, const PipeArrays& pa) {
  azmi_net_dev::NetDesc nd = view.nd;
  if (ps->whatif_depth > 0 && ps->whatif_depth < nd.depth) nd.depth = ps->whatif_depth;
  pipe_net_fn(mode, ps->x3)<<<wgs, 256, ps->lds_bytes, st>>>(nd, view.np, ps->np1_valid ? ps->np1 : view.np, pa);
  AZMI_HIP_TRY(hipGetLastError());
  return AZMI_OK;
}

void pipe_launch_pair_wait(uint32_t* flag, hipStream_t st) { k_pair_wait<<<1, 1, 0, st>>>(flag); }
void pipe_launch_pair_set(uint32_t* flag, hipStream_t st) { k_pair_set<<<1, 1, 0, st>>>(flag); }

void pipe_launch_tree(azmi_pm* pm, PipeState* ps, const PipeArrays& pa, hipStream_t st, bool prof) {
  if (ps->kind == 2) {
    if (ps->diag) k_pipe_tree_generic<Connect4, 256, true><<<ps->tree_wgs, 256, 0, st>>>(PipeKernArgs{pm->ep, pm->ar, pa});
    else k_pipe_tree_generic<Connect4, 256><<<ps->tree_wgs, 256, 0, st>>>(PipeKernArgs{pm->ep, pm->ar, pa});
  }
  else if (pm->ep.gumbel_on) k_pipe_tree<Connect4, 256, false, true, true><<<ps->tree_wgs, 256, 0, st>>>(PipeKernArgs{pm->ep, pm->ar, pa});
  else if (pa.n_groups > 1u) k_pipe_tree<Connect4, 256, false, true><<<ps->tree_wgs, 256, 0, st>>>(PipeKernArgs{pm->ep, pm->ar, pa});
  else if (prof) k_pipe_tree<Connect4, 256, true><<<ps->tree_wgs, 256, 0, st>>>(PipeKernArgs{pm->ep, pm->ar, pa});
  else k_pipe_tree<Connect4, 256, false><<<ps->tree_wgs, 256, 0, st>>>(PipeKernArgs{pm->ep, pm->ar, pa});
}

// one thread per slot, before and behind an epoch's persistent kernels
void pipe_launch_seed(azmi_pm* pm, const PipeArrays& pa, hipStream_t st) { k_pipe_seed<<<(pm->ep.S + 255u) / 256u, 256, 0, st>>>(pm->ep, pm->ar, pa); }
void pipe_launch_cache_insert(azmi_pm* pm, const PipeArrays& pa, uint32_t blocks, uint32_t late, hipStream_t st) {
  k_pipe_cache_insert<<<blocks, 256, 0, st>>>(pm->ar, pa, late);
}
void pipe_launch_settle(azmi_pm* pm, const PipeArrays& pa, hipStream_t st) { k_pipe_settle<<<(pm->ep.S + 255u) / 256u, 256, 0, st>>>(pm->ep, pm->ar, pa); }

// ---- diagnostics ------------------------------------------------------------------------------------------------------------------------
void pipe_launch_debug_group_select(uint32_t rows, const uint32_t* k8, const uint32_t* n64, const float* q64, const float* p64, const float* vpar8,
                                    const uint32_t* npar8, const float* fpu8, const float* cpuct8, const unsigned long long* pred, float* sum64,
                                    uint32_t* best64, uint32_t* all64) {
  k_debug_group_select<<<rows, 64>>>(k8, n64, q64, p64, vpar8, npar8, fpu8, cpuct8, pred, sum64, best64, all64);
}
void pipe_launch_debug_group_expand(bool lane_pack, uint32_t rows, uint32_t reps, uint32_t cap, NodeRec* nodes, Control* ctl, const uint64_t* bb0,
                                    const uint64_t* bb1, const uint32_t* player, const uint64_t* rng_in, uint32_t* words, uint64_t* rng_out) {
  if (lane_pack) k_debug_group_expand<true><<<rows, 64>>>(reps, cap, nodes, ctl, bb0, bb1, player, rng_in, words, rng_out);
  else k_debug_group_expand<false><<<rows, 64>>>(reps, cap, nodes, ctl, bb0, bb1, player, rng_in, words, rng_out);
}
// `n` synthetic requests behind the ring's tail, then the tail moved over them
void pipe_launch_fill(const PipeArrays& pa, uint32_t n, uint32_t S, uint64_t seed, hipStream_t st) {
  k_pipe_fill<<<(n + 255) / 256, 256, 0, st>>>(pa, n, S, seed);
  k_pipe_fill_done<<<1, 1, 0, st>>>(pa, n);
}
void pipe_launch_head_reset(const PipeArrays& pa, hipStream_t st) { k_pipe_head_reset<<<1, 1, 0, st>>>(pa); }
