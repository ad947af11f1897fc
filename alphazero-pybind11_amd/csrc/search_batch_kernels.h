// Batched position search: N independent search trees, each on its own position, advanced in lock step - one simulation of
// every tree per (find-leaves, process-results) launch pair.  What the reference's evaluation tools do from Python with N MCTS
// objects (frozen_eval.py:545-660, mcts_analysis.py:923-1049, play.py:292-343): search many positions to a fixed visit budget,
// leaves batched into one net call, no move played.
//
// Tree i lives in slot i of an engine with N slots (seat 0's tree, like the stand-alone MCTS object on its one slot) and is
// driven by the same per-tree functions: SlotCtx / BigSlot load, find_leaf, process_result, cache_lookup, emit_leaf, and the
// read-outs of mcts_query_slot.  The kernels here only map the grid to slots and keep the per-tree bookkeeping of a step:
//   pend[i]    what the tree's pending simulation waits for (SbPend)
//   status[i]  0, or why the tree stopped (-1 bad start position, -2 find_leaf failed: arena / path capacity)
//   row_of[i]  row of the compacted leaf batch that holds tree i's leaf (kNoRow = none)
//   rows[r]    tree index of compacted row r, ascending;  *n_rows = number of rows
//   n_term[i]  simulations of tree i that ended in a terminal leaf
#pragma once
#include "mcts_object_kernels.h"

namespace azmi {

enum SbPend : uint8_t {
  kPendNone = 0,    // nothing to back up: terminal leaf (backed up by the find kernel), or a stopped tree
  kPendRow = 1,     // the leaf's planes are in the slot's canonical row: the evaluator's answer is awaited
  kPendCached = 2,  // a cache hit: the answer is already in the slot's (v, pi) rows
  kPendRandom = 3   // EvalType::RANDOM: process_result synthesises dumb_eval
};
constexpr uint32_t kNoRow = 0xFFFFFFFFu;

struct SbArrays {
  uint8_t* pend;       // [N]
  int32_t* status;     // [N]
  uint32_t* row_of;    // [N]
  uint32_t* rows;      // [N]
  uint32_t* n_rows;    // [1]
  uint32_t* n_term;    // [N] simulations that ended in a terminal leaf since the last reset
};

// ---- seed: N serialized positions -> N root states, N empty trees, one pcg32 stream per tree -----------------------------
// moves[offs[i] .. offs[i + 1]) are tree i's moves from its start position (init + i * init_stride, NULL = initial position)
template <class GM>
__global__ __launch_bounds__(256) void k_sb_seed(EngineParams ep, EngineArrays ar, SbArrays sb, uint32_t n, const uint8_t* init, uint32_t init_stride,
                                                 const int32_t* moves, const uint32_t* offs, const uint64_t* seeds) {
  constexpr int G = GM::GROUP;
  const uint32_t gtid = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t slot = gtid / G, lane = gtid % G;
  if (slot >= n) return;
  SlotCtx<GM> c(ep, ar, slot, lane);
  c.load();
  c.start_game();          // empty trees (root = node 0, arena bump = 1), Gumbel target 0
  typename GM::State st;
  const uint32_t o0 = offs[slot], o1 = offs[slot + 1];
  const bool ok = mcts_replay_state<GM>(init ? init + static_cast<size_t>(slot) * init_stride : nullptr, moves + o0, o1 - o0, st);
  if (ok) c.gs = st;
  Pcg32 g; g.seed(seeds[slot]);       // MCTS::seed_thread_rng(seed): the stream of MCTS(seed=...)
  c.rng.state = g.state;
  c.cur = 0; c.plen = 0; c.flags = 0;
  if (lane == 0) {
    sb.status[slot] = ok ? 0 : -1; sb.pend[slot] = kPendNone; sb.row_of[slot] = kNoRow; sb.n_term[slot] = 0;
    ar.c_sims[slot] = 0; ar.c_evals[slot] = 0;
  }
  c.store(kSlotWaitEval);
}

template <class GM>
__global__ __launch_bounds__(64) void k_sb_big_seed(EngineParams ep, EngineArrays ar, SbArrays sb, uint32_t n, const uint8_t* init, uint32_t init_stride,
                                                    const int32_t* moves, const uint32_t* offs, const uint64_t* seeds) {
  __shared__ BigScratch<GM> sm;
  const uint32_t slot = blockIdx.x, lane = threadIdx.x;
  if (slot >= n) return;
  BigSlot<GM> c(ep, ar, sm, slot, lane);
  c.load();
  c.start_game();
  const uint32_t o0 = offs[slot], o1 = offs[slot + 1];
  const bool ok = mcts_big_replay<GM>(c, init ? init + static_cast<size_t>(slot) * init_stride : nullptr, init_stride, moves + o0, o1 - o0);
  c.sync();
  if (!ok) {     // a valid (unused) state behind the error status
    c.start_game();
    c.sync();
  }
  if constexpr (!is_stargambit<GM>::value) {   // the root's repetition list: load() reads it back from HBM
    uint64_t* gl = ar.rep_list + static_cast<size_t>(slot) * (GM::MAX_TURNS + 2);
    for (uint32_t i = lane; i < c.glen; i += 64) gl[i] = sm.glist[i];
  }
  Pcg32 g; g.seed(seeds[slot]);
  c.rng.state = g.state;
  c.cur = 0; c.plen = 0; c.flags = 0;
  if (lane == 0) {
    sb.status[slot] = ok ? 0 : -1; sb.pend[slot] = kPendNone; sb.row_of[slot] = kNoRow; sb.n_term[slot] = 0;
    ar.c_sims[slot] = 0; ar.c_evals[slot] = 0;
  }
  c.sync();
  c.store(kSlotWaitEval);
}

// ---- find-leaves step: one simulation's descent for every live tree ------------------------------------------------------
// A terminal leaf is backed up here.  Otherwise: RANDOM evaluator -> kPendRandom; cache hit -> the answer lands in the slot's
// (v, pi) rows, kPendCached; else the leaf's planes go to the slot's canonical row (and its key to ar.cache_keys when a cache
// is attached), kPendRow.  k_sb_compact then numbers the kPendRow trees in ascending tree order.
template <class GM>
__global__ __launch_bounds__(256) void k_sb_find(EngineParams ep, EngineArrays ar, SbArrays sb, uint32_t n, uint32_t eval_random) {
  constexpr int G = GM::GROUP;
  const uint32_t gtid = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t slot = gtid / G, lane = gtid % G;
  if (slot >= n) return;
  if (sb.status[slot] != 0) {
    if (lane == 0) { sb.pend[slot] = kPendNone; if (ep.cache_on) ar.cache_keys[slot] = 0; }
    return;
  }
  SlotCtx<GM> c(ep, ar, slot, lane);
  c.load();
  typename GM::State leaf;
  uint32_t term = 0;
  uint8_t pend = kPendNone;
  uint64_t ins_key = 0;
  if (!c.find_leaf(0, leaf, term)) {
    if (lane == 0) sb.status[slot] = -2;
  } else if (term != 0) {
    c.process_result(0, true, false);     // the cached terminal scores; neither priors nor root noise are involved
    if (lane == 0) sb.n_term[slot] += 1;
  } else if (eval_random) {
    pend = kPendRandom;
  } else {
    const uint64_t key = GM::key(leaf);
    float hit_pi = 0.0f, hit_v = 0.0f;
    if (ep.cache_on && c.cache_lookup(key, 0, hit_pi, hit_v)) pend = kPendCached;
    else {
      c.emit_leaf(leaf, key);
      if (lane == 0) ar.c_evals[slot] += 1;
      ins_key = cache_key(key);
      pend = kPendRow;
    }
  }
  if (lane == 0) { sb.pend[slot] = pend; if (ep.cache_on) ar.cache_keys[slot] = ins_key; }
  c.store(kSlotWaitEval);
}

template <class GM>
__global__ __launch_bounds__(64) void k_sb_big_find(EngineParams ep, EngineArrays ar, SbArrays sb, uint32_t n, uint32_t eval_random) {
  __shared__ BigScratch<GM> sm;
  const uint32_t slot = blockIdx.x, lane = threadIdx.x;
  if (slot >= n) return;
  if (sb.status[slot] != 0) {
    if (lane == 0) { sb.pend[slot] = kPendNone; if (ep.cache_on) ar.cache_keys[slot] = 0; }
    return;
  }
  BigSlot<GM> c(ep, ar, sm, slot, lane);
  c.load();
  typename GM::State leaf;
  uint32_t term = 0;
  uint8_t pend = kPendNone;
  uint64_t ins_key = 0;
  if (!c.find_leaf(0, leaf, term)) {
    if (lane == 0) sb.status[slot] = -2;
  } else if (term != 0) {
    c.process_result(0, true, false);
    if (lane == 0) sb.n_term[slot] += 1;
  } else if (eval_random) {
    pend = kPendRandom;
  } else {
    const uint64_t key = c.emit_leaf(leaf);
    if (ep.cache_on && c.cache_lookup(key, 0)) pend = kPendCached;
    else {
      if (lane == 0) ar.c_evals[slot] += 1;
      ins_key = cache_key(key);
      pend = kPendRow;
    }
  }
  if (lane == 0) { sb.pend[slot] = pend; if (ep.cache_on) ar.cache_keys[slot] = ins_key; }
  c.sync();
  c.store(kSlotWaitEval);
}

// ---- compaction: the kPendRow trees in ascending tree order (one workgroup; the order is deterministic) ---------------------
__global__ __launch_bounds__(1024) void k_sb_compact(SbArrays sb, uint32_t n) {
  __shared__ uint32_t s_sum[1024];
  const uint32_t tid = threadIdx.x;
  const uint32_t per = (n + 1023u) / 1024u;
  const uint32_t lo = min(n, tid * per), hi = min(n, lo + per);
  uint32_t cnt = 0;
  for (uint32_t i = lo; i < hi; ++i) cnt += sb.pend[i] == kPendRow ? 1u : 0u;
  s_sum[tid] = cnt;
  __syncthreads();
  for (uint32_t off = 1; off < 1024u; off <<= 1) {     // inclusive scan
    const uint32_t add = tid >= off ? s_sum[tid - off] : 0u;
    __syncthreads();
    s_sum[tid] += add;
    __syncthreads();
  }
  uint32_t row = s_sum[tid] - cnt;
  for (uint32_t i = lo; i < hi; ++i) {
    if (sb.pend[i] == kPendRow) { sb.row_of[i] = row; sb.rows[row] = i; ++row; }
    else sb.row_of[i] = kNoRow;
  }
  if (tid == 1023u) *sb.n_rows = s_sum[1023];
}

// the step API's leaf batch: row r = the canonical planes of tree rows[r]
__global__ __launch_bounds__(256) void k_sb_gather(SbArrays sb, uint32_t n, const float* canon, uint32_t chw, float* batch) {
  const uint32_t slot = blockIdx.x;
  if (slot >= n) return;
  const uint32_t r = sb.row_of[slot];
  if (r == kNoRow) return;
  const float* src = canon + static_cast<size_t>(slot) * chw;
  float* dst = batch + static_cast<size_t>(r) * chw;
  for (uint32_t e = threadIdx.x; e < chw; e += blockDim.x) dst[e] = src[e];
}

// ---- process-results step: priors, optional root noise, backup --------------------------------------------------------------
// v_rows / pi_rows: the evaluator's answers by COMPACTED row (step API), or NULL when they are already in the slot-indexed
// rows ar.v / ar.pi (the net ran over the row list; cache hits put theirs there)
template <class GM>
__global__ __launch_bounds__(256) void k_sb_process(EngineParams ep, EngineArrays ar, SbArrays sb, uint32_t n, uint32_t root_noise,
                                                    const float* v_rows, const float* pi_rows) {
  constexpr int G = GM::GROUP;
  constexpr uint32_t P = GM::P, M = GM::M;
  const uint32_t gtid = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t slot = gtid / G, lane = gtid % G;
  if (slot >= n) return;
  const uint8_t pend = sb.pend[slot];
  if (pend == kPendNone) return;
  SlotCtx<GM> c(ep, ar, slot, lane);
  c.load();
  if (pend == kPendRow && v_rows) {
    const uint32_t r = sb.row_of[slot];
    if (lane <= P) ar.v[static_cast<size_t>(slot) * (P + 1) + lane] = v_rows[static_cast<size_t>(r) * (P + 1) + lane];
    if (lane < M) ar.pi[static_cast<size_t>(slot) * M + lane] = pi_rows[static_cast<size_t>(r) * M + lane];
  }
  c.process_result(0, pend != kPendRandom, root_noise != 0);    // (starts with the lane group's fence)
  if (lane == 0) sb.pend[slot] = kPendNone;
  c.store(kSlotWaitEval);
}

template <class GM>
__global__ __launch_bounds__(64) void k_sb_big_process(EngineParams ep, EngineArrays ar, SbArrays sb, uint32_t n, uint32_t root_noise,
                                                       const float* v_rows, const float* pi_rows) {
  __shared__ BigScratch<GM> sm;
  constexpr uint32_t P = GM::P, M = GM::M;
  const uint32_t slot = blockIdx.x, lane = threadIdx.x;
  if (slot >= n) return;
  const uint8_t pend = sb.pend[slot];
  if (pend == kPendNone) return;
  BigSlot<GM> c(ep, ar, sm, slot, lane);
  c.load();
  if (pend == kPendRow && v_rows) {
    const uint32_t r = sb.row_of[slot];
    if (lane <= P) ar.v[static_cast<size_t>(slot) * (P + 1) + lane] = v_rows[static_cast<size_t>(r) * (P + 1) + lane];
    for (uint32_t m = lane; m < M; m += 64) ar.pi[static_cast<size_t>(slot) * M + m] = pi_rows[static_cast<size_t>(r) * M + m];
    c.sync();
  }
  c.process_result(0, pend != kPendRandom, root_noise != 0);
  if (lane == 0) sb.pend[slot] = kPendNone;
  c.sync();
  c.store(kSlotWaitEval);
}

// ---- read-out: one launch for all trees; tree i writes out_f + i * stride_f / out_u + i * stride_u ----------------------------
template <class GM>
__global__ __launch_bounds__(256) void k_sb_query(EngineParams ep, EngineArrays ar, uint32_t n, uint32_t kind, float temp, uint32_t arg,
                                                  float* out_f, uint32_t stride_f, uint32_t* out_u, uint32_t stride_u) {
  constexpr int G = GM::GROUP;
  const uint32_t gtid = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t slot = gtid / G, lane = gtid % G;
  if (slot >= n) return;
  mcts_query_slot<GM>(ep, ar, slot, lane, kind, temp, arg, out_f + static_cast<size_t>(slot) * stride_f, out_u + static_cast<size_t>(slot) * stride_u);
}

template <class GM>
__global__ __launch_bounds__(64) void k_sb_big_query(EngineParams ep, EngineArrays ar, uint32_t n, uint32_t kind, float temp, uint32_t arg,
                                                     float* out_f, uint32_t stride_f, uint32_t* out_u, uint32_t stride_u) {
  __shared__ BigScratch<GM> sm;
  const uint32_t slot = blockIdx.x;
  if (slot >= n) return;
  mcts_big_query_slot<GM>(ep, ar, sm, slot, threadIdx.x, kind, temp, arg, out_f + static_cast<size_t>(slot) * stride_f,
                          out_u + static_cast<size_t>(slot) * stride_u);
}

}  // namespace azmi
