// Batched position search: N independent search trees, each on its own position, advanced in lock step - one simulation of
// every tree per (find-leaves, process-results) launch pair.  What the reference's evaluation tools do from Python with N MCTS
// objects (frozen_eval.py:545-660, mcts_analysis.py:923-1049, play.py:292-343): search many positions to a fixed visit budget,
// leaves batched into one net call, no move played.
//
// Tree i lives in slot i of an engine with N slots (seat 0's tree, like the stand-alone MCTS object on its one slot) and is
// driven by the same per-tree functions: SlotCtx / BigSlot load, find_leaf, process_result, cache_lookup, emit_leaf, and the
// read-outs of mcts_query_slot.  The kernels here only map the grid to slots and keep the per-tree bookkeeping of a step:
//   pend[i]    what the tree's pending simulation waits for (SbPend)
//   status[i]  0, or why the tree stopped (SbStatus, < 0), or kSbFinished: the game is over (a move played on the batch
//              reached a terminal state).  Every kernel skips a tree whose status != 0
//   row_of[i]  row of the compacted leaf batch that holds tree i's leaf (kNoRow = none)
//   rows[r]    tree index of compacted row r, ascending;  *n_rows = number of rows
//   n_term[i]  simulations of tree i that ended in a terminal leaf
//
// Every step has two kernels: k_sb_X for Connect4's 8-lane engine (SlotCtx, 256 threads, slot = thread / GROUP) and k_sb_big_X
// for the wavefront-per-tree engine (BigSlot, 64 threads, slot = block, BigScratch in LDS).  They stay plain twins: a body
// shared through a template over the context type computes the same, but the compiler then allocates registers differently
// in most of them.  The grid-to-slot mapping and the loop over a step's descents are written per kernel.  What a second step
// shape would repeat is a named __forceinline__ helper - on the concrete context type (SlotCtx<GM>& or BigSlot<GM>&) where it
// calls a tree function (find_leaf, find_leaf_wu, process_result, playout_eval), across the engines only where it calls none -
// IF every kernel then compiles to the code it had.  That holds for the bookkeeping rows: sb_seed_tail, sb_scan_1024,
// sb_skip_tree, sb_checkpoint_tail, sb_dl_close_tree.  It does not hold for the verdict on a net leaf, the WU-UCT back-up at
// once, the PLAYOUT leaf and the copied (v, pi) row, which stay pasted ("Layout of search_batch_kernels.h").
#pragma once
#include "mcts_object_kernels.h"
#include "search_batch_types.h"      // SbPend, SbStatus, kNoRow and the Sb*Arrays views named below

namespace azmi {

// ---- seed: N serialized positions -> N root states, N empty trees, one pcg32 stream per tree -----------------------------
// moves[offs[i] .. offs[i + 1]) are tree i's moves from its start position (init + i * init_stride, NULL = initial position)
// what both seed kernels end with (before their store): the tree's pcg32 stream, no pending simulation, the tree's bookkeeping rows
template <class Ctx>
__device__ __forceinline__ void sb_seed_tail(Ctx& c, const SbArrays& sb, bool ok, uint64_t seed) {
  Pcg32 g; g.seed(seed);       // MCTS::seed_thread_rng(seed): the stream of MCTS(seed=...)
  c.rng.state = g.state;
  c.cur = 0; c.plen = 0; c.flags = 0;
  if (c.lane == 0) {
    sb.status[c.slot] = ok ? 0 : kSbBadStart; sb.pend[c.slot] = kPendNone; sb.row_of[c.slot] = kNoRow; sb.n_term[c.slot] = 0;
    c.ar.c_sims[c.slot] = 0; c.ar.c_evals[c.slot] = 0;
  }
}

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
  sb_seed_tail(c, sb, ok, seeds[slot]);
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
  sb_seed_tail(c, sb, ok, seeds[slot]);
  c.sync();
  c.store(kSlotWaitEval);
}

// ---- find-leaves step: one simulation's descent for every live tree ------------------------------------------------------
// A terminal leaf is backed up here.  Otherwise: RANDOM evaluator -> kPendRandom; cache hit -> the answer lands in the slot's
// (v, pi) rows, kPendCached; else the leaf's planes go to the slot's canonical row (and its key to ar.cache_keys when a cache
// is attached), kPendRow.  k_sb_compact then numbers the kPendRow trees in ascending tree order.

// a tree that sits a step out (stopped, finished, paused, nothing owed) leaves neither a pending simulation nor a key to insert
__device__ __forceinline__ void sb_skip_tree(const SbArrays& sb, const EngineParams& ep, const EngineArrays& ar, uint32_t slot, uint32_t lane) {
  if (lane == 0) { sb.pend[slot] = kPendNone; if (ep.cache_on) ar.cache_keys[slot] = 0; }
}

template <class GM>
__global__ __launch_bounds__(256) void k_sb_find(EngineParams ep, EngineArrays ar, SbArrays sb, uint32_t n, uint32_t eval_random) {
  constexpr int G = GM::GROUP;
  const uint32_t gtid = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t slot = gtid / G, lane = gtid % G;
  if (slot >= n) return;
  if (sb.status[slot] != 0) { sb_skip_tree(sb, ep, ar, slot, lane); return; }
  SlotCtx<GM> c(ep, ar, slot, lane);
  c.load();
  typename GM::State leaf;
  uint32_t term = 0;
  uint8_t pend = kPendNone;
  uint64_t ins_key = 0;
  if (!c.find_leaf(0, leaf, term)) {
    if (lane == 0) sb.status[slot] = kSbFindFailed;
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
  if (sb.status[slot] != 0) { sb_skip_tree(sb, ep, ar, slot, lane); return; }
  BigSlot<GM> c(ep, ar, sm, slot, lane);
  c.load();
  typename GM::State leaf;
  uint32_t term = 0;
  uint8_t pend = kPendNone;
  uint64_t ins_key = 0;
  if (!c.find_leaf(0, leaf, term)) {
    if (lane == 0) sb.status[slot] = kSbFindFailed;
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
// Inclusive scan of the 1024 threads' counts: -> the thread's exclusive prefix; s_sum[1023] is the total
__device__ __forceinline__ uint32_t sb_scan_1024(uint32_t* s_sum, uint32_t cnt) {
  const uint32_t tid = threadIdx.x;
  s_sum[tid] = cnt;
  __syncthreads();
  for (uint32_t off = 1; off < 1024u; off <<= 1) {
    const uint32_t add = tid >= off ? s_sum[tid - off] : 0u;
    __syncthreads();
    s_sum[tid] += add;
    __syncthreads();
  }
  return s_sum[tid] - cnt;
}

__global__ __launch_bounds__(1024) void k_sb_compact(SbArrays sb, uint32_t n) {
  __shared__ uint32_t s_sum[1024];
  const uint32_t tid = threadIdx.x;
  const uint32_t per = (n + 1023u) / 1024u;
  const uint32_t lo = min(n, tid * per), hi = min(n, lo + per);
  uint32_t cnt = 0;
  for (uint32_t i = lo; i < hi; ++i) cnt += sb.pend[i] == kPendRow ? 1u : 0u;
  uint32_t row = sb_scan_1024(s_sum, cnt);
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

// ======================= several leaves in flight per tree and step (WU-UCT, leaves_per_step = K > 1) ==========================
// One step of tree i = K calls of MCTS::find_leaf_batched (mcts.cc:752-784), each seeing the in-flight marks of the ones before
// it, a back-up at once for every leaf that needs no evaluator (terminal, RANDOM, cache hit), one evaluator call for the rest,
// then MCTS::process_result_batched (mcts.cc:786-851) for the pending ones in ascending order: play.py:_run_one_batch with the
// attempt count fixed at K.  Descent k of tree i owns entry k * N + i ("[K][N]-major") of every step-sized array, so that an
// EngineArrays copy whose canon / v / pi / cache_keys pointers are moved by k * N rows makes emit_leaf, cache_lookup,
// process_result and k_cache_insert, which address rows by slot, work on that entry.  The VISIBLE row order is ascending tree,
// then descent: k_sb_compact_wu numbers the pending entries in that order.  (SbWuArrays)

// `al` is the kernel's own copy of the engine arrays that the slot context reads through: entry (k, slot) becomes "the slot's row"
__device__ __forceinline__ void sb_wu_point(EngineArrays& al, const SbWuArrays& w, size_t row0, uint32_t chw, uint32_t nv, uint32_t np) {
  al.canon = w.canon + row0 * chw; al.v = w.v + row0 * nv; al.pi = w.pi + row0 * np; al.cache_keys = w.keys + row0;
}

// `kk` <= K descents of every live tree (the last step of a search whose visit count is no multiple of K runs the remainder)
template <class GM>
__global__ __launch_bounds__(256) void k_sb_find_wu(EngineParams ep, EngineArrays ar, SbArrays sb, SbWuArrays w, uint32_t n, uint32_t kk,
                                                    uint32_t eval_random, uint32_t root_noise) {
  constexpr int G = GM::GROUP;
  const uint32_t gtid = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t slot = gtid / G, lane = gtid % G;
  if (slot >= n) return;
  if (sb.status[slot] != 0) {
    if (lane == 0) for (uint32_t k = 0; k < kk; ++k) { w.pend[k * n + slot] = kPendNone; w.keys[k * n + slot] = 0; }
    return;
  }
  EngineArrays al = ar;
  SlotCtx<GM> c(ep, al, slot, lane);
  c.load();
  uint32_t* nif = w.wu.nif + c.tree_base(0);
  const uint32_t* path = ar.path + static_cast<size_t>(slot) * ep.max_depth;
  for (uint32_t k = 0; k < kk; ++k) {
    const uint32_t e = k * n + slot;
    sb_wu_point(al, w, static_cast<size_t>(k) * n, GM::CANON, GM::P + 1, GM::M);
    typename GM::State leaf;
    uint32_t term = 0;
    uint8_t pend = kPendNone;
    uint64_t ins_key = 0;
    bool now = false, from_net = true;      // back up at once / with the (v, pi) rows of the entry
    if (!c.find_leaf_wu(0, leaf, term, nif)) {
      // the tree stops: nothing of this step is backed up (reset() clears the root's mark, new nodes get theirs cleared)
      if (lane == 0) { sb.status[slot] = kSbFindFailed; for (uint32_t j = 0; j < kk; ++j) { w.pend[j * n + slot] = kPendNone; w.keys[j * n + slot] = 0; } }
      break;
    }
    if (term != 0) {
      now = true;
      if (lane == 0) sb.n_term[slot] += 1;
    } else if (eval_random) {
      now = true; from_net = false;
    } else {
      const uint64_t key = GM::key(leaf);
      float hit_pi = 0.0f, hit_v = 0.0f;
      if (ep.cache_on && c.cache_lookup(key, 0, hit_pi, hit_v)) now = true;
      else {
        c.emit_leaf(leaf, key);
        if (lane == 0) ar.c_evals[slot] += 1;
        ins_key = cache_key(key);
        pend = kPendRow;
      }
    }
    if (now) {      // process_result_batched(k, ...) right behind its find_leaf_batched: the record would be read back unchanged
      if (lane == 0) { --nif[c.cur]; for (uint32_t i = 0; i < c.plen; ++i) --nif[path[i]]; }
      c.sync_lanes();
      c.process_result(0, from_net, term == 0 && root_noise != 0);
    } else {
      uint32_t* rec = w.wu.ifl_path + static_cast<size_t>(e) * ep.max_depth;
      for (uint32_t i = lane; i < c.plen; i += G) rec[i] = path[i];
      if (lane == 0) { w.wu.ifl_plen[e] = c.plen; w.wu.ifl_cur[e] = c.cur; }
    }
    if (lane == 0) { w.pend[e] = pend; w.keys[e] = ins_key; }
  }
  c.store(kSlotWaitEval);
}

template <class GM>
__global__ __launch_bounds__(64) void k_sb_big_find_wu(EngineParams ep, EngineArrays ar, SbArrays sb, SbWuArrays w, uint32_t n, uint32_t kk,
                                                       uint32_t eval_random, uint32_t root_noise) {
  __shared__ BigScratch<GM> sm;
  const uint32_t slot = blockIdx.x, lane = threadIdx.x;
  if (slot >= n) return;
  if (sb.status[slot] != 0) {
    if (lane == 0) for (uint32_t k = 0; k < kk; ++k) { w.pend[k * n + slot] = kPendNone; w.keys[k * n + slot] = 0; }
    return;
  }
  EngineArrays al = ar;
  BigSlot<GM> c(ep, al, sm, slot, lane);
  c.load();
  uint32_t* nif = w.wu.nif + c.tree_base(0);
  const uint32_t* path = ar.path + static_cast<size_t>(slot) * ep.max_depth;
  for (uint32_t k = 0; k < kk; ++k) {
    const uint32_t e = k * n + slot;
    sb_wu_point(al, w, static_cast<size_t>(k) * n, GM::CANON, GM::P + 1, GM::M);
    typename GM::State leaf;
    uint32_t term = 0;
    uint8_t pend = kPendNone;
    uint64_t ins_key = 0;
    bool now = false, from_net = true;
    if (!c.find_leaf_wu(0, leaf, term, nif)) {
      if (lane == 0) { sb.status[slot] = kSbFindFailed; for (uint32_t j = 0; j < kk; ++j) { w.pend[j * n + slot] = kPendNone; w.keys[j * n + slot] = 0; } }
      break;
    }
    if (term != 0) {
      now = true;
      if (lane == 0) sb.n_term[slot] += 1;
    } else if (eval_random) {
      now = true; from_net = false;
    } else {
      const uint64_t key = c.emit_leaf(leaf);
      if (ep.cache_on && c.cache_lookup(key, 0)) now = true;
      else {
        if (lane == 0) ar.c_evals[slot] += 1;
        ins_key = cache_key(key);
        pend = kPendRow;
      }
    }
    if (now) {
      if (lane == 0) { --nif[c.cur]; for (uint32_t i = 0; i < c.plen; ++i) --nif[path[i]]; }
      c.sync();
      c.process_result(0, from_net, term == 0 && root_noise != 0);
    } else {
      uint32_t* rec = w.wu.ifl_path + static_cast<size_t>(e) * ep.max_depth;
      for (uint32_t i = lane; i < c.plen; i += 64) rec[i] = path[i];
      if (lane == 0) { w.wu.ifl_plen[e] = c.plen; w.wu.ifl_cur[e] = c.cur; }
    }
    if (lane == 0) { w.pend[e] = pend; w.keys[e] = ins_key; }
  }
  c.sync();
  c.store(kSlotWaitEval);
}

// the kPendRow entries of the step in ascending (tree, descent) order; the row count stays on the device
__global__ __launch_bounds__(1024) void k_sb_compact_wu(SbArrays sb, SbWuArrays w, uint32_t n, uint32_t kk) {
  __shared__ uint32_t s_sum[1024];
  const uint32_t tid = threadIdx.x;
  const uint32_t total = n * kk;
  const uint32_t per = (total + 1023u) / 1024u;
  const uint32_t lo = min(total, tid * per), hi = min(total, lo + per);
  uint32_t cnt = 0;
  for (uint32_t j = lo; j < hi; ++j) cnt += w.pend[(j % kk) * n + j / kk] == kPendRow ? 1u : 0u;
  uint32_t row = sb_scan_1024(s_sum, cnt);
  for (uint32_t j = lo; j < hi; ++j) {
    const uint32_t tree = j / kk, e = (j % kk) * n + tree;
    if (w.pend[e] == kPendRow) { w.row_of[e] = row; w.rows[row] = e; w.tree_of[row] = tree; ++row; }
    else w.row_of[e] = kNoRow;
  }
  if (tid == 1023u) *sb.n_rows = s_sum[1023];
}

// process_result_batched for the pending descents of every tree, ascending.  v_rows / pi_rows: the evaluator's answers by
// COMPACTED row (step API), or NULL when the net wrote them to the entries' own rows.
template <class GM>
__global__ __launch_bounds__(256) void k_sb_process_wu(EngineParams ep, EngineArrays ar, SbWuArrays w, uint32_t n, uint32_t kk, uint32_t root_noise,
                                                       const float* v_rows, const float* pi_rows) {
  constexpr int G = GM::GROUP;
  constexpr uint32_t P = GM::P, M = GM::M;
  const uint32_t gtid = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t slot = gtid / G, lane = gtid % G;
  if (slot >= n) return;
  uint32_t k = 0;
  while (k < kk && w.pend[k * n + slot] != kPendRow) ++k;
  if (k == kk) return;
  EngineArrays al = ar;
  SlotCtx<GM> c(ep, al, slot, lane);
  c.load();
  uint32_t* nif = w.wu.nif + c.tree_base(0);
  uint32_t* path = ar.path + static_cast<size_t>(slot) * ep.max_depth;
  for (; k < kk; ++k) {
    const uint32_t e = k * n + slot;
    if (w.pend[e] != kPendRow) continue;
    sb_wu_point(al, w, static_cast<size_t>(k) * n, GM::CANON, P + 1, M);
    if (v_rows) {
      const uint32_t r = w.row_of[e];
      if (lane <= P) al.v[static_cast<size_t>(slot) * (P + 1) + lane] = v_rows[static_cast<size_t>(r) * (P + 1) + lane];
      if (lane < M) al.pi[static_cast<size_t>(slot) * M + lane] = pi_rows[static_cast<size_t>(r) * M + lane];
    }
    c.cur = w.wu.ifl_cur[e]; c.plen = w.wu.ifl_plen[e];
    if (lane == 0) {
      const uint32_t* rec = w.wu.ifl_path + static_cast<size_t>(e) * ep.max_depth;
      --nif[c.cur];
      for (uint32_t i = 0; i < c.plen; ++i) { path[i] = rec[i]; --nif[rec[i]]; }
      w.pend[e] = kPendNone;
    }
    c.sync_lanes();
    c.process_result(0, true, root_noise != 0);
  }
  c.store(kSlotWaitEval);
}

template <class GM>
__global__ __launch_bounds__(64) void k_sb_big_process_wu(EngineParams ep, EngineArrays ar, SbWuArrays w, uint32_t n, uint32_t kk,
                                                          uint32_t root_noise, const float* v_rows, const float* pi_rows) {
  __shared__ BigScratch<GM> sm;
  constexpr uint32_t P = GM::P, M = GM::M;
  const uint32_t slot = blockIdx.x, lane = threadIdx.x;
  if (slot >= n) return;
  uint32_t k = 0;
  while (k < kk && w.pend[k * n + slot] != kPendRow) ++k;
  if (k == kk) return;
  EngineArrays al = ar;
  BigSlot<GM> c(ep, al, sm, slot, lane);
  c.load();
  uint32_t* nif = w.wu.nif + c.tree_base(0);
  uint32_t* path = ar.path + static_cast<size_t>(slot) * ep.max_depth;
  for (; k < kk; ++k) {
    const uint32_t e = k * n + slot;
    if (w.pend[e] != kPendRow) continue;
    sb_wu_point(al, w, static_cast<size_t>(k) * n, GM::CANON, P + 1, M);
    if (v_rows) {
      const uint32_t r = w.row_of[e];
      if (lane <= P) al.v[static_cast<size_t>(slot) * (P + 1) + lane] = v_rows[static_cast<size_t>(r) * (P + 1) + lane];
      for (uint32_t m = lane; m < M; m += 64) al.pi[static_cast<size_t>(slot) * M + m] = pi_rows[static_cast<size_t>(r) * M + m];
    }
    c.cur = w.wu.ifl_cur[e]; c.plen = w.wu.ifl_plen[e];
    if (lane == 0) {
      const uint32_t* rec = w.wu.ifl_path + static_cast<size_t>(e) * ep.max_depth;
      --nif[c.cur];
      for (uint32_t i = 0; i < c.plen; ++i) { path[i] = rec[i]; --nif[rec[i]]; }
      w.pend[e] = kPendNone;
    }
    c.sync();
    c.process_result(0, true, root_noise != 0);
  }
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

// ======================= moves played on the batch: pick, update_root, root prior ================================================
// What the evaluation tools do between two searches of a game they walk (play.py:274-346, mcts_analysis.py:995-1051): pick a move
// from the root's visit counts, MCTS::update_root (mcts.cc:151-173) on every tree, play the move on the root state, and search the
// successor with the reused subtree.  The root state of tree i lives in slot i (written by the seed kernel), so the move is played
// here, on the device.  Same grid-to-tree mapping as the find kernels.
//   move[i]        the move chosen by the pick kernel (-1 = none: finished or stopped tree, nothing picked since reset, or the
//                  pick was consumed by an update-root launch: an update_roots without a pick before it moves nothing)
//   log[i][0..len) the moves played on tree i since reset (capacity log_cap = max_turns + 8), log_len[i] = len
//   final[i][P+1]  GameState::scores() of a finished tree
// (SbPlayArrays)

// what the two update-root kernels share once the tree is re-rooted and `mv` is played: move log, finished rule
template <class GM, class State>
__device__ __forceinline__ void sb_after_move(const SbArrays& sb, const SbPlayArrays& pl, uint32_t slot, int32_t mv, const State& gs) {
  const uint32_t len = pl.log_len[slot];
  if (len < pl.log_cap) { pl.log[static_cast<size_t>(slot) * pl.log_cap + len] = mv; pl.log_len[slot] = len + 1; }
  const uint32_t term = GM::terminal(gs);
  if (term == 0) return;
  bool scored = true;       // StarGambit: over with no winner recorded scores all zeros (replay_kernels.h)
  if constexpr (is_stargambit<GM>::value) scored = GM::winner(gs) < 3;
  for (uint32_t i = 0; i <= static_cast<uint32_t>(GM::P); ++i)
    pl.final[static_cast<size_t>(slot) * (GM::P + 1) + i] = (scored && term - 1 == i) ? 1.0f : 0.0f;
  sb.status[slot] = kSbFinished;
}

// pick_move(probs(temp)) from the tree's own stream (PUCT), gumbel_final_action() (Gumbel): the read-outs of mcts_query_slot,
// kinds 1 + 10 / 7, through the tree's rows of the query buffers
template <class GM>
__global__ __launch_bounds__(256) void k_sb_pick(EngineParams ep, EngineArrays ar, SbArrays sb, SbPlayArrays pl, uint32_t n, float temp,
                                                 float* out_f, uint32_t stride_f, uint32_t* out_u, uint32_t stride_u) {
  constexpr int G = GM::GROUP;
  const uint32_t gtid = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t slot = gtid / G, lane = gtid % G;
  if (slot >= n) return;
  if (sb.status[slot] != 0) { if (lane == 0) pl.move[slot] = -1; return; }
  const uint32_t t = slot * GM::P;
  if (ar.nodes[static_cast<size_t>(t) * ep.cap + ar.root[t]].n == 0) {      // pick_move of an all-zero vector: "this shouldn't be possible."
    if (lane == 0) { pl.move[slot] = -1; sb.status[slot] = kSbNoVisits; }
    return;
  }
  float* f = out_f + static_cast<size_t>(slot) * stride_f;
  uint32_t* u = out_u + static_cast<size_t>(slot) * stride_u;
  if (ep.gumbel_on) {
    mcts_query_slot<GM>(ep, ar, slot, lane, kQGumbelFinal, 0.0f, 0u, f, u);
  } else {
    mcts_query_slot<GM>(ep, ar, slot, lane, kQProbs, temp, 0u, f, u);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");      // the slot state lane 0 stored is loaded again by every lane
    mcts_query_slot<GM>(ep, ar, slot, lane, kQPickMove, 0.0f, 0u, f, u);
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  if (lane == 0) pl.move[slot] = static_cast<int32_t>(u[0]);
}

template <class GM>
__global__ __launch_bounds__(64) void k_sb_big_pick(EngineParams ep, EngineArrays ar, SbArrays sb, SbPlayArrays pl, uint32_t n, float temp,
                                                    float* out_f, uint32_t stride_f, uint32_t* out_u, uint32_t stride_u) {
  __shared__ BigScratch<GM> sm;
  const uint32_t slot = blockIdx.x, lane = threadIdx.x;
  if (slot >= n) return;
  if (sb.status[slot] != 0) { if (lane == 0) pl.move[slot] = -1; return; }
  const uint32_t t = slot * GM::P;
  if (ar.N[static_cast<size_t>(t) * ep.cap + ar.root[t]] == 0) {
    if (lane == 0) { pl.move[slot] = -1; sb.status[slot] = kSbNoVisits; }
    return;
  }
  float* f = out_f + static_cast<size_t>(slot) * stride_f;
  uint32_t* u = out_u + static_cast<size_t>(slot) * stride_u;
  if (ep.gumbel_on) {
    mcts_big_query_slot<GM>(ep, ar, sm, slot, lane, kQGumbelFinal, 0.0f, 0u, f, u);
  } else {
    mcts_big_query_slot<GM>(ep, ar, sm, slot, lane, kQProbs, temp, 0u, f, u);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    mcts_big_query_slot<GM>(ep, ar, sm, slot, lane, kQPickMove, 0.0f, 0u, f, u);
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  if (lane == 0) pl.move[slot] = static_cast<int32_t>(u[0]);
}

// tree i advances by moves[i] (< 0: stays): update_root (which expands an unexpanded root first, as the reference does), the move
// on the slot's root state, the marks of the nodes created here cleared (nif: only with K > 1), the move log, the finished rule.
// A move the root does not have raises the engine's bit 32 and stops that tree alone (kSbBadMove); the host clears both.
template <class GM>
__global__ __launch_bounds__(256) void k_sb_update_root(EngineParams ep, EngineArrays ar, SbArrays sb, SbPlayArrays pl, uint32_t n,
                                                        const int32_t* moves, uint32_t* nif) {
  constexpr int G = GM::GROUP;
  const uint32_t gtid = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t slot = gtid / G, lane = gtid % G;
  if (slot >= n) return;
  if (sb.status[slot] != 0) return;
  const int32_t mv = moves[slot];
  if (mv < 0) return;
  SlotCtx<GM> c(ep, ar, slot, lane);
  c.load();
  const uint32_t bump0 = c.t_bump[0];
  const bool ok = c.update_root(0, static_cast<uint32_t>(mv));
  if (nif) for (uint32_t i = bump0 + lane; i < c.t_bump[0]; i += G) nif[c.tree_base(0) + i] = 0;
  if (lane == 0) pl.move[slot] = -1;      // a pick is played once (every lane of the group has read its move above)
  if (!ok) {
    if (lane == 0) sb.status[slot] = kSbBadMove;
    c.store(kSlotWaitEval);      // the root may have been expanded; the tree itself is where it was
    return;
  }
  if (!GM::play(c.gs, static_cast<uint32_t>(mv))) {      // unreachable: a child of the root is a legal move.  Nothing is stored: the tree stops at its old root
    if (lane == 0) sb.status[slot] = kSbBadState;
    return;
  }
  c.cur = c.t_root[0]; c.plen = 0;
  if (lane == 0) sb_after_move<GM>(sb, pl, slot, mv, c.gs);
  c.store(kSlotWaitEval);
}

template <class GM>
__global__ __launch_bounds__(64) void k_sb_big_update_root(EngineParams ep, EngineArrays ar, SbArrays sb, SbPlayArrays pl, uint32_t n,
                                                           const int32_t* moves, uint32_t* nif) {
  __shared__ BigScratch<GM> sm;
  const uint32_t slot = blockIdx.x, lane = threadIdx.x;
  if (slot >= n) return;
  if (sb.status[slot] != 0) return;
  const int32_t mv = moves[slot];
  if (mv < 0) return;
  BigSlot<GM> c(ep, ar, sm, slot, lane);
  c.load();
  const uint32_t bump0 = c.t_bump[0];
  const bool ok = c.update_root(0, static_cast<uint32_t>(mv));
  if (nif) for (uint32_t i = bump0 + lane; i < c.t_bump[0]; i += 64) nif[c.tree_base(0) + i] = 0;
  if (lane == 0) pl.move[slot] = -1;      // a pick is played once (the wavefront has read its move above)
  if (!ok) {
    if (lane == 0) sb.status[slot] = kSbBadMove;
    c.sync();
    c.store(kSlotWaitEval);
    return;
  }
  bool base_valid = true;
  // unreachable behind a successful update_root for the Tafl family (false = a move the rules refuse, and a child of the root is
  // legal); StarGambit: its position history is full.  Nothing is stored: the tree stops at its old root until the next reset
  if (!c.step_state(c.gs, static_cast<uint32_t>(mv), c.game_list(), c.glen, base_valid, 0)) {
    if (lane == 0) sb.status[slot] = kSbBadState;
    return;
  }
  if constexpr (!is_stargambit<GM>::value) {   // the root's repetition list, as k_sb_big_seed writes it (whole list: a capture may have cleared it)
    uint64_t* gl = ar.rep_list + static_cast<size_t>(slot) * (GM::MAX_TURNS + 2);
    for (uint32_t i = lane; i < c.glen; i += 64) gl[i] = sm.glist[i];
  }
  if (lane == 0) {
    if (ep.half_nodes) {      // ask k_compact to move the tree when its active half is filling up (k_mcts_big_update_root's rule)
      const uint32_t b = c.t_bump[0];
      if (b - ((b - 1) / ep.half_nodes) * ep.half_nodes > ep.compact_above) ar.compact_flag[slot * GM::P] = 1;
    }
    sb_after_move<GM>(sb, pl, slot, mv, c.gs);
  }
  c.cur = c.t_root[0]; c.plen = 0;      // no pending simulation for k_compact to re-point
  c.sync();
  c.store(kSlotWaitEval);
}

// MCTS::apply_root_policy_temp, then MCTS::add_root_noise, on the root of every live tree: what the reference does to a reused
// root (play_manager.cc:523-555), through the read-out bodies of kinds 9 and 8
template <class GM>
__global__ __launch_bounds__(256) void k_sb_root_prior(EngineParams ep, EngineArrays ar, SbArrays sb, uint32_t n, uint32_t apply_temp, uint32_t noise,
                                                       float* out_f, uint32_t stride_f, uint32_t* out_u, uint32_t stride_u) {
  constexpr int G = GM::GROUP;
  const uint32_t gtid = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t slot = gtid / G, lane = gtid % G;
  if (slot >= n || sb.status[slot] != 0) return;
  float* f = out_f + static_cast<size_t>(slot) * stride_f;
  uint32_t* u = out_u + static_cast<size_t>(slot) * stride_u;
  if (apply_temp) mcts_query_slot<GM>(ep, ar, slot, lane, kQApplyRootTemp, 0.0f, 0u, f, u);
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");      // the priors and the slot state written above are read again below
  if (noise) mcts_query_slot<GM>(ep, ar, slot, lane, kQAddRootNoise, 0.0f, 0u, f, u);
}

template <class GM>
__global__ __launch_bounds__(64) void k_sb_big_root_prior(EngineParams ep, EngineArrays ar, SbArrays sb, uint32_t n, uint32_t apply_temp, uint32_t noise,
                                                          float* out_f, uint32_t stride_f, uint32_t* out_u, uint32_t stride_u) {
  __shared__ BigScratch<GM> sm;
  const uint32_t slot = blockIdx.x, lane = threadIdx.x;
  if (slot >= n || sb.status[slot] != 0) return;
  float* f = out_f + static_cast<size_t>(slot) * stride_f;
  uint32_t* u = out_u + static_cast<size_t>(slot) * stride_u;
  if (apply_temp) mcts_big_query_slot<GM>(ep, ar, sm, slot, lane, kQApplyRootTemp, 0.0f, 0u, f, u);
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  if (noise) mcts_big_query_slot<GM>(ep, ar, sm, slot, lane, kQAddRootNoise, 0.0f, 0u, f, u);
}

// ======================= EvalType::PLAYOUT: every non-terminal leaf is evaluated by a random rollout on the device =================
// alphazero.playout_eval(leaf, seed) (game_state.cc:10-95; play.py:306, mcts_analysis.py:649): the uniform policy over the leaf's
// legal moves and the scores of one uniformly random rollout, backed up by the unchanged process_result.  Every rollout draws
// from a FRESH pcg32 stream, so a tree's search depends neither on N, K nor on the launch geometry: the j-th rollout of tree i
// since reset (j counts from 0, in descent order) is seeded sb_rollout_seed(seeds[i], j), the way k_playout seeds its own.
// No compaction, no net call, no cache.
//   Connect4, K == 1   k_sb_find_po parks the leaf state, k_sb_rollout runs ONE LANE per pending rollout (inside the find kernel
//                      the 8 lanes of a tree's group would all play the same rollout), k_sb_process backs up: 3 launches a step
//   wide games, K == 1 the rules are wave-cooperative and the rollout continues the descent's path-local repetition list, so it
//                      runs in k_sb_big_find_po behind the descent; k_sb_big_process backs up: 2 launches a step
//   K > 1              a playout leaf is an immediate: its process_result_batched runs before the tree's next descent, which has to
//                      see the back-up and not the in-flight mark (play.py:306-307).  So the rollout sits between two descents of
//                      one tree, inside the *_find_wu_po loop, and a step is 1 launch
// (SbRollArrays: the rollout seed and count of every tree, the parked leaf states)
__host__ __device__ __forceinline__ uint64_t sb_rollout_seed(uint64_t tree_seed, uint32_t j) {
  return mix64(tree_seed + kRollSalt * (static_cast<uint64_t>(j) + 1));
}

template <class GM>
__global__ __launch_bounds__(256) void k_sb_find_po(EngineParams ep, EngineArrays ar, SbArrays sb, SbRollArrays ro, uint32_t n) {
  constexpr int G = GM::GROUP;
  const uint32_t gtid = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t slot = gtid / G, lane = gtid % G;
  if (slot >= n) return;
  if (sb.status[slot] != 0) {
    if (lane == 0) sb.pend[slot] = kPendNone;
    return;
  }
  SlotCtx<GM> c(ep, ar, slot, lane);
  c.load();
  typename GM::State leaf;
  uint32_t term = 0;
  uint8_t pend = kPendNone;
  if (!c.find_leaf(0, leaf, term)) {
    if (lane == 0) sb.status[slot] = kSbFindFailed;
  } else if (term != 0) {
    c.process_result(0, true, false);
    if (lane == 0) sb.n_term[slot] += 1;
  } else {
    if (lane == 0) { reinterpret_cast<typename GM::State*>(ro.states)[slot] = leaf; ar.c_evals[slot] += 1; }
    pend = kPendRollout;
  }
  if (lane == 0) sb.pend[slot] = pend;
  c.store(kSlotWaitEval);
}

// one lane per pending rollout: k_playout's body from the parked leaf state; the answer goes to the tree's (v, pi) rows, where
// k_sb_process reads a net's
template <class GM>
__global__ __launch_bounds__(64) void k_sb_rollout(EngineArrays ar, SbArrays sb, SbRollArrays ro, uint32_t n) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n || sb.pend[g] != kPendRollout) return;
  typename GM::State s = reinterpret_cast<const typename GM::State*>(ro.states)[g];
  const uint32_t j = ro.count[g];
  ro.count[g] = j + 1;
  const uint32_t kl = GM::num_valid(s);
  const float ksum = static_cast<float>(kl & 0xFFu);
  for (int m = 0; m < GM::M; ++m)
    ar.pi[static_cast<size_t>(g) * GM::M + m] = (((GM::valid_mask(s) >> m) & 1u) && ksum > 0.0f) ? 1.0f / ksum : 0.0f;
  Pcg32 roll;
  roll.seed(sb_rollout_seed(ro.seeds[g], j));
  uint32_t term = GM::terminal(s);
  while (term == 0) {
    const uint32_t k = GM::num_valid(s);
    if (k == 0) break;
    GM::play(s, GM::nth_valid(s, lemire_below(roll, k)));
    term = GM::terminal(s);
  }
  for (int i = 0; i <= GM::P; ++i)
    ar.v[static_cast<size_t>(g) * (GM::P + 1) + i] = term ? ((static_cast<int>(term) - 1 == i) ? 1.0f : 0.0f) : static_cast<float>(1.0 / (GM::P + 1));
}

template <class GM>
__global__ __launch_bounds__(64) void k_sb_big_find_po(EngineParams ep, EngineArrays ar, SbArrays sb, SbRollArrays ro, uint32_t n) {
  __shared__ BigScratch<GM> sm;
  const uint32_t slot = blockIdx.x, lane = threadIdx.x;
  if (slot >= n) return;
  if (sb.status[slot] != 0) {
    if (lane == 0) sb.pend[slot] = kPendNone;
    return;
  }
  BigSlot<GM> c(ep, ar, sm, slot, lane);
  c.load();
  typename GM::State leaf;
  uint32_t term = 0;
  uint8_t pend = kPendNone;
  if (!c.find_leaf(0, leaf, term)) {
    if (lane == 0) sb.status[slot] = kSbFindFailed;
  } else if (term != 0) {
    c.process_result(0, true, false);
    if (lane == 0) sb.n_term[slot] += 1;
  } else {
    const uint32_t j = ro.count[slot];
    c.playout_eval(leaf, sb_rollout_seed(ro.seeds[slot], j));      // (ends with the wavefront's fence: every lane has read j)
    if (lane == 0) { ro.count[slot] = j + 1; ar.c_evals[slot] += 1; }
    pend = kPendRollout;
  }
  if (lane == 0) sb.pend[slot] = pend;
  c.sync();
  c.store(kSlotWaitEval);
}

// K > 1: `kk` <= K x (find_leaf_batched, the rollout of a non-terminal leaf, process_result_batched at once).  Every descent is
// backed up here, so no in-flight record and no pending entry is left behind; entry k * N + i still holds the (v, pi) rows of
// descent k of tree i, as for the other evaluators
template <class GM>
__global__ __launch_bounds__(256) void k_sb_find_wu_po(EngineParams ep, EngineArrays ar, SbArrays sb, SbWuArrays w, SbRollArrays ro, uint32_t n,
                                                       uint32_t kk, uint32_t root_noise) {
  constexpr int G = GM::GROUP;
  const uint32_t gtid = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t slot = gtid / G, lane = gtid % G;
  if (slot >= n || sb.status[slot] != 0) return;
  EngineArrays al = ar;
  SlotCtx<GM> c(ep, al, slot, lane);
  c.load();
  uint32_t* nif = w.wu.nif + c.tree_base(0);
  const uint32_t* path = ar.path + static_cast<size_t>(slot) * ep.max_depth;
  const uint64_t tree_seed = ro.seeds[slot];
  uint32_t j = ro.count[slot], n_term = 0;
  const uint32_t j0 = j;
  for (uint32_t k = 0; k < kk; ++k) {
    sb_wu_point(al, w, static_cast<size_t>(k) * n, GM::CANON, GM::P + 1, GM::M);
    typename GM::State leaf;
    uint32_t term = 0;
    if (!c.find_leaf_wu(0, leaf, term, nif)) {      // the tree stops (reset() clears the root's mark, new nodes get theirs cleared)
      if (lane == 0) sb.status[slot] = kSbFindFailed;
      break;
    }
    if (term != 0) ++n_term;
    else c.playout_eval(leaf, sb_rollout_seed(tree_seed, j++));
    if (lane == 0) { --nif[c.cur]; for (uint32_t i = 0; i < c.plen; ++i) --nif[path[i]]; }
    c.sync_lanes();
    c.process_result(0, true, term == 0 && root_noise != 0);
  }
  if (lane == 0) { ro.count[slot] = j; ar.c_evals[slot] += j - j0; sb.n_term[slot] += n_term; }
  c.store(kSlotWaitEval);
}

// find_leaf leaves the path-local repetition bookkeeping of its descent in leaf_rep_len / leaf_base_valid for the rollout;
// find_leaf_wu keeps it to itself, so the recorded path is played once more (a few moves next to the rollout's many)
template <class GM>
__device__ __forceinline__ void sb_big_replay_path(BigSlot<GM>& c, const uint32_t* path) {
  typename GM::State st = c.gs;
  const size_t tb = c.tree_base(0);
  uint32_t len = 0;
  bool base_valid = true;
  for (uint32_t i = 0; i < c.plen; ++i) {
    const uint32_t node = (i + 1 < c.plen) ? path[i + 1] : c.cur;
    if (!c.step_state(st, meta_mv(c.ar.META[tb + node]), c.path_list(), len, base_valid, c.glen)) break;      // (find_leaf_wu took every one of them)
  }
  c.leaf_rep_len = len; c.leaf_base_valid = base_valid;
}

template <class GM>
__global__ __launch_bounds__(64) void k_sb_big_find_wu_po(EngineParams ep, EngineArrays ar, SbArrays sb, SbWuArrays w, SbRollArrays ro, uint32_t n,
                                                          uint32_t kk, uint32_t root_noise) {
  __shared__ BigScratch<GM> sm;
  const uint32_t slot = blockIdx.x, lane = threadIdx.x;
  if (slot >= n || sb.status[slot] != 0) return;
  EngineArrays al = ar;
  BigSlot<GM> c(ep, al, sm, slot, lane);
  c.load();
  uint32_t* nif = w.wu.nif + c.tree_base(0);
  const uint32_t* path = ar.path + static_cast<size_t>(slot) * ep.max_depth;
  const uint64_t tree_seed = ro.seeds[slot];
  uint32_t j = ro.count[slot], n_term = 0;
  const uint32_t j0 = j;
  for (uint32_t k = 0; k < kk; ++k) {
    sb_wu_point(al, w, static_cast<size_t>(k) * n, GM::CANON, GM::P + 1, GM::M);
    typename GM::State leaf;
    uint32_t term = 0;
    if (!c.find_leaf_wu(0, leaf, term, nif)) {
      if (lane == 0) sb.status[slot] = kSbFindFailed;
      break;
    }
    if (term != 0) ++n_term;
    else {
      sb_big_replay_path(c, path);
      c.playout_eval(leaf, sb_rollout_seed(tree_seed, j++));
    }
    if (lane == 0) { --nif[c.cur]; for (uint32_t i = 0; i < c.plen; ++i) --nif[path[i]]; }
    c.sync();
    c.process_result(0, true, term == 0 && root_noise != 0);
  }
  c.sync();
  if (lane == 0) { ro.count[slot] = j; ar.c_evals[slot] += j - j0; sb.n_term[slot] += n_term; }
  c.store(kSlotWaitEval);
}

// ======================= search to per-tree visit targets, snapshots at checkpoints ================================================
// The inner loop of mcts_analysis.py:run_analysis (:884-972, batched :975-1063): `while mcts.root_n() < target` with the policy and
// the value captured once at every smaller visit count of the sweep.  The step kernels above stay as they are: a tree that has
// reached its target gets status kSbPaused (> 0: no error; not kSbFinished) here, which every one of them skips like any other non-zero status, and the call's
// last checkpoint launch turns every kSbPaused back to 0 (`resume`), so the value never outlives the call that set it.
//   target[i]     tree i descends while root_n(i) < target[i]
//   cps[j]        the J <= 32 checkpoints, strictly ascending
//   taken[i]      bit j: snapshot j of tree i is taken; it is taken once, at the first launch that sees root_n(i) >= cps[j]
//   root_n / counts / probs / root_values / root_q   row (i, j) of [N, J] / [N, J, M] / [N, J, M] / [N, J, 3] / [N, J, M]
// The rows are written by the read-out bodies of kinds 0, 1 | 2, 3, 4 (mcts_query_slot / mcts_big_query_slot), the same bodies
// the pick kernel reuses; rows that were not taken keep the zeros the host cleared them to.  (SbSweepArrays, kSbMaxCheckpoints)

// what both checkpoint kernels end with: pause at the target, resume at the end of the call (lane 0 of the tree)
__device__ __forceinline__ void sb_checkpoint_tail(const SbArrays& sb, const SbSweepArrays& sw, uint32_t slot, int32_t status, uint32_t root_n,
                                                   uint32_t resume) {
  int32_t next = status;
  if (next == 0 && root_n >= sw.target[slot]) next = kSbPaused;
  if (resume && next == kSbPaused) next = 0;
  if (next != status) sb.status[slot] = next;
}

template <class GM>
__global__ __launch_bounds__(256) void k_sb_checkpoint(EngineParams ep, EngineArrays ar, SbArrays sb, SbSweepArrays sw, uint32_t n, float temp,
                                                       uint32_t pruned, uint32_t resume) {
  constexpr int G = GM::GROUP;
  constexpr uint32_t M = GM::M;
  const uint32_t gtid = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t slot = gtid / G, lane = gtid % G;
  if (slot >= n) return;
  const int32_t status = sb.status[slot];
  uint32_t root_n = 0;
  if (status == 0) {
    const uint32_t t = slot * GM::P;
    root_n = ar.nodes[static_cast<size_t>(t) * ep.cap + ar.root[t]].n;
    const uint32_t taken = sw.taken[slot];
    uint32_t now = taken;
    for (uint32_t j = 0; j < sw.n_cp; ++j) {
      if (((now >> j) & 1u) || sw.cps[j] > root_n) continue;
      const size_t row = static_cast<size_t>(slot) * sw.n_cp + j;
      uint32_t* cu = sw.counts + row * M;
      float* pf = sw.probs + row * M;
      mcts_query_slot<GM>(ep, ar, slot, lane, kQCounts, 0.0f, 0u, pf, cu);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");      // the slot state lane 0 stored is loaded again by every lane
      mcts_query_slot<GM>(ep, ar, slot, lane, pruned ? kQProbsPruned : kQProbs, temp, 0u, pf, cu);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
      mcts_query_slot<GM>(ep, ar, slot, lane, kQRootValue, 0.0f, 0u, sw.root_values + row * 3, cu);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
      mcts_query_slot<GM>(ep, ar, slot, lane, kQRootQ, 0.0f, 0u, sw.root_q + row * M, cu);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
      if (lane == 0) sw.root_n[row] = root_n;
      now |= 1u << j;
    }
    if (lane == 0 && now != taken) sw.taken[slot] = now;
  }
  if (lane == 0) sb_checkpoint_tail(sb, sw, slot, status, root_n, resume);
}

template <class GM>
__global__ __launch_bounds__(64) void k_sb_big_checkpoint(EngineParams ep, EngineArrays ar, SbArrays sb, SbSweepArrays sw, uint32_t n, float temp,
                                                          uint32_t pruned, uint32_t resume) {
  __shared__ BigScratch<GM> sm;
  constexpr uint32_t M = GM::M;
  const uint32_t slot = blockIdx.x, lane = threadIdx.x;
  if (slot >= n) return;
  const int32_t status = sb.status[slot];
  uint32_t root_n = 0;
  if (status == 0) {
    const uint32_t t = slot * GM::P;
    root_n = ar.N[static_cast<size_t>(t) * ep.cap + ar.root[t]];
    const uint32_t taken = sw.taken[slot];
    uint32_t now = taken;
    for (uint32_t j = 0; j < sw.n_cp; ++j) {
      if (((now >> j) & 1u) || sw.cps[j] > root_n) continue;
      const size_t row = static_cast<size_t>(slot) * sw.n_cp + j;
      uint32_t* cu = sw.counts + row * M;
      float* pf = sw.probs + row * M;
      mcts_big_query_slot<GM>(ep, ar, sm, slot, lane, kQCounts, 0.0f, 0u, pf, cu);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
      mcts_big_query_slot<GM>(ep, ar, sm, slot, lane, pruned ? kQProbsPruned : kQProbs, temp, 0u, pf, cu);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
      mcts_big_query_slot<GM>(ep, ar, sm, slot, lane, kQRootValue, 0.0f, 0u, sw.root_values + row * 3, cu);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
      mcts_big_query_slot<GM>(ep, ar, sm, slot, lane, kQRootQ, 0.0f, 0u, sw.root_q + row * M, cu);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
      if (lane == 0) sw.root_n[row] = root_n;
      now |= 1u << j;
    }
    if (lane == 0 && now != taken) sw.taken[slot] = now;
  }
  if (lane == 0) sb_checkpoint_tail(sb, sw, slot, status, root_n, resume);
}

// ======================= descents that need no evaluator do not end a tree's step (descents_per_step = L > 1) ======================
// The per-tree loop of the evaluation tools (mcts_analysis.py:921-951): `while root_n < target: find_leaf; a cache hit is backed up
// and the loop goes on; a miss ends the tree's turn in the round`.  One step of a live tree is up to L calls of find_leaf, each
// backed up at once by process_result while it needs nothing from the evaluator (terminal leaf, RANDOM, cache hit); the first leaf
// that does becomes the tree's ONE row of the step and ends its loop, so k_sb_compact, the net call over the row list,
// k_cache_insert, k_sb_rollout and the process kernels run behind these kernels as they run behind k_sb_find / k_sb_find_po.  The
// calls a tree makes, and their order, are those of L == 1: only where the step boundaries fall changes.
//   todo[i]       descents tree i still owes the running search / move (set by k_sb_todo_set, 0 for a finished or stopped tree)
//   todo_max[2]   the largest todo a step leaves behind, by step parity: the find kernel of step t raises word t & 1 with one
//                 atomicMax per tree that still owes descents and clears word (t + 1) & 1 for the step behind it, so the word
//                 costs no launch of its own.  The host reads word t & 1 behind step t: 0 = the search is complete
// (SbDlArrays)

__global__ __launch_bounds__(256) void k_sb_todo_set(SbArrays sb, SbDlArrays dl, uint32_t n, uint32_t visits) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 2) dl.todo_max[i] = 0;
  if (i < n) dl.todo[i] = sb.status[i] == 0 ? visits : 0u;
}

// what a tree's step leaves behind (lane 0 of the tree): its pending leaf, the key to insert (KEYS: the net path; the PLAYOUT
// kernels have no cache), the terminal leaves it met, the descents it still owes and their share of the step's maximum
template <bool KEYS>
__device__ __forceinline__ void sb_dl_close_tree(const SbArrays& sb, const SbDlArrays& dl, const EngineParams& ep, const EngineArrays& ar, uint32_t slot,
                                                 uint32_t parity, uint32_t pend, uint32_t n_term, uint32_t left, uint64_t ins_key) {
  sb.pend[slot] = static_cast<uint8_t>(pend);
  if constexpr (KEYS) if (ep.cache_on) ar.cache_keys[slot] = ins_key;
  if (n_term) sb.n_term[slot] += n_term;
  dl.todo[slot] = left;
  if (left) atomicMax(&dl.todo_max[parity], left);
}

template <class GM>
__global__ __launch_bounds__(256) void k_sb_find_dl(EngineParams ep, EngineArrays ar, SbArrays sb, SbDlArrays dl, uint32_t n, uint32_t L,
                                                    uint32_t parity, uint32_t eval_random, uint32_t root_noise) {
  constexpr int G = GM::GROUP;
  const uint32_t gtid = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t slot = gtid / G, lane = gtid % G;
  if (gtid == 0) dl.todo_max[parity ^ 1u] = 0;
  if (slot >= n) return;
  uint32_t left = dl.todo[slot];
  if (sb.status[slot] != 0 || left == 0) { sb_skip_tree(sb, ep, ar, slot, lane); return; }      // (the step before left nothing pending)
  SlotCtx<GM> c(ep, ar, slot, lane);
  c.load();
  uint32_t pend = kPendNone, n_term = 0;
  uint64_t ins_key = 0;
  for (uint32_t d = 0; d < L && left > 0; ++d) {
    --left;
    typename GM::State leaf;
    uint32_t term = 0, from_net = 1;
    if (!c.find_leaf(0, leaf, term)) {      // the tree stops: it owes nothing more
      if (lane == 0) sb.status[slot] = kSbFindFailed;
      left = 0;
      break;
    }
    if (term != 0) ++n_term;
    else if (eval_random) from_net = 0;
    else {
      const uint64_t key = GM::key(leaf);
      float hit_pi = 0.0f, hit_v = 0.0f;
      if (!(ep.cache_on && c.cache_lookup(key, 0, hit_pi, hit_v))) {
        c.emit_leaf(leaf, key);
        if (lane == 0) ar.c_evals[slot] += 1;
        ins_key = cache_key(key);
        pend = kPendRow;
        break;
      }
    }
    c.process_result(0, from_net != 0, term == 0 && root_noise != 0);     // what k_sb_find / k_sb_process pass for this kind of leaf
  }
  if (lane == 0) sb_dl_close_tree<true>(sb, dl, ep, ar, slot, parity, pend, n_term, left, ins_key);
  c.store(kSlotWaitEval);
}

template <class GM>
__global__ __launch_bounds__(64) void k_sb_big_find_dl(EngineParams ep, EngineArrays ar, SbArrays sb, SbDlArrays dl, uint32_t n, uint32_t L,
                                                       uint32_t parity, uint32_t eval_random, uint32_t root_noise) {
  __shared__ BigScratch<GM> sm;
  const uint32_t slot = blockIdx.x, lane = threadIdx.x;
  if (slot == 0 && lane == 0) dl.todo_max[parity ^ 1u] = 0;
  if (slot >= n) return;
  uint32_t left = dl.todo[slot];
  if (sb.status[slot] != 0 || left == 0) { sb_skip_tree(sb, ep, ar, slot, lane); return; }
  BigSlot<GM> c(ep, ar, sm, slot, lane);
  c.load();
  uint32_t pend = kPendNone, n_term = 0;
  uint64_t ins_key = 0;
  for (uint32_t d = 0; d < L && left > 0; ++d) {
    --left;
    typename GM::State leaf;
    uint32_t term = 0, from_net = 1;
    if (!c.find_leaf(0, leaf, term)) {
      if (lane == 0) sb.status[slot] = kSbFindFailed;
      left = 0;
      break;
    }
    if (term != 0) ++n_term;
    else if (eval_random) from_net = 0;
    else {
      const uint64_t key = c.emit_leaf(leaf);
      if (!(ep.cache_on && c.cache_lookup(key, 0))) {
        if (lane == 0) ar.c_evals[slot] += 1;
        ins_key = cache_key(key);
        pend = kPendRow;
        break;
      }
    }
    c.process_result(0, from_net != 0, term == 0 && root_noise != 0);
  }
  if (lane == 0) sb_dl_close_tree<true>(sb, dl, ep, ar, slot, parity, pend, n_term, left, ins_key);
  c.sync();
  c.store(kSlotWaitEval);
}

// EvalType::PLAYOUT: a terminal leaf is free, a leaf that needs a rollout ends the tree's step like a net row (Connect4: parked
// for k_sb_rollout; wide games: rolled out here, behind its descent).  No further rollout is inlined, so the j-th rollout of a
// tree is the j-th of the L == 1 search and keeps its seed
template <class GM>
__global__ __launch_bounds__(256) void k_sb_find_dl_po(EngineParams ep, EngineArrays ar, SbArrays sb, SbDlArrays dl, SbRollArrays ro, uint32_t n,
                                                       uint32_t L, uint32_t parity) {
  constexpr int G = GM::GROUP;
  const uint32_t gtid = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t slot = gtid / G, lane = gtid % G;
  if (gtid == 0) dl.todo_max[parity ^ 1u] = 0;
  if (slot >= n) return;
  uint32_t left = dl.todo[slot];
  if (sb.status[slot] != 0 || left == 0) {
    if (lane == 0) sb.pend[slot] = kPendNone;
    return;
  }
  SlotCtx<GM> c(ep, ar, slot, lane);
  c.load();
  uint32_t pend = kPendNone, n_term = 0;
  for (uint32_t d = 0; d < L && left > 0; ++d) {
    --left;
    typename GM::State leaf;
    uint32_t term = 0;
    if (!c.find_leaf(0, leaf, term)) {
      if (lane == 0) sb.status[slot] = kSbFindFailed;
      left = 0;
      break;
    }
    if (term == 0) {
      if (lane == 0) { reinterpret_cast<typename GM::State*>(ro.states)[slot] = leaf; ar.c_evals[slot] += 1; }
      pend = kPendRollout;
      break;
    }
    ++n_term;
    c.process_result(0, true, false);
  }
  if (lane == 0) sb_dl_close_tree<false>(sb, dl, ep, ar, slot, parity, pend, n_term, left, 0);
  c.store(kSlotWaitEval);
}

template <class GM>
__global__ __launch_bounds__(64) void k_sb_big_find_dl_po(EngineParams ep, EngineArrays ar, SbArrays sb, SbDlArrays dl, SbRollArrays ro, uint32_t n,
                                                          uint32_t L, uint32_t parity) {
  __shared__ BigScratch<GM> sm;
  const uint32_t slot = blockIdx.x, lane = threadIdx.x;
  if (slot == 0 && lane == 0) dl.todo_max[parity ^ 1u] = 0;
  if (slot >= n) return;
  uint32_t left = dl.todo[slot];
  if (sb.status[slot] != 0 || left == 0) {
    if (lane == 0) sb.pend[slot] = kPendNone;
    return;
  }
  BigSlot<GM> c(ep, ar, sm, slot, lane);
  c.load();
  uint32_t pend = kPendNone, n_term = 0;
  for (uint32_t d = 0; d < L && left > 0; ++d) {
    --left;
    typename GM::State leaf;
    uint32_t term = 0;
    if (!c.find_leaf(0, leaf, term)) {
      if (lane == 0) sb.status[slot] = kSbFindFailed;
      left = 0;
      break;
    }
    if (term == 0) {
      const uint32_t j = ro.count[slot];
      c.playout_eval(leaf, sb_rollout_seed(ro.seeds[slot], j));      // (ends with the wavefront's fence: every lane has read j)
      if (lane == 0) { ro.count[slot] = j + 1; ar.c_evals[slot] += 1; }
      pend = kPendRollout;
      break;
    }
    ++n_term;
    c.process_result(0, true, false);
  }
  if (lane == 0) sb_dl_close_tree<false>(sb, dl, ep, ar, slot, parity, pend, n_term, left, 0);
  c.sync();
  c.store(kSlotWaitEval);
}

}  // namespace azmi
