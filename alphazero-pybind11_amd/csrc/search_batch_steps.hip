// Batched position search, the steps: the checks every entry point starts with, the evaluator's arguments, one step and one search
// enqueued on a stream, and the step API / azmi_search_run* entry points over them.  Host code only (search_batch_host.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "cache_host.h"
#include "search_batch_host.h"

using namespace azmi;

// why `more` descents do not fit (0: they do).  Connect4's flat arena never reclaims, so max_simulations counts every descent
// since reset(), the searches between moves included; the wide games compact behind update_roots (the PlayManager engine's rule),
// so it counts the descents since the last one.
int sb_check_budget(const azmi_search* s, const char* what, uint64_t more) {
  if (more <= s->max_sims - s->sims_done) return AZMI_OK;
  if (s->flat_arena)
    return SB_FAIL(AZMI_ERR_OVERFLOW, "%s: %llu more simulations, %u of max_simulations = %u are already used: a Connect4 arena never "
                   "reclaims, so the budget counts every descent since reset(), moves included (a game needs visits x moves)", what,
                   static_cast<unsigned long long>(more), s->sims_done, s->max_sims);
  return SB_FAIL(AZMI_ERR_OVERFLOW, "%s: %llu more simulations, %u of max_simulations = %u are already used: the budget counts the "
                 "descents since the last update_roots (its compaction reclaims the discarded siblings)", what,
                 static_cast<unsigned long long>(more), s->sims_done, s->max_sims);
}

// synchronises `st` and turns a stopped tree / a raised overflow bit into an error that names the tree.  A finished tree
// (status > 0) is no error.  The two errors of a move (a move the root does not have, a root without visits) left their tree as
// it was: the tree is named, its status and the engine's "unknown move" bit are cleared, and the object stays usable.
int sb_check_device(azmi_search* s, hipStream_t st) {
  Control c;
  std::vector<int32_t> status(s->n);
  SB_TRY(hipMemcpyAsync(&c, s->pm->ar.ctl, sizeof(c), hipMemcpyDeviceToHost, st));
  SB_TRY(hipMemcpyAsync(status.data(), s->sb.status, static_cast<size_t>(s->n) * 4, hipMemcpyDeviceToHost, st));
  SB_TRY(hipStreamSynchronize(st));
  // the errors of a move are cleared wherever they sit, so that one of them never outlives its report behind another tree's stop
  uint32_t first = s->n, first_move = s->n;
  for (uint32_t i = 0; i < s->n; ++i) {
    if (status[i] >= 0) continue;
    if (status[i] == kSbBadMove || status[i] == kSbNoVisits) { if (first_move == s->n) first_move = i; }
    else if (first == s->n) first = i;
  }
  const int32_t move_code = first_move < s->n ? status[first_move] : 0;
  if (first_move < s->n) {
    for (uint32_t i = 0; i < s->n; ++i) if (status[i] == kSbBadMove || status[i] == kSbNoVisits) status[i] = 0;
    SB_TRY(hipMemcpy(s->sb.status, status.data(), static_cast<size_t>(s->n) * 4, hipMemcpyHostToDevice));
    if (c.overflow & 32u) {      // as azmi_mcts_update_root does for its one tree
      c.overflow &= ~32u; if (!c.overflow) c.stop = 0;
      SB_TRY(hipMemcpy(s->pm->ar.ctl, &c, sizeof(c), hipMemcpyHostToDevice));
    }
  }
  if (first < s->n) {
    const int32_t code = status[first];
    return SB_FAIL(code == kSbBadStart ? AZMI_ERR_INVALID : AZMI_ERR_OVERFLOW, "tree %u: %s (device overflow mask 0x%x)", first,
                   code == kSbBadStart ? "illegal move in the game record or malformed start position"
                   : code == kSbBadState ? "the root state did not take the move (rules or position-history capacity)"
                                         : "find_leaf failed (tree arena or path capacity)",
                   c.overflow);
  }
  if (move_code == kSbBadMove)
    return SB_FAIL(AZMI_ERR_INVALID, "tree %u: ahh, what is this move (update_roots: not a move of the tree's root; that tree is left "
                   "where it was, the other trees' moves of the call are applied)", first_move);
  if (move_code == kSbNoVisits) return SB_FAIL(AZMI_ERR_STATE, "tree %u: pick_moves: the root has no visits; search first", first_move);
  if (c.overflow) return SB_FAIL(AZMI_ERR_OVERFLOW, "device search stopped: overflow mask 0x%x", c.overflow);
  return AZMI_OK;
}

int sb_begin_step(azmi_search* s, const char* what) {
  if (!s) return SB_FAIL(AZMI_ERR_INVALID, "null argument");
  if (!s->ready) return SB_FAIL(AZMI_ERR_STATE, "%s: the trees have no positions; call reset first", what);
  return AZMI_OK;
}

// A NULL handle is what a caller holds whose create failed.  On a machine without a device that failure was the no-device one, and
// the move entry points repeat it (AZMI_ERR_NO_DEVICE); with a device a NULL handle is an invalid argument (include/azmi.h says so).
int sb_begin_read(azmi_search* s, const char* what) {
  if (!s) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return SB_FAIL(AZMI_ERR_NO_DEVICE, "no HIP device: libazmi has no CPU path");
  }
  return sb_begin_step(s, what);
}
// the calls that change the trees: not while a find_leaves step is pending
int sb_begin_move(azmi_search* s, const char* what) {
  int rc = sb_begin_read(s, what); if (rc) return rc;
  if (s->step_pending) return SB_FAIL(AZMI_ERR_STATE, "%s: a find_leaves step is pending; call process_results first", what);
  return AZMI_OK;
}

// the evaluator of azmi_search_run_eval / play_eval: NN needs a net, RANDOM and PLAYOUT take none; PLAYOUT takes no cache either
// (the reference's playout branch sits before the cache probe, play.py:306 / :320)
int sb_search_args(azmi_search* s, const char* what, int eval_type, azmi_net* net, azmi_cache* cache, SbSearchArgs* out) {
  azmi_pm* pm = s->pm;
  if (eval_type != AZMI_EVAL_NN && eval_type != AZMI_EVAL_RANDOM && eval_type != AZMI_EVAL_PLAYOUT)
    return SB_FAIL(AZMI_ERR_INVALID, "%s: eval_type %d is none of NN, RANDOM, PLAYOUT", what, eval_type);
  if (eval_type == AZMI_EVAL_NN && !net) return SB_FAIL(AZMI_ERR_INVALID, "%s: the NN evaluator needs a net", what);
  if (eval_type != AZMI_EVAL_NN && net)
    return SB_FAIL(AZMI_ERR_INVALID, "%s: the %s evaluator takes no net", what, eval_type == AZMI_EVAL_PLAYOUT ? "PLAYOUT" : "RANDOM");
  if (eval_type == AZMI_EVAL_PLAYOUT && cache)
    return SB_FAIL(AZMI_ERR_INVALID, "%s: the PLAYOUT evaluator takes no cache (a rollout's answer is not a function of the position)", what);
  out->ep = pm->ep; out->ar = pm->ar; out->net = net; out->playout = eval_type == AZMI_EVAL_PLAYOUT;
  if (cache && net) {
    if (cache->device != pm->device) return SB_FAIL(AZMI_ERR_INVALID, "cache lives on another device");
    if (cache->c.np != pm->gi.M || cache->c.nv != pm->gi.P + 1) return SB_FAIL(AZMI_ERR_INVALID, "cache: num_policy / num_value do not match the game");
    if (cache->c.cap != kWaveCap)
      return SB_FAIL(AZMI_ERR_INVALID, "cache: the engine probes 64-entry shards; create the cache with shards = max_size / 64 "
                     "(ShardedS3FIFOCache.for_engine)");
    if (!wave_layout(cache->c))      // a lane of a wave shard holds one ghost-ring entry (dev_cache.h)
      return SB_FAIL(AZMI_ERR_INVALID, "cache: ghost_size / shards = %u, but a 64-entry wave shard keeps at most 64 ghost keys; create the cache "
                     "with ghost_size <= max_size (ShardedS3FIFOCache.for_engine)", cache->c.ghost_cap);
    out->ep.cache_on = 1; out->ep.num_groups = 1;
    out->ar.cache = cache->c; out->ar.cache_keys = s->d_keys;
  }
  return AZMI_OK;
}

static EngineArrays wu_rows(const azmi_search* s, EngineArrays ar) {     // the engine arrays with the step-sized [K * N] row buffers in place
  ar.canon = s->wu.canon; ar.v = s->wu.v; ar.pi = s->wu.pi; ar.cache_keys = s->wu.keys;
  return ar;
}

// the leaf net over the step's rows (`rows`: their list, at most `cap` of them, in the row buffers of `ar`), its answers into the cache
static int sb_eval_rows(azmi_search* s, const EngineParams& ep, const EngineArrays& ar, const uint32_t* rows, uint32_t cap, azmi_net* net, hipStream_t st) {
  const int rc = azmi_net_forward_rows(net, ar.canon, ar.v, ar.pi, rows, s->sb.n_rows, cap, st);
  if (rc != AZMI_OK) return SB_FAIL(rc, "leaf net: %s", azmi_net_last_error());
  s->net_calls += 1;
  if (ep.cache_on) sb_launch_cache_insert(s, ep, ar, cap, st);
  return AZMI_OK;
}

// one step of every live tree on `st`: `kk` descents each (1 unless leaves_per_step > 1), the evaluator, the back-up
int sb_enqueue_step(azmi_search* s, const SbSearchArgs& a, uint32_t kk, uint32_t rn, hipStream_t st) {
  const EngineParams& ep = a.ep;
  const EngineArrays& ar = a.ar;
  azmi_net* net = a.net;
  int rc = AZMI_OK;
  if (s->dl_L > 1) {      // up to L descents of every tree that still owes some; at most one row per tree, so the rest of the step is K == 1's
    const uint32_t parity = s->dl_parity;
    s->dl_parity ^= 1u;
    if (a.playout) sb_launch_find_dl_playout(s, ep, ar, parity, st);
    else {
      sb_launch_find_dl(s, ep, ar, parity, net ? 0u : 1u, rn, st);
      if (net) { rc = sb_eval_rows(s, ep, ar, s->sb.rows, s->n, net, st); if (rc) return rc; }
    }
    // RANDOM leaves nothing pending (every descent is backed up by the find kernel): no process launch
    if (net || a.playout) sb_launch_process(s, ep, ar, rn, nullptr, nullptr, st);
  } else if (a.playout) {
    if (s->k_leaves > 1) sb_launch_step_playout_wu(s, ep, ar, kk, rn, st);
    else sb_launch_step_playout(s, ep, ar, rn, st);
  } else if (s->k_leaves > 1) {
    sb_launch_find_wu(s, ep, ar, kk, net ? 0u : 1u, rn, st);
    if (net) { rc = sb_eval_rows(s, ep, wu_rows(s, ar), s->wu.rows, s->n * kk, net, st); if (rc) return rc; }
    sb_launch_process_wu(s, ep, ar, kk, rn, nullptr, nullptr, st);
  } else {
    sb_launch_find(s, ep, ar, net ? 0u : 1u, st);
    if (net) { rc = sb_eval_rows(s, ep, ar, s->sb.rows, s->n, net, st); if (rc) return rc; }
    sb_launch_process(s, ep, ar, rn, nullptr, nullptr, st);
  }
  s->steps += 1;
  return AZMI_OK;
}

// descents_per_step = L > 1: every live tree owes `visits` descents (todo, set by one launch) and pays up to L of them per step, as
// long as they need no evaluator.  RANDOM: every descent is immediate, so ceil(visits / L) steps complete the search and nothing
// is read.  Net / PLAYOUT: ceil(visits / L) steps, then repeat { read r = the largest todo the last step left (4 bytes); stop at 0;
// enqueue m more steps }: m = ceil(r / L) behind the first read (the fewest steps that can finish: all that a search whose leaves
// are terminal or cached needs), max(ceil(r / L), twice the previous m) behind every later one, and never more than r.  Every step
// gives every tree that owes descents at least one, so r steps always finish, and round k >= 1 holds at least 2^(k-1) steps unless it
// is capped at r: the search is complete behind round ceil(log2(visits)) at the latest, after at most 1 + ceil(log2(visits)) reads.
// (Halving r instead - max(1, ceil(r / 2)) steps per read - takes 1 + visits / 2 steps where the leaves are all immediate and 2 do.)
// The call returns behind the read of 0: only the last step's back-up may still be running
static int enqueue_search_dl(azmi_search* s, const SbSearchArgs& a, uint32_t visits, uint32_t rn, hipStream_t st) {
  if (!visits) return AZMI_OK;
  sb_launch_todo_set(s, visits, st);
  s->dl_parity = 0;
  const bool blind = !a.net && !a.playout;
  uint32_t more = (visits + s->dl_L - 1) / s->dl_L;
  for (uint32_t reads = 0;; ++reads) {      // round `reads` of `more` steps
    for (uint32_t i = 0; i < more; ++i) {
      const int rc = sb_enqueue_step(s, a, 1, rn, st);
      if (rc != AZMI_OK) return rc;
    }
    SB_TRY(hipGetLastError());
    if (blind) break;
    if (reads > 40) return SB_FAIL(AZMI_ERR_STATE, "search: the trees' descent counters did not reach 0 (descents_per_step)");      // (unreachable: 33 reads bound a uint32 budget)
    uint32_t r = 0;
    SB_TRY(hipMemcpyAsync(&r, s->dl.todo_max + (s->dl_parity ^ 1u), 4, hipMemcpyDeviceToHost, st));
    SB_TRY(hipStreamSynchronize(st));
    s->host_reads += 1;
    if (r == 0) break;
    const uint32_t fewest = (r + s->dl_L - 1) / s->dl_L;
    more = std::min<uint32_t>(r, reads == 0 ? fewest : std::max<uint32_t>(fewest, more > 0x7FFFFFFFu ? more : 2u * more));
  }
  s->sims_done += visits;
  return AZMI_OK;
}

// the steps of search(visits) on `st`, nothing read back: azmi_search_run, and every move of azmi_search_play.  Enqueued back to
// back: the row count of a step never leaves the device.  K > 1: visits / K steps of K descents and one of the remainder
int sb_enqueue_search(azmi_search* s, const SbSearchArgs& a, uint32_t visits, uint32_t rn, hipStream_t st) {
  if (s->gumbel && visits) sb_launch_query(s, kQSetGumbelSims, 0.0f, visits, st);     // set_gumbel_num_sims(visits) on every tree
  if (s->dl_L > 1) return enqueue_search_dl(s, a, visits, rn, st);
  for (uint32_t left = visits; left;) {
    const uint32_t kk = std::min<uint32_t>(s->k_leaves, left);
    const int rc = sb_enqueue_step(s, a, kk, rn, st);
    if (rc != AZMI_OK) return rc;
    left -= kk;
  }
  SB_TRY(hipGetLastError());
  s->sims_done += visits;
  return AZMI_OK;
}

extern "C" {

int azmi_search_find_leaves(azmi_search* s, void* stream, float** dev_canonical, uint32_t** dev_tree_index, uint32_t* n_rows) {
  int rc = sb_begin_step(s, "find_leaves"); if (rc) return rc;
  if (!n_rows) return SB_FAIL(AZMI_ERR_INVALID, "null argument");
  if (s->step_pending) return SB_FAIL(AZMI_ERR_STATE, "find_leaves: the previous step's process_results has not been called");
  if (s->dl_L > 1)
    return SB_FAIL(AZMI_ERR_INVALID, "find_leaves with descents_per_step = %u: the step API's caller owns the evaluator and the step, one "
                   "descent of every tree each; use search / play, or descents_per_step = 1", s->dl_L);
  rc = sb_check_budget(s, "find_leaves", 1); if (rc) return rc;
  azmi_pm* pm = s->pm;
  SB_TRY(hipSetDevice(pm->device));
  hipStream_t st = pm->pick(stream);
  const bool wu = s->k_leaves > 1;
  const uint32_t kk = std::min<uint32_t>(s->k_leaves, s->max_sims - s->sims_done);     // fewer than K left: the remainder only
  if (wu) sb_launch_find_wu(s, pm->ep, pm->ar, kk, 0u, 0u, st);
  else sb_launch_find(s, pm->ep, pm->ar, 0u, st);
  sb_launch_gather(s, kk, st);
  SB_TRY(hipGetLastError());
  uint32_t rows = 0;
  SB_TRY(hipMemcpyAsync(&rows, s->sb.n_rows, 4, hipMemcpyDeviceToHost, st));
  rc = sb_check_device(s, st); if (rc) return rc;
  s->step_pending = true; s->step_rows = rows; s->step_k = kk;
  if (dev_canonical) *dev_canonical = wu ? s->d_batch_wu : s->d_batch;
  if (dev_tree_index) *dev_tree_index = wu ? s->wu.tree_of : s->sb.rows;
  *n_rows = rows;
  return AZMI_OK;
}

int azmi_search_leaves_to_host(azmi_search* s, float* canonical, uint32_t* tree_index) {
  if (!s) return SB_FAIL(AZMI_ERR_INVALID, "null argument");
  if (!s->step_pending) return SB_FAIL(AZMI_ERR_STATE, "no leaf batch: call find_leaves first");
  SB_TRY(hipSetDevice(s->pm->device));
  hipStream_t st = s->pm->last;
  const bool wu = s->k_leaves > 1;
  if (canonical && s->step_rows)
    SB_TRY(hipMemcpyAsync(canonical, wu ? s->d_batch_wu : s->d_batch, static_cast<size_t>(s->step_rows) * s->chw * 4, hipMemcpyDeviceToHost, st));
  if (tree_index && s->step_rows)
    SB_TRY(hipMemcpyAsync(tree_index, wu ? s->wu.tree_of : s->sb.rows, static_cast<size_t>(s->step_rows) * 4, hipMemcpyDeviceToHost, st));
  SB_TRY(hipStreamSynchronize(st));
  return AZMI_OK;
}

int azmi_search_leaf_keys(azmi_search* s, void* stream, uint64_t** dev_keys, uint32_t* n_rows) {
  if (!s || !dev_keys || !n_rows) return SB_FAIL(AZMI_ERR_INVALID, "leaf_keys: null argument");
  if (!s->step_pending) return SB_FAIL(AZMI_ERR_STATE, "leaf_keys: no leaf batch is pending; call find_leaves first");
  azmi_pm* pm = s->pm;
  SB_TRY(hipSetDevice(pm->device));
  const size_t need = static_cast<size_t>(s->n) * s->k_leaves * 8;
  if (!s->leaf_keys_block.p || need > s->leaf_keys_block.bytes) {      // the first call / a larger leaves_per_step only
    if (s->leaf_keys_block.reserve(need) != hipSuccess) return SB_FAIL(AZMI_ERR_OOM, "leaf_keys: %zu bytes of device memory", need);
    s->d_leaf_keys = static_cast<uint64_t*>(s->leaf_keys_block.p);
  }
  hipStream_t st = pm->pick(stream);
  sb_launch_leaf_keys(s, st);
  SB_TRY(hipGetLastError());
  SB_TRY(hipStreamSynchronize(st));      // the caller's evaluator runs on a stream of its own
  *dev_keys = s->d_leaf_keys; *n_rows = s->step_rows;
  return AZMI_OK;
}

int azmi_search_process_results(azmi_search* s, const float* dev_v, const float* dev_pi, int root_noise_enabled, void* stream) {
  int rc = sb_begin_step(s, "process_results"); if (rc) return rc;
  if (!s->step_pending) return SB_FAIL(AZMI_ERR_STATE, "process_results: no leaf batch is pending; call find_leaves first");
  if (s->step_rows && (!dev_v || !dev_pi)) return SB_FAIL(AZMI_ERR_INVALID, "null argument");
  azmi_pm* pm = s->pm;
  SB_TRY(hipSetDevice(pm->device));
  hipStream_t st = pm->pick(stream);
  // (with no rows the pointers are not read: every pending tree is a terminal leaf already backed up)
  if (s->k_leaves > 1)
    sb_launch_process_wu(s, pm->ep, pm->ar, s->step_k, root_noise_enabled ? 1u : 0u, s->step_rows ? dev_v : nullptr, s->step_rows ? dev_pi : nullptr, st);
  else
    sb_launch_process(s, pm->ep, pm->ar, root_noise_enabled ? 1u : 0u, s->step_rows ? dev_v : nullptr, s->step_rows ? dev_pi : nullptr, st);
  SB_TRY(hipGetLastError());
  s->step_pending = false;
  s->sims_done += s->step_k; s->steps += 1;
  return AZMI_OK;
}

int azmi_search_process_results_host(azmi_search* s, const float* v, const float* pi, int root_noise_enabled) {
  int rc = sb_begin_step(s, "process_results"); if (rc) return rc;
  if (!s->step_pending) return SB_FAIL(AZMI_ERR_STATE, "process_results: no leaf batch is pending; call find_leaves first");
  if (s->step_rows && (!v || !pi)) return SB_FAIL(AZMI_ERR_INVALID, "null argument");
  azmi_pm* pm = s->pm;
  SB_TRY(hipSetDevice(pm->device));
  hipStream_t st = pm->last;
  float* d_v = s->k_leaves > 1 ? s->d_vrows_wu : s->d_vrows;
  float* d_pi = s->k_leaves > 1 ? s->d_pirows_wu : s->d_pirows;
  if (s->step_rows) {
    SB_TRY(hipMemcpyAsync(d_v, v, static_cast<size_t>(s->step_rows) * (pm->gi.P + 1) * 4, hipMemcpyHostToDevice, st));
    SB_TRY(hipMemcpyAsync(d_pi, pi, static_cast<size_t>(s->step_rows) * pm->gi.M * 4, hipMemcpyHostToDevice, st));
  }
  rc = azmi_search_process_results(s, d_v, d_pi, root_noise_enabled, st);
  if (rc) return rc;
  SB_TRY(hipStreamSynchronize(st));     // the host arrays may be reused by the caller
  return AZMI_OK;
}

int azmi_search_run_eval(azmi_search* s, int eval_type, azmi_net* net, azmi_cache* cache, uint32_t visits, int root_noise_enabled, void* stream) {
  int rc = sb_begin_step(s, "search"); if (rc) return rc;
  if (s->step_pending) return SB_FAIL(AZMI_ERR_STATE, "search: a find_leaves step is pending; call process_results first");
  rc = sb_check_budget(s, "search", visits); if (rc) return rc;
  SbSearchArgs a;
  rc = sb_search_args(s, "search", eval_type, net, cache, &a); if (rc) return rc;
  SB_TRY(hipSetDevice(s->pm->device));
  return sb_enqueue_search(s, a, visits, root_noise_enabled ? 1u : 0u, s->pm->pick(stream));
}

int azmi_search_run(azmi_search* s, azmi_net* net, azmi_cache* cache, uint32_t visits, int root_noise_enabled, void* stream) {
  return azmi_search_run_eval(s, net ? AZMI_EVAL_NN : AZMI_EVAL_RANDOM, net, cache, visits, root_noise_enabled, stream);
}

}  // extern "C"
