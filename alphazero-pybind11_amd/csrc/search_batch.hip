// Batched position search (azmi_search_*, include/azmi.h): N search trees on N different positions in ONE engine arena, all of
// them advanced by one simulation per (find-leaves, process-results) launch pair, the leaf net and the position cache on the
// device.  Host side of csrc/search_batch_kernels.h.  The engine behind it is a PlayManager engine with N slots built from the
// MCTS constructor's arguments (azmi_host_mcts_params, as azmi_mcts_create does for its one slot); the engine's own game loop never
// runs on it.  Moves ARE played on the trees: azmi_search_pick_moves / update_roots / root_prior / play below advance every tree's
// root on the device (update_root with tree reuse) and cross moves without the host.
// azmi_search_set_leaves_per_step(K > 1) switches every step to K descents per tree with K leaves in flight (WU-UCT): the *_wu
// kernels and launch helpers below; K == 1 runs the original ones.
// azmi_search_run_eval / play_eval with AZMI_EVAL_PLAYOUT evaluate every leaf by a random rollout on the device (the *_po kernels):
// no compaction, no net call, no cache insert, at most 3 launches a step.
// azmi_search_set_descents_per_step(L > 1) lets a tree go on descending inside a step while its leaves need no evaluator (terminal,
// RANDOM, cache hit): the *_dl kernels; a search then needs fewer steps than visits, and reads one word back to know how many.
// This file is also the ONE device module of the four search_*_kernels.h: a kernel header defines non-template kernels, and the
// code of a kernel depends on the kernels it shares a module with and on the order they are instantiated in (DESIGN.md sections
// 1 and 8.3).  So every launch lives here, one thin sb_launch_* function per kernel family (search_batch_host.h), in the order the
// families were added; the entry points of the visit sweep, of capture / dedup / net metrics and of the opening-tree frontier are
// host code only, in search_batch_sweep.hip, search_batch_pool.hip and search_batch_frontier.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <type_traits>
#include <vector>

#include "cache_host.h"
#include "search_batch_host.h"
#include "search_batch_kernels.h"
#include "search_pool_kernels.h"
#include "search_frontier_kernels.h"
#include "search_sweep_metrics_kernels.h"

using namespace azmi;

namespace {

constexpr uint32_t kSmallThreads = 256;
inline uint32_t small_blocks(uint32_t n) { return (n * static_cast<uint32_t>(Connect4::GROUP) + kSmallThreads - 1) / kSmallThreads; }

// small(Connect4{}) / big(GM{}) as for_game, with this file's own last arm: any other id runs as StarGambit (ids are validated at create)
template <class Small, class Big>
void sb_for_game(int game, Small&& small, Big&& big) {
  switch (game) {
    case AZMI_GAME_CONNECT4: small(Connect4{}); break;
    case AZMI_GAME_TAWLBWRDD: big(Tawlbwrdd{}); break;
    case AZMI_GAME_BRANDUBH: big(Brandubh{}); break;
    case AZMI_GAME_OPENTAFL: big(OpenTafl{}); break;
    default: big(StarGambit{}); break;
  }
}

// one launch of a step over the s->n trees: Connect4's kernel on its 8-lane groups, the wide games' on one wavefront per tree
#define SB_LAUNCH(s, st, k_small, k_big, ...)                                                                                              \
  do {                                                                                                                                     \
    sb_for_game((s)->pm->game,                                                                                                             \
                [&](auto tag) { using GM = decltype(tag); k_small<GM><<<small_blocks((s)->n), kSmallThreads, 0, st>>>(__VA_ARGS__); },     \
                [&](auto tag) { using GM = decltype(tag); k_big<GM><<<(s)->n, 64, 0, st>>>(__VA_ARGS__); });                               \
    (s)->launches += 1;                                                                                                                    \
  } while (0)

}  // namespace

void sb_launch_find(azmi_search* s, const EngineParams& ep, const EngineArrays& ar, uint32_t eval_random, hipStream_t st) {
  SB_LAUNCH(s, st, k_sb_find, k_sb_big_find, ep, ar, s->sb, s->n, eval_random);
  k_sb_compact<<<1, 1024, 0, st>>>(s->sb, s->n);
  s->launches += 1;
}

void sb_launch_process(azmi_search* s, const EngineParams& ep, const EngineArrays& ar, uint32_t root_noise, const float* v_rows, const float* pi_rows,
                    hipStream_t st) {
  SB_LAUNCH(s, st, k_sb_process, k_sb_big_process, ep, ar, s->sb, s->n, root_noise, v_rows, pi_rows);
}

void sb_launch_query(azmi_search* s, uint32_t kind, float temp, uint32_t arg, hipStream_t st) {
  SB_LAUNCH(s, st, k_sb_query, k_sb_big_query, s->pm->ep, s->pm->ar, s->n, kind, temp, arg, s->d_qf, s->vec_f, s->d_qu, s->vec_u);
}
void sb_launch_query_scalars(azmi_search* s, hipStream_t st) { sb_launch_query(s, kQScalars, 0.0f, 0u, st); }

// the answers of the step's net call go into the cache (PlayManager::update_inferences -> insert_many, play_manager.cc:631-640):
// keys left by the find kernel in ar.cache_keys, (pi, v) rows indexed like them; `total` = N entries (K > 1: the kk * N of the
// step, `ar` = wu_rows); ceil(total / kApplyMax) launches
void sb_launch_cache_insert(azmi_search* s, const EngineParams& ep, const EngineArrays& ar, uint32_t total, hipStream_t st) {
  for (uint32_t off = 0; off < total; off += kApplyMax) {
    const uint32_t m = std::min<uint32_t>(kApplyMax, total - off);
    auto insert = [&](auto tag) { using GM = decltype(tag); k_cache_insert<GM><<<(m + 3) / 4, 256, 0, st>>>(ep, ar, ar.cache_keys, off, m, 0xFFFFFFFFu, 0u, 0u); };
    sb_for_game(s->pm->game, insert, insert);
    s->launches += 1;
  }
}

// ---- K > 1: the same steps over K descents of every tree; the launch counts do not depend on N or K ---------------------------
static EngineArrays wu_rows(const azmi_search* s, EngineArrays ar) {     // the engine arrays with the step-sized [K * N] row buffers in place
  ar.canon = s->wu.canon; ar.v = s->wu.v; ar.pi = s->wu.pi; ar.cache_keys = s->wu.keys;
  return ar;
}

void sb_launch_find_wu(azmi_search* s, const EngineParams& ep, const EngineArrays& ar, uint32_t kk, uint32_t eval_random, uint32_t root_noise, hipStream_t st) {
  SB_LAUNCH(s, st, k_sb_find_wu, k_sb_big_find_wu, ep, ar, s->sb, s->wu, s->n, kk, eval_random, root_noise);
  k_sb_compact_wu<<<1, 1024, 0, st>>>(s->sb, s->wu, s->n, kk);
  s->launches += 1;
}

void sb_launch_process_wu(azmi_search* s, const EngineParams& ep, const EngineArrays& ar, uint32_t kk, uint32_t root_noise, const float* v_rows,
                       const float* pi_rows, hipStream_t st) {
  SB_LAUNCH(s, st, k_sb_process_wu, k_sb_big_process_wu, ep, ar, s->wu, s->n, kk, root_noise, v_rows, pi_rows);
}

static void wu_free(azmi_search* s) {
  for (void* q : s->wu_allocs) (void)hipFree(q);
  s->wu_allocs.clear();
  s->wu = SbWuArrays{};
  s->d_batch_wu = nullptr; s->d_vrows_wu = nullptr; s->d_pirows_wu = nullptr;
}

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

// one step of every live tree on `st`: `kk` descents each (1 unless leaves_per_step > 1), the evaluator, the back-up
int sb_enqueue_step(azmi_search* s, const SbSearchArgs& a, uint32_t kk, uint32_t rn, hipStream_t st) {
  const EngineParams& ep = a.ep;
  const EngineArrays& ar = a.ar;
  azmi_net* net = a.net;
  if (s->dl_L > 1) {      // up to L descents of every tree that still owes some; at most one row per tree, so the rest of the step is K == 1's
    const uint32_t parity = s->dl_parity;
    s->dl_parity ^= 1u;
    if (a.playout) sb_launch_find_dl_playout(s, ep, ar, parity, st);
    else {
      sb_launch_find_dl(s, ep, ar, parity, net ? 0u : 1u, rn, st);
      if (net) {
        const int rc = azmi_net_forward_rows(net, ar.canon, ar.v, ar.pi, s->sb.rows, s->sb.n_rows, s->n, st);
        if (rc != AZMI_OK) return SB_FAIL(rc, "leaf net: %s", azmi_net_last_error());
        s->net_calls += 1;
        if (ep.cache_on) sb_launch_cache_insert(s, ep, ar, s->n, st);
      }
    }
    // RANDOM leaves nothing pending (every descent is backed up by the find kernel): no process launch
    if (net || a.playout) sb_launch_process(s, ep, ar, rn, nullptr, nullptr, st);
  } else if (a.playout) {
    if (s->k_leaves > 1) sb_launch_step_playout_wu(s, ep, ar, kk, rn, st);
    else sb_launch_step_playout(s, ep, ar, rn, st);
  } else if (s->k_leaves > 1) {
    const EngineArrays aw = wu_rows(s, ar);
    sb_launch_find_wu(s, ep, ar, kk, net ? 0u : 1u, rn, st);
    if (net) {
      const int rc = azmi_net_forward_rows(net, aw.canon, aw.v, aw.pi, s->wu.rows, s->sb.n_rows, s->n * kk, st);
      if (rc != AZMI_OK) return SB_FAIL(rc, "leaf net: %s", azmi_net_last_error());
      s->net_calls += 1;
      if (ep.cache_on) sb_launch_cache_insert(s, ep, aw, s->n * kk, st);
    }
    sb_launch_process_wu(s, ep, ar, kk, rn, nullptr, nullptr, st);
  } else {
    sb_launch_find(s, ep, ar, net ? 0u : 1u, st);
    if (net) {
      const int rc = azmi_net_forward_rows(net, ar.canon, ar.v, ar.pi, s->sb.rows, s->sb.n_rows, s->n, st);
      if (rc != AZMI_OK) return SB_FAIL(rc, "leaf net: %s", azmi_net_last_error());
      s->net_calls += 1;
      if (ep.cache_on) sb_launch_cache_insert(s, ep, ar, s->n, st);
    }
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

// ---- a move: pick, update-root (+ compaction for the wide games), root prior; one launch each, whatever N is ------------------
void sb_launch_pick(azmi_search* s, float temp, hipStream_t st) {
  SB_LAUNCH(s, st, k_sb_pick, k_sb_big_pick, s->pm->ep, s->pm->ar, s->sb, s->pl, s->n, temp, s->d_qf, s->vec_f, s->d_qu, s->vec_u);
}

// `moves`: [N] on the device.  The wide games compact behind it (k_compact lives in engine.hip's device module)
void sb_launch_update_root(azmi_search* s, const int32_t* moves, hipStream_t st) {
  uint32_t* nif = s->k_leaves > 1 ? s->wu.wu.nif : nullptr;
  SB_LAUNCH(s, st, k_sb_update_root, k_sb_big_update_root, s->pm->ep, s->pm->ar, s->sb, s->pl, s->n, moves, nif);
  if (s->pm->ep.half_nodes) {
    azmi_host_launch_compact(s->pm, st, s->n * s->pm->gi.P, nif);
    s->launches += 1;
  }
}

void sb_launch_root_prior(azmi_search* s, uint32_t apply_temp, uint32_t noise, hipStream_t st) {
  SB_LAUNCH(s, st, k_sb_root_prior, k_sb_big_root_prior, s->pm->ep, s->pm->ar, s->sb, s->n, apply_temp, noise, s->d_qf, s->vec_f, s->d_qu, s->vec_u);
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

extern "C" {

int azmi_search_create(int game, const azmi_mcts_config* cfg, uint32_t n_trees, int device, azmi_search** out) {
  if (!cfg || !out) return SB_FAIL(AZMI_ERR_INVALID, "null argument");
  if (n_trees == 0) return SB_FAIL(AZMI_ERR_INVALID, "n_trees must be > 0");
  if (cfg->max_simulations == 0)
    return SB_FAIL(AZMI_ERR_INVALID, "max_simulations is required for a batched search (it sizes every tree's arena; the one-tree default "
                   "of 50000 times n_trees would not fit)");
  azmi_play_params p;
  int rc = azmi_host_mcts_params(game, cfg, cfg->max_simulations, &p);
  if (rc != AZMI_OK) return rc;
  if (game != AZMI_GAME_CONNECT4 && cfg->max_simulations > 8000u)
    return SB_FAIL(AZMI_ERR_INVALID, "max_simulations: at most 8000 per tree for the wide games, got %u", cfg->max_simulations);
  p.history_enabled = 0;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return SB_FAIL(AZMI_ERR_NO_DEVICE, "no HIP device: libazmi has no CPU path");
  if (device < 0 || device >= ndev) return SB_FAIL(AZMI_ERR_INVALID, "device %d out of range", device);
  SB_TRY(hipSetDevice(device));
  azmi_engine_opts o;
  azmi_engine_opts_default(&o);
  o.device = device;
  // does it fit?  Every array of the engine scales with the slot count: a one-slot engine tells the bytes per tree
  {
    azmi_pm* probe = nullptr;
    rc = azmi_pm_create(game, &p, &o, &probe);
    if (rc != AZMI_OK) return rc;
    const size_t per_tree = probe->bytes;
    azmi_pm_destroy(probe);
    size_t free_b = 0, total_b = 0;
    SB_TRY(hipMemGetInfo(&free_b, &total_b));
    const unsigned long long need = static_cast<unsigned long long>(per_tree) * n_trees;
    if (need > free_b)
      return SB_FAIL(AZMI_ERR_OOM, "%u trees x %u simulations need %llu bytes of device memory (%llu per tree), %llu are free", n_trees,
                     cfg->max_simulations, need, static_cast<unsigned long long>(per_tree), static_cast<unsigned long long>(free_b));
  }
  p.concurrent_games = n_trees; p.games_to_play = n_trees; p.max_batch_size = n_trees;
  auto s = new azmi_search();
  rc = azmi_pm_create(game, &p, &o, &s->pm);
  if (rc != AZMI_OK) { delete s; return rc; }
  azmi_pm* pm = s->pm;
  s->n = n_trees; s->max_sims = cfg->max_simulations; s->gumbel = cfg->gumbel_enabled != 0;
  s->flat_arena = game == AZMI_GAME_CONNECT4; s->root_temp = cfg->root_policy_temp;
  s->pl.log_cap = pm->gi.max_turns + 8;      // the MCTS object's moves_cap
  s->chw = pm->gi.C * pm->gi.H * pm->gi.W;
  s->vec_f = std::max<uint32_t>(pm->gi.M, 64u);
  s->vec_u = s->vec_f + 64u;
  const size_t N = n_trees;
  auto A = [&](auto*& ptr, size_t cnt) { return pm->alloc(ptr, cnt, true); };
  rc = A(s->sb.pend, N); if (rc == AZMI_OK) rc = A(s->sb.status, N); if (rc == AZMI_OK) rc = A(s->sb.row_of, N);
  if (rc == AZMI_OK) rc = A(s->sb.rows, N); if (rc == AZMI_OK) rc = A(s->sb.n_rows, 1); if (rc == AZMI_OK) rc = A(s->sb.n_term, N);
  if (rc == AZMI_OK) rc = A(s->d_keys, N);
  if (rc == AZMI_OK) rc = A(s->d_batch, N * s->chw);
  if (rc == AZMI_OK) rc = A(s->d_vrows, N * (pm->gi.P + 1)); if (rc == AZMI_OK) rc = A(s->d_pirows, N * pm->gi.M);
  if (rc == AZMI_OK) rc = A(s->d_qf, N * s->vec_f); if (rc == AZMI_OK) rc = A(s->d_qu, N * s->vec_u);
  if (rc == AZMI_OK) rc = A(s->pl.move, N); if (rc == AZMI_OK) rc = A(s->pl.log, N * s->pl.log_cap); if (rc == AZMI_OK) rc = A(s->pl.log_len, N);
  if (rc == AZMI_OK) rc = A(s->pl.final, N * (pm->gi.P + 1)); if (rc == AZMI_OK) rc = A(s->d_moves_in, N);
  if (rc == AZMI_OK) rc = A(s->ro.seeds, N); if (rc == AZMI_OK) rc = A(s->ro.count, N);
  if (rc == AZMI_OK) rc = A(s->ro.states, game == AZMI_GAME_CONNECT4 ? N * sizeof(Connect4::State) : 1);
  if (rc == AZMI_OK) rc = A(s->dl.todo, N); if (rc == AZMI_OK) rc = A(s->dl.todo_max, 2);
  if (rc != AZMI_OK) { azmi_pm_destroy(pm); delete s; return rc; }
  *out = s;
  return AZMI_OK;
}

void azmi_search_destroy(azmi_search* s) {
  if (!s) return;
  (void)hipSetDevice(s->pm->device);
  wu_free(s);        // (hipFree waits for the device)
  if (s->sw_block.p) (void)hipFree(s->sw_block.p);
  if (s->sm_block.p) (void)hipFree(s->sm_block.p);
  if (s->fr_trees) (void)hipFree(s->fr_trees);
  if (s->fr_records.p) (void)hipFree(s->fr_records.p);
  if (s->fr_host) (void)hipHostFree(s->fr_host);
  if (s->fr_uploaded) (void)hipEventDestroy(s->fr_uploaded);
  azmi_pm_destroy(s->pm);
  delete s;
}

int azmi_search_set_leaves_per_step(azmi_search* s, uint32_t k) {
  if (!s) return SB_FAIL(AZMI_ERR_INVALID, "null argument");
  if (k < 1 || k > 64) return SB_FAIL(AZMI_ERR_INVALID, "leaves_per_step must be in [1, 64], got %u", k);
  if (k > 1 && s->gumbel)
    return SB_FAIL(AZMI_ERR_INVALID, "leaves_per_step = %u with gumbel_enabled: the batched descent (find_leaf_batched) is plain PUCT; "
                   "use leaves_per_step = 1 for a Gumbel search", k);
  if (k > 1 && s->dl_L > 1)
    return SB_FAIL(AZMI_ERR_INVALID, "leaves_per_step = %u with descents_per_step = %u: a step holds either several leaves of a tree in flight "
                   "or goes on descending past the leaves that need no evaluator, not both", k, s->dl_L);
  if (s->step_pending) return SB_FAIL(AZMI_ERR_STATE, "set_leaves_per_step: a find_leaves step is pending; call process_results first");
  if (s->sims_done != 0) return SB_FAIL(AZMI_ERR_STATE, "set_leaves_per_step: the trees have been searched; call reset first");
  azmi_pm* pm = s->pm;
  SB_TRY(hipSetDevice(pm->device));
  SB_TRY(hipStreamSynchronize(pm->last));
  wu_free(s);
  s->k_leaves = 1;
  if (k == 1) return AZMI_OK;
  const size_t N = s->n, E = N * k, P = pm->gi.P, M = pm->gi.M;
  const size_t nif_cnt = N * P * pm->ep.cap;
  const unsigned long long need = 4ull * nif_cnt + E * (4ull * pm->ep.max_depth + 8 + 1 + 12 + 8) +
                                  8ull * E * (static_cast<size_t>(s->chw) + (P + 1) + M);
  size_t free_b = 0, total_b = 0;
  SB_TRY(hipMemGetInfo(&free_b, &total_b));
  if (need > free_b)
    return SB_FAIL(AZMI_ERR_OOM, "leaves_per_step = %u on %u trees needs %llu bytes of device memory for the in-flight records and the "
                   "step's row buffers, %llu are free", k, s->n, need, static_cast<unsigned long long>(free_b));
  hipError_t e = hipSuccess;
  auto A = [&](auto*& ptr, size_t cnt) {
    if (e != hipSuccess) return;
    void* q = nullptr;
    const size_t sz = std::max<size_t>(cnt, 1) * sizeof(*ptr);
    e = hipMalloc(&q, sz);
    if (e != hipSuccess) return;
    s->wu_allocs.push_back(q);
    e = hipMemset(q, 0, sz);
    ptr = static_cast<std::remove_reference_t<decltype(ptr)>>(q);
  };
  SbWuArrays& w = s->wu;
  A(w.wu.nif, nif_cnt); A(w.wu.ifl_path, E * pm->ep.max_depth); A(w.wu.ifl_plen, E); A(w.wu.ifl_cur, E);
  A(w.pend, E); A(w.row_of, E); A(w.rows, E); A(w.tree_of, E);
  A(w.canon, E * s->chw); A(w.v, E * (P + 1)); A(w.pi, E * M); A(w.keys, E);
  A(s->d_batch_wu, E * s->chw); A(s->d_vrows_wu, E * (P + 1)); A(s->d_pirows_wu, E * M);
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  if (e != hipSuccess) {
    wu_free(s);
    return SB_FAIL(AZMI_ERR_OOM, "leaves_per_step = %u: %llu bytes of device memory: %s", k, need, hipGetErrorString(e));
  }
  s->k_leaves = k;
  return AZMI_OK;
}

int azmi_search_set_descents_per_step(azmi_search* s, uint32_t l) {
  if (!s) return SB_FAIL(AZMI_ERR_INVALID, "null argument");
  if (l < 1 || l > 256) return SB_FAIL(AZMI_ERR_INVALID, "descents_per_step must be in [1, 256], got %u", l);
  if (l > 1 && s->k_leaves > 1)
    return SB_FAIL(AZMI_ERR_INVALID, "descents_per_step = %u with leaves_per_step = %u: a step holds either several leaves of a tree in flight "
                   "or goes on descending past the leaves that need no evaluator, not both", l, s->k_leaves);
  if (s->step_pending) return SB_FAIL(AZMI_ERR_STATE, "set_descents_per_step: a find_leaves step is pending; call process_results first");
  if (s->sims_done != 0) return SB_FAIL(AZMI_ERR_STATE, "set_descents_per_step: the trees have been searched; call reset first");
  s->dl_L = l;
  return AZMI_OK;
}

int azmi_search_host_reads(azmi_search* s, uint64_t* out) {
  if (!s || !out) return SB_FAIL(AZMI_ERR_INVALID, "null argument");
  *out = s->host_reads;
  return AZMI_OK;
}

int azmi_search_reset(azmi_search* s, const uint8_t* init, uint32_t init_stride, const int32_t* moves, const uint32_t* move_offsets,
                      const uint64_t* seeds) {
  if (!s || !move_offsets || !seeds) return SB_FAIL(AZMI_ERR_INVALID, "null argument");
  azmi_pm* pm = s->pm;
  const uint32_t n = s->n;
  if (move_offsets[0] != 0) return SB_FAIL(AZMI_ERR_INVALID, "move_offsets[0] must be 0");
  for (uint32_t i = 0; i < n; ++i) {
    if (move_offsets[i + 1] < move_offsets[i]) return SB_FAIL(AZMI_ERR_INVALID, "tree %u: move_offsets must not decrease", i);
    if (move_offsets[i + 1] - move_offsets[i] > pm->gi.max_turns + 8) return SB_FAIL(AZMI_ERR_INVALID, "tree %u: game record too long", i);
  }
  const uint32_t total = move_offsets[n];
  if (total && !moves) return SB_FAIL(AZMI_ERR_INVALID, "null argument");
  if (init) {
    uint32_t extra = 0;
    const int rc = azmi_host_check_init_rows(pm->game, init, init_stride, n, &extra);
    if (rc != AZMI_OK) return rc;
  }
  SB_TRY(hipSetDevice(pm->device));
  hipStream_t st = pm->stream;
  s->ready = false; s->step_pending = false; s->sims_done = 0;
  s->tree_seeds.assign(seeds, seeds + n);
  std::vector<uint64_t> roll(n);      // the default rollout seeds (azmi_search_set_rollout_seeds replaces them)
  for (uint32_t i = 0; i < n; ++i) roll[i] = mix64(seeds[i] ^ kRollSalt);
  DevTemps tmp(16);
  uint8_t* d_init = nullptr; int32_t* d_moves = nullptr; uint32_t* d_offs = nullptr; uint64_t* d_seeds = nullptr;
  auto stage = [&]() -> hipError_t {      // uploads, resets and the seed launch, queued on st; the first error ends it
    hipError_t e = init ? tmp.upload_async(d_init, init, static_cast<size_t>(n) * init_stride, st) : hipSuccess;
    if (e == hipSuccess) e = tmp.upload_async(d_moves, moves, total, st);
    if (e == hipSuccess) e = tmp.upload_async(d_offs, move_offsets, static_cast<size_t>(n) + 1, st);
    if (e == hipSuccess) e = tmp.upload_async(d_seeds, seeds, n, st);
    if (e == hipSuccess) e = hipMemsetAsync(pm->ar.ctl, 0, sizeof(Control), st);       // a stopped search does not outlive its positions
    if (e == hipSuccess) e = hipMemsetAsync(s->pl.log_len, 0, static_cast<size_t>(n) * 4, st);      // nor do the moves played on the old ones
    if (e == hipSuccess) e = hipMemsetAsync(s->pl.move, 0xFF, static_cast<size_t>(n) * 4, st);      // (-1: nothing picked yet)
    if (e == hipSuccess) e = hipMemcpyAsync(s->ro.seeds, roll.data(), static_cast<size_t>(n) * 8, hipMemcpyHostToDevice, st);      // (st is synchronised below)
    if (e == hipSuccess) e = hipMemsetAsync(s->ro.count, 0, static_cast<size_t>(n) * 4, st);
    if (e == hipSuccess && s->cp.len) e = hipMemsetAsync(s->cp.len, 0, static_cast<size_t>(n) * 4, st);      // the captured roots were the old positions'
    if (e == hipSuccess && pm->ep.half_nodes) e = hipMemsetAsync(pm->ar.compact_flag, 0, static_cast<size_t>(n) * pm->gi.P * 4, st);
    if (e == hipSuccess && s->k_leaves > 1)     // the in-flight mark of every root (node 0 of its tree); every other node gets its mark cleared when it is created
      e = hipMemset2DAsync(s->wu.wu.nif, static_cast<size_t>(pm->gi.P) * pm->ep.cap * 4, 0, 4, n, st);
    if (e != hipSuccess) return e;
    SB_LAUNCH(s, st, k_sb_seed, k_sb_big_seed, pm->ep, pm->ar, s->sb, n, d_init, init_stride, d_moves, d_offs, d_seeds);
    return hipGetLastError();
  };
  const hipError_t e = stage();
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(st);     // what was queued may still read the buffers tmp is about to free
    return SB_FAIL(AZMI_ERR_NO_DEVICE, "azmi_search_reset: %s", hipGetErrorString(e));
  }
  pm->last = st;
  const int rc = sb_check_device(s, st);   // synchronises st: tmp is freed after it
  if (rc != AZMI_OK) return rc;
  s->ready = true;
  return AZMI_OK;
}

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
  if (wu) {
    sb_launch_find_wu(s, pm->ep, pm->ar, kk, 0u, 0u, st);
    SbArrays rows_of_step = s->sb;       // k_sb_gather over the step's kk * N entries
    rows_of_step.row_of = s->wu.row_of;
    k_sb_gather<<<s->n * kk, 256, 0, st>>>(rows_of_step, s->n * kk, s->wu.canon, s->chw, s->d_batch_wu);
  } else {
    sb_launch_find(s, pm->ep, pm->ar, 0u, st);
    k_sb_gather<<<s->n, 256, 0, st>>>(s->sb, s->n, pm->ar.canon, s->chw, s->d_batch);
  }
  s->launches += 1;
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

int azmi_search_set_rollout_seeds(azmi_search* s, const uint64_t* seeds) {
  int rc = sb_begin_move(s, "set_rollout_seeds"); if (rc) return rc;
  azmi_pm* pm = s->pm;
  SB_TRY(hipSetDevice(pm->device));
  std::vector<uint64_t> roll(s->n);
  for (uint32_t i = 0; i < s->n; ++i) roll[i] = seeds ? seeds[i] : mix64(s->tree_seeds[i] ^ kRollSalt);
  SB_TRY(hipStreamSynchronize(pm->last));      // a search that is still running reads the old ones
  SB_TRY(hipMemcpy(s->ro.seeds, roll.data(), static_cast<size_t>(s->n) * 8, hipMemcpyHostToDevice));
  return AZMI_OK;
}

int azmi_search_pick_moves(azmi_search* s, float temp, int32_t* host_moves, void* stream) {
  int rc = sb_begin_move(s, "pick_moves"); if (rc) return rc;
  azmi_pm* pm = s->pm;
  SB_TRY(hipSetDevice(pm->device));
  hipStream_t st = pm->pick(stream);
  sb_launch_pick(s, temp, st);
  SB_TRY(hipGetLastError());
  if (!host_moves) return AZMI_OK;
  SB_TRY(hipMemcpyAsync(host_moves, s->pl.move, static_cast<size_t>(s->n) * 4, hipMemcpyDeviceToHost, st));
  return sb_check_device(s, st);
}

int azmi_search_update_roots(azmi_search* s, const int32_t* host_moves, void* stream) {
  int rc = sb_begin_move(s, "update_roots"); if (rc) return rc;
  azmi_pm* pm = s->pm;
  SB_TRY(hipSetDevice(pm->device));
  hipStream_t st = pm->pick(stream);
  bool all = true;
  if (host_moves) {
    for (uint32_t i = 0; i < s->n; ++i) {
      if (host_moves[i] >= static_cast<int32_t>(pm->gi.M)) return SB_FAIL(AZMI_ERR_INVALID, "tree %u: move %d out of range", i, host_moves[i]);
      all = all && host_moves[i] >= 0;
    }
    SB_TRY(hipMemcpyAsync(s->d_moves_in, host_moves, static_cast<size_t>(s->n) * 4, hipMemcpyHostToDevice, st));
  }
  sb_launch_update_root(s, host_moves ? s->d_moves_in : s->pl.move, st);
  SB_TRY(hipGetLastError());
  // a caller's moves may be unknown to a root: that is reported here, with the tree's index (the picked ones are children of their roots)
  rc = host_moves ? sb_check_device(s, st) : AZMI_OK;
  // every live tree moved, none refused its move: compaction has made room for the next search
  if (!s->flat_arena && all && rc == AZMI_OK) s->sims_done = 0;
  return rc;
}

int azmi_search_root_prior(azmi_search* s, int apply_temp, int add_noise, void* stream) {
  int rc = sb_begin_move(s, "root_prior"); if (rc) return rc;
  if (!apply_temp && !add_noise) return AZMI_OK;
  azmi_pm* pm = s->pm;
  SB_TRY(hipSetDevice(pm->device));
  hipStream_t st = pm->pick(stream);
  sb_launch_root_prior(s, apply_temp ? 1u : 0u, add_noise ? 1u : 0u, st);
  SB_TRY(hipGetLastError());
  return AZMI_OK;
}

int azmi_search_play(azmi_search* s, azmi_net* net, azmi_cache* cache, uint32_t visits, float temp, uint32_t max_moves, int root_noise,
                     void* stream) {
  return azmi_search_play_eval(s, net ? AZMI_EVAL_NN : AZMI_EVAL_RANDOM, net, cache, visits, temp, max_moves, root_noise, stream);
}

int azmi_search_play_eval(azmi_search* s, int eval_type, azmi_net* net, azmi_cache* cache, uint32_t visits, float temp, uint32_t max_moves,
                          int root_noise, void* stream) {
  int rc = sb_begin_move(s, "play"); if (rc) return rc;
  // the whole call's budget before anything is enqueued: Connect4 counts every move's search; a wide game's first search comes on
  // top of the descents since the last update_roots, and every later one starts behind a compaction
  rc = sb_check_budget(s, "play", s->flat_arena ? static_cast<uint64_t>(visits) * max_moves : (max_moves ? visits : 0u)); if (rc) return rc;
  SbSearchArgs a;
  rc = sb_search_args(s, "play", eval_type, net, cache, &a); if (rc) return rc;
  azmi_pm* pm = s->pm;
  SB_TRY(hipSetDevice(pm->device));
  hipStream_t st = pm->pick(stream);
  const uint32_t rn = root_noise ? 1u : 0u, rt = s->root_temp != 1.0f ? 1u : 0u;
  for (uint32_t m = 0; m < max_moves; ++m) {
    if (s->capture) sb_launch_capture(s, st);
    rc = sb_enqueue_search(s, a, visits, rn, st); if (rc) return rc;
    sb_launch_pick(s, temp, st);
    sb_launch_update_root(s, s->pl.move, st);
    if (!s->flat_arena) s->sims_done = 0;
    if (rn || rt) sb_launch_root_prior(s, rt, rn, st);
  }
  SB_TRY(hipGetLastError());
  return AZMI_OK;
}

int azmi_search_game_state(azmi_search* s, int32_t* status, uint32_t* log_len, int32_t* log, float* final_scores) {
  int rc = sb_begin_read(s, "game_state"); if (rc) return rc;      // a read-out: legal while a find_leaves step is pending
  azmi_pm* pm = s->pm;
  SB_TRY(hipSetDevice(pm->device));
  hipStream_t st = pm->last;
  const size_t N = s->n;
  rc = sb_check_device(s, st); if (rc) return rc;      // (synchronises)
  if (status) SB_TRY(hipMemcpy(status, s->sb.status, N * 4, hipMemcpyDeviceToHost));
  if (log_len) SB_TRY(hipMemcpy(log_len, s->pl.log_len, N * 4, hipMemcpyDeviceToHost));
  if (log) SB_TRY(hipMemcpy(log, s->pl.log, N * s->pl.log_cap * 4, hipMemcpyDeviceToHost));
  if (final_scores) SB_TRY(hipMemcpy(final_scores, s->pl.final, N * (pm->gi.P + 1) * 4, hipMemcpyDeviceToHost));
  return AZMI_OK;
}

int azmi_search_query(azmi_search* s, uint32_t kind, float temp, uint32_t arg, float* out_f, uint32_t* out_u) {
  int rc = sb_begin_step(s, "query"); if (rc) return rc;
  if (!(kind <= kQGumbelFinal || kind == kQPrincipalVariation || kind == kQSetGumbelSims))
    return SB_FAIL(AZMI_ERR_INVALID, "query kind %u is not available on a batched search", kind);
  if (kind == kQPrincipalVariation && arg > 60) arg = 60;
  azmi_pm* pm = s->pm;
  SB_TRY(hipSetDevice(pm->device));
  hipStream_t st = pm->last;
  sb_launch_query(s, kind, temp, arg, st);
  SB_TRY(hipGetLastError());
  if (out_f) SB_TRY(hipMemcpyAsync(out_f, s->d_qf, static_cast<size_t>(s->n) * s->vec_f * 4, hipMemcpyDeviceToHost, st));
  if (out_u) SB_TRY(hipMemcpyAsync(out_u, s->d_qu, static_cast<size_t>(s->n) * s->vec_u * 4, hipMemcpyDeviceToHost, st));
  return sb_check_device(s, st);
}

int azmi_search_sync(azmi_search* s) {
  if (!s) return SB_FAIL(AZMI_ERR_INVALID, "null argument");
  SB_TRY(hipSetDevice(s->pm->device));
  return sb_check_device(s, s->pm->last);
}

int azmi_search_stats(azmi_search* s, uint64_t out[6]) {
  if (!s || !out) return SB_FAIL(AZMI_ERR_INVALID, "null argument");
  azmi_pm* pm = s->pm;
  SB_TRY(hipSetDevice(pm->device));
  std::vector<uint64_t> sims(s->n), evals(s->n);
  std::vector<uint32_t> term(s->n);
  SB_TRY(hipStreamSynchronize(pm->last));
  SB_TRY(hipMemcpy(sims.data(), pm->ar.c_sims, static_cast<size_t>(s->n) * 8, hipMemcpyDeviceToHost));
  SB_TRY(hipMemcpy(evals.data(), pm->ar.c_evals, static_cast<size_t>(s->n) * 8, hipMemcpyDeviceToHost));
  SB_TRY(hipMemcpy(term.data(), s->sb.n_term, static_cast<size_t>(s->n) * 4, hipMemcpyDeviceToHost));
  uint64_t a = 0, b = 0, t = 0;
  for (uint32_t i = 0; i < s->n; ++i) { a += sims[i]; b += evals[i]; t += term[i]; }
  out[0] = s->launches; out[1] = s->net_calls; out[2] = s->steps; out[3] = a; out[4] = b; out[5] = t;
  return AZMI_OK;
}

}  // extern "C"

// ---- EvalType::PLAYOUT: rollouts on the device; see search_batch_kernels.h for the three step shapes ----------------------------
void sb_launch_step_playout(azmi_search* s, const EngineParams& ep, const EngineArrays& ar, uint32_t root_noise, hipStream_t st) {
  const uint32_t n = s->n;
  sb_for_game(s->pm->game,
              [&](auto tag) {
                using GM = decltype(tag);
                k_sb_find_po<GM><<<small_blocks(n), kSmallThreads, 0, st>>>(ep, ar, s->sb, s->ro, n);
                k_sb_rollout<GM><<<(n + 63) / 64, 64, 0, st>>>(ar, s->sb, s->ro, n);
                s->launches += 2;
              },
              [&](auto tag) { using GM = decltype(tag); k_sb_big_find_po<GM><<<n, 64, 0, st>>>(ep, ar, s->sb, s->ro, n); s->launches += 1; });
  sb_launch_process(s, ep, ar, root_noise, nullptr, nullptr, st);
}

void sb_launch_step_playout_wu(azmi_search* s, const EngineParams& ep, const EngineArrays& ar, uint32_t kk, uint32_t root_noise, hipStream_t st) {
  SB_LAUNCH(s, st, k_sb_find_wu_po, k_sb_big_find_wu_po, ep, ar, s->sb, s->wu, s->ro, s->n, kk, root_noise);
}

// ---- search to per-tree root_n targets, snapshots at checkpoints (mcts_analysis.py:884-972, 975-1063) ---------------------------
void sb_launch_checkpoint(azmi_search* s, float temp, uint32_t pruned, uint32_t resume, hipStream_t st) {
  SB_LAUNCH(s, st, k_sb_checkpoint, k_sb_big_checkpoint, s->pm->ep, s->pm->ar, s->sb, s->sw, s->n, temp, pruned, resume);
}

// ---- descents_per_step > 1: the kernels of search_batch_kernels.h's last section, instantiated behind everything else -------------
void sb_launch_todo_set(azmi_search* s, uint32_t visits, hipStream_t st) {
  k_sb_todo_set<<<(s->n + 255) / 256, 256, 0, st>>>(s->sb, s->dl, s->n, visits);
  s->launches += 1;
}

void sb_launch_find_dl(azmi_search* s, const EngineParams& ep, const EngineArrays& ar, uint32_t parity, uint32_t eval_random, uint32_t root_noise,
                    hipStream_t st) {
  SB_LAUNCH(s, st, k_sb_find_dl, k_sb_big_find_dl, ep, ar, s->sb, s->dl, s->n, s->dl_L, parity, eval_random, root_noise);
  if (eval_random) return;      // no row is ever pending: nothing to number
  k_sb_compact<<<1, 1024, 0, st>>>(s->sb, s->n);
  s->launches += 1;
}

void sb_launch_find_dl_playout(azmi_search* s, const EngineParams& ep, const EngineArrays& ar, uint32_t parity, hipStream_t st) {
  const uint32_t n = s->n;
  SB_LAUNCH(s, st, k_sb_find_dl_po, k_sb_big_find_dl_po, ep, ar, s->sb, s->dl, s->ro, n, s->dl_L, parity);
  sb_for_game(s->pm->game,
              [&](auto tag) { using GM = decltype(tag); k_sb_rollout<GM><<<(n + 63) / 64, 64, 0, st>>>(ar, s->sb, s->ro, n); s->launches += 1; },
              [&](auto) {});
}

// ---- frozen-set capture, first-occurrence dedup, net versus search: the kernels of search_pool_kernels.h, behind everything else ---
void sb_launch_capture(azmi_search* s, hipStream_t st) {
  SB_LAUNCH(s, st, k_sb_capture, k_sb_big_capture, s->pm->ep, s->pm->ar, s->sb, s->pl, s->cp, s->n);
}

void sb_launch_root_canon(azmi_search* s, hipStream_t st) {
  azmi_pm* pm = s->pm;
  SB_LAUNCH(s, st, k_sb_root_canon, k_sb_big_root_canon, pm->ep, pm->ar, s->sb, s->n, s->d_batch, s->d_nm_valid);
}

void sb_launch_net_metrics(azmi_search* s, hipStream_t st) {
  azmi_pm* pm = s->pm;
  SB_LAUNCH(s, st, k_sb_net_metrics, k_sb_big_net_metrics, pm->ep, pm->ar, s->n, s->d_nm_valid, s->d_vrows, s->d_pirows, s->d_nm_out, s->d_qf,
            s->vec_f, s->d_qu, s->vec_u);
}

void sb_launch_pool_claim(const uint64_t* d_keys, const uint8_t* d_valid, uint32_t n, uint32_t mask, uint32_t* d_owner, uint32_t* d_first,
                          uint32_t* d_slot_of, hipStream_t st) {
  k_pool_claim<<<(n + 255u) / 256u, 256, 0, st>>>(d_keys, d_valid, n, mask, d_owner, d_first, d_slot_of);
}

void sb_launch_pool_compact(const uint8_t* d_valid, uint32_t n, const uint32_t* d_first, const uint32_t* d_slot_of, uint32_t* d_out, uint32_t* d_counts,
                            hipStream_t st) {
  k_pool_compact<<<1, 1024, 0, st>>>(d_valid, n, d_first, d_slot_of, d_out, d_counts);
}

// ---- opening-tree frontier: the kernels of search_frontier_kernels.h, behind everything else -------------------------------------
void sb_launch_frontier_policy(azmi_search* s, double min_reach, hipStream_t st) {
  azmi_pm* pm = s->pm;
  SB_LAUNCH(s, st, k_sb_frontier_policy, k_sb_big_frontier_policy, pm->ep, pm->ar, s->sb, s->fr, s->n, min_reach, s->d_qf, s->vec_f, s->d_qu, s->vec_u);
}

void sb_launch_frontier_scan(azmi_search* s, hipStream_t st) {
  k_frontier_scan<1024><<<1, 1024, 0, st>>>(s->fr.kept, s->n, s->fr.first_child, s->fr.total);
  s->launches += 1;
}

void sb_launch_frontier_emit(azmi_search* s, hipStream_t st) {
  azmi_pm* pm = s->pm;
  SB_LAUNCH(s, st, k_sb_frontier_emit, k_sb_big_frontier_emit, pm->ep, pm->ar, s->fr, s->n);
}

// ---- sweep metrics: the kernels of search_sweep_metrics_kernels.h, behind everything else ------------------------------------------
void sb_launch_sweep_metrics(azmi_search* s, const azmi_search* ref, uint32_t anchor, int32_t raw, const double* d_outcomes, const SweepMetricsOut& o,
                             hipStream_t st) {
  SB_LAUNCH(s, st, k_sb_sweep_metrics, k_sb_big_sweep_metrics, s->sw, ref->sw, s->n, anchor, raw, d_outcomes, o.rows, o.ceiling, o.valid);
}

void sb_launch_sweep_mean(azmi_search* s, uint32_t J, const SweepMetricsOut& o, hipStream_t st) {
  k_sb_sweep_mean<<<std::max(J, 1u), kSweepMeanThreads, 0, st>>>(o.rows, s->n, J, o.mean, o.count);
  s->launches += 1;
}

void sb_launch_policy_divergences(const float* d_p, const float* d_q, uint32_t rows, uint32_t M, double* d_out, hipStream_t st) {
  if (M <= 8) k_policy_divergences<8><<<(rows + 31u) / 32u, 256, 0, st>>>(d_p, d_q, rows, M, d_out);
  else k_policy_divergences<64><<<(rows + 3u) / 4u, 256, 0, st>>>(d_p, d_q, rows, M, d_out);
}
