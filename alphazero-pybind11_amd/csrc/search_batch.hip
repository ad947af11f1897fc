// Batched position search (azmi_search_*, include/azmi.h): the ONE device module of the four search_*_kernels.h, and nothing else.
// A kernel header defines non-template kernels, and the code of a kernel depends on the kernels it shares a module with and on the
// order they are instantiated in (DESIGN.md sections 1 and 8.3).  So every launch lives here, one thin sb_launch_* function per
// kernel family (search_batch_host.h), in the order the families were added; a new family goes behind the last one.
// N search trees on N different positions sit in ONE engine arena, all of them advanced by one simulation per (find-leaves,
// process-results) launch pair; the K > 1 steps (*_wu), the PLAYOUT steps (*_po) and the descents_per_step > 1 steps (*_dl) have
// launch functions of their own.  The entry points are host code only, in search_batch_create.hip, search_batch_steps.hip and
// search_batch_moves.hip (the core) and in search_batch_sweep.hip, search_batch_pool.hip and search_batch_frontier.hip.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "cache_host.h"
#include "search_batch_host.h"
#include "search_batch_kernels.h"
#include "search_pool_kernels.h"
#include "search_frontier_kernels.h"
#include "search_sweep_metrics_kernels.h"
#include "search_leaf_keys_kernels.h"

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
void sb_launch_find_wu(azmi_search* s, const EngineParams& ep, const EngineArrays& ar, uint32_t kk, uint32_t eval_random, uint32_t root_noise, hipStream_t st) {
  SB_LAUNCH(s, st, k_sb_find_wu, k_sb_big_find_wu, ep, ar, s->sb, s->wu, s->n, kk, eval_random, root_noise);
  k_sb_compact_wu<<<1, 1024, 0, st>>>(s->sb, s->wu, s->n, kk);
  s->launches += 1;
}

void sb_launch_process_wu(azmi_search* s, const EngineParams& ep, const EngineArrays& ar, uint32_t kk, uint32_t root_noise, const float* v_rows,
                       const float* pi_rows, hipStream_t st) {
  SB_LAUNCH(s, st, k_sb_process_wu, k_sb_big_process_wu, ep, ar, s->wu, s->n, kk, root_noise, v_rows, pi_rows);
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

// ---- reset and the step API: the trees' positions from the uploaded start rows and game records; the step's rows into one batch ---
void sb_launch_seed(azmi_search* s, const uint8_t* d_init, uint32_t init_stride, const int32_t* d_moves, const uint32_t* d_offs, const uint64_t* d_seeds,
                    hipStream_t st) {
  SB_LAUNCH(s, st, k_sb_seed, k_sb_big_seed, s->pm->ep, s->pm->ar, s->sb, s->n, d_init, init_stride, d_moves, d_offs, d_seeds);
}

void sb_launch_gather(azmi_search* s, uint32_t kk, hipStream_t st) {
  if (s->k_leaves > 1) {
    SbArrays rows_of_step = s->sb;       // k_sb_gather over the step's kk * N entries
    rows_of_step.row_of = s->wu.row_of;
    k_sb_gather<<<s->n * kk, 256, 0, st>>>(rows_of_step, s->n * kk, s->wu.canon, s->chw, s->d_batch_wu);
  } else {
    k_sb_gather<<<s->n, 256, 0, st>>>(s->sb, s->n, s->pm->ar.canon, s->chw, s->d_batch);
  }
  s->launches += 1;
}

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

// ---- the step API's leaf keys: the kernel of search_leaf_keys_kernels.h, behind everything else ------------------------------------
void sb_launch_leaf_keys(azmi_search* s, hipStream_t st) {
  const uint32_t cap = s->n * s->k_leaves;
  if (s->k_leaves > 1) k_sb_leaf_keys<<<(cap + 255u) / 256u, 256, 0, st>>>(s->wu.keys, s->wu.rows, s->sb.n_rows, cap, s->d_leaf_keys);
  else k_sb_leaf_keys<<<(cap + 255u) / 256u, 256, 0, st>>>(s->pm->ar.leaf_key, s->sb.rows, s->sb.n_rows, cap, s->d_leaf_keys);
  s->launches += 1;
}
