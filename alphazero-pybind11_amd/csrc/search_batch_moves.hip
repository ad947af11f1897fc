// Batched position search, moves and read-outs: azmi_search_pick_moves / update_roots / root_prior / play* advance every tree's root
// on the device (tree reuse, no host between moves); game_state / query / sync / stats read back.  Host code only (search_batch_host.h).
#include <hip/hip_runtime.h>

#include <vector>

#include "search_batch_host.h"

using namespace azmi;

extern "C" {

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
