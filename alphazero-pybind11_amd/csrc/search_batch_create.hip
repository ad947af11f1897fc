// Batched position search, life cycle: azmi_search_create / destroy, the knobs set before a search (leaves_per_step with its
// allocation, descents_per_step, host_reads), azmi_search_reset and set_rollout_seeds.  Host code only (search_batch_host.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>
#include <vector>

#include "dev_games.h"
#include "search_batch_host.h"

using namespace azmi;

static void wu_free(azmi_search* s) {
  for (void* q : s->wu_allocs) (void)hipFree(q);
  s->wu_allocs.clear();
  s->wu = SbWuArrays{};
  s->d_batch_wu = nullptr; s->d_vrows_wu = nullptr; s->d_pirows_wu = nullptr;
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
  if (s->leaf_keys_block.p) (void)hipFree(s->leaf_keys_block.p);
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
    sb_launch_seed(s, d_init, init_stride, d_moves, d_offs, d_seeds, st);
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

}  // extern "C"
