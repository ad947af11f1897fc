// The stand-alone MCTS object (azmi_mcts_*, include/azmi.h; py_wrapper.cc:192-220): one search tree on a one-slot PlayManager
// engine, driven call by call from the host - find_leaf / process_result, their WU-UCT batched forms (mcts.cc:752-851),
// update_root and the read-out queries.  Host side of csrc/mcts_object_kernels.h; the kernels are part of engine.hip's device
// module and launched through azmi_host_launch_mcts_*.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "../../include/azmi.h"
#include "engine_host.h"
#include "mcts_object_kernels.h"

using namespace azmi;

extern "C" {

struct azmi_mcts {
  azmi_pm* pm = nullptr;
  uint8_t* d_init = nullptr; int32_t* d_moves = nullptr; int32_t* d_out_moves = nullptr;
  uint32_t* d_len = nullptr; int32_t* d_status = nullptr; float* d_f = nullptr; uint32_t* d_u = nullptr;
  uint32_t moves_cap = 0, vec = 0;
  uint32_t init_bytes = 0;               // size of the image in d_init (0 = the game's initial position)
  WuArrays wu{};                         // Node::n_in_flight + MCTS::in_flight_ (mcts.h:24,171)
  uint32_t ifl_count = 0, ifl_cap = 0;
};

namespace {
// capacity of the start-position buffer: Connect4's 89 bytes; a Tafl pickle image with up to 512 repetition entries
uint32_t mcts_init_bytes(int game) {
  if (game == AZMI_GAME_STARGAMBIT) return 25u + 4u + 9u * 20u + 20u + 8u * (StarGambit::MAX_TURNS + 2);
  return game == AZMI_GAME_CONNECT4 ? Connect4::SERIALIZED : game == AZMI_GAME_BRANDUBH ? TaflImage<Brandubh>::bytes(512) : TaflImage<OpenTafl>::bytes(512);
}
}  // namespace

// the PlayParams of the engine behind MCTS(...) ctor arguments: `sims` simulations of arena per tree, every seat on model group 0
// (shared with the batched search, search_batch.hip)
int azmi_host_mcts_params(int game, const azmi_mcts_config* cfg, uint32_t sims, azmi_play_params* out_p) {
  if (!cfg || !out_p) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  GameInfo gi;
  if (!azmi_host_game_info(game, &gi)) return azmi_host_fail(AZMI_ERR_INVALID, "unknown game id %d", game);
  if (cfg->num_players != gi.P || cfg->num_moves != gi.M) return azmi_host_fail(AZMI_ERR_INVALID, "MCTS(num_players, num_moves) do not match the game");
  // MCTS(..., relative_values, ...) (mcts.h:54): on the device the rotation is part of the game's instantiation
  if ((cfg->relative_values != 0) != (game == AZMI_GAME_STARGAMBIT))
    return azmi_host_fail(AZMI_ERR_INVALID, "relative_values must be the game's relative_values() (true for StarGambit only)");
  azmi_play_params& p = *out_p;
  azmi_play_params_default(&p);
  p.games_to_play = 1; p.concurrent_games = 1; p.max_batch_size = 1;
  p.num_mcts_visits = gi.P;
  // Connect4: arena = (21 * visits + 42) * 7 nodes >= sims * 7.  Wide games: two halves of 4 x (visits + 16) x 240 nodes,
  // compacted after update_root when the active half fills up
  for (uint32_t i = 0; i < gi.P; ++i) p.mcts_visits[i] = game == AZMI_GAME_CONNECT4 ? (sims + 20) / 21 : std::min<uint32_t>(sims, 8000u);
  p.cpuct = cfg->cpuct; p.epsilon = cfg->epsilon; p.mcts_root_temp = cfg->root_policy_temp; p.fpu_reduction = cfg->fpu_reduction;
  p.root_fpu_zero = cfg->root_fpu_zero; p.shaped_dirichlet = cfg->shaped_dirichlet;
  p.gumbel_enabled = cfg->gumbel_enabled; p.gumbel_m = cfg->gumbel_m; p.gumbel_c_visit = cfg->gumbel_c_visit;
  p.gumbel_c_scale = cfg->gumbel_c_scale; p.gumbel_full = cfg->gumbel_full;
  p.num_model_groups_given = gi.P;
  for (uint32_t i = 0; i < gi.P; ++i) p.model_groups[i] = 0;
  return AZMI_OK;
}
int azmi_mcts_create(int game, const azmi_mcts_config* cfg, uint64_t seed, int device, azmi_mcts** out) {
  if (!cfg || !out) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  GameInfo gi;
  if (!azmi_host_game_info(game, &gi)) return azmi_host_fail(AZMI_ERR_INVALID, "unknown game id %d", game);
  azmi_play_params p;
  int rc = azmi_host_mcts_params(game, cfg, cfg->max_simulations ? cfg->max_simulations : 50000u, &p);
  if (rc != AZMI_OK) return rc;
  azmi_engine_opts o;
  azmi_engine_opts_default(&o);
  o.seed = seed; o.device = device;
  auto m = new azmi_mcts();
  rc = azmi_pm_create(game, &p, &o, &m->pm);
  if (rc != AZMI_OK) { delete m; return rc; }
  // the slot's stream is the object's stream; seed it directly (not through slot_seed) so that `seed` means what
  // MCTS::seed_thread_rng(seed) means in the reference tests
  {
    Pcg32 g; g.seed(seed);
    const uint64_t st = g.state;
    if (hipMemcpy(m->pm->ar.rng, &st, 8, hipMemcpyHostToDevice) != hipSuccess) { azmi_pm_destroy(m->pm); delete m; return azmi_host_fail(AZMI_ERR_NO_DEVICE, "rng init failed"); }
  }
  m->moves_cap = gi.max_turns + 8;
  m->vec = std::max<uint32_t>(gi.M, 64u);
  auto A = [&](auto*& ptr, size_t n) { return m->pm->alloc(ptr, n, true); };
  rc = A(m->d_init, mcts_init_bytes(game)); if (rc == AZMI_OK) rc = A(m->d_moves, m->moves_cap); if (rc == AZMI_OK) rc = A(m->d_out_moves, m->moves_cap);
  if (rc == AZMI_OK) rc = A(m->d_len, 1); if (rc == AZMI_OK) rc = A(m->d_status, 1);
  if (rc == AZMI_OK) rc = A(m->d_f, m->vec); if (rc == AZMI_OK) rc = A(m->d_u, m->vec + 64);
  m->ifl_cap = 1024;
  if (rc == AZMI_OK) rc = A(m->wu.nif, static_cast<size_t>(gi.P) * m->pm->ep.cap);
  if (rc == AZMI_OK) rc = A(m->wu.ifl_path, static_cast<size_t>(m->ifl_cap) * m->pm->ep.max_depth);
  if (rc == AZMI_OK) rc = A(m->wu.ifl_plen, m->ifl_cap); if (rc == AZMI_OK) rc = A(m->wu.ifl_cur, m->ifl_cap);
  if (rc != AZMI_OK) { azmi_pm_destroy(m->pm); delete m; return rc; }
  *out = m;
  return AZMI_OK;
}

void azmi_mcts_destroy(azmi_mcts* m) {
  if (!m) return;
  azmi_pm_destroy(m->pm);
  delete m;
}

namespace {
int mcts_upload_state(azmi_mcts* m, const uint8_t* init, uint32_t init_bytes, const int32_t* moves, uint32_t len, hipStream_t st) {
  if (len > m->moves_cap) return azmi_host_fail(AZMI_ERR_INVALID, "game record too long");
  if (init) {
    uint32_t extra = 0;
    const int rc = azmi_host_check_init_rows(m->pm->game, init, init_bytes, 1, &extra);
    if (rc != AZMI_OK) return rc;
    if (init_bytes > mcts_init_bytes(m->pm->game)) return azmi_host_fail(AZMI_ERR_INVALID, "start position: image too large (%u bytes)", init_bytes);
  }
  m->init_bytes = init ? init_bytes : 0;
  if (init) AZMI_HIP_TRY(hipMemcpyAsync(m->d_init, init, init_bytes, hipMemcpyHostToDevice, st));
  if (len) AZMI_HIP_TRY(hipMemcpyAsync(m->d_moves, moves, static_cast<size_t>(len) * 4, hipMemcpyHostToDevice, st));
  return AZMI_OK;
}
int mcts_check(azmi_mcts* m, hipStream_t st) {
  Control c;
  return azmi_host_read_ctl(m->pm, st, &c, false);
}
}  // namespace

int azmi_mcts_find_leaf(azmi_mcts* m, const uint8_t* init, uint32_t init_bytes, const int32_t* moves, uint32_t len,
                        int32_t* leaf_moves, uint32_t cap, uint32_t* leaf_len) {
  if (!m || !leaf_len || (len && !moves)) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  AZMI_HIP_TRY(hipSetDevice(m->pm->device));
  hipStream_t st = m->pm->stream;
  int rc = mcts_upload_state(m, init, init_bytes, moves, len, st); if (rc) return rc;
  const uint8_t* di = init ? m->d_init : nullptr;
  azmi_host_launch_mcts_find_leaf(m->pm, st, m->wu.nif, di, init_bytes, m->d_moves, len, m->d_out_moves, m->d_len, m->d_status);
  int32_t status = 0; uint32_t n = 0;
  AZMI_HIP_TRY(hipMemcpyAsync(&status, m->d_status, 4, hipMemcpyDeviceToHost, st));
  AZMI_HIP_TRY(hipMemcpyAsync(&n, m->d_len, 4, hipMemcpyDeviceToHost, st));
  AZMI_HIP_TRY(hipStreamSynchronize(st));
  if (status == -1) return azmi_host_fail(AZMI_ERR_INVALID, "illegal move in the game record");
  rc = mcts_check(m, st); if (rc) return rc;
  if (status != 0) return azmi_host_fail(AZMI_ERR_OVERFLOW, "find_leaf failed (tree arena or path capacity)");
  if (n > cap) return azmi_host_fail(AZMI_ERR_INVALID, "leaf_moves too small");
  if (n && leaf_moves) AZMI_HIP_TRY(hipMemcpy(leaf_moves, m->d_out_moves, static_cast<size_t>(n) * 4, hipMemcpyDeviceToHost));
  *leaf_len = n;
  return AZMI_OK;
}

int azmi_mcts_process_result(azmi_mcts* m, const float* value, const float* pi, int root_noise_enabled, float* value_out) {
  if (!m || !value || !pi) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  AZMI_HIP_TRY(hipSetDevice(m->pm->device));
  hipStream_t st = m->pm->stream;
  const uint32_t V = m->pm->gi.P + 1, M = m->pm->gi.M;
  AZMI_HIP_TRY(hipMemcpyAsync(m->pm->ar.v, value, V * 4, hipMemcpyHostToDevice, st));
  AZMI_HIP_TRY(hipMemcpyAsync(m->pm->ar.pi, pi, M * 4, hipMemcpyHostToDevice, st));
  const uint32_t rn = root_noise_enabled ? 1u : 0u;
  azmi_host_launch_mcts_process_result(m->pm, st, rn, m->d_f);
  float tmp[8];
  AZMI_HIP_TRY(hipMemcpyAsync(tmp, m->d_f, V * 4, hipMemcpyDeviceToHost, st));
  AZMI_HIP_TRY(hipStreamSynchronize(st));
  if (value_out) std::memcpy(value_out, tmp, V * 4);
  return mcts_check(m, st);
}

// ---- WU-UCT batched API, mcts.cc:752-851 -----------------------------------------------------------------------
int azmi_mcts_find_leaf_batched(azmi_mcts* m, const uint8_t* init, uint32_t init_bytes, const int32_t* moves, uint32_t len,
                                int32_t* leaf_moves, uint32_t cap, uint32_t* leaf_len) {
  if (!m || !leaf_len || (len && !moves)) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  if (m->ifl_count >= m->ifl_cap) return azmi_host_fail(AZMI_ERR_OVERFLOW, "%u leaves in flight: call reset_batch", m->ifl_count);
  AZMI_HIP_TRY(hipSetDevice(m->pm->device));
  hipStream_t st = m->pm->stream;
  int rc = mcts_upload_state(m, init, init_bytes, moves, len, st); if (rc) return rc;
  const uint8_t* di = init ? m->d_init : nullptr;
  const uint32_t idx = m->ifl_count;
  azmi_host_launch_mcts_find_leaf_batched(m->pm, st, m->wu, idx, di, init_bytes, m->d_moves, len, m->d_out_moves, m->d_len, m->d_status);
  int32_t status = 0; uint32_t n = 0;
  AZMI_HIP_TRY(hipMemcpyAsync(&status, m->d_status, 4, hipMemcpyDeviceToHost, st));
  AZMI_HIP_TRY(hipMemcpyAsync(&n, m->d_len, 4, hipMemcpyDeviceToHost, st));
  AZMI_HIP_TRY(hipStreamSynchronize(st));
  if (status == -1) return azmi_host_fail(AZMI_ERR_INVALID, "illegal move in the game record");
  rc = mcts_check(m, st); if (rc) return rc;
  if (status != 0) return azmi_host_fail(AZMI_ERR_OVERFLOW, "find_leaf_batched failed (tree arena or path capacity)");
  if (n > cap) return azmi_host_fail(AZMI_ERR_INVALID, "leaf_moves too small");
  if (n && leaf_moves) AZMI_HIP_TRY(hipMemcpy(leaf_moves, m->d_out_moves, static_cast<size_t>(n) * 4, hipMemcpyDeviceToHost));
  *leaf_len = n;
  ++m->ifl_count;
  return AZMI_OK;
}

int azmi_mcts_process_result_batched(azmi_mcts* m, uint32_t leaf_index, const float* value, const float* pi, int root_noise_enabled,
                                     float* value_out) {
  if (!m || !value || !pi) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  if (leaf_index >= m->ifl_count) return azmi_host_fail(AZMI_ERR_RANGE, "leaf_index %u out of range (%u in flight)", leaf_index, m->ifl_count);
  AZMI_HIP_TRY(hipSetDevice(m->pm->device));
  hipStream_t st = m->pm->stream;
  const uint32_t V = m->pm->gi.P + 1, M = m->pm->gi.M;
  AZMI_HIP_TRY(hipMemcpyAsync(m->pm->ar.v, value, V * 4, hipMemcpyHostToDevice, st));
  AZMI_HIP_TRY(hipMemcpyAsync(m->pm->ar.pi, pi, M * 4, hipMemcpyHostToDevice, st));
  const uint32_t rn = root_noise_enabled ? 1u : 0u;
  azmi_host_launch_mcts_process_result_batched(m->pm, st, m->wu, leaf_index, rn, m->d_f);
  float tmp[8];
  AZMI_HIP_TRY(hipMemcpyAsync(tmp, m->d_f, V * 4, hipMemcpyDeviceToHost, st));
  AZMI_HIP_TRY(hipStreamSynchronize(st));
  if (value_out) std::memcpy(value_out, tmp, V * 4);
  return mcts_check(m, st);
}

int azmi_mcts_in_flight_count(const azmi_mcts* m, uint32_t* out) {
  if (!m || !out) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  *out = m->ifl_count;
  return AZMI_OK;
}

int azmi_mcts_reset_batch(azmi_mcts* m) {
  if (!m) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  m->ifl_count = 0;
  return AZMI_OK;
}

int azmi_mcts_update_root(azmi_mcts* m, const uint8_t* init, uint32_t init_bytes, const int32_t* moves, uint32_t len, uint32_t move) {
  if (!m || (len && !moves)) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  AZMI_HIP_TRY(hipSetDevice(m->pm->device));
  hipStream_t st = m->pm->stream;
  int rc = mcts_upload_state(m, init, init_bytes, moves, len, st); if (rc) return rc;
  const uint8_t* di = init ? m->d_init : nullptr;
  azmi_host_launch_mcts_update_root(m->pm, st, m->wu.nif, di, init_bytes, m->d_moves, len, move, m->d_status);
  int32_t status = 0;
  AZMI_HIP_TRY(hipMemcpyAsync(&status, m->d_status, 4, hipMemcpyDeviceToHost, st));
  AZMI_HIP_TRY(hipStreamSynchronize(st));
  if (status == -1) return azmi_host_fail(AZMI_ERR_INVALID, "illegal move in the game record");
  if (status == -3) {   // the device raised its "unknown move" bit; clear it so the object stays usable
    Control c; AZMI_HIP_TRY(hipMemcpy(&c, m->pm->ar.ctl, sizeof(c), hipMemcpyDeviceToHost));
    c.overflow &= ~32u; if (!c.overflow) c.stop = 0;
    AZMI_HIP_TRY(hipMemcpy(m->pm->ar.ctl, &c, sizeof(c), hipMemcpyHostToDevice));
    return azmi_host_fail(AZMI_ERR_INVALID, "ahh, what is this move: %u", move);
  }
  return mcts_check(m, st);
}

int azmi_mcts_query(azmi_mcts* m, uint32_t kind, float temp, uint32_t arg, const float* in_f, float* out_f, uint32_t* out_u) {
  if (!m) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  AZMI_HIP_TRY(hipSetDevice(m->pm->device));
  hipStream_t st = m->pm->stream;
  if (kind == kQPickMove) {
    if (!in_f) return azmi_host_fail(AZMI_ERR_INVALID, "pick_move needs a probability vector");
    AZMI_HIP_TRY(hipMemcpyAsync(m->d_f, in_f, static_cast<size_t>(m->pm->gi.M) * 4, hipMemcpyHostToDevice, st));
  }
  if (kind == kQPrincipalVariation && arg > 60) arg = 60;
  azmi_host_launch_mcts_query(m->pm, st, kind, temp, arg, m->d_f, m->d_u);
  if (out_f) AZMI_HIP_TRY(hipMemcpyAsync(out_f, m->d_f, static_cast<size_t>(m->vec) * 4, hipMemcpyDeviceToHost, st));
  if (out_u) AZMI_HIP_TRY(hipMemcpyAsync(out_u, m->d_u, static_cast<size_t>(m->vec) * 4, hipMemcpyDeviceToHost, st));
  AZMI_HIP_TRY(hipStreamSynchronize(st));
  return mcts_check(m, st);
}

}  // extern "C"

