// Rules replay, playout evaluation, StarGambit state images and the RNG probe: the entry points of include/azmi.h that run the
// device rules and RNG on their own, with no engine behind them (parity tiers T0 / RNG, playout_eval, pickling of the Python
// game objects).  Every call stages its rows in temporary device buffers, runs one kernel on the null stream and copies back.
// Host side of csrc/replay_kernels.h; the kernels are part of engine.hip's device module and launched through azmi_host_launch_*.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "../../include/azmi.h"
#include "dev_games.h"
#include "engine_host.h"

using namespace azmi;

namespace {
int require_device(int device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return azmi_host_fail(AZMI_ERR_NO_DEVICE, "no HIP device: libazmi has no CPU path");
  AZMI_HIP_TRY(hipSetDevice(device));
  return AZMI_OK;
}

// start-position rows: Connect4 = the 89-byte to_bytes image; Tafl family = the reference pickle image (dev_games.h TaflImage),
// rows zero-padded to a common stride.  *extra_reps = the most repetition keys any row brings along.
int check_init_rows(int game, const uint8_t* init, uint32_t init_stride, uint32_t n, uint32_t* extra_reps) {
  *extra_reps = 0;
  if (!init) return AZMI_OK;
  if (game == AZMI_GAME_CONNECT4) {
    if (init_stride != Connect4::SERIALIZED) return azmi_host_fail(AZMI_ERR_INVALID, "start positions: Connect4 images are %u bytes", Connect4::SERIALIZED);
    return AZMI_OK;
  }
  if (game == AZMI_GAME_STARGAMBIT) {   // rows hold one StarGambitUnifiedGS::to_bytes image each, zero-padded; the history rides along
    if (init_stride < 25u + 24u) return azmi_host_fail(AZMI_ERR_INVALID, "start positions: a StarGambit image is at least 49 bytes, got %u", init_stride);
    for (uint32_t g = 0; g < n; ++g) {
      const uint8_t* row = init + static_cast<size_t>(g) * init_stride;
      const uint32_t inner = uint32_t(row[21]) | uint32_t(row[22]) << 8 | uint32_t(row[23]) << 16 | uint32_t(row[24]) << 24;
      if (25ull + inner > init_stride) return azmi_host_fail(AZMI_ERR_INVALID, "start position %u: image longer than the row", g);
      const uint32_t nu = uint32_t(row[25]) | uint32_t(row[26]) << 8 | uint32_t(row[27]) << 16 | uint32_t(row[28]) << 24;
      if (nu > 20u || 9ull * nu + 24ull > inner) return azmi_host_fail(AZMI_ERR_INVALID, "start position %u: malformed image", g);
      const uint8_t* hl = row + 25 + 9 * nu + 20;
      *extra_reps = std::max(*extra_reps, uint32_t(hl[0]) | uint32_t(hl[1]) << 8 | uint32_t(hl[2]) << 16 | uint32_t(hl[3]) << 24);
    }
    return AZMI_OK;
  }
  const uint32_t sq = game == AZMI_GAME_BRANDUBH ? Brandubh::SQ : 121u, bb = 3u * sq, header = bb + 6u, entry = bb + 2u;
  if (init_stride < header + 4u) return azmi_host_fail(AZMI_ERR_INVALID, "start positions: a Tafl image is at least %u bytes, got %u", header + 4u, init_stride);
  for (uint32_t g = 0; g < n; ++g) {
    const uint8_t* row = init + static_cast<size_t>(g) * init_stride;
    const uint8_t* h = row + header;
    const uint32_t cnt = uint32_t(h[0]) | uint32_t(h[1]) << 8 | uint32_t(h[2]) << 16 | uint32_t(h[3]) << 24;
    if (cnt > 4096u || header + 4u + static_cast<uint64_t>(cnt) * entry > init_stride)
      return azmi_host_fail(AZMI_ERR_INVALID, "start position %u: repetition entry count mismatch", g);
    uint32_t keys = 0;
    for (uint32_t i = 0; i < cnt; ++i) keys += row[header + 4u + static_cast<size_t>(i) * entry + bb + 1u];
    *extra_reps = std::max(*extra_reps, keys);
  }
  return AZMI_OK;
}
}  // namespace

extern "C" {


int azmi_rng_probe(int device, int kind, uint64_t seed, float param, uint32_t n, uint32_t reps, void* out) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return azmi_host_fail(AZMI_ERR_NO_DEVICE, "no HIP device: libazmi has no CPU path");
  if (kind < 0 || kind > 4 || !out) return azmi_host_fail(AZMI_ERR_INVALID, "bad rng probe arguments");
  AZMI_HIP_TRY(hipSetDevice(device));
  const size_t count = static_cast<size_t>(n) * (kind == 1 ? std::max(reps, 1u) : 1u);
  void* d = nullptr;
  AZMI_HIP_TRY(hipMalloc(&d, std::max<size_t>(count, 1) * 4));
  azmi_host_launch_rng_probe(kind, seed, param, n, std::max(reps, 1u), static_cast<uint32_t*>(d), static_cast<float*>(d));
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, d, count * 4, hipMemcpyDeviceToHost);
  (void)hipFree(d);
  if (e != hipSuccess) return azmi_host_fail(AZMI_ERR_NO_DEVICE, "rng probe: %s", hipGetErrorString(e));
  return AZMI_OK;
}

int azmi_host_check_init_rows(int game, const uint8_t* init, uint32_t init_stride, uint32_t n, uint32_t* extra_reps) {
  return check_init_rows(game, init, init_stride, n, extra_reps);
}

int azmi_game_replay(int game, int device, const int32_t* moves, uint32_t n, uint32_t len, uint8_t* valid,
                     float* scores, float* canonical, uint32_t* player, uint32_t* turn, uint64_t* key,
                     int32_t* status) {
  return azmi_game_replay_from(game, device, nullptr, 0, moves, n, len, valid, scores, canonical, player, turn, key, status);
}

int azmi_game_replay_from(int game, int device, const uint8_t* init, uint32_t init_stride, const int32_t* moves,
                          uint32_t n, uint32_t len, uint8_t* valid, float* scores, float* canonical,
                          uint32_t* player, uint32_t* turn, uint64_t* key, int32_t* status) {
  return azmi_game_replay_ex(game, device, init, init_stride, moves, n, len, valid, scores, canonical, player, turn, key, status, 0u);
}

int azmi_playout_eval(int game, int device, const uint8_t* init, uint32_t init_stride, const int32_t* moves, uint32_t n, uint32_t len,
                      const uint64_t* seeds, float* v, float* pi) {
  GameInfo gi;
  if (!azmi_host_game_info(game, &gi)) return azmi_host_fail(AZMI_ERR_INVALID, "unknown game id %d", game);
  if (!seeds || !v || !pi || (!moves && n * len)) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  uint32_t extra_reps = 0;
  { const int rc_init = check_init_rows(game, init, init_stride, n, &extra_reps); if (rc_init != AZMI_OK) return rc_init; }
  if (n == 0) return AZMI_OK;
  { const int rc_dev = require_device(device); if (rc_dev != AZMI_OK) return rc_dev; }
  DevTemps tmp;
  int32_t* d_moves = nullptr; uint8_t* d_init = nullptr; uint64_t* d_seeds = nullptr; float *d_v = nullptr, *d_pi = nullptr; int32_t* d_status = nullptr;
  uint64_t* d_rep = nullptr;    // the repetition / position-history row of every state (not Connect4)
  const uint32_t V = gi.P + 1, stride = len + gi.max_turns + 4 + extra_reps;
  AZMI_HIP_TRY_NODEV(tmp.upload(d_moves, moves, static_cast<size_t>(n) * len));
  if (init) AZMI_HIP_TRY_NODEV(tmp.upload(d_init, init, static_cast<size_t>(n) * init_stride));
  AZMI_HIP_TRY_NODEV(tmp.upload(d_seeds, seeds, n));
  AZMI_HIP_TRY_NODEV(tmp.alloc(d_v, static_cast<size_t>(n) * V));
  AZMI_HIP_TRY_NODEV(tmp.alloc(d_pi, static_cast<size_t>(n) * gi.M));
  AZMI_HIP_TRY_NODEV(tmp.alloc(d_status, n));
  if (game != AZMI_GAME_CONNECT4) AZMI_HIP_TRY_NODEV(tmp.alloc(d_rep, static_cast<size_t>(n) * stride));
  azmi_host_launch_playout(game, d_init, init_stride, d_moves, n, len, d_rep, stride, d_seeds, d_v, d_pi, d_status);
  AZMI_HIP_TRY_NODEV(hipGetLastError());
  AZMI_HIP_TRY_NODEV(hipDeviceSynchronize());
  std::vector<int32_t> st(n);
  AZMI_HIP_TRY_NODEV(hipMemcpy(st.data(), d_status, static_cast<size_t>(n) * 4, hipMemcpyDeviceToHost));
  AZMI_HIP_TRY_NODEV(hipMemcpy(v, d_v, static_cast<size_t>(n) * V * 4, hipMemcpyDeviceToHost));
  AZMI_HIP_TRY_NODEV(hipMemcpy(pi, d_pi, static_cast<size_t>(n) * gi.M * 4, hipMemcpyDeviceToHost));
  for (uint32_t i = 0; i < n; ++i) if (st[i]) return azmi_host_fail(AZMI_ERR_INVALID, "illegal move in the game record of state %u", i);
  return AZMI_OK;
}

int azmi_game_replay_ex(int game, int device, const uint8_t* init, uint32_t init_stride, const int32_t* moves,
                        uint32_t n, uint32_t len, uint8_t* valid, float* scores, float* canonical,
                        uint32_t* player, uint32_t* turn, uint64_t* key, int32_t* status, uint32_t flags) {
  GameInfo gi;
  if (!azmi_host_game_info(game, &gi)) return azmi_host_fail(AZMI_ERR_INVALID, "unknown game id %d", game);
  if (!moves && n * len) return azmi_host_fail(AZMI_ERR_INVALID, "null moves");
  uint32_t extra_reps = 0;
  { const int rc_init = check_init_rows(game, init, init_stride, n, &extra_reps); if (rc_init != AZMI_OK) return rc_init; }
  { const int rc_dev = require_device(device); if (rc_dev != AZMI_OK) return rc_dev; }
  const uint32_t CANON = gi.C * gi.H * gi.W, V = gi.P + 1;
  DevTemps tmp;
  int32_t* d_moves = nullptr; uint8_t* d_init = nullptr; uint8_t* d_valid = nullptr; float *d_scores = nullptr, *d_canon = nullptr;
  uint32_t *d_player = nullptr, *d_turn = nullptr; uint64_t* d_key = nullptr; int32_t* d_status = nullptr;
  AZMI_HIP_TRY_NODEV(tmp.upload(d_moves, moves, static_cast<size_t>(n) * len));
  if (init && n) AZMI_HIP_TRY_NODEV(tmp.upload(d_init, init, static_cast<size_t>(n) * init_stride));
  if (valid) AZMI_HIP_TRY_NODEV(tmp.alloc(d_valid, static_cast<size_t>(n) * gi.M));
  if (scores) AZMI_HIP_TRY_NODEV(tmp.alloc(d_scores, static_cast<size_t>(n) * V));
  if (canonical) AZMI_HIP_TRY_NODEV(tmp.alloc(d_canon, static_cast<size_t>(n) * CANON));
  if (player) AZMI_HIP_TRY_NODEV(tmp.alloc(d_player, n));
  if (turn) AZMI_HIP_TRY_NODEV(tmp.alloc(d_turn, n));
  if (key) AZMI_HIP_TRY_NODEV(tmp.alloc(d_key, n));
  if (status) AZMI_HIP_TRY_NODEV(tmp.alloc(d_status, n));
  if (n) {
    uint64_t* d_rep = nullptr;    // the repetition / position-history row of every game (not Connect4)
    const uint32_t stride = len + (game == AZMI_GAME_STARGAMBIT ? 4 : 2) + extra_reps;
    if (game != AZMI_GAME_CONNECT4) AZMI_HIP_TRY_NODEV(tmp.alloc(d_rep, static_cast<size_t>(n) * stride));
    azmi_host_launch_replay(game, d_init, init_stride, d_moves, n, len, d_rep, stride, d_valid, d_scores, d_canon, d_player, d_turn, d_key, d_status, flags);
    AZMI_HIP_TRY_NODEV(hipGetLastError());
    AZMI_HIP_TRY_NODEV(hipDeviceSynchronize());
  }
  if (valid) AZMI_HIP_TRY_NODEV(hipMemcpy(valid, d_valid, static_cast<size_t>(n) * gi.M, hipMemcpyDeviceToHost));
  if (scores) AZMI_HIP_TRY_NODEV(hipMemcpy(scores, d_scores, static_cast<size_t>(n) * V * 4, hipMemcpyDeviceToHost));
  if (canonical) AZMI_HIP_TRY_NODEV(hipMemcpy(canonical, d_canon, static_cast<size_t>(n) * CANON * 4, hipMemcpyDeviceToHost));
  if (player) AZMI_HIP_TRY_NODEV(hipMemcpy(player, d_player, static_cast<size_t>(n) * 4, hipMemcpyDeviceToHost));
  if (turn) AZMI_HIP_TRY_NODEV(hipMemcpy(turn, d_turn, static_cast<size_t>(n) * 4, hipMemcpyDeviceToHost));
  if (key) AZMI_HIP_TRY_NODEV(hipMemcpy(key, d_key, static_cast<size_t>(n) * 8, hipMemcpyDeviceToHost));
  if (status) AZMI_HIP_TRY_NODEV(hipMemcpy(status, d_status, static_cast<size_t>(n) * 4, hipMemcpyDeviceToHost));
  return AZMI_OK;
}

// StarGambitUnifiedGS::to_bytes (star_gambit_gs.cc:2451-2465) of n states given as start image + moves: rows of out_stride
// bytes (probs / pinned_variant fields zero: they belong to the caller's object), sizes in out_len
int azmi_sg_image(int device, const uint8_t* init, uint32_t init_stride, const int32_t* moves, uint32_t n, uint32_t len,
                  uint8_t* out, uint32_t out_stride, uint32_t* out_len, int32_t* status, uint32_t flags) {
  if (!out || !out_len || !status || (!moves && n * len)) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  uint32_t extra_reps = 0;
  { const int rc_init = check_init_rows(AZMI_GAME_STARGAMBIT, init, init_stride, n, &extra_reps); if (rc_init != AZMI_OK) return rc_init; }
  if (n == 0) return AZMI_OK;
  { const int rc_dev = require_device(device); if (rc_dev != AZMI_OK) return rc_dev; }
  DevTemps tmp;
  int32_t* d_moves = nullptr; uint8_t* d_init = nullptr; uint64_t* d_rep = nullptr; uint8_t* d_out = nullptr; uint32_t* d_len = nullptr; int32_t* d_status = nullptr;
  const uint32_t stride = len + 4 + extra_reps;
  AZMI_HIP_TRY_NODEV(tmp.upload(d_moves, moves, static_cast<size_t>(n) * len));
  if (init) AZMI_HIP_TRY_NODEV(tmp.upload(d_init, init, static_cast<size_t>(n) * init_stride));
  AZMI_HIP_TRY_NODEV(tmp.alloc(d_rep, static_cast<size_t>(n) * stride));
  AZMI_HIP_TRY_NODEV(tmp.alloc(d_out, static_cast<size_t>(n) * out_stride));
  AZMI_HIP_TRY_NODEV(tmp.alloc(d_len, n));
  AZMI_HIP_TRY_NODEV(tmp.alloc(d_status, n));
  azmi_host_launch_sg_image(d_init, init_stride, d_moves, n, len, d_rep, stride, d_out, out_stride, d_len, d_status, flags);
  AZMI_HIP_TRY_NODEV(hipGetLastError());
  AZMI_HIP_TRY_NODEV(hipDeviceSynchronize());
  AZMI_HIP_TRY_NODEV(hipMemcpy(out, d_out, static_cast<size_t>(n) * out_stride, hipMemcpyDeviceToHost));
  AZMI_HIP_TRY_NODEV(hipMemcpy(out_len, d_len, static_cast<size_t>(n) * 4, hipMemcpyDeviceToHost));
  AZMI_HIP_TRY_NODEV(hipMemcpy(status, d_status, static_cast<size_t>(n) * 4, hipMemcpyDeviceToHost));
  return AZMI_OK;
}

}  // extern "C"
