// Host side of libazmi.so: owns the HBM arrays of one PlayManager, launches the
// round kernels, and implements the C ABI declared in include/azmi.h.
// There is deliberately no CPU code path: every entry point that computes
// requires a HIP device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <string>
#include <vector>

#include "../../include/azmi.h"
#include <atomic>
#include <mutex>

#include "cache_host.h"
#include "engine_host.h"
#include "engine_kernels.h"
#include "leafnet_c4.h"
#include "engine_kernels_big.h"
#include "game_dispatch.h"
#include "mcts_object_kernels.h"

using namespace azmi;

namespace {
thread_local std::string g_err;
}  // namespace
int azmi_host_fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

bool azmi_host_game_info(int game, GameInfo* gi) {
  switch (game) {
    case AZMI_GAME_CONNECT4:
      *gi = GameInfo{Connect4::P, Connect4::M, Connect4::C, Connect4::H, Connect4::W, Connect4::MAXK,
                     Connect4::MAX_TURNS, 3, Connect4::MAXK};
      return true;
    case AZMI_GAME_TAWLBWRDD:
      *gi = GameInfo{Tawlbwrdd::P, Tawlbwrdd::M, Tawlbwrdd::C, Tawlbwrdd::H, Tawlbwrdd::W, Tawlbwrdd::MAXK,
                     Tawlbwrdd::MAX_TURNS, Tawlbwrdd::STATE_WORDS, 160};
      return true;
    case AZMI_GAME_BRANDUBH:
      *gi = GameInfo{Brandubh::P, Brandubh::M, Brandubh::C, Brandubh::H, Brandubh::W, Brandubh::MAXK,
                     Brandubh::MAX_TURNS, Brandubh::STATE_WORDS, 48};
      return true;
    case AZMI_GAME_OPENTAFL:
      *gi = GameInfo{OpenTafl::P, OpenTafl::M, OpenTafl::C, OpenTafl::H, OpenTafl::W, OpenTafl::MAXK,
                     OpenTafl::MAX_TURNS, OpenTafl::STATE_WORDS, 160};
      return true;
    case AZMI_GAME_STARGAMBIT:   // max_turns = the engine's bound on the ACTIONS of a game (dev_stargambit.h)
      *gi = GameInfo{StarGambit::P, StarGambit::M, StarGambit::C, StarGambit::H, StarGambit::W, StarGambit::MAXK,
                     StarGambit::MAX_TURNS, StarGambit::STATE_WORDS, 32};
      return true;
    default:
      return false;
  }
}

namespace azmi {
// the one plain (non-template) kernel over engine_kernels.h: defined here, launched through azmi_host_launch_assign elsewhere
__global__ void k_assign(EngineParams ep, EngineArrays ar, uint32_t count_round) { assign_body(ep, ar, count_round); }
}  // namespace azmi

namespace {

__global__ void k_seed(EngineArrays ar, uint32_t S, uint64_t seed) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  Pcg32 g;
  const uint64_t sd = slot_seed(seed, s);
  g.seed(sd);
  ar.rng[s] = g.state;
  g.seed(sd ^ kCoinSalt);
  ar.coin[s] = g.state;
  g.seed(sd ^ kRollSalt);
  ar.roll[s] = g.state;
}

// start of a round: cache insert of last round's leaves + the restart/retire bookkeeping in one launch
template <class GM>
void launch_pre_round(azmi_pm* pm, hipStream_t st) {
  if (!pm->ep.cache_on) { k_assign<<<1, 256, 0, st>>>(pm->ep, pm->ar, 1u); return; }
  for (uint32_t g = 0; g < pm->ep.num_groups; ++g)
    for (uint32_t off = 0; off < pm->ep.S; off += kApplyMax) {
      const uint32_t m = std::min<uint32_t>(kApplyMax, pm->ep.S - off);
      const uint32_t nb = (m + 3) / 4;
      const bool with_assign = g == 0 && off == 0;
      k_cache_insert<GM><<<nb + (with_assign ? 1u : 0u), 256, 0, st>>>(pm->ep, pm->ar, pm->ar.cache_keys, off, m,
                                                                      with_assign ? nb : 0xFFFFFFFFu, 1u, g);
    }
}

// defer_moves: split rounds only - leave the move step to the fused net launch that follows (launch_net_move)
int launch_round(azmi_pm* pm, hipStream_t st, bool defer_moves = false) {
  const uint32_t threads = 256;
  switch (pm->game) {
    case AZMI_GAME_CONNECT4: {
      launch_pre_round<Connect4>(pm, st);
      const uint32_t slots_per_block = threads / Connect4::GROUP;
      const uint32_t blocks = (pm->ep.S + slots_per_block - 1) / slots_per_block;
      if (pm->any_playout) k_round<Connect4, true><<<blocks, threads, 0, st>>>(pm->ep, pm->ar);
      else if (pm->split_rounds) {
        // split round: the lean per-simulation kernel over every slot, then the move step over the slots it listed
        k_sim<Connect4><<<blocks, threads, 0, st>>>(pm->ep, pm->ar);
        if (!defer_moves) k_round<Connect4, false, true><<<blocks, threads, 0, st>>>(pm->ep, pm->ar);
      }
      else k_round<Connect4><<<blocks, threads, 0, st>>>(pm->ep, pm->ar);
      break;
    }
    case AZMI_GAME_TAWLBWRDD:
      launch_pre_round<Tawlbwrdd>(pm, st);
      if (pm->any_playout) k_round_big<Tawlbwrdd, true><<<pm->ep.S, 64, 0, st>>>(pm->ep, pm->ar);
      else if (pm->big_split) { k_round_big_sim<Tawlbwrdd><<<pm->ep.S, 64, 0, st>>>(pm->ep, pm->ar); k_round_big_move<Tawlbwrdd><<<pm->ep.S, 64, 0, st>>>(pm->ep, pm->ar); }
      else k_round_big_o2<Tawlbwrdd><<<pm->ep.S, 64, 0, st>>>(pm->ep, pm->ar);
      if (pm->ep.half_nodes) k_compact<Tawlbwrdd><<<std::min(pm->ep.S * pm->gi.P, kCompactBlocks), 256, 0, st>>>(pm->ep, pm->ar, pm->ep.S * pm->gi.P);
      break;
    case AZMI_GAME_BRANDUBH:
      launch_pre_round<Brandubh>(pm, st);
      if (pm->any_playout) k_round_big<Brandubh, true><<<pm->ep.S, 64, 0, st>>>(pm->ep, pm->ar);
      else if (pm->big_split) { k_round_big_sim<Brandubh><<<pm->ep.S, 64, 0, st>>>(pm->ep, pm->ar); k_round_big_move<Brandubh><<<pm->ep.S, 64, 0, st>>>(pm->ep, pm->ar); }
      else k_round_big_o2<Brandubh><<<pm->ep.S, 64, 0, st>>>(pm->ep, pm->ar);
      if (pm->ep.half_nodes) k_compact<Brandubh><<<std::min(pm->ep.S * pm->gi.P, kCompactBlocks), 256, 0, st>>>(pm->ep, pm->ar, pm->ep.S * pm->gi.P);
      break;
    case AZMI_GAME_OPENTAFL:
      launch_pre_round<OpenTafl>(pm, st);
      if (pm->any_playout) k_round_big<OpenTafl, true><<<pm->ep.S, 64, 0, st>>>(pm->ep, pm->ar);
      else if (pm->big_split) { k_round_big_sim<OpenTafl><<<pm->ep.S, 64, 0, st>>>(pm->ep, pm->ar); k_round_big_move<OpenTafl><<<pm->ep.S, 64, 0, st>>>(pm->ep, pm->ar); }
      else k_round_big_o2<OpenTafl><<<pm->ep.S, 64, 0, st>>>(pm->ep, pm->ar);
      if (pm->ep.half_nodes) k_compact<OpenTafl><<<std::min(pm->ep.S * pm->gi.P, kCompactBlocks), 256, 0, st>>>(pm->ep, pm->ar, pm->ep.S * pm->gi.P);
      break;
    case AZMI_GAME_STARGAMBIT:
      launch_pre_round<StarGambit>(pm, st);
      if (pm->any_playout) k_round_big<StarGambit, true><<<pm->ep.S, 64, 0, st>>>(pm->ep, pm->ar);
      else if (pm->big_split) { k_round_big_sim1<StarGambit><<<pm->ep.S, 64, 0, st>>>(pm->ep, pm->ar); k_round_big_move<StarGambit><<<pm->ep.S, 64, 0, st>>>(pm->ep, pm->ar); }
      else k_round_big<StarGambit><<<pm->ep.S, 64, 0, st>>>(pm->ep, pm->ar);
      if (pm->ep.half_nodes) k_compact<StarGambit><<<std::min(pm->ep.S * pm->gi.P, kCompactBlocks), 256, 0, st>>>(pm->ep, pm->ar, pm->ep.S * pm->gi.P);
      break;
    default:
      return azmi_host_fail(AZMI_ERR_INVALID, "game %d has no device kernels", pm->game);
  }
  AZMI_HIP_TRY(hipGetLastError());
  return AZMI_OK;
}

// The net + move-step launch of a split round (Connect4 engine, one model group): workgroups [0, net_tiles) carry the tiles
// of the round's eval list through the leaf net (leafnet_c4.h), the workgroups behind them run the round's move step
// (round_body<kMover> over ar.mover_list).  The two are independent - a listed mover was not evaluated this round, its
// new leaf is only queued for the next one - so the 20-60 us move chains hide behind the net instead of stretching the
// tree kernel of every round.
__global__ __launch_bounds__(256, 2) void k_net_move(azmi_net_dev::NetDesc nd, azmi_net_dev::NetPtrs np, EngineParams ep, EngineArrays ar,
                                                     uint32_t net_tiles) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds_fused[];
  if (blockIdx.x < net_tiles)
    azmi_net_dev::c4::tile<azmi_net_dev::c4::TileSmall, 4, 4, 16>(nd, np, ar.canon, ar.v, ar.pi, ep.S, ar.eval_list, &ar.ctl->eval_count[0], blockIdx.x, lds_fused);
  else
    round_body<Connect4, false, true>(ep, ar, (blockIdx.x - net_tiles) * blockDim.x + threadIdx.x);
}

}  // namespace
// the two between-epoch steps of the asynchronous pipeline (pipeline_run.hip): the move step of a split round over the slots the
// tree side listed, as a launch of its own, and the restart / retire bookkeeping
unsigned long long azmi_host_pipe_l0_hits(azmi_pm* pm, hipStream_t st);    // pipeline_state.hip
int azmi_host_launch_move_step(azmi_pm* pm, hipStream_t st) {
  const uint32_t blocks = (pm->ep.S * Connect4::GROUP + 255u) / 256u;
  k_round<Connect4, false, true><<<blocks, 256, 0, st>>>(pm->ep, pm->ar);
  AZMI_HIP_TRY(hipGetLastError());
  return AZMI_OK;
}
int azmi_host_launch_assign(azmi_pm* pm, hipStream_t st, uint32_t count_round) {
  k_assign<<<1, 256, 0, st>>>(pm->ep, pm->ar, count_round);
  AZMI_HIP_TRY(hipGetLastError());
  return AZMI_OK;
}
int azmi_host_read_ctl(azmi_pm* pm, hipStream_t st, Control* out, bool settle) {
  if (settle) k_assign<<<1, 256, 0, st>>>(pm->ep, pm->ar, 0u);
  AZMI_HIP_TRY(hipMemcpyAsync(out, pm->ar.ctl, sizeof(Control), hipMemcpyDeviceToHost, st));
  AZMI_HIP_TRY(hipStreamSynchronize(st));
  if (out->overflow)
    return azmi_host_fail(AZMI_ERR_OVERFLOW, "device engine stopped: overflow mask 0x%x (1 tree arena, 2 history, 4 move log, "
                          "8 path/children, 16 pick_move, 32 unknown move, 64 illegal move)", out->overflow);
  return AZMI_OK;
}
namespace {

template <class T>
int d2h(std::vector<T>& dst, const T* src, size_t n, hipStream_t st) {
  dst.resize(n);
  AZMI_HIP_TRY(hipMemcpyAsync(dst.data(), src, n * sizeof(T), hipMemcpyDeviceToHost, st));
  AZMI_HIP_TRY(hipStreamSynchronize(st));
  return AZMI_OK;
}

}  // namespace

#include "replay_kernels.h"   // (here, behind the engine's own kernels: the order of the device module is kept)

extern "C" {

const char* azmi_last_error(void) { return g_err.c_str(); }
int azmi_abi_version(void) { return AZMI_ABI_VERSION; }
int azmi_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

void azmi_play_params_default(azmi_play_params* p) {  // play_manager.h:60-154
  std::memset(p, 0, sizeof(*p));
  p->max_batch_size = 1;
  p->cache_shards = 1;
  p->cpuct = 2.0f;
  p->start_temp = 1.0f;
  p->final_temp = 1.0f;
  p->tree_reuse = 1;
  p->mcts_root_temp = 1.0f;
  p->playout_cap_depth = 25;
  p->playout_cap_percent = 0.75f;
  p->gumbel_m = 16;
  p->gumbel_c_visit = 50.0f;
  p->gumbel_c_scale = 1.0f;
}
void azmi_engine_opts_default(azmi_engine_opts* o) {
  std::memset(o, 0, sizeof(*o));
  o->seed = 20240601ULL;  // mcts_test.cc:515
}

int azmi_game_info(int game, uint32_t* num_players, uint32_t* num_moves, uint32_t chw[3]) {
  GameInfo gi;
  if (!azmi_host_game_info(game, &gi)) return azmi_host_fail(AZMI_ERR_INVALID, "unknown game id %d", game);
  if (num_players) *num_players = gi.P;
  if (num_moves) *num_moves = gi.M;
  if (chw) { chw[0] = gi.C; chw[1] = gi.H; chw[2] = gi.W; }
  return AZMI_OK;
}

namespace {
// PlayManager ctor normalisation of model groups, seat permutations and the per-seat override matrices
// (play_manager.cc:24-113): mcts_visits / eval_type are given per PLAYER, folded per model group (the last player
// of a group wins), then expanded per (permutation, seat).
struct SeatTables {
  uint32_t num_groups = 1, num_perms = 1, max_visits = 0;
  bool all_random = true, any_random = false;
  bool any_gumbel = false, any_seat_resign = false, any_playout = false;
  uint32_t nn_groups = 0;        // bit g: a seat of model group g evaluates with the net
  std::vector<uint32_t> words;   // [perm][seat][kSeatWords]
};
int build_seat_tables(const azmi_play_params* p, uint32_t P, SeatTables* out) {
  uint8_t groups[AZMI_MAX_PLAYERS];
  if (p->num_model_groups_given == 0) for (uint32_t i = 0; i < P; ++i) groups[i] = static_cast<uint8_t>(i);
  else {
    if (p->num_model_groups_given != P) return azmi_host_fail(AZMI_ERR_INVALID, "model_groups must be empty or have one entry per player");
    for (uint32_t i = 0; i < P; ++i) groups[i] = p->model_groups[i];
  }
  uint32_t ng = 0;
  for (uint32_t i = 0; i < P; ++i) ng = std::max<uint32_t>(ng, groups[i] + 1u);
  if (ng > AZMI_MAX_GROUPS) return azmi_host_fail(AZMI_ERR_INVALID, "at most %d model groups", AZMI_MAX_GROUPS);
  uint32_t visits_g[AZMI_MAX_GROUPS] = {0, 0, 0, 0};
  int32_t eval_g[AZMI_MAX_GROUPS] = {AZMI_EVAL_NN, AZMI_EVAL_NN, AZMI_EVAL_NN, AZMI_EVAL_NN};
  for (uint32_t i = 0; i < P; ++i) {
    visits_g[groups[i]] = p->mcts_visits[i];
    if (p->num_eval_type) eval_g[groups[i]] = p->eval_type[i];
  }
  uint32_t np = p->num_seat_perms;
  uint8_t perms[AZMI_MAX_PERMS][AZMI_MAX_PLAYERS];
  if (np == 0) { np = 1; for (uint32_t s = 0; s < P; ++s) perms[0][s] = groups[s]; }
  else {
    if (np > AZMI_MAX_PERMS) return azmi_host_fail(AZMI_ERR_INVALID, "at most %d seat permutations", AZMI_MAX_PERMS);
    for (uint32_t q = 0; q < np; ++q)
      for (uint32_t s = 0; s < P; ++s) {
        if (p->seat_perms[q][s] >= ng) return azmi_host_fail(AZMI_ERR_INVALID, "seat_perms refers to model group %u but there are %u", unsigned(p->seat_perms[q][s]), ng);
        perms[q][s] = p->seat_perms[q][s];
      }
  }
  out->num_groups = ng; out->num_perms = np;
  out->words.assign(static_cast<size_t>(np) * P * kSeatWords, 0u);
  out->max_visits = p->playout_cap_randomization ? p->playout_cap_depth : 0;
  for (uint32_t q = 0; q < np; ++q)
    for (uint32_t s = 0; s < P; ++s) {
      const uint32_t g = perms[q][s];
      const uint32_t visits = p->has_seat_visits ? p->seat_visits[q][s] : visits_g[g];
      const uint32_t capv = p->has_seat_cap_visits ? p->seat_cap_visits[q][s] : p->playout_cap_depth;
      const float eps = p->has_seat_epsilon ? p->seat_epsilon[q][s] : p->epsilon;
      const float rt = p->has_seat_mcts_root_temp ? p->seat_mcts_root_temp[q][s] : p->mcts_root_temp;
      const uint32_t fz = p->has_seat_root_fpu_zero ? (p->seat_root_fpu_zero[q][s] != 0) : (p->root_fpu_zero != 0);
      const bool playout = eval_g[g] == AZMI_EVAL_PLAYOUT;
      const bool rnd = eval_g[g] == AZMI_EVAL_RANDOM;   // all_random below: "no seat needs a net" (RANDOM or PLAYOUT)
      out->any_playout = out->any_playout || playout;
      if (capv > 0xFFFFFFu) return azmi_host_fail(AZMI_ERR_INVALID, "seat_cap_visits too large");
      out->all_random = out->all_random && (rnd || playout); out->any_random = out->any_random || rnd || playout;
      if (!(rnd || playout)) out->nn_groups |= 1u << g;
      out->max_visits = std::max(out->max_visits, visits);
      if (p->playout_cap_randomization) out->max_visits = std::max(out->max_visits, capv);
      // per-seat Gumbel / resign overrides, play_manager.cc:116-176
      const uint32_t gum = p->has_seat_gumbel_enabled ? (p->seat_gumbel_enabled[q][s] != 0) : (p->gumbel_enabled != 0);
      const uint32_t gfull = p->has_seat_gumbel_full ? (p->seat_gumbel_full[q][s] != 0) : (p->gumbel_full != 0);
      const uint32_t g3 = p->has_seat_gumbel_use_improved_policy ? (p->seat_gumbel_use_improved_policy[q][s] != 0) : 0u;
      const uint32_t gm = p->has_seat_gumbel_m ? p->seat_gumbel_m[q][s] : p->gumbel_m;
      const float gcv = p->has_seat_gumbel_c_visit ? p->seat_gumbel_c_visit[q][s] : p->gumbel_c_visit;
      const float gcs = p->has_seat_gumbel_c_scale ? p->seat_gumbel_c_scale[q][s] : p->gumbel_c_scale;
      const float rth = p->has_seat_resign_threshold ? p->seat_resign_threshold[q][s] : -2.0f;
      const uint32_t rneed = std::max<uint32_t>(1u, p->has_seat_resign_consecutive ? p->seat_resign_consecutive[q][s] : 1u);
      if (gum && gm > kGumMaxM) return azmi_host_fail(AZMI_ERR_INVALID, "gumbel_m %u exceeds the engine limit %u", gm, kGumMaxM);
      if (rneed > 255u) return azmi_host_fail(AZMI_ERR_INVALID, "seat_resign_consecutive %u exceeds the engine limit 255", rneed);
      if (rth > -2.0f && P != 2) return azmi_host_fail(AZMI_ERR_INVALID, "Per-seat resign only works in 2 player games");
      out->any_gumbel = out->any_gumbel || gum;
      out->any_seat_resign = out->any_seat_resign || rth > -2.0f;
      uint32_t* w = &out->words[(static_cast<size_t>(q) * P + s) * kSeatWords];
      w[0] = visits; w[1] = seat_w1_pack(capv, fz, rnd ? 1u : 0u, g, playout ? 1u : 0u);
      std::memcpy(&w[2], &eps, 4); std::memcpy(&w[3], &rt, 4);
      w[4] = seat_gum_pack(gum, gfull, g3, gm, rneed);
      std::memcpy(&w[5], &gcv, 4); std::memcpy(&w[6], &gcs, 4); std::memcpy(&w[7], &rth, 4);
    }
  return AZMI_OK;
}
}  // namespace

namespace {
int pm_create_impl(int game, const azmi_play_params* params, const azmi_engine_opts* opts_in, azmi_cache* const* ext_caches,
                   uint32_t num_ext, bool use_ext, azmi_pm** out);
}
int azmi_pm_create(int game, const azmi_play_params* params, const azmi_engine_opts* opts_in, azmi_pm** out) {
  return pm_create_impl(game, params, opts_in, nullptr, 0, false, out);
}
// PlayManager(gs, params, caches), play_manager.cc:644-649: max_cache_size is forced to 0 and the given caches are used
int azmi_pm_create_with_caches(int game, const azmi_play_params* params, const azmi_engine_opts* opts_in, azmi_cache* const* caches,
                               uint32_t num_caches, azmi_pm** out) {
  if (num_caches && !caches) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  return pm_create_impl(game, params, opts_in, caches, num_caches, true, out);
}
namespace {
int pm_create_impl(int game, const azmi_play_params* params, const azmi_engine_opts* opts_in, azmi_cache* const* ext_caches,
                   uint32_t num_ext, bool use_ext, azmi_pm** out) {
  if (!params || !out) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  GameInfo gi;
  if (!azmi_host_game_info(game, &gi)) return azmi_host_fail(AZMI_ERR_INVALID, "unknown game id %d", game);
  azmi_engine_opts opts;
  if (opts_in) opts = *opts_in; else azmi_engine_opts_default(&opts);
  // play_manager.cc:20-22
  if (params->num_mcts_visits != gi.P) return azmi_host_fail(AZMI_ERR_INVALID, "You must specify MCTS visits for each player");
  if (params->concurrent_games == 0) return azmi_host_fail(AZMI_ERR_INVALID, "concurrent_games must be > 0");
  if (params->num_eval_type != 0 && params->num_eval_type != gi.P)
    return azmi_host_fail(AZMI_ERR_INVALID, "eval_type must be empty or have one entry per player");
  SeatTables seats;
  { const int rc_seats = build_seat_tables(params, gi.P, &seats); if (rc_seats != AZMI_OK) return rc_seats; }
  if (params->resign_percent > 0 && gi.P != 2) return azmi_host_fail(AZMI_ERR_INVALID, "Resigning only works in 2 player games");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return azmi_host_fail(AZMI_ERR_NO_DEVICE, "no HIP device: libazmi has no CPU path");
  if (opts.device < 0 || opts.device >= ndev) return azmi_host_fail(AZMI_ERR_INVALID, "device %d out of range", opts.device);
  AZMI_HIP_TRY(hipSetDevice(opts.device));

  auto pm = new azmi_pm();
  pm->game = game; pm->device = opts.device; pm->gi = gi; pm->params = *params;
  EngineParams& ep = pm->ep;
  ep.S = params->concurrent_games;
  ep.games_to_play = params->games_to_play;
  const uint32_t max_visits = seats.max_visits;
  for (uint32_t i = 0; i < gi.P; ++i) ep.visits[i] = params->mcts_visits[i];   // kept for reference; kernels read ar.seat_tab
  ep.cap_visits = params->playout_cap_depth;
  ep.num_perms = seats.num_perms; ep.num_groups = seats.num_groups;
  pm->all_random = seats.all_random;
  pm->nn_groups = seats.nn_groups;
  pm->any_playout = seats.any_playout;
  pm->split_rounds = game == AZMI_GAME_CONNECT4 && !seats.any_gumbel && !seats.any_playout && getenv("AZMI_NO_SPLIT") == nullptr;
  pm->big_split = (game == AZMI_GAME_TAWLBWRDD || game == AZMI_GAME_BRANDUBH || game == AZMI_GAME_OPENTAFL || game == AZMI_GAME_STARGAMBIT) && !seats.any_playout && getenv("AZMI_NO_BIG_SPLIT") == nullptr;
  // (StarGambit, round 6: its simulation kernel keeps the whole register file - k_round_big_sim1, one wave per SIMD: held to 256
  // registers it spills 232 of them)
  ep.cpuct = params->cpuct; ep.start_temp = params->start_temp; ep.final_temp = params->final_temp;
  ep.half_life = params->temp_decay_half_life;
  ep.n_half_life_v = 0;
  if (game == AZMI_GAME_STARGAMBIT) {
    if (params->num_temp_decay_half_life_by_variant > 4) { delete pm; return azmi_host_fail(AZMI_ERR_INVALID, "temp_decay_half_life_by_variant: at most 4 entries"); }
    ep.n_half_life_v = params->num_temp_decay_half_life_by_variant;
    for (uint32_t i = 0; i < 4; ++i) ep.half_life_v[i] = i < ep.n_half_life_v ? params->temp_decay_half_life_by_variant[i] : 0.0f;
    const bool given = opts.sg_variant_probs[0] != 0 || opts.sg_variant_probs[1] != 0 || opts.sg_variant_probs[2] != 0 || opts.sg_variant_probs[3] != 0;
    ep.sg_pinned = given || opts.sg_pinned_variant != 0 ? opts.sg_pinned_variant : -1;   // zeroed opts = the constructor's defaults
    for (uint32_t i = 0; i < 4; ++i) ep.sg_probs[i] = given ? opts.sg_variant_probs[i] : 0.25f;
  }
  ep.epsilon = params->epsilon; ep.root_temp = params->mcts_root_temp; ep.fpu_reduction = params->fpu_reduction;
  ep.cap_percent = params->playout_cap_percent; ep.resign_percent = params->resign_percent;
  ep.resign_playthrough = params->resign_playthrough_percent;
  ep.history = params->history_enabled != 0; ep.tree_reuse = params->tree_reuse != 0;
  ep.cap_rand = params->playout_cap_randomization != 0; ep.root_fpu_zero = params->root_fpu_zero != 0;
  ep.shaped = params->shaped_dirichlet != 0; ep.pruning = params->policy_target_pruning != 0;
  for (uint32_t i = 0; i < gi.P; ++i) ep.eval_random[i] = 0;
  ep.gumbel_on = seats.any_gumbel ? 1u : 0u;
  ep.gumbel_hist = params->gumbel_enabled != 0;
  ep.fast_gumbel = params->fast_search_uses_gumbel != 0;
  ep.seat_resign = seats.any_seat_resign ? 1u : 0u;
  ep.gum_stride = gi.maxk;
  // simulations a slot may finish inside one round without the net.  A round lasts as long as its SLOWEST slot, so inline
  // continuation pays only where a simulation is cheap next to the net launch (Connect4 with NN seats: 3 - measured 2588 / 2637 /
  // 2559 / 2502 games/s at 2 / 3 / 4 / 5 with the 3-board net tiles; 4 was the optimum behind the slower 6-board tiles).  In the wide-game engine a
  // simulation costs ~100 us: with NN seats one chain of cache hits / terminal leaves would stretch the round for every slot
  // (measured: Tawlbwrdd 4.49 -> 5.01 M sims/s, StarGambit 1.74 -> 2.14 M sims/s with 1 instead of 4); with RANDOM / PLAYOUT
  // seats only there is no net to wait for and 4 stands.
  ep.max_inline = opts.max_inline ? opts.max_inline : (seats.all_random ? 4u : game == AZMI_GAME_CONNECT4 ? 3u : 1u);
  pm->max_inline_explicit = opts.max_inline != 0;
  ep.sim_budget = getenv("AZMI_SIM_BUDGET_US") ? static_cast<uint32_t>(100.0 * atof(getenv("AZMI_SIM_BUDGET_US"))) : 0u;
  ep.max_hist_rows = gi.max_turns;
  ep.max_depth = gi.max_turns + 2;
  // every search expands at most one node (<= maxk children) per simulation and a tree is
  // searched on at most ceil(max_turns/2) turns; re-rooting an empty tree expands once more.
  // Connect4: cap_branch == maxk, a hard bound.  Wide games: sized for the average branching factor and
  // capped at 16 M nodes per tree; running out raises overflow bit 1 (arena compaction is the next step).
  uint64_t cap64 = (static_cast<uint64_t>((gi.max_turns + 1) / 2) * max_visits + gi.max_turns) * gi.cap_branch + 8;
  ep.half_nodes = 0; ep.compact_above = 0;
  if (gi.cap_branch != gi.maxk) {
    // wide games: two halves of 4 searches' worth of nodes each; the live subtree is copied into the idle
    // half (k_compact) when a move leaves less than one search of room in the active one
    const uint64_t growth = (static_cast<uint64_t>(max_visits) + 12 + (opts.max_inline ? opts.max_inline : 4)) * (gi.cap_branch * 3 / 2);
    const uint64_t half = std::min<uint64_t>(std::max<uint64_t>(4 * growth, 64u << 10), 8u << 20);
    ep.half_nodes = static_cast<uint32_t>(half);
    ep.compact_above = static_cast<uint32_t>(half > growth ? half - growth : half / 2);
    cap64 = 2 * half;
    if (const char* e = getenv("AZMI_COMPACT_ABOVE")) ep.compact_above = static_cast<uint32_t>(atoi(e));  // test hook: 0 = compact after every move
  }
  if (cap64 > 0xFFFFFFF0ULL) { delete pm; return azmi_host_fail(AZMI_ERR_INVALID, "tree arena too large"); }
  ep.cap = static_cast<uint32_t>(cap64);
  ep.log_moves = opts.log_moves != 0;
  ep.log_cap = ep.log_moves ? (opts.move_log_capacity ? opts.move_log_capacity
                                                       : (params->games_to_play + ep.S) * gi.max_turns) : 0;
  // finished-sample ring (rows): by default every row of the run, (games_to_play + S) * max_turns, computed in 64 bits and
  // bounded to 8 GiB of rows (never less than two full games per slot) — a longer run has to drain it
  // (build_history_batch / azmi_pm_history_consume), like the reference's hist_saver drains the unbounded queue
  if (ep.history && opts.history_capacity) {
    ep.hist_cap = opts.history_capacity;
  } else if (ep.history) {
    const uint64_t row_bytes = 4ull * (static_cast<uint64_t>(gi.C) * gi.H * gi.W + gi.P + 1 + gi.M + 4);
    // rows one game can produce: max_turns, except StarGambit whose 4096 is a hard bound on ACTIONS far above any real game
    // (self-play games: ~220 sample rows; thousands of random games peak below 800) - the default ring counts 1024 per game
    const uint64_t game_rows = game == AZMI_GAME_STARGAMBIT ? 1024u : gi.max_turns;
    const uint64_t all_rows = (static_cast<uint64_t>(params->games_to_play) + ep.S) * game_rows;
    const uint64_t bound = std::max<uint64_t>(2ull * ep.S * game_rows, (8ull << 30) / row_bytes);
    ep.hist_cap = static_cast<uint32_t>(std::min<uint64_t>(std::min(all_rows, bound), 0x7FFFFFFFull));
  } else {
    ep.hist_cap = 0;
  }

  const uint32_t S = ep.S, P = gi.P, M = gi.M, CANON = gi.C * gi.H * gi.W;
  const size_t T = static_cast<size_t>(S) * P, NODES = T * ep.cap;
  EngineArrays& ar = pm->ar;
  int rc = AZMI_OK;
#define A(field, count, zero) if (rc == AZMI_OK) rc = pm->alloc(ar.field, (count), (zero))
  A(ctl, 1, true);
  A(ended_list, S, true);
  A(mover_list, S, true);
  A(pend, game == AZMI_GAME_CONNECT4 ? static_cast<size_t>(S) * Connect4::GROUP : 0, true);
  A(eval_list, static_cast<size_t>(S) * ep.num_groups, true);
  A(seat_tab, seats.words.size(), false);
  A(perm, S, true);
  A(leaf_group, S, true);
  A(a_perm_scores, static_cast<size_t>(S) * ep.num_perms * (P + 1), true);
  A(a_perm_games, static_cast<size_t>(S) * ep.num_perms, true);
  A(gs_words, static_cast<size_t>(gi.state_words) * S, true);
  A(rng, S, true); A(coin, S, true);
  A(sstate, S, true); A(flags, S, true);
  A(cur, S, true); A(plen, S, true);
  A(path, static_cast<size_t>(S) * ep.max_depth, true);
  A(slot_games, S, true);
  A(rep_list, game != AZMI_GAME_CONNECT4 ? static_cast<size_t>(S) * (gi.max_turns + 2) : 0, true);
  A(rep_len, S, true);
  A(g_dsum, 5 * static_cast<size_t>(S), true); A(g_cnt, 3 * static_cast<size_t>(S), true);
  A(a_scores, static_cast<size_t>(S) * (P + 1), true); A(a_resign, static_cast<size_t>(S) * (P + 1), true);
  A(a_len, S, true); A(a_dsum, 5 * static_cast<size_t>(S), true); A(a_cnt, 3 * static_cast<size_t>(S), true);
  A(c_sims, S, true); A(c_evals, S, true);
  A(ph_count, S, true);
  A(ph_canon, ep.history ? static_cast<size_t>(S) * ep.max_hist_rows * (game == AZMI_GAME_CONNECT4 ? 2 * kPendingWords : game == AZMI_GAME_STARGAMBIT ? 2 * kSgPendWords : CANON) : 0, false);
  A(ph_pi, ep.history ? static_cast<size_t>(S) * ep.max_hist_rows * M : 0, false);
  A(ph_meta, ep.history ? static_cast<size_t>(S) * ep.max_hist_rows * 2 : 0, false);
  A(root, T, true); A(bump, T, true); A(depth, T, true); A(tld, T, true);
  if (game == AZMI_GAME_CONNECT4) {
    A(nodes, NODES, false);
  } else {
    A(N, NODES, false); A(Q, NODES, false); A(Pr, NODES, false); A(D, NODES, false); A(V, NODES, false);
    A(META, NODES, false);
  }
  A(canon, static_cast<size_t>(S) * CANON, true);
  A(v, static_cast<size_t>(S) * (P + 1), true);
  A(pi, static_cast<size_t>(S) * M, true);
  A(leaf_key, S, true);
  if (game == AZMI_GAME_CONNECT4) { A(leaf_pos, 3 * static_cast<size_t>(S), true); A(req_seq, S, true); }
  A(h_canon, static_cast<size_t>(ep.hist_cap) * CANON, false);
  A(h_v, static_cast<size_t>(ep.hist_cap) * (P + 1), false);
  A(h_pi, static_cast<size_t>(ep.hist_cap) * M, false);
  A(h_meta, static_cast<size_t>(ep.hist_cap) * 4, false);
  A(log_rows, static_cast<size_t>(ep.log_cap) * 8, false);
  A(log_counts, static_cast<size_t>(ep.log_cap) * M, false);
  // position cache: play_manager.cc:195-203 (one model group): ghost = 9/10 of the capacity.  The
  // reference's cache_shards (<= 255) exists to spread a mutex; here a shard is one wavefront's worth
  // of entries (64) and the unit of parallelism of the insert kernel.
  bool any_ext = false;
  if (use_ext) {
    // caches_[group] is indexed by model group (play_manager.cc:619-642): the list must cover every group; None entries
    // (groups that never reach the net) are allowed
    if (num_ext != 0 && num_ext < ep.num_groups) { delete pm; return azmi_host_fail(AZMI_ERR_INVALID, "caches: %u entries for %u model groups", num_ext, ep.num_groups); }
    for (uint32_t g = 0; g < std::min<uint32_t>(num_ext, ep.num_groups); ++g) {
      const azmi_cache* c = ext_caches[g];
      if (!c) continue;
      any_ext = true;
      if (c->device != opts.device) { delete pm; return azmi_host_fail(AZMI_ERR_INVALID, "caches[%u] lives on another device", g); }
      if (c->c.np != M || c->c.nv != P + 1) { delete pm; return azmi_host_fail(AZMI_ERR_INVALID, "caches[%u]: num_policy / num_value do not match the game", g); }
      if (c->c.cap != kWaveCap) {
        delete pm;
        return azmi_host_fail(AZMI_ERR_INVALID, "caches[%u]: the engine probes 64-entry shards; create the cache with shards = max_size / 64 "
                    "(ShardedS3FIFOCache.for_engine)", g);
      }
      if (!wave_layout(c->c)) {      // a lane of a wave shard holds one ghost-ring entry (dev_cache.h)
        delete pm;
        return azmi_host_fail(AZMI_ERR_INVALID, "caches[%u]: ghost_size / shards = %u, but a 64-entry wave shard keeps at most 64 ghost keys; create the "
                    "cache with ghost_size <= max_size (ShardedS3FIFOCache.for_engine)", g, c->c.ghost_cap);
      }
    }
  }
  ep.cache_on = use_ext ? any_ext : params->max_cache_size > 0;
  if (ep.cache_on) {
    // wave-resident shards: 64 entries each (dev_cache.h); max_cache_size is rounded down to a multiple of 64
    // one cache per model group, max_cache_size / num_model_groups entries each (play_manager.cc:195-203)
    const uint32_t shards = use_ext ? 1u : std::max<uint32_t>(1, params->max_cache_size / ep.num_groups / kWaveCap);
    pm->cache_shards = shards;
    A(cache_keys, S, true);
    pm->group_caches.resize(ep.num_groups);
    pm->group_cache_counted.assign(ep.num_groups, 1);
    for (uint32_t g = 0; g < ep.num_groups && rc == AZMI_OK; ++g) {
      if (use_ext && g < num_ext && ext_caches[g]) { pm->group_caches[g] = ext_caches[g]->c; continue; }
      if (use_ext) pm->group_cache_counted[g] = 0;   // a None entry: one private 64-entry shard stands in, outside the statistics
      if (cache_alloc(pm->group_caches[g], pm->allocs, shards * kWaveCap, shards, static_cast<uint32_t>(static_cast<uint64_t>(shards) * kWaveCap * 9 / 10), M, P + 1) != hipSuccess) {
        delete pm;
        return azmi_host_fail(AZMI_ERR_OOM, "position cache allocation failed");
      }
    }
    if (rc == AZMI_OK) {
      ar.cache = pm->group_caches[0];
      CacheView* dev_views = nullptr;
      rc = pm->alloc(dev_views, ep.num_groups, false);
      if (rc == AZMI_OK && hipMemcpy(dev_views, pm->group_caches.data(), sizeof(CacheView) * ep.num_groups, hipMemcpyHostToDevice) != hipSuccess) rc = AZMI_ERR_NO_DEVICE;
      ar.caches = dev_views;
    }
  }
  ep.trace_slot = getenv("AZMI_TRACE_SLOT") ? static_cast<uint32_t>(atoi(getenv("AZMI_TRACE_SLOT"))) : 0xFFFFFFFFu;
  ep.trace_cap = ep.trace_slot != 0xFFFFFFFFu ? (1u << 16) : 1u;
  ep.trace_after = getenv("AZMI_TRACE_AFTER") ? static_cast<uint32_t>(atoi(getenv("AZMI_TRACE_AFTER"))) : 0u;
  A(trace, 2 * static_cast<size_t>(ep.trace_cap), true);
  if (ep.half_nodes) A(compact_flag, T, true);
  if (ep.gumbel_on) {
    A(gum_state, static_cast<size_t>(S) * P * 8, true);
    A(gum_g, static_cast<size_t>(S) * P * ep.gum_stride, true);
    A(gum_surv, static_cast<size_t>(S) * P * kGumMaxM, true);
  }
  A(resign_streak, static_cast<size_t>(S) * P, true);
  A(roll, S, true);
  if (game == AZMI_GAME_STARGAMBIT) {
    A(rep_path, static_cast<size_t>(S) * (gi.max_turns + 2), true);
    A(a_var_scores, static_cast<size_t>(S) * 4 * ep.num_perms * (P + 1), true);
    A(a_var_games, static_cast<size_t>(S) * 4 * ep.num_perms, true);
    A(a_var_len, static_cast<size_t>(S) * 4, true);
    A(a_var_dsum, static_cast<size_t>(S) * 4 * 5, true);
    A(a_var_cnt, static_cast<size_t>(S) * 4 * 3, true);
  }
#undef A
  if (rc != AZMI_OK) { delete pm; return rc; }
  if (hipDeviceSynchronize() != hipSuccess) { delete pm; return azmi_host_fail(AZMI_ERR_NO_DEVICE, "device sync failed"); }
  if (hipStreamCreateWithFlags(&pm->stream, hipStreamNonBlocking) != hipSuccess) {
    delete pm;
    return azmi_host_fail(AZMI_ERR_NO_DEVICE, "hipStreamCreate failed");
  }
  Control c{};
  c.games_started = S;  // play_manager.cc:15
  c.live_slots = S;
  if (hipMemcpy(ar.ctl, &c, sizeof(c), hipMemcpyHostToDevice) != hipSuccess) { delete pm; return azmi_host_fail(AZMI_ERR_NO_DEVICE, "ctl init failed"); }
  if (hipMemcpy(ar.seat_tab, seats.words.data(), seats.words.size() * 4, hipMemcpyHostToDevice) != hipSuccess) { delete pm; return azmi_host_fail(AZMI_ERR_NO_DEVICE, "seat table upload failed"); }
  {
    std::vector<uint32_t> perm0(S);
    for (uint32_t i = 0; i < S; ++i) perm0[i] = i % ep.num_perms;   // gd.perm_index = i % seat_perms_.size(), play_manager.cc:218
    if (hipMemcpy(ar.perm, perm0.data(), S * 4, hipMemcpyHostToDevice) != hipSuccess) { delete pm; return azmi_host_fail(AZMI_ERR_NO_DEVICE, "perm init failed"); }
  }
  pm->pending_g.resize(ep.num_groups);
  k_seed<<<(S + 255) / 256, 256, 0, pm->stream>>>(ar, S, opts.seed);
  if (hipStreamSynchronize(pm->stream) != hipSuccess) { delete pm; return azmi_host_fail(AZMI_ERR_NO_DEVICE, "seed kernel failed"); }
  pm->host_v.assign(static_cast<size_t>(S) * (P + 1), 0.0f);
  pm->host_pi.assign(static_cast<size_t>(S) * M, 0.0f);
  pm->last = pm->stream;
  *out = pm;
  return AZMI_OK;
}
}  // namespace

void azmi_pm_destroy(azmi_pm* pm) {
  if (!pm) return;
  (void)hipSetDevice(pm->device);
  (void)hipDeviceSynchronize();
  delete pm;
}

int azmi_pm_round(azmi_pm* pm, void* stream) {
  if (!pm) return azmi_host_fail(AZMI_ERR_INVALID, "null pm");
  std::lock_guard<std::recursive_mutex> lock_(pm->mu);
  return launch_round(pm, pm->pick(stream));
}

namespace {
constexpr uint32_t kGraphRounds = 16;
// the net on this engine's leaf batch: only the rows k_round listed (Connect4 engine), else the whole batch
int pm_net_forward(azmi_pm* pm, uint32_t group, azmi_net* net, hipStream_t st) {
  int rc;
  if (pm->game == AZMI_GAME_CONNECT4 || pm->ep.num_groups > 1 || pm->ep.cache_on)
    rc = azmi_net_forward_rows(net, pm->ar.canon, pm->ar.v, pm->ar.pi, pm->ar.eval_list + static_cast<size_t>(group) * pm->ep.S,
                               &pm->ar.ctl->eval_count[group], pm->ep.S, st);
  else
    rc = azmi_net_forward(net, pm->ar.canon, pm->ar.v, pm->ar.pi, pm->ep.S, st);
  if (rc != AZMI_OK) return azmi_host_fail(rc, "%s", azmi_net_last_error());
  return AZMI_OK;
}
// split round + a Connect4-family bf16 net + one model group: the move step rides in the net launch (k_net_move)
bool can_fuse(const azmi_pm* pm, const azmi_net* net, azmi_net_c4_view* view) {
  return pm->split_rounds && pm->ep.num_groups == 1 && !pm->all_random && getenv("AZMI_NO_FUSE") == nullptr && azmi_net_c4_view_get(net, view) != 0 && view->x3 == 0;
}
int launch_net_move(azmi_pm* pm, const azmi_net_c4_view& view, hipStream_t st) {
  // (per device: the attribute belongs to the device's copy of the kernel; the tile's LDS need is a constant of the geometry)
  static std::mutex reserved_mu;
  static std::vector<int> reserved_devices;
  {
    std::lock_guard<std::mutex> l(reserved_mu);
    if (std::find(reserved_devices.begin(), reserved_devices.end(), pm->device) == reserved_devices.end()) {
      AZMI_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_net_move), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(view.lds_bytes)));
      reserved_devices.push_back(pm->device);
    }
  }
  const uint32_t net_tiles = (pm->ep.S + azmi_net_dev::c4::TileSmall::TBW - 1) / azmi_net_dev::c4::TileSmall::TBW;
  const uint32_t move_blocks = (pm->ep.S * Connect4::GROUP + 255) / 256;
  k_net_move<<<net_tiles + move_blocks, 256, view.lds_bytes, st>>>(view.nd, view.np, pm->ep, pm->ar, net_tiles);
  AZMI_HIP_TRY(hipGetLastError());
  return AZMI_OK;
}
int one_round_with_net(azmi_pm* pm, azmi_net* net, hipStream_t st) {
  azmi_net_c4_view view;
  if (can_fuse(pm, net, &view)) {
    const int rc = launch_round(pm, st, true);
    return rc != AZMI_OK ? rc : launch_net_move(pm, view, st);
  }
  int rc = launch_round(pm, st);
  if (rc != AZMI_OK) return rc;
  for (uint32_t g = 0; g < pm->ep.num_groups; ++g) {   // one net given: it serves every model group
    rc = pm_net_forward(pm, g, net, st);
    if (rc != AZMI_OK) return rc;
  }
  return AZMI_OK;
}
int ensure_graph(azmi_pm* pm, azmi_net* net, hipStream_t st) {
  if (pm->graph_exec && pm->graph_stream == st && pm->graph_net == net) return AZMI_OK;
  if (pm->graph_exec) { (void)hipGraphExecDestroy(pm->graph_exec); pm->graph_exec = nullptr; }
  hipGraph_t graph = nullptr;
  if (azmi_net_reserve_stream(net, st, pm->ep.S) != AZMI_OK) return azmi_host_fail(AZMI_ERR_OOM, "%s", azmi_net_last_error());
  AZMI_HIP_TRY(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
  int rc = AZMI_OK;
  for (uint32_t r = 0; r < kGraphRounds && rc == AZMI_OK; ++r) rc = one_round_with_net(pm, net, st);
  const hipError_t e = hipStreamEndCapture(st, &graph);
  if (rc != AZMI_OK) { if (graph) (void)hipGraphDestroy(graph); return rc; }
  if (e != hipSuccess) return azmi_host_fail(AZMI_ERR_NO_DEVICE, "hipStreamEndCapture: %s", hipGetErrorString(e));
  const hipError_t e2 = hipGraphInstantiate(&pm->graph_exec, graph, nullptr, nullptr, 0);
  (void)hipGraphDestroy(graph);
  if (e2 != hipSuccess) { pm->graph_exec = nullptr; return azmi_host_fail(AZMI_ERR_NO_DEVICE, "hipGraphInstantiate: %s", hipGetErrorString(e2)); }
  pm->graph_stream = st;
  pm->graph_net = net;
  return AZMI_OK;
}
}  // namespace

// holds a stream for about `us` microseconds (wall_clock64 ticks at 100 MHz)
__global__ void k_delay(uint32_t us) {
  const uint64_t t0 = wall_clock64();
  while (wall_clock64() - t0 < static_cast<uint64_t>(us) * 100u) __builtin_amdgcn_s_sleep(32);
}

int azmi_run_rounds(azmi_pm* const* pms, azmi_net* net, uint32_t k, uint32_t rounds, void* const* streams) {
  if (!pms || !net || !streams || k == 0) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  for (uint32_t i = 0; i < k; ++i)      // PlayManager::stop(): the workers leave their loop (play_manager.cc:272)
    if (pms[i] && pms[i]->stopped.load(std::memory_order_relaxed)) return AZMI_OK;
  if (const char* sg = getenv("AZMI_STAGGER_US")) {     // experiment: odd shards start half a cycle late
    const uint32_t us = static_cast<uint32_t>(atoi(sg));
    for (uint32_t i = 1; i < k && us; i += 2) k_delay<<<1, 64, 0, pms[i]->pick(streams[i])>>>(us);
  }
  // hipGraph replay of 16 rounds per launch is available (AZMI_GRAPH=1) but off by default: measured equal to plain
  // launches on this workload (2300 vs 2304 games/s — the host is ahead of the GPU either way), and capturing and
  // instantiating a graph per engine costs about a second at start-up
  const bool use_graph = getenv("AZMI_GRAPH") != nullptr && getenv("AZMI_NO_GRAPH") == nullptr;
  uint32_t done = 0;
  if (use_graph) {
    for (uint32_t i = 0; i < k; ++i) {
      const int rc = ensure_graph(pms[i], net, pms[i]->pick(streams[i]));
      if (rc != AZMI_OK) return rc;
    }
    for (; done + kGraphRounds <= rounds; done += kGraphRounds)
      for (uint32_t i = 0; i < k; ++i) AZMI_HIP_TRY(hipGraphLaunch(pms[i]->graph_exec, pms[i]->graph_stream));
  }
  for (; done < rounds; ++done)
    for (uint32_t i = 0; i < k; ++i) {
      const int rc = one_round_with_net(pms[i], net, pms[i]->pick(streams[i]));
      if (rc != AZMI_OK) return rc;
    }
  return AZMI_OK;
}

// The round loop with one net PER MODEL GROUP (gating / benchmark matches, game_runner.py:2184-2332: two models, seats
// swapped by the permutations): nets[g] evaluates the leaves of model group g; NULL = that group needs no net (RANDOM /
// PLAYOUT evaluator).
int azmi_run_rounds_groups(azmi_pm* const* pms, azmi_net* const* nets, uint32_t num_nets, uint32_t k, uint32_t rounds, void* const* streams) {
  if (!pms || !nets || !streams || k == 0) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  for (uint32_t i = 0; i < k; ++i)
    if (pms[i]->ep.num_groups > num_nets) return azmi_host_fail(AZMI_ERR_INVALID, "engine %u has %u model groups but %u nets were given", i, pms[i]->ep.num_groups, num_nets);
  for (uint32_t r = 0; r < rounds; ++r)
    for (uint32_t i = 0; i < k; ++i) {
      azmi_pm* pm = pms[i];
      hipStream_t st = pm->pick(streams[i]);
      int rc = launch_round(pm, st);
      if (rc != AZMI_OK) return rc;
      for (uint32_t g = 0; g < pm->ep.num_groups; ++g) {
        if (!nets[g]) continue;
        rc = pm_net_forward(pm, g, nets[g], st);
        if (rc != AZMI_OK) return rc;
      }
    }
  return AZMI_OK;
}

int azmi_pm_net_forward(azmi_pm* pm, azmi_net* net, void* stream) {
  if (!pm || !net) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  std::lock_guard<std::recursive_mutex> lock_(pm->mu);
  for (uint32_t g = 0; g < pm->ep.num_groups; ++g) {   // the same net for every model group
    const int rc = pm_net_forward(pm, g, net, pm->pick(stream));
    if (rc != AZMI_OK) return rc;
  }
  return AZMI_OK;
}

int azmi_pm_round_net(azmi_pm* pm, azmi_net* net, void* stream, uint32_t part) {
  if (!pm || !net) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  std::lock_guard<std::recursive_mutex> lock_(pm->mu);
  hipStream_t st = pm->pick(stream);
  azmi_net_c4_view view;
  const bool fused = can_fuse(pm, net, &view);
  if (part == 0 || part == 1) {          // the tree half of the round
    const int rc = launch_round(pm, st, fused);
    if (rc != AZMI_OK || part == 1) return rc;
  }
  if (fused) return launch_net_move(pm, view, st);
  for (uint32_t g = 0; g < pm->ep.num_groups; ++g) {
    const int rc = pm_net_forward(pm, g, net, st);
    if (rc != AZMI_OK) return rc;
  }
  return AZMI_OK;
}

int azmi_pm_net_forward_group(azmi_pm* pm, uint32_t group, azmi_net* net, void* stream) {
  if (!pm || !net) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  std::lock_guard<std::recursive_mutex> lock_(pm->mu);
  if (group >= pm->ep.num_groups) return azmi_host_fail(AZMI_ERR_INVALID, "model group %u out of range", group);
  return pm_net_forward(pm, group, net, pm->pick(stream));
}

int azmi_pm_groups(azmi_pm* pm, uint32_t* num_model_groups, uint32_t* num_seat_perms) {
  if (!pm) return azmi_host_fail(AZMI_ERR_INVALID, "null pm");
  if (num_model_groups) *num_model_groups = pm->ep.num_groups;
  if (num_seat_perms) *num_seat_perms = pm->ep.num_perms;
  return AZMI_OK;
}

int azmi_pm_perm_scores(azmi_pm* pm, uint32_t perm, float* out_scores, uint32_t* games_completed) {
  if (!pm) return azmi_host_fail(AZMI_ERR_INVALID, "null pm");
  std::lock_guard<std::recursive_mutex> lock_(pm->mu);
  if (perm >= pm->ep.num_perms) return azmi_host_fail(AZMI_ERR_INVALID, "seat permutation %u out of range", perm);
  const uint32_t S = pm->ep.S, V = pm->gi.P + 1, NP = pm->ep.num_perms;
  std::vector<float> a; std::vector<uint32_t> g;
  int rc = d2h(a, pm->ar.a_perm_scores, static_cast<size_t>(S) * NP * V, pm->last); if (rc) return rc;
  rc = d2h(g, pm->ar.a_perm_games, static_cast<size_t>(S) * NP, pm->last); if (rc) return rc;
  if (out_scores) {
    for (uint32_t i = 0; i < V; ++i) out_scores[i] = 0.0f;
    for (uint32_t s = 0; s < S; ++s) for (uint32_t i = 0; i < V; ++i) out_scores[i] += a[(static_cast<size_t>(s) * NP + perm) * V + i];
  }
  if (games_completed) { uint32_t n = 0; for (uint32_t s = 0; s < S; ++s) n += g[static_cast<size_t>(s) * NP + perm]; *games_completed = n; }
  return AZMI_OK;
}

int azmi_pm_io_buffers(azmi_pm* pm, float** dev_canonical, float** dev_v, float** dev_pi) {
  if (!pm) return azmi_host_fail(AZMI_ERR_INVALID, "null pm");
  if (dev_canonical) *dev_canonical = pm->ar.canon;
  if (dev_v) *dev_v = pm->ar.v;
  if (dev_pi) *dev_pi = pm->ar.pi;
  return AZMI_OK;
}

int azmi_pm_poll(azmi_pm* pm, void* stream, uint32_t* games_completed, uint32_t* live_slots) {
  if (!pm) return azmi_host_fail(AZMI_ERR_INVALID, "null pm");
  std::lock_guard<std::recursive_mutex> lock_(pm->mu);
  Control c;
  const int rc = azmi_host_read_ctl(pm, pm->pick(stream), &c, true);
  if (rc != AZMI_OK) return rc;
  if (games_completed) *games_completed = c.games_completed;
  if (live_slots) *live_slots = c.stop ? 0u : c.live_slots;
  return AZMI_OK;
}

// ---- PlayManager::stop / stopped / queue sizes / one slot's GameState (play_manager.h:177-186, 285-324) ----------
int azmi_pm_stop(azmi_pm* pm) {
  if (!pm) return azmi_host_fail(AZMI_ERR_INVALID, "null pm");
  pm->stopped.store(true, std::memory_order_relaxed);
  return AZMI_OK;
}
int azmi_pm_stopped(azmi_pm* pm, int* out) {
  if (!pm || !out) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  *out = pm->stopped.load(std::memory_order_relaxed) ? 1 : 0;
  return AZMI_OK;
}
// awaiting_inference_count(): leaves waiting to be handed out by build_batch / pop_games; awaiting_mcts_count(): live
// slots that hold their answer (or need none) and wait for the next round
int azmi_pm_queue_counts(azmi_pm* pm, uint32_t* awaiting_inference, uint32_t* awaiting_mcts) {
  if (!pm) return azmi_host_fail(AZMI_ERR_INVALID, "null pm");
  std::lock_guard<std::recursive_mutex> lock_(pm->mu);
  Control c;
  const int rc = azmi_host_read_ctl(pm, pm->last, &c, true);
  if (rc != AZMI_OK) return rc;
  uint32_t pend = 0;
  for (auto& q : pm->pending_g) pend += static_cast<uint32_t>(q.size());
  const uint32_t live = c.stop ? 0u : c.live_slots;
  if (awaiting_inference) *awaiting_inference = pend;
  if (awaiting_mcts) *awaiting_mcts = live > pend + pm->outstanding ? live - pend - pm->outstanding : 0u;
  return AZMI_OK;
}
// game_data(i).gs: the packed state words of slot `slot` (Connect4: stones of player 0, stones of player 1,
// turn | player << 32; Tafl family: defenders lo/hi, attackers lo/hi, king | turn << 8 | player << 24 | repetitions << 32)
int azmi_pm_slot_state(azmi_pm* pm, uint32_t slot, uint64_t* words, uint32_t cap, uint32_t* n) {
  if (!pm || !words || !n) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  std::lock_guard<std::recursive_mutex> lock_(pm->mu);
  if (slot >= pm->ep.S) return azmi_host_fail(AZMI_ERR_RANGE, "game index %u out of range", slot);
  const uint32_t W = pm->gi.state_words;
  if (cap < W + 1) return azmi_host_fail(AZMI_ERR_INVALID, "words too small");
  AZMI_HIP_TRY(hipStreamSynchronize(pm->last));
  for (uint32_t w = 0; w < W; ++w)
    AZMI_HIP_TRY(hipMemcpy(words + w, pm->ar.gs_words + static_cast<size_t>(w) * pm->ep.S + slot, 8, hipMemcpyDeviceToHost));
  uint32_t perm = 0;
  AZMI_HIP_TRY(hipMemcpy(&perm, pm->ar.perm + slot, 4, hipMemcpyDeviceToHost));
  words[W] = perm;      // GameData::perm_index, play_manager.h:41
  *n = W + 1;
  return AZMI_OK;
}

// game_data(i).gs of a game with a position history (StarGambit: position_history_, star_gambit_gs.h:745): the slot's
// history entries (the reference's own position hashes since the last deploy)
int azmi_pm_slot_history(azmi_pm* pm, uint32_t slot, uint64_t* out, uint32_t cap, uint32_t* n) {
  if (!pm || !out || !n) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  std::lock_guard<std::recursive_mutex> lock_(pm->mu);
  if (slot >= pm->ep.S) return azmi_host_fail(AZMI_ERR_RANGE, "game index %u out of range", slot);
  if (pm->game == AZMI_GAME_CONNECT4) { *n = 0; return AZMI_OK; }
  AZMI_HIP_TRY(hipStreamSynchronize(pm->last));
  uint32_t len = 0;
  AZMI_HIP_TRY(hipMemcpy(&len, pm->ar.rep_len + slot, 4, hipMemcpyDeviceToHost));
  if (len > cap) return azmi_host_fail(AZMI_ERR_INVALID, "history of %u entries does not fit %u", len, cap);
  if (len) AZMI_HIP_TRY(hipMemcpy(out, pm->ar.rep_list + static_cast<size_t>(slot) * (pm->gi.max_turns + 2), static_cast<size_t>(len) * 8, hipMemcpyDeviceToHost));
  *n = len;
  return AZMI_OK;
}

// game_data(i).canonical(): the planes of the leaf slot `slot` is waiting on (host array [C,H,W])
int azmi_pm_slot_canonical(azmi_pm* pm, uint32_t slot, float* out) {
  if (!pm || !out) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  std::lock_guard<std::recursive_mutex> lock_(pm->mu);
  if (slot >= pm->ep.S) return azmi_host_fail(AZMI_ERR_RANGE, "game index %u out of range", slot);
  const size_t CANON = static_cast<size_t>(pm->gi.C) * pm->gi.H * pm->gi.W;
  AZMI_HIP_TRY(hipStreamSynchronize(pm->last));
  AZMI_HIP_TRY(hipMemcpy(out, pm->ar.canon + slot * CANON, CANON * 4, hipMemcpyDeviceToHost));
  return AZMI_OK;
}

int azmi_pm_play(azmi_pm* pm, void* stream) {
  if (!pm) return azmi_host_fail(AZMI_ERR_INVALID, "null pm");
  if (!pm->all_random) return azmi_host_fail(AZMI_ERR_STATE, "azmi_pm_play needs EvalType::RANDOM on every seat; drive NN seats with azmi_pm_round");
  hipStream_t st = pm->pick(stream);
  for (;;) {
    if (pm->stopped.load(std::memory_order_relaxed)) return AZMI_OK;   // play_manager.cc:272
    // several threads may sit in play() at once (the reference starts mcts_workers of them): each takes the engine for a
    // chunk of rounds, all of them return when the games are done
    std::lock_guard<std::recursive_mutex> lock_(pm->mu);
    for (int r = 0; r < 32; ++r) {
      const int rc = launch_round(pm, st);
      if (rc != AZMI_OK) return rc;
    }
    Control c;
    const int rc = azmi_host_read_ctl(pm, st, &c, true);
    if (rc != AZMI_OK) return rc;
    if (c.stop) return AZMI_OK;
  }
}

int azmi_pm_scores(azmi_pm* pm, float* out) {
  if (!pm || !out) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  std::lock_guard<std::recursive_mutex> lock_(pm->mu);
  std::vector<float> a;
  const uint32_t V = pm->gi.P + 1;
  const int rc = d2h(a, pm->ar.a_scores, static_cast<size_t>(pm->ep.S) * V, pm->last);
  if (rc != AZMI_OK) return rc;
  for (uint32_t i = 0; i < V; ++i) out[i] = 0.0f;
  for (uint32_t s = 0; s < pm->ep.S; ++s) for (uint32_t i = 0; i < V; ++i) out[i] += a[static_cast<size_t>(s) * V + i];
  return AZMI_OK;
}
int azmi_pm_resign_scores(azmi_pm* pm, float* out) {
  if (!pm || !out) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  std::lock_guard<std::recursive_mutex> lock_(pm->mu);
  std::vector<float> a;
  const uint32_t V = pm->gi.P + 1;
  const int rc = d2h(a, pm->ar.a_resign, static_cast<size_t>(pm->ep.S) * V, pm->last);
  if (rc != AZMI_OK) return rc;
  for (uint32_t i = 0; i < V; ++i) out[i] = 0.0f;
  for (uint32_t s = 0; s < pm->ep.S; ++s) for (uint32_t i = 0; i < V; ++i) out[i] += a[static_cast<size_t>(s) * V + i];
  return AZMI_OK;
}

// the sums behind azmi_pm_stats, for callers that combine several engines (shards / ranks) into one set of averages:
// out[10] = game_length, games completed, total / full / fast move counts, leaf depth, entropy, fast leaf depth,
//           fast entropy, valid moves (the accumulators of play_manager.h:398-424)
int azmi_pm_stat_sums(azmi_pm* pm, double* out) {
  if (!pm || !out) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  std::lock_guard<std::recursive_mutex> lock_(pm->mu);
  const uint32_t S = pm->ep.S;
  std::vector<uint64_t> len, cnt; std::vector<double> ds; std::vector<uint32_t> games;
  int rc = d2h(len, pm->ar.a_len, S, pm->last); if (rc) return rc;
  rc = d2h(cnt, pm->ar.a_cnt, 3 * static_cast<size_t>(S), pm->last); if (rc) return rc;
  rc = d2h(ds, pm->ar.a_dsum, 5 * static_cast<size_t>(S), pm->last); if (rc) return rc;
  rc = d2h(games, pm->ar.slot_games, S, pm->last); if (rc) return rc;
  for (int i = 0; i < 10; ++i) out[i] = 0.0;
  for (uint32_t s = 0; s < S; ++s) {
    out[0] += static_cast<double>(len[s]); out[1] += games[s];
    for (int j = 0; j < 3; ++j) out[2 + j] += static_cast<double>(cnt[static_cast<size_t>(j) * S + s]);
    for (int j = 0; j < 5; ++j) out[5 + j] += ds[static_cast<size_t>(j) * S + s];
  }
  return AZMI_OK;
}

uint32_t azmi_pm_num_variants(azmi_pm* pm) { return pm && pm->game == AZMI_GAME_STARGAMBIT ? 4u : 0u; }   // num_variants(), star_gambit_gs.h:863
int azmi_pm_variant_sums(azmi_pm* pm, uint32_t variant, float* perm_scores, uint32_t* perm_games, double* sums) {
  if (!pm || !perm_scores || !perm_games || !sums) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  if (variant >= azmi_pm_num_variants(pm)) return azmi_host_fail(AZMI_ERR_RANGE, "variant %u out of range", variant);
  std::lock_guard<std::recursive_mutex> lock_(pm->mu);
  const uint32_t S = pm->ep.S, NP = pm->ep.num_perms, V = pm->gi.P + 1;
  std::vector<float> sc; std::vector<uint32_t> gm; std::vector<uint64_t> len, cnt; std::vector<double> ds;
  int rc = d2h(sc, pm->ar.a_var_scores, static_cast<size_t>(S) * 4 * NP * V, pm->last); if (rc) return rc;
  rc = d2h(gm, pm->ar.a_var_games, static_cast<size_t>(S) * 4 * NP, pm->last); if (rc) return rc;
  rc = d2h(len, pm->ar.a_var_len, static_cast<size_t>(S) * 4, pm->last); if (rc) return rc;
  rc = d2h(ds, pm->ar.a_var_dsum, static_cast<size_t>(S) * 4 * 5, pm->last); if (rc) return rc;
  rc = d2h(cnt, pm->ar.a_var_cnt, static_cast<size_t>(S) * 4 * 3, pm->last); if (rc) return rc;
  for (uint32_t i = 0; i < NP * V; ++i) perm_scores[i] = 0.0f;
  for (uint32_t i = 0; i < NP; ++i) perm_games[i] = 0;
  for (int i = 0; i < 10; ++i) sums[i] = 0.0;
  for (uint32_t s = 0; s < S; ++s) {      // slot order: a deterministic sum
    const size_t sv = static_cast<size_t>(s) * 4 + variant;
    for (uint32_t q = 0; q < NP; ++q) {
      for (uint32_t i = 0; i < V; ++i) perm_scores[q * V + i] += sc[(sv * NP + q) * V + i];
      perm_games[q] += gm[sv * NP + q];
      sums[1] += gm[sv * NP + q];
    }
    sums[0] += static_cast<double>(len[sv]);
    for (int j = 0; j < 3; ++j) sums[2 + j] += static_cast<double>(cnt[sv * 3 + j]);
    for (int j = 0; j < 5; ++j) sums[5 + j] += ds[sv * 5 + j];
  }
  return AZMI_OK;
}

int azmi_pm_stats(azmi_pm* pm, float* out) {  // play_manager.h:288-315
  if (!pm || !out) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  std::lock_guard<std::recursive_mutex> lock_(pm->mu);
  const uint32_t S = pm->ep.S;
  std::vector<uint64_t> len, cnt; std::vector<double> ds; std::vector<uint32_t> games;
  int rc = d2h(len, pm->ar.a_len, S, pm->last); if (rc) return rc;
  rc = d2h(cnt, pm->ar.a_cnt, 3 * static_cast<size_t>(S), pm->last); if (rc) return rc;
  rc = d2h(ds, pm->ar.a_dsum, 5 * static_cast<size_t>(S), pm->last); if (rc) return rc;
  rc = d2h(games, pm->ar.slot_games, S, pm->last); if (rc) return rc;
  uint64_t game_length = 0, mc[3] = {0, 0, 0}, completed = 0; double d[5] = {0, 0, 0, 0, 0};
  for (uint32_t s = 0; s < S; ++s) {
    game_length += len[s]; completed += games[s];
    for (int j = 0; j < 3; ++j) mc[j] += cnt[static_cast<size_t>(j) * S + s];
    for (int j = 0; j < 5; ++j) d[j] += ds[static_cast<size_t>(j) * S + s];
  }
  out[0] = static_cast<float>(game_length) / static_cast<float>(completed);
  out[1] = mc[1] == 0 ? 0.0f : static_cast<float>(d[0] / static_cast<double>(mc[1]));
  out[2] = mc[1] == 0 ? 0.0f : static_cast<float>(d[1] / static_cast<double>(mc[1]));
  out[3] = mc[2] == 0 ? 0.0f : static_cast<float>(d[2] / static_cast<double>(mc[2]));
  out[4] = mc[2] == 0 ? 0.0f : static_cast<float>(d[3] / static_cast<double>(mc[2]));
  out[5] = game_length == 0 ? 0.0f : static_cast<float>(mc[0]) / static_cast<float>(game_length);
  out[6] = mc[0] == 0 ? 0.0f : static_cast<float>(d[4] / static_cast<double>(mc[0]));
  return AZMI_OK;
}

// cache_hits / misses / evictions / reinserts / size / max_size summed over the model groups' caches (play_manager.h:325-366)
int azmi_pm_cache_stats(azmi_pm* pm, uint64_t out[6]) {
  if (!pm || !out) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  std::lock_guard<std::recursive_mutex> lock_(pm->mu);
  for (int i = 0; i < 6; ++i) out[i] = 0;
  if (!pm->ep.cache_on) return AZMI_OK;
  for (uint32_t g = 0; g < pm->ep.num_groups; ++g) {
    if (!pm->group_cache_counted[g]) continue;
    const CacheView& c = pm->group_caches[g];
    std::vector<unsigned long long> st; std::vector<uint32_t> state;
    int rc = d2h(st, c.stats, static_cast<size_t>(c.shards) * 4, pm->last); if (rc) return rc;
    rc = d2h(state, c.state, static_cast<size_t>(c.shards) * 8, pm->last); if (rc) return rc;
    for (uint32_t s = 0; s < c.shards; ++s) {
      for (int j = 0; j < 4; ++j) out[j] += st[static_cast<size_t>(s) * 4 + j];
      out[4] += state[static_cast<size_t>(s) * 8 + kSize];
    }
    out[5] += static_cast<uint64_t>(c.cap) * c.shards;
  }
  // the pipeline's in-epoch answer table answers probes the S3-FIFO shard counted as misses (pipe_types.h)
  const unsigned long long l0 = azmi_host_pipe_l0_hits(pm, pm->last);
  out[0] += l0; out[1] -= std::min<uint64_t>(out[1], l0);
  return AZMI_OK;
}

int azmi_pm_counters(azmi_pm* pm, uint64_t* out) {
  if (!pm || !out) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  std::lock_guard<std::recursive_mutex> lock_(pm->mu);
  const uint32_t S = pm->ep.S;
  std::vector<uint64_t> sims, evals;
  int rc = d2h(sims, pm->ar.c_sims, S, pm->last); if (rc) return rc;
  rc = d2h(evals, pm->ar.c_evals, S, pm->last); if (rc) return rc;
  Control c;
  rc = azmi_host_read_ctl(pm, pm->last, &c, true); if (rc) return rc;
  out[0] = out[1] = 0;
  for (uint32_t s = 0; s < S; ++s) { out[0] += sims[s]; out[1] += evals[s]; }
  uint64_t cs[6];
  rc = azmi_pm_cache_stats(pm, cs); if (rc) return rc;
  out[2] = cs[0]; out[3] = cs[1];
  out[4] = c.hist_rows - pm->hist_read;   // free-running 64-bit counters: the difference is the live row count
  out[5] = c.rounds;
  return AZMI_OK;
}

namespace {
// tells the device how far the host has consumed the finished-sample ring (ordered behind the rounds already queued)
int publish_hist_read(azmi_pm* pm) {
  AZMI_HIP_TRY(hipMemcpyAsync(&pm->ar.ctl->hist_read, &pm->hist_read, sizeof(pm->hist_read), hipMemcpyHostToDevice, pm->last));
  AZMI_HIP_TRY(hipStreamSynchronize(pm->last));
  return AZMI_OK;
}
}  // namespace

int azmi_pm_pop_history(azmi_pm* pm, float* canonical, float* v, float* pi, uint32_t cap, uint32_t* n) {
  if (!pm || !n) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  std::lock_guard<std::recursive_mutex> lock_(pm->mu);
  Control c;
  int rc = azmi_host_read_ctl(pm, pm->last, &c, true); if (rc) return rc;
  const uint32_t avail = static_cast<uint32_t>(c.hist_rows - pm->hist_read);
  const uint32_t take = std::min(avail, cap);
  const uint32_t CANON = pm->gi.C * pm->gi.H * pm->gi.W, V = pm->gi.P + 1, M = pm->gi.M;
  if (take) {
    const uint32_t first = static_cast<uint32_t>(pm->hist_read % pm->ep.hist_cap);
    const uint32_t n1 = std::min(take, pm->ep.hist_cap - first);
    for (int seg = 0; seg < 2; ++seg) {     // the window may wrap around the end of the ring
      const size_t r0 = seg == 0 ? first : 0, nr = seg == 0 ? n1 : take - n1, o = seg == 0 ? 0 : n1;
      if (!nr) continue;
      AZMI_HIP_TRY(hipMemcpy(canonical + o * CANON, pm->ar.h_canon + r0 * CANON, nr * CANON * 4, hipMemcpyDeviceToHost));
      AZMI_HIP_TRY(hipMemcpy(v + o * V, pm->ar.h_v + r0 * V, nr * V * 4, hipMemcpyDeviceToHost));
      AZMI_HIP_TRY(hipMemcpy(pi + o * M, pm->ar.h_pi + r0 * M, nr * M * 4, hipMemcpyDeviceToHost));
    }
    pm->hist_read += take;
    rc = publish_hist_read(pm); if (rc) return rc;
  }
  *n = take;
  return AZMI_OK;
}

int azmi_pm_history_device(azmi_pm* pm, float** dev_canonical, float** dev_v, float** dev_pi, uint32_t** dev_meta,
                           uint32_t* rows) {
  if (!pm) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  std::lock_guard<std::recursive_mutex> lock_(pm->mu);
  Control c;
  int rc = azmi_host_read_ctl(pm, pm->last, &c, true); if (rc) return rc;
  if (dev_canonical) *dev_canonical = pm->ar.h_canon;
  if (dev_v) *dev_v = pm->ar.h_v;
  if (dev_pi) *dev_pi = pm->ar.h_pi;
  if (dev_meta) *dev_meta = pm->ar.h_meta;
  if (rows) *rows = static_cast<uint32_t>(std::min<unsigned long long>(c.hist_rows, pm->ep.hist_cap));   // rows of the run while nothing has wrapped; use the window call for a ring
  return AZMI_OK;
}

int azmi_pm_history_window(azmi_pm* pm, uint32_t* first_row, uint32_t* rows, uint32_t* capacity) {
  if (!pm) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  std::lock_guard<std::recursive_mutex> lock_(pm->mu);
  Control c;
  int rc = azmi_host_read_ctl(pm, pm->last, &c, true); if (rc) return rc;
  if (first_row) *first_row = pm->ep.hist_cap ? static_cast<uint32_t>(pm->hist_read % pm->ep.hist_cap) : 0;
  if (rows) *rows = static_cast<uint32_t>(c.hist_rows - pm->hist_read);
  if (capacity) *capacity = pm->ep.hist_cap;
  return AZMI_OK;
}

int azmi_pm_history_consume(azmi_pm* pm, uint32_t rows) {
  if (!pm) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  std::lock_guard<std::recursive_mutex> lock_(pm->mu);
  Control c;
  int rc = azmi_host_read_ctl(pm, pm->last, &c, true); if (rc) return rc;
  if (rows > c.hist_rows - pm->hist_read) return azmi_host_fail(AZMI_ERR_INVALID, "history_consume: %u rows asked, %u unread", rows, static_cast<uint32_t>(c.hist_rows - pm->hist_read));
  pm->hist_read += rows;
  return publish_hist_read(pm);
}

int azmi_pm_move_log(azmi_pm* pm, uint32_t* rows, uint32_t* counts, uint32_t cap, uint32_t* n) {
  if (!pm || !n) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  std::lock_guard<std::recursive_mutex> lock_(pm->mu);
  if (!pm->ep.log_moves) return azmi_host_fail(AZMI_ERR_STATE, "move log was not enabled (azmi_engine_opts.log_moves)");
  Control c;
  int rc = azmi_host_read_ctl(pm, pm->last, &c, true); if (rc) return rc;
  const uint32_t take = std::min(std::min(c.log_rows, pm->ep.log_cap), cap);
  if (take && rows) AZMI_HIP_TRY(hipMemcpy(rows, pm->ar.log_rows, static_cast<size_t>(take) * 8 * 4, hipMemcpyDeviceToHost));
  if (take && counts) AZMI_HIP_TRY(hipMemcpy(counts, pm->ar.log_counts, static_cast<size_t>(take) * pm->gi.M * 4, hipMemcpyDeviceToHost));
  *n = take;
  return AZMI_OK;
}

// debug: keys of the leaves the last round sent to the net (0 = none), one per slot
int azmi_debug_eval_keys(azmi_pm* pm, uint64_t* out, uint32_t cap, uint32_t* n) {
  if (!pm || !out || !n) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  if (!pm->ep.cache_on) return azmi_host_fail(AZMI_ERR_STATE, "cache is off");
  std::vector<uint64_t> k;
  const int rc = d2h(k, pm->ar.cache_keys, pm->ep.S, pm->last);
  if (rc) return rc;
  const uint32_t cnt = std::min<uint32_t>(cap, pm->ep.S);
  std::memcpy(out, k.data(), static_cast<size_t>(cnt) * 8);
  *n = cnt;
  return AZMI_OK;
}

int azmi_debug_trace(azmi_pm* pm, uint64_t* out, uint32_t cap, uint32_t* n) {
  std::vector<uint64_t> t;
  const int rc = d2h(t, pm->ar.trace, 2 * static_cast<size_t>(pm->ep.trace_cap), pm->last);
  if (rc) return rc;
  const uint32_t cnt = static_cast<uint32_t>(std::min<uint64_t>(t[0], cap));
  std::memcpy(out, t.data() + 2, static_cast<size_t>(cnt) * 16);
  *n = cnt;
  return AZMI_OK;
}

int azmi_pm_slot_games(azmi_pm* pm, uint32_t* out) {
  if (!pm || !out) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  std::lock_guard<std::recursive_mutex> lock_(pm->mu);
  std::vector<uint32_t> g;
  const int rc = d2h(g, pm->ar.slot_games, pm->ep.S, pm->last);
  if (rc) return rc;
  std::memcpy(out, g.data(), g.size() * 4);
  return AZMI_OK;
}

// ---- host-buffer compatibility path ------------------------------------------------------------------
int azmi_pm_build_batch(azmi_pm* pm, float* batch, uint32_t cap, uint32_t* indices, uint32_t* n) {
  return azmi_pm_build_batch_group(pm, 0xFFFFFFFFu, batch, cap, indices, n);
}

// group == 0xFFFFFFFF: leaves of any model group (single-evaluator callers)
int azmi_pm_build_batch_group(azmi_pm* pm, uint32_t group, float* batch, uint32_t cap, uint32_t* indices, uint32_t* n) {
  if (!pm || !indices || !n) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");   // batch == NULL: pop_games_upto (indices only)
  std::lock_guard<std::recursive_mutex> lock_(pm->mu);
  *n = 0;
  if (cap == 0 || pm->stopped.load(std::memory_order_relaxed)) return AZMI_OK;
  if (group != 0xFFFFFFFFu && group >= pm->ep.num_groups) return azmi_host_fail(AZMI_ERR_INVALID, "model group %u out of range", group);
  const uint32_t S = pm->ep.S, CANON = pm->gi.C * pm->gi.H * pm->gi.W;
  hipStream_t st = pm->pick(AZMI_STREAM_ENGINE);
  int guard = 0;
  auto any_pending = [&]() { for (auto& q : pm->pending_g) if (!q.empty()) return true; return false; };
  auto mine = [&]() -> std::deque<uint32_t>* {
    if (group != 0xFFFFFFFFu) return pm->pending_g[group].empty() ? nullptr : &pm->pending_g[group];
    for (auto& q : pm->pending_g) if (!q.empty()) return &q;
    return nullptr;
  };
  while (!any_pending()) {
    if (pm->outstanding != 0) return AZMI_OK;  // rows handed out, answers not back yet
    Control c;
    int rc = azmi_host_read_ctl(pm, st, &c, true); if (rc) return rc;
    if (c.stop) return AZMI_OK;
    rc = launch_round(pm, st); if (rc) return rc;
    // the round's eval lists name exactly the leaves that need a network answer, per model group (a slot whose
    // last leaf was a cache hit or terminal is not listed); sorted so the hand-out order is deterministic
    Control c2;
    rc = azmi_host_read_ctl(pm, st, &c2, false); if (rc) return rc;
    for (uint32_t g = 0; g < pm->ep.num_groups; ++g) {
      const uint32_t cnt = std::min<uint32_t>(c2.eval_count[g], S);
      if (cnt == 0) continue;
      std::vector<uint32_t> lst;
      rc = d2h(lst, pm->ar.eval_list + static_cast<size_t>(g) * S, cnt, st); if (rc) return rc;
      std::sort(lst.begin(), lst.end());
      for (uint32_t sidx : lst) pm->pending_g[g].push_back(sidx);
    }
    if (++guard > (1 << 20)) return azmi_host_fail(AZMI_ERR_STATE, "build_batch made no progress");
  }
  std::deque<uint32_t>* q = mine();
  if (!q) return AZMI_OK;   // other groups have pending leaves, this one has none right now
  const uint32_t take = std::min<uint32_t>(cap, static_cast<uint32_t>(q->size()));
  for (uint32_t r = 0; r < take; ++r) {
    const uint32_t s = q->front();
    q->pop_front();
    indices[r] = s;
    if (batch) AZMI_HIP_TRY(hipMemcpyAsync(batch + static_cast<size_t>(r) * CANON, pm->ar.canon + static_cast<size_t>(s) * CANON,
                           CANON * 4, hipMemcpyDeviceToHost, st));
  }
  AZMI_HIP_TRY(hipStreamSynchronize(st));
  pm->outstanding += take;
  *n = take;
  return AZMI_OK;
}

int azmi_pm_update_inferences(azmi_pm* pm, const uint32_t* indices, uint32_t n, const float* v, const float* pi) {
  if (!pm || (n && (!indices || !v || !pi))) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  std::lock_guard<std::recursive_mutex> lock_(pm->mu);
  const uint32_t S = pm->ep.S, V = pm->gi.P + 1, M = pm->gi.M;
  if (n > pm->outstanding) return azmi_host_fail(AZMI_ERR_STATE, "update_inferences: more rows than build_batch handed out");
  // rows go straight to the slot-indexed device buffers: rows of other slots (cache hits written by the round
  // kernel) must not be touched, so there is no whole-buffer mirror upload
  for (uint32_t r = 0; r < n; ++r) {
    if (indices[r] >= S) return azmi_host_fail(AZMI_ERR_INVALID, "slot index out of range");
    AZMI_HIP_TRY(hipMemcpyAsync(pm->ar.v + static_cast<size_t>(indices[r]) * V, v + static_cast<size_t>(r) * V, V * 4, hipMemcpyHostToDevice, pm->stream));
    AZMI_HIP_TRY(hipMemcpyAsync(pm->ar.pi + static_cast<size_t>(indices[r]) * M, pi + static_cast<size_t>(r) * M, M * 4, hipMemcpyHostToDevice, pm->stream));
  }
  AZMI_HIP_TRY(hipStreamSynchronize(pm->stream));
  pm->outstanding -= n;
  return AZMI_OK;
}

}  // extern "C"

// ---- launches for replay.hip and mcts_object.hip: their kernels live in this device module (replay_kernels.h) --------------
void azmi_host_launch_replay(int game, const uint8_t* d_init, uint32_t init_stride, const int32_t* d_moves, uint32_t n, uint32_t len, uint64_t* d_rep,
                             uint32_t stride, uint8_t* d_valid, float* d_scores, float* d_canon, uint32_t* d_player, uint32_t* d_turn, uint64_t* d_key,
                             int32_t* d_status, uint32_t flags) {
  for_game(game,
    [&](auto tag) { using GM = decltype(tag); k_replay<GM><<<(n + 255) / 256, 256>>>(d_init, d_moves, n, len, d_valid, d_scores, d_canon, d_player, d_turn, d_key, d_status); },
    [&](auto tag) {
      using GM = decltype(tag);
      if constexpr (GM::kGameId == StarGambit::kGameId)     // its rules are wave-cooperative: a plain kernel of its own
        k_replay_sg<<<n, 64>>>(d_init, init_stride, d_moves, n, len, d_rep, stride, d_valid, d_scores, d_canon, d_player, d_turn, d_key, d_status, flags);
      else
        k_replay_tafl<GM><<<(n + 63) / 64, 64>>>(d_init, init_stride, d_moves, n, len, d_rep, stride, d_valid, d_scores, d_canon, d_player, d_turn, d_key, d_status, flags);
    });
}
void azmi_host_launch_playout(int game, const uint8_t* d_init, uint32_t init_stride, const int32_t* d_moves, uint32_t n, uint32_t len, uint64_t* d_rep,
                              uint32_t stride, const uint64_t* d_seeds, float* d_v, float* d_pi, int32_t* d_status) {
  for_game(game,
    [&](auto tag) { using GM = decltype(tag); k_playout<GM><<<(n + 63) / 64, 64>>>(d_init, d_moves, n, len, d_seeds, d_v, d_pi, d_status); },
    [&](auto tag) {
      using GM = decltype(tag);
      if constexpr (GM::kGameId == StarGambit::kGameId)
        k_playout_sg<<<n, 64>>>(d_init, init_stride, d_moves, n, len, d_rep, stride, d_seeds, d_v, d_pi, d_status);
      else
        k_playout_tafl<GM><<<(n + 63) / 64, 64>>>(d_init, init_stride, d_moves, n, len, d_rep, stride, d_seeds, d_v, d_pi, d_status);
    });
}
void azmi_host_launch_sg_image(const uint8_t* d_init, uint32_t init_stride, const int32_t* d_moves, uint32_t n, uint32_t len, uint64_t* d_rep, uint32_t stride,
                               uint8_t* d_out, uint32_t out_stride, uint32_t* d_len, int32_t* d_status, uint32_t flags) {
  k_sg_image<<<n, 64>>>(d_init, init_stride, d_moves, n, len, d_rep, stride, d_out, out_stride, d_len, d_status, flags);
}
void azmi_host_launch_rng_probe(int kind, uint64_t seed, float param, uint32_t n, uint32_t reps, uint32_t* out_u, float* out_f) {
  k_rng_probe<<<1, 64>>>(kind, seed, param, n, reps, out_u, out_f);
}

void azmi_host_launch_mcts_find_leaf(azmi_pm* pm, hipStream_t st, uint32_t* nif, const uint8_t* di, uint32_t init_bytes, const int32_t* d_moves, uint32_t len,
                                     int32_t* d_out_moves, uint32_t* d_len, int32_t* d_status) {
  for_game(pm->game,
    [&](auto tag) { using GM = decltype(tag); k_mcts_find_leaf<GM><<<1, 64, 0, st>>>(pm->ep, pm->ar, nif, di, d_moves, len, d_out_moves, d_len, d_status); },
    [&](auto tag) { using GM = decltype(tag); k_mcts_big_find_leaf<GM><<<1, 64, 0, st>>>(pm->ep, pm->ar, nif, di, init_bytes, d_moves, len, d_out_moves, d_len, d_status); });
}
void azmi_host_launch_mcts_process_result(azmi_pm* pm, hipStream_t st, uint32_t rn, float* d_f) {
  for_game(pm->game,
    [&](auto tag) { using GM = decltype(tag); k_mcts_process_result<GM><<<1, 64, 0, st>>>(pm->ep, pm->ar, rn, d_f); },
    [&](auto tag) { using GM = decltype(tag); k_mcts_big_process_result<GM><<<1, 64, 0, st>>>(pm->ep, pm->ar, rn, d_f); });
}
void azmi_host_launch_mcts_find_leaf_batched(azmi_pm* pm, hipStream_t st, const WuArrays& wu, uint32_t idx, const uint8_t* di, uint32_t init_bytes,
                                             const int32_t* d_moves, uint32_t len, int32_t* d_out_moves, uint32_t* d_len, int32_t* d_status) {
  for_game(pm->game,
    [&](auto tag) { using GM = decltype(tag); k_mcts_find_leaf_batched<GM><<<1, 64, 0, st>>>(pm->ep, pm->ar, wu, idx, di, d_moves, len, d_out_moves, d_len, d_status); },
    [&](auto tag) { using GM = decltype(tag); k_mcts_big_find_leaf_batched<GM><<<1, 64, 0, st>>>(pm->ep, pm->ar, wu, idx, di, init_bytes, d_moves, len, d_out_moves, d_len, d_status); });
}
void azmi_host_launch_mcts_process_result_batched(azmi_pm* pm, hipStream_t st, const WuArrays& wu, uint32_t leaf_index, uint32_t rn, float* d_f) {
  for_game(pm->game,
    [&](auto tag) { using GM = decltype(tag); k_mcts_process_result_batched<GM><<<1, 64, 0, st>>>(pm->ep, pm->ar, wu, leaf_index, rn, d_f); },
    [&](auto tag) { using GM = decltype(tag); k_mcts_big_process_result_batched<GM><<<1, 64, 0, st>>>(pm->ep, pm->ar, wu, leaf_index, rn, d_f); });
}
// (wide games: the live subtree moves to the idle half of the arena when the active one has filled up)
void azmi_host_launch_mcts_update_root(azmi_pm* pm, hipStream_t st, uint32_t* nif, const uint8_t* di, uint32_t init_bytes, const int32_t* d_moves, uint32_t len,
                                       uint32_t move, int32_t* d_status) {
  const uint32_t trees = pm->gi.P;
  for_game(pm->game,
    [&](auto tag) { using GM = decltype(tag); k_mcts_update_root<GM><<<1, 64, 0, st>>>(pm->ep, pm->ar, nif, di, d_moves, len, move, d_status); },
    [&](auto tag) {
      using GM = decltype(tag);
      k_mcts_big_update_root<GM><<<1, 64, 0, st>>>(pm->ep, pm->ar, nif, di, init_bytes, d_moves, len, move, d_status);
      if (pm->ep.half_nodes) k_compact<GM><<<std::min<uint32_t>(trees, kCompactBlocks), 256, 0, st>>>(pm->ep, pm->ar, trees, nif);
    });
}
// the batched search's compaction behind an update-root launch: the flagged ones of `trees` = N * P trees (search_batch.hip)
void azmi_host_launch_compact(azmi_pm* pm, hipStream_t st, uint32_t trees, uint32_t* nif) {
  if (!pm->ep.half_nodes) return;
  for_game(pm->game, [&](auto) {},
    [&](auto tag) { using GM = decltype(tag); k_compact<GM><<<std::min<uint32_t>(trees, kCompactBlocks), 256, 0, st>>>(pm->ep, pm->ar, trees, nif); });
}
void azmi_host_launch_mcts_query(azmi_pm* pm, hipStream_t st, uint32_t kind, float temp, uint32_t arg, float* d_f, uint32_t* d_u) {
  for_game(pm->game,
    [&](auto tag) { using GM = decltype(tag); k_mcts_query<GM><<<1, 64, 0, st>>>(pm->ep, pm->ar, kind, temp, arg, d_f, d_u); },
    [&](auto tag) { using GM = decltype(tag); k_mcts_big_query<GM><<<1, 64, 0, st>>>(pm->ep, pm->ar, kind, temp, arg, d_f, d_u); });
}

#ifdef AZMI_BIG_PROF
extern "C" int azmi_debug_big_prof(unsigned long long* out) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(azmi::g_big_prof), sizeof(unsigned long long) * 16) != hipSuccess) return -1;
  unsigned long long z[16] = {};
  return hipMemcpyToSymbol(HIP_SYMBOL(azmi::g_big_prof), z, sizeof(z)) == hipSuccess ? 0 : -1;
}
#endif
