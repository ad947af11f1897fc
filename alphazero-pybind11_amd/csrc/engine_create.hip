// Creation of one PlayManager engine: the defaults, the static description of a game, the seat tables, the HBM arrays sized once
// in azmi_pm_create* - and the library's basics (error text, ABI version, device count).  Host code only: the seed kernel is
// launched through engine.hip (engine_host.h).
// There is deliberately no CPU code path: every entry point that computes requires a HIP device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/azmi.h"
#include "cache_host.h"
#include "dev_games.h"
#include "dev_stargambit.h"
#include "engine_host.h"
#include "host_error.h"

using namespace azmi;

namespace {
thread_local std::string g_err;
}  // namespace
int azmi_host_fail(int code, const char* fmt, ...) {
  AZMI_FORMAT_ERROR(g_err, fmt);
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
  azmi_host_launch_seed(pm, opts.seed);
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

}  // extern "C"
