// The ONE device module of the lock-step engine, the MCTS object and the rules replay: the kernel headers in this order, the
// engine's own four kernels (k_assign, k_seed, k_net_move, k_delay) and one thin launch function per launch (engine_host.h) -
// nothing else.  A kernel's code depends on its module-mates and on the order they are instantiated in (DESIGN.md sections 1 and
// 8.3), so the host code of the engine lives in engine_create.hip, engine_rounds.hip, engine_results.hip and engine_hostbuf.hip,
// of the MCTS object in mcts_object.hip and of the replay in replay.hip: an edit there cannot move a kernel.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "../../include/azmi.h"
#include "engine_host.h"
#include "engine_kernels.h"
#include "leafnet_c4.h"
#include "engine_kernels_big.h"
#include "game_dispatch.h"
#include "mcts_object_kernels.h"

using namespace azmi;

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

// the round of a wide game, one wavefront per slot.  StarGambit's simulation kernel keeps the whole register file
// (k_round_big_sim1) and its one-kernel round is the plain k_round_big
template <class GM>
void launch_round_big(azmi_pm* pm, hipStream_t st) {
  constexpr bool kStarGambit = GM::kGameId == StarGambit::kGameId;
  launch_pre_round<GM>(pm, st);
  if (pm->any_playout) k_round_big<GM, true><<<pm->ep.S, 64, 0, st>>>(pm->ep, pm->ar);
  else if (pm->big_split) {
    if constexpr (kStarGambit) k_round_big_sim1<GM><<<pm->ep.S, 64, 0, st>>>(pm->ep, pm->ar);
    else k_round_big_sim<GM><<<pm->ep.S, 64, 0, st>>>(pm->ep, pm->ar);
    k_round_big_move<GM><<<pm->ep.S, 64, 0, st>>>(pm->ep, pm->ar);
  }
  else if constexpr (kStarGambit) k_round_big<GM><<<pm->ep.S, 64, 0, st>>>(pm->ep, pm->ar);
  else k_round_big_o2<GM><<<pm->ep.S, 64, 0, st>>>(pm->ep, pm->ar);
  if (pm->ep.half_nodes) k_compact<GM><<<std::min(pm->ep.S * pm->gi.P, kCompactBlocks), 256, 0, st>>>(pm->ep, pm->ar, pm->ep.S * pm->gi.P);
}

}  // namespace

// defer_moves: split rounds only - leave the move step to the fused net launch that follows (azmi_host_launch_net_move)
int azmi_host_launch_round(azmi_pm* pm, hipStream_t st, bool defer_moves) {
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
    case AZMI_GAME_TAWLBWRDD: launch_round_big<Tawlbwrdd>(pm, st); break;
    case AZMI_GAME_BRANDUBH: launch_round_big<Brandubh>(pm, st); break;
    case AZMI_GAME_OPENTAFL: launch_round_big<OpenTafl>(pm, st); break;
    case AZMI_GAME_STARGAMBIT: launch_round_big<StarGambit>(pm, st); break;
    default:
      return azmi_host_fail(AZMI_ERR_INVALID, "game %d has no device kernels", pm->game);
  }
  AZMI_HIP_TRY(hipGetLastError());
  return AZMI_OK;
}

namespace {

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
void azmi_host_launch_settle(azmi_pm* pm, hipStream_t st) { k_assign<<<1, 256, 0, st>>>(pm->ep, pm->ar, 0u); }
void azmi_host_launch_seed(azmi_pm* pm, uint64_t seed) { k_seed<<<(pm->ep.S + 255) / 256, 256, 0, pm->stream>>>(pm->ar, pm->ep.S, seed); }
int azmi_host_launch_net_move(azmi_pm* pm, const azmi_net_c4_view& view, hipStream_t st) {
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

#include "replay_kernels.h"   // (here, behind the engine's own kernels: the order of the device module is kept)

// holds a stream for about `us` microseconds (wall_clock64 ticks at 100 MHz)
extern "C" __global__ void k_delay(uint32_t us) {
  const uint64_t t0 = wall_clock64();
  while (wall_clock64() - t0 < static_cast<uint64_t>(us) * 100u) __builtin_amdgcn_s_sleep(32);
}
void azmi_host_launch_delay(uint32_t us, hipStream_t st) { k_delay<<<1, 64, 0, st>>>(us); }

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
