// Rules replay, playout and StarGambit-image kernels and the RNG probe kernel (host side: replay.hip).  Included by engine.hip alone:
// every kernel of the lock-step engine, the MCTS object and these share one device module, because the code the compiler makes of a
// kernel depends on the kernels it shares helpers with.  The kernels sit in an anonymous namespace, as they
// always have: their symbol names are part of what scripts/kernel_identity.py compares.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dev_games.h"
#include "dev_rng.h"
#include "dev_stargambit.h"

namespace {
using namespace azmi;

// ---- batched rules replay (parity tier T0) --------------------------------------------------------
template <class GM>
__global__ void k_replay(const uint8_t* init, const int32_t* moves, uint32_t n, uint32_t len, uint8_t* valid, float* scores,
                         float* canonical, uint32_t* player, uint32_t* turn, uint64_t* key, int32_t* status) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  typename GM::State s = GM::initial();
  if (init) s = GM::from_bytes(init + static_cast<size_t>(g) * GM::SERIALIZED);
  int32_t stt = 0;
  for (uint32_t i = 0; i < len; ++i) {
    const int32_t mv = moves[static_cast<size_t>(g) * len + i];
    if (mv < 0) break;
    if (mv >= GM::M || !((GM::valid_mask(s) >> mv) & 1u) || !GM::play(s, static_cast<uint32_t>(mv))) { stt = -1; break; }
  }
  if (status) status[g] = stt;
  if (valid) for (int m = 0; m < GM::M; ++m) valid[static_cast<size_t>(g) * GM::M + m] = (GM::valid_mask(s) >> m) & 1u;
  if (scores) {
    const uint32_t t = GM::terminal(s);
    for (int i = 0; i <= GM::P; ++i)
      scores[static_cast<size_t>(g) * (GM::P + 1) + i] = t == 0 ? -1.0f : (static_cast<int>(t) - 1 == i ? 1.0f : 0.0f);
  }
  if (canonical) for (int e = 0; e < GM::CANON; ++e) canonical[static_cast<size_t>(g) * GM::CANON + e] = GM::canonical_at(s, e);
  if (player) player[g] = s.player;
  if (turn) turn[g] = s.turn;
  if (key) key[g] = GM::key(s);
}

// playout_eval / playout_eval_batch (game_state.cc:10-95) for a batch of states given as start position + move list: one
// thread per state, its rollout stream seeded with seeds[g]
template <class GM>
__global__ void k_playout(const uint8_t* init, const int32_t* moves, uint32_t n, uint32_t len, const uint64_t* seeds, float* v, float* pi,
                          int32_t* status) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  typename GM::State s = GM::initial();
  if (init) s = GM::from_bytes(init + static_cast<size_t>(g) * GM::SERIALIZED);
  int32_t stt = 0;
  for (uint32_t i = 0; i < len; ++i) {
    const int32_t mv = moves[static_cast<size_t>(g) * len + i];
    if (mv < 0) break;
    if (mv >= GM::M || !((GM::valid_mask(s) >> mv) & 1u) || !GM::play(s, static_cast<uint32_t>(mv))) { stt = -1; break; }
  }
  status[g] = stt;
  if (stt) return;
  const uint32_t kl = GM::num_valid(s);
  const float ksum = static_cast<float>(kl & 0xFFu);
  for (int m = 0; m < GM::M; ++m)
    pi[static_cast<size_t>(g) * GM::M + m] = (((GM::valid_mask(s) >> m) & 1u) && ksum > 0.0f) ? 1.0f / ksum : 0.0f;
  Pcg32 roll;
  roll.seed(seeds[g]);
  uint32_t term = GM::terminal(s);
  while (term == 0) {
    const uint32_t k = GM::num_valid(s);
    if (k == 0) break;
    GM::play(s, GM::nth_valid(s, lemire_below(roll, k)));
    term = GM::terminal(s);
  }
  for (int i = 0; i <= GM::P; ++i)
    v[static_cast<size_t>(g) * (GM::P + 1) + i] = term ? ((static_cast<int>(term) - 1 == i) ? 1.0f : 0.0f) : static_cast<float>(1.0 / (GM::P + 1));
}

// StarGambit replay / rollout: ONE WAVEFRONT per game (its rules are wave-cooperative, dev_stargambit.h); the position
// history of game g lives in row g of `hist` (hist_stride entries)
struct SgListRep {
  uint64_t* list; uint32_t& len; uint32_t cap; uint32_t lane; bool overflow = false;
  __device__ __forceinline__ void clear() { len = 0; }
  __device__ __forceinline__ uint32_t push(unsigned long long k) {
    uint32_t cnt = 0;
    for (uint32_t i = lane; i < len; i += 64) cnt += list[i] == k;
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
    if (len >= cap) { overflow = true; return cnt + 1; }
    if (lane == 0) list[len] = k;
    ++len;
    StarGambit::lds_sync();
    return cnt + 1;
  }
};
__device__ __forceinline__ bool sg_start(const uint8_t* init, uint32_t stride, uint32_t g, uint32_t lane, StarGambit::State& s, uint64_t* hist,
                                         uint32_t& nh, uint32_t cap) {
  if (!init) {
    s = StarGambit::initial(0, lane);
    const unsigned long long h0 = StarGambit::position_hash(s);
    if (lane == 0) hist[0] = h0;
    nh = 1;
    StarGambit::lds_sync();
    return true;
  }
  const uint8_t* row = init + static_cast<size_t>(g) * stride;
  const uint32_t inner = uint32_t(row[21]) | uint32_t(row[22]) << 8 | uint32_t(row[23]) << 16 | uint32_t(row[24]) << 24;
  return sg_parse_image(row, 25u + inner, lane, s, hist, nh, cap);
}
// flags bit 0: play_move as the reference does (no validity check; a move that names no unit is ignored)
__global__ __launch_bounds__(64) void k_replay_sg(const uint8_t* init, uint32_t init_stride, const int32_t* moves, uint32_t n, uint32_t len,
                                                   uint64_t* hist, uint32_t hist_stride, uint8_t* valid, float* scores, float* canonical,
                                                   uint32_t* player, uint32_t* turn, uint64_t* key, int32_t* status, uint32_t flags) {
  using G = StarGambit;
  __shared__ SgScratch sm;
  const uint32_t g = blockIdx.x, lane = threadIdx.x;
  if (g >= n) return;
  G::State s;
  uint64_t* hl = hist + static_cast<size_t>(g) * hist_stride;
  uint32_t nh = 0;
  int32_t stt = sg_start(init, init_stride, g, lane, s, hl, nh, hist_stride) ? 0 : -1;
  SgListRep rep{hl, nh, hist_stride, lane};
  for (uint32_t i = 0; i < len && stt == 0; ++i) {
    const int32_t mv = moves[static_cast<size_t>(g) * len + i];
    if (mv < 0) break;
    if (mv >= G::M) { stt = -1; break; }
    if (!(flags & 1u)) {
      G::gen_valid(s, lane, sm);
      const bool ok = G::is_valid_bit(sm, static_cast<uint32_t>(mv));
      G::lds_sync();
      if (!ok) { stt = -1; break; }
    }
    G::apply_move(s, static_cast<uint32_t>(mv), lane, sm, rep);
    if (rep.overflow) { stt = -1; break; }
  }
  if (status && lane == 0) status[g] = stt;
  if (valid) {
    G::gen_valid(s, lane, sm);
    for (uint32_t m = lane; m < static_cast<uint32_t>(G::M); m += 64) valid[static_cast<size_t>(g) * G::M + m] = G::is_valid_bit(sm, m) ? 1 : 0;
    G::lds_sync();
  }
  if (scores && lane <= static_cast<uint32_t>(G::P)) {
    const uint32_t t = G::terminal(s);
    // over with no winner recorded (only reachable through a hand-made image): all zeros, like the reference's scores()
    scores[static_cast<size_t>(g) * (G::P + 1) + lane] = t == 0 ? -1.0f : ((G::winner(s) < 3 && t - 1 == lane) ? 1.0f : 0.0f);
  }
  if (canonical) G::write_canonical(s, canonical + static_cast<size_t>(g) * G::CANON, lane, sm);
  const uint64_t k = G::key(s, lane);
  if (lane == 0) {
    if (player) player[g] = s.player;
    if (turn) turn[g] = s.turn;
    if (key) key[g] = k;
  }
}
// the state itself for the Python objects: to_bytes image of game g after its moves (row of out_stride bytes, size in out_len)
__global__ __launch_bounds__(64) void k_sg_image(const uint8_t* init, uint32_t init_stride, const int32_t* moves, uint32_t n, uint32_t len,
                                                  uint64_t* hist, uint32_t hist_stride, uint8_t* out, uint32_t out_stride, uint32_t* out_len,
                                                  int32_t* status, uint32_t flags) {
  using G = StarGambit;
  __shared__ SgScratch sm;
  const uint32_t g = blockIdx.x, lane = threadIdx.x;
  if (g >= n) return;
  G::State s;
  uint64_t* hl = hist + static_cast<size_t>(g) * hist_stride;
  uint32_t nh = 0;
  int32_t stt = sg_start(init, init_stride, g, lane, s, hl, nh, hist_stride) ? 0 : -1;
  SgListRep rep{hl, nh, hist_stride, lane};
  for (uint32_t i = 0; i < len && stt == 0; ++i) {
    const int32_t mv = moves[static_cast<size_t>(g) * len + i];
    if (mv < 0) break;
    if (mv >= G::M) { stt = -1; break; }
    if (!(flags & 1u)) {
      G::gen_valid(s, lane, sm);
      const bool ok = G::is_valid_bit(sm, static_cast<uint32_t>(mv));
      G::lds_sync();
      if (!ok) { stt = -1; break; }
    }
    G::apply_move(s, static_cast<uint32_t>(mv), lane, sm, rep);
    if (rep.overflow) { stt = -1; break; }
  }
  if (lane == 0) status[g] = stt;
  // inner image (star_gambit_gs.cc:2253-2288) behind a 25-byte Unified header whose probs / pinned fields the caller fills in
  uint8_t* row = out + static_cast<size_t>(g) * out_stride;
  const uint32_t nu = G::nunits(s);
  const uint32_t inner = 4u + 9u * nu + 8u + 12u + 8u * nh;
  if (25u + inner > out_stride) { if (lane == 0) { status[g] = -2; out_len[g] = 0; } return; }
  auto wr32 = [&](uint8_t* p, uint32_t x) { p[0] = uint8_t(x); p[1] = uint8_t(x >> 8); p[2] = uint8_t(x >> 16); p[3] = uint8_t(x >> 24); };
  uint8_t* in = row + 25;
  if (lane < nu) {
    const uint32_t u = s.unit;
    uint8_t* r = in + 4 + 9 * lane;
    r[0] = uint8_t(G::u_type(u)); r[1] = uint8_t(G::u_player(u)); r[2] = uint8_t(G::u_slot(u)); r[3] = uint8_t(G::u_hp(u)); r[4] = uint8_t(G::u_facing(u));
    r[5] = uint8_t(int8_t(G::u_q(u))); r[6] = uint8_t(int8_t(G::u_r(u))); r[7] = uint8_t(G::u_moves(u)); r[8] = uint8_t(G::u_cannons(u));
  }
  for (uint32_t i = lane; i < nh; i += 64) {
    uint8_t* p = in + 4 + 9 * nu + 20 + 8 * i;
    const uint64_t x = hl[i];
    for (int k = 0; k < 8; ++k) p[k] = uint8_t(x >> (8 * k));
  }
  if (lane == 0) {
    for (int i = 0; i < 20; ++i) row[i] = 0;
    row[20] = uint8_t(G::variant(s));
    wr32(row + 21, inner);
    wr32(in, nu);
    uint8_t* t = in + 4 + 9 * nu;
    for (uint32_t pl = 0; pl < 2; ++pl) { for (uint32_t ty = 0; ty < 3; ++ty) t[pl * 4 + ty] = uint8_t(G::reserve(s, pl, ty)); t[pl * 4 + 3] = 0; }
    t[8] = uint8_t(s.player);
    wr32(t + 9, s.turn);
    t[13] = G::acted(s) ? 1 : 0; t[14] = G::over(s) ? 1 : 0;
    t[15] = uint8_t(int8_t(G::winner(s) < 3 ? int(G::winner(s)) : -1));
    wr32(t + 16, nh);
    out_len[g] = 25u + inner;
  }
}
// playout_eval (game_state.cc:10-54) for StarGambit: pi uniform over the legal moves, v the scores of a uniformly random rollout
__global__ __launch_bounds__(64) void k_playout_sg(const uint8_t* init, uint32_t init_stride, const int32_t* moves, uint32_t n, uint32_t len,
                                                    uint64_t* hist, uint32_t hist_stride, const uint64_t* seeds, float* v, float* pi, int32_t* status) {
  using G = StarGambit;
  __shared__ SgScratch sm;
  const uint32_t g = blockIdx.x, lane = threadIdx.x;
  if (g >= n) return;
  G::State s;
  uint64_t* hl = hist + static_cast<size_t>(g) * hist_stride;
  uint32_t nh = 0;
  int32_t stt = sg_start(init, init_stride, g, lane, s, hl, nh, hist_stride) ? 0 : -1;
  SgListRep rep{hl, nh, hist_stride, lane};
  for (uint32_t i = 0; i < len && stt == 0; ++i) {
    const int32_t mv = moves[static_cast<size_t>(g) * len + i];
    if (mv < 0) break;
    G::gen_valid(s, lane, sm);
    const bool ok = mv < G::M && G::is_valid_bit(sm, static_cast<uint32_t>(mv));
    G::lds_sync();
    if (!ok) { stt = -1; break; }
    G::apply_move(s, static_cast<uint32_t>(mv), lane, sm, rep);
    if (rep.overflow) { stt = -1; break; }
  }
  if (lane == 0) status[g] = stt;
  if (stt) return;
  const uint32_t kl = G::gen_valid(s, lane, sm);
  const float ksum = static_cast<float>(kl & 0xFFu);
  for (uint32_t m = lane; m < static_cast<uint32_t>(G::M); m += 64)
    pi[static_cast<size_t>(g) * G::M + m] = (G::is_valid_bit(sm, m) && ksum > 0.0f) ? 1.0f / ksum : 0.0f;
  G::lds_sync();
  Pcg32 roll;
  roll.seed(seeds[g]);
  uint32_t term = G::terminal(s);
  while (term == 0) {
    const uint32_t k = G::gen_valid(s, lane, sm);
    if (k == 0) break;
    const uint32_t r = lemire_below(roll, k);
    const unsigned long long w = lane < 27 ? sm.vbits[lane] : 0ull;
    const uint32_t cnt = static_cast<uint32_t>(__builtin_popcountll(w));
    uint32_t in = cnt;
    for (int off = 1; off < 64; off <<= 1) { const uint32_t o = __shfl_up(in, off, 64); if (lane >= static_cast<uint32_t>(off)) in += o; }
    const uint32_t lo = in - cnt;
    uint32_t mine = 0xFFFFFFFFu;
    if (r >= lo && r < lo + cnt) { unsigned long long m = w; for (uint32_t j = lo; j < r; ++j) m &= m - 1; mine = lane * 64 + static_cast<uint32_t>(__builtin_ctzll(m)); }
    const uint64_t owner = __ballot(mine != 0xFFFFFFFFu);
    const uint32_t mv = __shfl(mine, static_cast<int>(__builtin_ctzll(owner)), 64);
    G::lds_sync();
    G::apply_move(s, mv, lane, sm, rep);
    if (rep.overflow) break;
    term = G::terminal(s);
  }
  if (lane <= static_cast<uint32_t>(G::P))
    v[static_cast<size_t>(g) * (G::P + 1) + lane] = term ? ((term - 1 == lane) ? 1.0f : 0.0f) : static_cast<float>(1.0 / (G::P + 1));
}

// Tafl-family replay: one thread per game, repetition list in a global scratch row per game
// start position of game g: the game's initial position, or the reference pickle image in row g of `init` (dev_games.h
// TaflImage) with its repetition keys; false = malformed image
template <class GM>
__device__ bool tafl_start(const uint8_t* init, uint32_t stride, uint32_t g, typename GM::State& s, uint64_t* reps, uint32_t& nrep, uint32_t cap) {
  nrep = 0;
  if (!init) { s = GM::initial(); return true; }
  return tafl_parse_image<GM>(init + static_cast<size_t>(g) * stride, stride, s, reps, nrep, cap);
}
template <class GM>
__global__ void k_replay_tafl(const uint8_t* init, uint32_t init_stride, const int32_t* moves, uint32_t n, uint32_t len,
                              uint64_t* rep_scratch, uint32_t rep_stride,
                              uint8_t* valid, float* scores, float* canonical, uint32_t* player, uint32_t* turn,
                              uint64_t* key, int32_t* status, uint32_t flags) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  const bool unchecked = (flags & 1u) && GM::kGameId != Tawlbwrdd::kGameId;
  constexpr uint32_t SPAN = GM::W + GM::H;
  uint64_t* reps = rep_scratch + static_cast<size_t>(g) * rep_stride;
  uint32_t nrep = 0;
  typename GM::State s;
  int32_t stt = tafl_start<GM>(init, init_stride, g, s, reps, nrep, rep_stride) ? 0 : -1;
  if (stt != 0) s = GM::initial();
  for (uint32_t i = 0; i < len && stt == 0; ++i) {
    const int32_t mv = moves[static_cast<size_t>(g) * len + i];
    if (mv < 0) break;
    bool legal = mv < GM::M;
    if (legal && !unchecked) {
      const uint32_t from = static_cast<uint32_t>(mv) / SPAN, tgt = static_cast<uint32_t>(mv) % SPAN;
      legal = GM::own_piece(s, s.player, from) && ((GM::slide_mask(s, from) >> tgt) & 1u);
    }
    if (!legal) { stt = -1; break; }
    typename GM::State before = s;
    bool cap = false;
    bool ok;
    if constexpr (GM::kGameId == Tawlbwrdd::kGameId) ok = GM::apply_move(s, static_cast<uint32_t>(mv), &cap);
    else ok = GM::apply_move(s, static_cast<uint32_t>(mv), &cap, unchecked);
    if (!ok) { stt = -1; break; }
    if (before.turn == 0) { reps[0] = GM::rep_key(before); nrep = 1; }   // tawlbwrdd_gs.cc:253-259
    if (cap) nrep = 0;
    const uint64_t k = GM::rep_key(s);
    uint32_t cnt = 1;
    for (uint32_t j = 0; j < nrep; ++j) cnt += reps[j] == k;
    if (nrep < rep_stride) reps[nrep++] = k;
    s.rep = cnt;
  }
  if (status) status[g] = stt;
  if (valid) {
    uint8_t* vr = valid + static_cast<size_t>(g) * GM::M;
    for (int m = 0; m < GM::M; ++m) vr[m] = 0;
    for (uint32_t sq = 0; sq < static_cast<uint32_t>(GM::SQ); ++sq) {
      if (!GM::own_piece(s, s.player, sq)) continue;
      const uint32_t mask = GM::slide_mask(s, sq);
      for (uint32_t b = 0; b < SPAN; ++b) if ((mask >> b) & 1u) vr[sq * SPAN + b] = 1;
    }
  }
  if (scores) {
    const uint32_t t = GM::terminal(s);
    for (int i = 0; i <= GM::P; ++i)
      scores[static_cast<size_t>(g) * (GM::P + 1) + i] = t == 0 ? -1.0f : (static_cast<int>(t) - 1 == i ? 1.0f : 0.0f);
  }
  if (canonical) for (int e = 0; e < GM::CANON; ++e) canonical[static_cast<size_t>(g) * GM::CANON + e] = GM::canonical_at(s, e);
  if (player) player[g] = s.player;
  if (turn) turn[g] = s.turn;
  if (key) key[g] = GM::key(s);
}

// playout_eval / playout_eval_batch for the Tafl family: one thread per state; the repetition list of the game record and
// of the rollout lives in the thread's scratch row (rep_stride >= record length + max_turns + 2 entries)
template <class GM>
__global__ void k_playout_tafl(const uint8_t* init, uint32_t init_stride, const int32_t* moves, uint32_t n, uint32_t len,
                               uint64_t* rep_scratch, uint32_t rep_stride, const uint64_t* seeds, float* v, float* pi, int32_t* status) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  constexpr uint32_t SPAN = GM::W + GM::H;
  uint64_t* reps = rep_scratch + static_cast<size_t>(g) * rep_stride;
  uint32_t nrep = 0;
  typename GM::State s;
  if (!tafl_start<GM>(init, init_stride, g, s, reps, nrep, rep_stride)) { if (status) status[g] = -1; return; }
  auto step = [&](uint32_t mv, bool unchecked) -> bool {     // one move with the reference's repetition bookkeeping
    typename GM::State before = s;
    bool cap = false, ok;
    if constexpr (GM::kGameId == Tawlbwrdd::kGameId) ok = GM::apply_move(s, mv, &cap);
    else ok = GM::apply_move(s, mv, &cap, unchecked);
    if (!ok) return false;
    if (before.turn == 0) { reps[0] = GM::rep_key(before); nrep = 1; }
    if (cap) nrep = 0;
    const uint64_t k = GM::rep_key(s);
    uint32_t cnt = 1;
    for (uint32_t j = 0; j < nrep; ++j) cnt += reps[j] == k;
    if (nrep < rep_stride) reps[nrep++] = k;
    s.rep = cnt;
    return true;
  };
  int32_t stt = 0;
  const bool unchecked = GM::kGameId != Tawlbwrdd::kGameId;       // the objects of these games replay like the reference's play_move
  for (uint32_t i = 0; i < len; ++i) {
    const int32_t mv = moves[static_cast<size_t>(g) * len + i];
    if (mv < 0) break;
    if (mv >= GM::M || !step(static_cast<uint32_t>(mv), unchecked)) { stt = -1; break; }
  }
  status[g] = stt;
  if (stt) return;
  auto count_moves = [&]() {
    uint32_t k = 0;
    for (uint32_t sq = 0; sq < static_cast<uint32_t>(GM::SQ); ++sq)
      if (GM::own_piece(s, s.player, sq)) k += __builtin_popcount(GM::slide_mask(s, sq));
    return k;
  };
  {   // policy: uniform over the leaf's legal moves, the u8 sum of the mask wraps mod 256 like dumb_eval
    float* pr = pi + static_cast<size_t>(g) * GM::M;
    for (int m = 0; m < GM::M; ++m) pr[m] = 0.0f;
    const float ksum = static_cast<float>(count_moves() & 0xFFu);
    if (ksum > 0.0f)
      for (uint32_t sq = 0; sq < static_cast<uint32_t>(GM::SQ); ++sq) {
        if (!GM::own_piece(s, s.player, sq)) continue;
        const uint32_t mask = GM::slide_mask(s, sq);
        for (uint32_t b = 0; b < SPAN; ++b) if ((mask >> b) & 1u) pr[sq * SPAN + b] = 1.0f / ksum;
      }
  }
  Pcg32 roll;
  roll.seed(seeds[g]);
  uint32_t term = GM::terminal(s);
  while (term == 0) {
    const uint32_t k = count_moves();
    if (k == 0) break;
    uint32_t r = lemire_below(roll, k), mv = 0;
    for (uint32_t sq = 0; sq < static_cast<uint32_t>(GM::SQ); ++sq) {    // the r-th legal move in ascending move order
      if (!GM::own_piece(s, s.player, sq)) continue;
      uint32_t mask = GM::slide_mask(s, sq);
      const uint32_t c = __builtin_popcount(mask);
      if (r >= c) { r -= c; continue; }
      for (uint32_t j = 0; j < r; ++j) mask &= mask - 1;
      mv = sq * SPAN + __builtin_ctz(mask);
      break;
    }
    if (!step(mv, false)) break;
    term = GM::terminal(s);
  }
  for (int i = 0; i <= GM::P; ++i)
    v[static_cast<size_t>(g) * (GM::P + 1) + i] = term ? ((static_cast<int>(term) - 1 == i) ? 1.0f : 0.0f) : static_cast<float>(1.0 / (GM::P + 1));
}

// ---- RNG probe: the device RNG layer on its own (parity tier "RNG") -------------------------------
__global__ void k_rng_probe(int kind, uint64_t seed, float param, uint32_t n, uint32_t reps, uint32_t* out_u, float* out_f) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  Pcg32 g;
  g.seed(seed);
  if (kind == 0) {
    for (uint32_t i = 0; i < n; ++i) out_u[i] = g.next();
  } else if (kind == 1) {  // std::shuffle of iota(n), `reps` times from one stream (one lane, plain arrays)
    for (uint32_t r = 0; r < reps; ++r) {
      uint32_t* a = out_u + static_cast<size_t>(r) * n;
      for (uint32_t i = 0; i < n; ++i) a[i] = i;
      if (n > 1) {
        uint32_t i = 1;
        if ((n & 1u) == 0) { const uint32_t j = lemire_below(g, 2); const uint32_t t = a[i]; a[i] = a[j]; a[j] = t; ++i; }
        while (i != n) {
          const uint32_t sr = i + 1, b1 = sr + 1;
          const uint32_t x = lemire_below(g, sr * b1);
          const uint32_t p0 = x / b1, p1 = x % b1;
          uint32_t t = a[i]; a[i] = a[p0]; a[p0] = t; ++i;
          t = a[i]; a[i] = a[p1]; a[p1] = t; ++i;
        }
      }
    }
  } else if (kind == 2) {
    for (uint32_t i = 0; i < n; ++i) out_f[i] = canonical01(g) * 1.0f + 0.0f;
  } else if (kind == 3) {  // one gamma object across draws (mcts.cc:435-440)
    Gamma d(param);
    for (uint32_t i = 0; i < n; ++i) out_f[i] = d.draw(g);
  } else if (kind == 4) {  // fresh gamma object per draw (mcts.cc:430)
    for (uint32_t i = 0; i < n; ++i) { Gamma d(param); out_f[i] = d.draw(g); }
  }
}

}  // namespace
