// Opening trees by reach probability on the batched position search: the step from N searched roots to the next level's frontier,
// the part of the reference's opening_analysis.py build_tree (:261-355) between two searches, on the device.
//   policy   evaluate_node's raw_pi (opening_analysis.py:233-257), apply_temperature (play.py:256-266), the entropy of the sampling
//            distribution and the kept set `reach * p >= min_reach` of every tree, in float64 (k_sb_frontier_policy /
//            k_sb_big_frontier_policy)
//   scan     first_child[i] = the kept moves of the trees before i (k_frontier_scan, one workgroup)
//   emit     one record per kept move, in (tree, action) order: the root state with the action played on a copy - the successor's
//            engine key, player to move, variant, terminal flag and scores() (k_sb_frontier_emit / k_sb_big_frontier_emit)
// Same grid-to-tree mapping and twins as search_pool_kernels.h; none of these kernels stores a slot back.
#pragma once
#include "search_pool_kernels.h"

namespace azmi {

// (the arrays: SbFrontierArrays, search_batch_types.h)

// The sum of one float64 term per move over the L lanes of a tree; `acc` is the lane's own strided sum.  With M <= L lane m holds
// term m alone and the terms are added in ascending move order, numpy's order for fewer than 8 terms; otherwise the lanes' sums
// are folded: not numpy's order, a few ulp of a sum of at most M terms.
template <int L>
__device__ __forceinline__ double fr_sum(uint32_t M, double acc) {
  if (M <= static_cast<uint32_t>(L)) {
    double s = 0.0;
    for (uint32_t m = 0; m < M; ++m) s += __shfl(acc, static_cast<int>(m), L);
    return s;
  }
  for (int off = L / 2; off > 0; off >>= 1) acc += __shfl_xor(acc, off, L);
  return acc;
}

// the policies of one searched live root by its L lanes, expression for expression:
//   raw_pi       gumbel: ip = float64(gumbel_improved_policy()); ip / ip.sum() if ip.sum() > 0                (opening_analysis.py:238-244)
//                else counts = float64(counts()); counts / total if total > 0; else valids / valids.sum()    (:246-257)
//   sampling_pi  temp == 0: one-hot at np.argmax(raw_pi); temp == 1: raw_pi; else s = (raw_pi + 1e-10) ** (1 / temp); s / s.sum()
//   entropy      -sum over sampling_pi > 0 of p * log(p)                                                      (:328-329)
//   keep[a]      sampling_pi[a] > 0 and reach * sampling_pi[a] >= min_reach (:340-346) and a is legal: the reference would raise from
//                play_move where the `+ 1e-10` branch gives an illegal move its tiny mass
// counts [M] and gp [M] are the tree's rows of the read-out buffers (kinds 0 and 6).  A lane writes and reads its own strided
// entries of the rows only.  -> the number of kept moves
template <int L, class Legal>
__device__ __forceinline__ uint32_t fr_policy_row(uint32_t lane, uint32_t M, bool gumbel, const uint32_t* counts, const float* gp, Legal legal, double reach,
                                                  double temp, double min_reach, double* raw_pi, double* samp_pi, uint8_t* keep, double* entropy) {
  double total = 0.0, gsum = 0.0;
  for (uint32_t m = lane; m < M; m += L) {
    total += static_cast<double>(counts[m]);      // (exact: integers below 2^53)
    if (gumbel) gsum += static_cast<double>(gp[m]);
  }
  total = fr_sum<L>(M, total);
  if (gumbel) gsum = fr_sum<L>(M, gsum);
  const bool use_g = gsum > 0.0;
  double n_legal = 0.0;
  if (!use_g && !(total > 0.0)) {      // no visits below the root (one descent only expands it): uniform over the legal moves
    for (uint32_t m = lane; m < M; m += L) n_legal += legal(m) ? 1.0 : 0.0;
    n_legal = fr_sum<L>(M, n_legal);
  }
  auto raw = [&](uint32_t m) -> double {
    if (use_g) return static_cast<double>(gp[m]) / gsum;
    if (total > 0.0) return static_cast<double>(counts[m]) / total;
    return (n_legal > 0.0 && legal(m)) ? 1.0 / n_legal : 0.0;
  };
  const double inv_t = temp != 0.0 ? 1.0 / temp : 0.0;
  double ssum = 0.0;
  uint32_t arg = 0xFFFFFFFFu;
  if (temp == 0.0) {      // the first index of a maximum, as in np.argmax
    double best = -1.0;
    for (uint32_t m = lane; m < M; m += L) { const double r = raw(m); if (arg == 0xFFFFFFFFu || r > best) { best = r; arg = m; } }
    for (int off = L / 2; off > 0; off >>= 1) {
      const double ob = __shfl_xor(best, off, L); const uint32_t oa = __shfl_xor(arg, off, L);
      if (oa != 0xFFFFFFFFu && (arg == 0xFFFFFFFFu || ob > best || (ob == best && oa < arg))) { best = ob; arg = oa; }
    }
  } else if (temp != 1.0) {
    for (uint32_t m = lane; m < M; m += L) ssum += pow(raw(m) + 1e-10, inv_t);
    ssum = fr_sum<L>(M, ssum);
  }
  double ent = 0.0;
  uint32_t cnt = 0;
  for (uint32_t m = lane; m < M; m += L) {
    const double r = raw(m);
    const double p = temp == 0.0 ? (m == arg ? 1.0 : 0.0) : temp == 1.0 ? r : pow(r + 1e-10, inv_t) / ssum;
    raw_pi[m] = r; samp_pi[m] = p;
    if (p > 0.0) ent += p * log(p);
    const bool k = p > 0.0 && reach * p >= min_reach && legal(m);
    keep[m] = k ? 1 : 0;
    cnt += k ? 1u : 0u;
  }
  ent = fr_sum<L>(M, ent);
  for (int off = L / 2; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, L);
  if (lane == 0) *entropy = ent == 0.0 ? 0.0 : -ent;
  return cnt;
}

// a tree without policies (kinds 1 and 2): zero rows, no kept move
__device__ __forceinline__ void fr_zero_rows(uint32_t lane, uint32_t L, uint32_t M, double* raw_pi, double* samp_pi, uint8_t* keep) {
  for (uint32_t m = lane; m < M; m += L) { raw_pi[m] = 0.0; samp_pi[m] = 0.0; keep[m] = 0; }
}

// GameState::scores() of a state whose terminal code is `term` (0: running, all zeros), entry j
__device__ __forceinline__ float fr_score(uint32_t term, bool scored, uint32_t j) { return (term != 0 && scored && term - 1 == j) ? 1.0f : 0.0f; }

// one lane writes record r (r < max_children)
__device__ __forceinline__ void fr_store_record(const SbFrontierArrays& fr, uint32_t r, uint32_t V, uint32_t tree, uint32_t action, double child_reach,
                                                uint64_t key, uint32_t player, int32_t variant, uint32_t term, bool scored) {
  fr.parent[r] = tree; fr.action[r] = action; fr.child_reach[r] = child_reach; fr.child_key[r] = key;
  fr.child_player[r] = static_cast<uint8_t>(player); fr.child_variant[r] = static_cast<int8_t>(variant);
  fr.child_terminal[r] = term != 0 ? 1 : 0;
  for (uint32_t j = 0; j < V; ++j) fr.child_scores[static_cast<size_t>(r) * V + j] = fr_score(term, scored, j);
}

template <class GM>
__global__ __launch_bounds__(256) void k_sb_frontier_policy(EngineParams ep, EngineArrays ar, SbArrays sb, SbFrontierArrays fr, uint32_t n, double min_reach,
                                                            float* q_f, uint32_t stride_f, uint32_t* q_u, uint32_t stride_u) {
  constexpr int G = GM::GROUP;
  constexpr uint32_t V = GM::P + 1, M = GM::M;
  static_assert(G == 8 && V == 3, "lane-group shuffles of width 8; root_value() and scores() have three entries");
  const uint32_t gtid = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t slot = gtid / G, lane = gtid % G;
  if (slot >= n) return;
  double* rp = fr.raw_pi + static_cast<size_t>(slot) * M;
  double* sp = fr.samp_pi + static_cast<size_t>(slot) * M;
  uint8_t* kp = fr.keep + static_cast<size_t>(slot) * M;
  double* val = fr.value + static_cast<size_t>(slot) * 3;
  const double reach = fr.reach[slot];
  uint32_t kind = 2, term = 0;
  uint64_t key = 0;
  typename GM::State root = GM::initial();
  if (sb.status[slot] == 0 && reach != 0.0) {
    SlotCtx<GM> c(ep, ar, slot, lane);
    c.load();
    root = c.gs;
    term = GM::terminal(root);
    key = GM::key(root);
    kind = term != 0 ? 1u : 0u;
  }
  uint32_t cnt = 0;
  if (kind == 0) {
    float* f = q_f + static_cast<size_t>(slot) * stride_f;
    uint32_t* u = q_u + static_cast<size_t>(slot) * stride_u;
    mcts_query_slot<GM>(ep, ar, slot, lane, kQCounts, 0.0f, 0u, f, u);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");      // the slot state lane 0 stored is loaded again by every lane
    if (ep.gumbel_on) {
      mcts_query_slot<GM>(ep, ar, slot, lane, kQGumbelPolicy, 0.0f, 0u, f, u);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    }
    const uint32_t vm = GM::valid_mask(root);
    double ent = 0.0;
    cnt = fr_policy_row<G>(lane, M, ep.gumbel_on != 0, u, f, [&](uint32_t m) { return ((vm >> m) & 1u) != 0; }, reach, fr.temp[slot], min_reach, rp, sp, kp,
                           &ent);
    if (lane == 0) fr.entropy[slot] = ent;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");      // every lane has read its entries of f: root_value() goes to f[0..2]
    mcts_query_slot<GM>(ep, ar, slot, lane, kQRootValue, 0.0f, 0u, f, u);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");      // the row lane 0 wrote is read by lanes 0..2
    if (lane < V) val[lane] = static_cast<double>(f[lane]);
  } else {
    fr_zero_rows(lane, G, M, rp, sp, kp);
    if (lane < V) val[lane] = static_cast<double>(fr_score(term, true, lane));
    if (lane == 0) fr.entropy[slot] = 0.0;
  }
  if (lane == 0) { fr.kind[slot] = static_cast<uint8_t>(kind); fr.key[slot] = key; fr.kept[slot] = cnt; }
}

template <class GM>
__global__ __launch_bounds__(64) void k_sb_big_frontier_policy(EngineParams ep, EngineArrays ar, SbArrays sb, SbFrontierArrays fr, uint32_t n, double min_reach,
                                                               float* q_f, uint32_t stride_f, uint32_t* q_u, uint32_t stride_u) {
  __shared__ BigScratch<GM> sm;
  constexpr uint32_t V = GM::P + 1, M = GM::M;
  static_assert(V == 3, "root_value() and scores() have three entries");
  const uint32_t slot = blockIdx.x, lane = threadIdx.x;
  if (slot >= n) return;
  double* rp = fr.raw_pi + static_cast<size_t>(slot) * M;
  double* sp = fr.samp_pi + static_cast<size_t>(slot) * M;
  uint8_t* kp = fr.keep + static_cast<size_t>(slot) * M;
  double* val = fr.value + static_cast<size_t>(slot) * 3;
  const double reach = fr.reach[slot];
  uint32_t kind = 2, term = 0, cnt = 0;
  uint64_t key = 0;
  bool scored = true;
  if (sb.status[slot] == 0 && reach != 0.0) {
    BigSlot<GM> c(ep, ar, sm, slot, lane);
    c.load();
    term = GM::terminal(c.gs);
    if constexpr (is_stargambit<GM>::value) { key = GM::key(c.gs, lane); scored = GM::winner(c.gs) < 3; }
    else key = GM::key(c.gs);
    kind = term != 0 ? 1u : 0u;
    if (kind == 0) {
      float* f = q_f + static_cast<size_t>(slot) * stride_f;
      uint32_t* u = q_u + static_cast<size_t>(slot) * stride_u;
      mcts_big_query_slot<GM>(ep, ar, sm, slot, lane, kQCounts, 0.0f, 0u, f, u);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
      if (ep.gumbel_on) {
        mcts_big_query_slot<GM>(ep, ar, sm, slot, lane, kQGumbelPolicy, 0.0f, 0u, f, u);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
      }
      double ent = 0.0;
      const double temp = fr.temp[slot];
      if constexpr (is_stargambit<GM>::value) {      // the dense bit map of valid_moves() (dev_stargambit.h), behind the read-outs that share the scratch
        GM::gen_valid(c.gs, lane, sm.rules);
        c.sync();
        cnt = fr_policy_row<64>(lane, M, ep.gumbel_on != 0, u, f, [&](uint32_t m) { return GM::is_valid_bit(sm.rules, m); }, reach, temp, min_reach, rp, sp,
                                kp, &ent);
      } else {      // move = from * (W + H) + slide: legal when the mover owns `from` and the slide is one of its mask (expand_node's list)
        const typename GM::State& gs = c.gs;
        cnt = fr_policy_row<64>(lane, M, ep.gumbel_on != 0, u, f,
                                [&](uint32_t m) {
                                  const uint32_t sq = m / (GM::W + GM::H), b = m % (GM::W + GM::H);
                                  return sq < static_cast<uint32_t>(GM::SQ) && GM::own_piece(gs, gs.player, sq) && ((GM::slide_mask(gs, sq) >> b) & 1u) != 0;
                                },
                                reach, temp, min_reach, rp, sp, kp, &ent);
      }
      if (lane == 0) fr.entropy[slot] = ent;
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");      // every lane has read its entries of f: root_value() goes to f[0..2]
      mcts_big_query_slot<GM>(ep, ar, sm, slot, lane, kQRootValue, 0.0f, 0u, f, u);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
      if (lane < V) val[lane] = static_cast<double>(f[lane]);
    }
  }
  if (kind != 0) {
    fr_zero_rows(lane, 64u, M, rp, sp, kp);
    if (lane < V) val[lane] = static_cast<double>(fr_score(term, scored, lane));
    if (lane == 0) fr.entropy[slot] = 0.0;
  }
  if (lane == 0) { fr.kind[slot] = static_cast<uint8_t>(kind); fr.key[slot] = key; fr.kept[slot] = cnt; }
}

// first_child[i] = kept[0] + ... + kept[i - 1], first_child[n] = *total = the number of records; one workgroup, each thread
// takes ceil(n / 1024) trees as in k_pool_compact.  (A template, so that it is emitted where it is first launched, behind every
// kernel that was there before: a plain kernel is emitted where it is defined and moves the code behind it.)
template <uint32_t T>
__global__ __launch_bounds__(T) void k_frontier_scan(const uint32_t* kept, uint32_t n, uint32_t* first_child, uint32_t* total) {
  static_assert(T == 1024, "sb_scan_1024 scans the counts of 1024 threads");
  __shared__ uint32_t s_sum[1024];
  const uint32_t tid = threadIdx.x;
  const uint32_t per = (n + 1023u) / 1024u;
  const uint32_t lo = min(n, tid * per), hi = min(n, lo + per);
  uint32_t cnt = 0;
  for (uint32_t i = lo; i < hi; ++i) cnt += kept[i];
  uint32_t row = sb_scan_1024(s_sum, cnt);
  for (uint32_t i = lo; i < hi; ++i) { first_child[i] = row; row += kept[i]; }
  if (tid == 1023u) { first_child[n] = s_sum[1023]; *total = s_sum[1023]; }
}

// lane a of the group plays move a on its own copy of the root state
template <class GM>
__global__ __launch_bounds__(256) void k_sb_frontier_emit(EngineParams ep, EngineArrays ar, SbFrontierArrays fr, uint32_t n) {
  constexpr int G = GM::GROUP;
  constexpr uint32_t V = GM::P + 1, M = GM::M;
  const uint32_t gtid = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t slot = gtid / G, lane = gtid % G;
  if (slot >= n || fr.kept[slot] == 0) return;
  SlotCtx<GM> c(ep, ar, slot, lane);
  c.load();
  const bool k = lane < M && fr.keep[static_cast<size_t>(slot) * M + lane] != 0;
  const uint32_t before = c.group_ballot(k) & ((1u << lane) - 1u);
  if (!k) return;
  const uint32_t r = fr.first_child[slot] + static_cast<uint32_t>(__builtin_popcount(before));
  if (r >= fr.max_children) return;
  typename GM::State st = c.gs;
  (void)GM::play(st, lane);      // (a kept move is legal)
  fr_store_record(fr, r, V, slot, lane, fr.reach[slot] * fr.samp_pi[static_cast<size_t>(slot) * M + lane], GM::key(st), st.player, -1, GM::terminal(st), true);
}

// the wavefront plays the kept moves one after the other, in ascending order: a ballot over 64 moves at a time numbers them.  Every
// move starts from the root state with an empty path-local repetition list, as the first level of a descent does
template <class GM>
__global__ __launch_bounds__(64) void k_sb_big_frontier_emit(EngineParams ep, EngineArrays ar, SbFrontierArrays fr, uint32_t n) {
  __shared__ BigScratch<GM> sm;
  constexpr uint32_t V = GM::P + 1, M = GM::M;
  const uint32_t slot = blockIdx.x, lane = threadIdx.x;
  if (slot >= n || fr.kept[slot] == 0) return;
  BigSlot<GM> c(ep, ar, sm, slot, lane);
  c.load();
  const uint8_t* keep = fr.keep + static_cast<size_t>(slot) * M;
  const double* sp = fr.samp_pi + static_cast<size_t>(slot) * M;
  const double reach = fr.reach[slot];
  uint32_t r = fr.first_child[slot];
  for (uint32_t base = 0; base < M && r < fr.max_children; base += 64) {
    const uint32_t m = base + lane;
    uint64_t bits = __ballot(m < M && keep[m] != 0);
    while (bits != 0 && r < fr.max_children) {
      const uint32_t a = base + static_cast<uint32_t>(__builtin_ctzll(bits));
      bits &= bits - 1;
      typename GM::State st = c.gs;
      uint32_t len = 0;
      bool base_valid = true;
      const bool ok = c.step_state(st, a, c.path_list(), len, base_valid, c.glen);      // (false: the engine's overflow bit is raised, the read-out reports it)
      uint64_t key;
      int32_t variant = -1;
      bool scored = true;
      if constexpr (is_stargambit<GM>::value) { key = GM::key(st, lane); variant = static_cast<int32_t>(GM::variant(st)); scored = GM::winner(st) < 3; }
      else key = GM::key(st);
      if (lane == 0) fr_store_record(fr, r, V, slot, a, reach * sp[a], key, st.player, variant, ok ? GM::terminal(st) : 0u, scored);
      ++r;
      c.sync();
    }
  }
}

}  // namespace azmi
