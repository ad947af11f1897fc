// Frozen-set capture and net-versus-search metrics of the batched position search: the two thirds of the reference's
// frozen_eval.py around its search loop, on the device.
//   capture       _burst_capture_one_variant (frozen_eval.py:330-413) keeps every position of the games it plays whose key it has
//                 not seen.  k_sb_capture / k_sb_big_capture record the root of every live tree before a move's search: engine key,
//                 player to move, variant, at [tree][ply = log_len[tree]].
//   pool unique   the first occurrence of every key among n records, in record order (k_pool_claim, k_pool_compact): what the
//                 reference's `seen_keys` set does one position at a time.
//   net metrics   the raw forward of the roots and KL(search || net), value MAE, top-1 agreement per tree (frozen_eval.py:509-514,
//                 573-575, 649-672): k_sb_root_canon / k_sb_big_root_canon write the roots' planes into the [N, C, H, W] batch,
//                 the leaf net runs over the N rows, k_sb_net_metrics / k_sb_big_net_metrics compare in float64.
// Same grid-to-tree mapping and twins as search_batch_kernels.h; none of these kernels stores a slot back.
#pragma once
#include "search_batch_kernels.h"

namespace azmi {

// ======================= root capture (SbCaptureArrays, search_batch_types.h) ===========================================================
// one lane records; capturing the same ply again stores the same values
__device__ __forceinline__ void sb_capture_store(const SbCaptureArrays& cp, const SbPlayArrays& pl, uint32_t slot, uint64_t key, uint32_t player,
                                                 int32_t variant) {
  const uint32_t p = pl.log_len[slot];
  if (p >= pl.log_cap) return;
  const size_t at = static_cast<size_t>(slot) * pl.log_cap + p;
  cp.key[at] = key; cp.player[at] = static_cast<uint8_t>(player); cp.variant[at] = static_cast<int8_t>(variant);
  if (cp.len[slot] < p + 1) cp.len[slot] = p + 1;
}

template <class GM>
__global__ __launch_bounds__(256) void k_sb_capture(EngineParams ep, EngineArrays ar, SbArrays sb, SbPlayArrays pl, SbCaptureArrays cp, uint32_t n) {
  constexpr int G = GM::GROUP;
  const uint32_t gtid = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t slot = gtid / G, lane = gtid % G;
  if (slot >= n || sb.status[slot] != 0) return;
  SlotCtx<GM> c(ep, ar, slot, lane);
  c.load();
  if (lane == 0) sb_capture_store(cp, pl, slot, GM::key(c.gs), c.gs.player, -1);
}

template <class GM>
__global__ __launch_bounds__(64) void k_sb_big_capture(EngineParams ep, EngineArrays ar, SbArrays sb, SbPlayArrays pl, SbCaptureArrays cp, uint32_t n) {
  __shared__ BigScratch<GM> sm;
  const uint32_t slot = blockIdx.x, lane = threadIdx.x;
  if (slot >= n || sb.status[slot] != 0) return;
  BigSlot<GM> c(ep, ar, sm, slot, lane);
  c.load();
  uint64_t key;
  int32_t variant = -1;
  if constexpr (is_stargambit<GM>::value) { key = GM::key(c.gs, lane); variant = static_cast<int32_t>(GM::variant(c.gs)); }
  else key = GM::key(c.gs);
  if (lane == 0) sb_capture_store(cp, pl, slot, key, c.gs.player, variant);
}

// ======================= first occurrence of every key ================================================================================
// Open addressing over `mask + 1` slots (a power of two, at least 2 n, so a probe always ends).  A slot is claimed once, by the
// INDEX of a record (owner: kPoolEmpty -> i, one 32-bit compare-and-swap), and stands for that record's key from then on: the
// keys themselves stay in the input array, which nobody writes, so a key of 0 is a key like any other and no 64-bit atomic is
// needed.  Which record claims a slot, and therefore where a key sits, depends on scheduling; first[slot] = the smallest index
// among the records of that key (atomicMin) does not, and k_pool_compact emits exactly the records that are their key's smallest
// index, in ascending order, from one workgroup.  (kPoolEmpty, kPoolMaxRecords: search_batch_types.h)
__global__ __launch_bounds__(256) void k_pool_claim(const uint64_t* keys, const uint8_t* valid, uint32_t n, uint32_t mask, uint32_t* owner,
                                                    uint32_t* first, uint32_t* slot_of) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (!valid[i]) { slot_of[i] = kPoolEmpty; return; }
  const uint64_t key = keys[i];
  uint32_t s = static_cast<uint32_t>(mix64(key)) & mask;
  for (uint32_t probes = 0; probes <= mask; ++probes, s = (s + 1u) & mask) {
    const uint32_t o = atomicCAS(&owner[s], kPoolEmpty, i);
    if (o == kPoolEmpty || keys[o] == key) {
      atomicMin(&first[s], i);
      slot_of[i] = s;
      return;
    }
  }
  slot_of[i] = kPoolEmpty;      // (unreachable: at most n of the 2 n slots are ever claimed)
}

// record i is kept when it is the smallest index of its key; out[0 .. *n_unique) = the kept indices, ascending; one workgroup
__global__ __launch_bounds__(1024) void k_pool_compact(const uint8_t* valid, uint32_t n, const uint32_t* first, const uint32_t* slot_of, uint32_t* out,
                                                       uint32_t* counts) {
  __shared__ uint32_t s_sum[1024];
  const uint32_t tid = threadIdx.x;
  const uint32_t per = (n + 1023u) / 1024u;
  const uint32_t lo = min(n, tid * per), hi = min(n, lo + per);
  auto kept = [&](uint32_t i) { const uint32_t s = slot_of[i]; return s != kPoolEmpty && first[s] == i; };
  uint32_t cnt = 0, val = 0;
  for (uint32_t i = lo; i < hi; ++i) { cnt += kept(i) ? 1u : 0u; val += valid[i] ? 1u : 0u; }
  uint32_t row = sb_scan_1024(s_sum, cnt);
  for (uint32_t i = lo; i < hi; ++i) if (kept(i)) out[row++] = i;
  const uint32_t uniq = s_sum[1023];
  __syncthreads();
  (void)sb_scan_1024(s_sum, val);
  if (tid == 1023u) { counts[0] = uniq; counts[1] = s_sum[1023] - uniq; }
}

// ======================= net versus search ============================================================================================
// A tree takes part when it is live (status == 0) and its root is not terminal.  valid[i] says so; the row of a tree that does not
// is zeroed here, so that the net reads defined planes, and set to NaN by the metrics kernel.
template <class GM>
__global__ __launch_bounds__(256) void k_sb_root_canon(EngineParams ep, EngineArrays ar, SbArrays sb, uint32_t n, float* batch, uint8_t* valid) {
  constexpr int G = GM::GROUP;
  const uint32_t gtid = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t slot = gtid / G, lane = gtid % G;
  if (slot >= n) return;
  float* row = batch + static_cast<size_t>(slot) * GM::CANON;
  bool ok = sb.status[slot] == 0;
  if (ok) {
    SlotCtx<GM> c(ep, ar, slot, lane);
    c.load();
    ok = GM::terminal(c.gs) == 0;
    if (ok) for (uint32_t e = lane; e < static_cast<uint32_t>(GM::CANON); e += G) row[e] = GM::canonical_at(c.gs, e);
  }
  if (!ok) for (uint32_t e = lane; e < static_cast<uint32_t>(GM::CANON); e += G) row[e] = 0.0f;
  if (lane == 0) valid[slot] = ok ? 1 : 0;
}

template <class GM>
__global__ __launch_bounds__(64) void k_sb_big_root_canon(EngineParams ep, EngineArrays ar, SbArrays sb, uint32_t n, float* batch, uint8_t* valid) {
  __shared__ BigScratch<GM> sm;
  const uint32_t slot = blockIdx.x, lane = threadIdx.x;
  if (slot >= n) return;
  float* row = batch + static_cast<size_t>(slot) * GM::CANON;
  bool ok = sb.status[slot] == 0;
  if (ok) {
    BigSlot<GM> c(ep, ar, sm, slot, lane);
    c.load();
    ok = GM::terminal(c.gs) == 0;
    if (ok) {
      if constexpr (is_stargambit<GM>::value) GM::write_canonical(c.gs, row, lane, sm.rules);
      else GM::write_canonical_wave(c.gs, row, lane);
    }
  }
  if (!ok) for (uint32_t e = lane; e < static_cast<uint32_t>(GM::CANON); e += 64) row[e] = 0.0f;
  if (lane == 0) valid[slot] = ok ? 1 : 0;
}

// the comparison of one tree by its L lanes (8: a lane group, 64: a wavefront), in float64, expression for expression
// frozen_eval.py:509-514 and :653-671:
//   counts = float64(mcts.counts()); total = counts.sum(); pi_mcts = counts / total if total > 0 else 1 / M
//   kl     = sum over pi_mcts > 0 of pi_mcts * log(pi_mcts / (raw_pi + 1e-10))          (raw_pi: the net's float32, widened)
//   mae    = mean over the P + 1 entries of |raw_v - root_value()|
//   top1   = argmax(pi_mcts) == argmax(raw_pi), the first index of a maximum as in np.argmax
// counts [M] and root_value [P + 1] are the tree's rows of the read-out buffers (kinds 0 and 3), so they are what counts() and
// root_values() return.  The sums run lane-strided and are folded across the lanes: not numpy's order, a few ulp of a sum of at
// most M terms.  out[0..2] = kl, mae, top1
template <int L>
__device__ __forceinline__ void sb_net_metrics_row(uint32_t lane, uint32_t M, uint32_t V, const uint32_t* counts, const float* root_value, const float* raw_v,
                                                   const float* raw_pi, double* out) {
  double total = 0.0;
  for (uint32_t m = lane; m < M; m += L) total += static_cast<double>(counts[m]);      // (exact: integers below 2^53)
  for (int off = L / 2; off > 0; off >>= 1) total += __shfl_xor(total, off, L);
  const double uniform = 1.0 / static_cast<double>(M);
  double kl = 0.0, best_p = -1.0;
  float best_q = 0.0f;
  uint32_t arg_p = 0xFFFFFFFFu, arg_q = 0xFFFFFFFFu;
  for (uint32_t m = lane; m < M; m += L) {
    const double p = total > 0.0 ? static_cast<double>(counts[m]) / total : uniform;
    const float qf = raw_pi[m];
    if (p > 0.0) kl += p * log(p / (static_cast<double>(qf) + 1e-10));
    if (arg_p == 0xFFFFFFFFu || p > best_p) { best_p = p; arg_p = m; }
    if (arg_q == 0xFFFFFFFFu || qf > best_q) { best_q = qf; arg_q = m; }
  }
  for (int off = L / 2; off > 0; off >>= 1) {
    kl += __shfl_xor(kl, off, L);
    const double op = __shfl_xor(best_p, off, L); const uint32_t oap = __shfl_xor(arg_p, off, L);
    if (oap != 0xFFFFFFFFu && (arg_p == 0xFFFFFFFFu || op > best_p || (op == best_p && oap < arg_p))) { best_p = op; arg_p = oap; }
    const float oq = __shfl_xor(best_q, off, L); const uint32_t oaq = __shfl_xor(arg_q, off, L);
    if (oaq != 0xFFFFFFFFu && (arg_q == 0xFFFFFFFFu || oq > best_q || (oq == best_q && oaq < arg_q))) { best_q = oq; arg_q = oaq; }
  }
  if (lane != 0) return;
  double mae = 0.0;
  for (uint32_t i = 0; i < V; ++i) mae += fabs(static_cast<double>(raw_v[i]) - static_cast<double>(root_value[i]));
  out[0] = kl; out[1] = mae / static_cast<double>(V); out[2] = arg_p == arg_q ? 1.0 : 0.0;
}

// a tree that takes no part: NaN in its metrics and in its rows of the raw forward
__device__ __forceinline__ void sb_net_metrics_nan(uint32_t lane, uint32_t L, uint32_t M, uint32_t V, float* raw_v, float* raw_pi, double* out) {
  const float nanf_ = __uint_as_float(0x7FC00000u);
  for (uint32_t m = lane; m < M; m += L) raw_pi[m] = nanf_;
  if (lane < V) raw_v[lane] = nanf_;
  if (lane < 3) out[lane] = static_cast<double>(nanf_);
}

template <class GM>
__global__ __launch_bounds__(256) void k_sb_net_metrics(EngineParams ep, EngineArrays ar, uint32_t n, const uint8_t* valid, float* raw_v, float* raw_pi,
                                                        double* out, float* q_f, uint32_t stride_f, uint32_t* q_u, uint32_t stride_u) {
  constexpr int G = GM::GROUP;
  constexpr uint32_t V = GM::P + 1, M = GM::M;
  static_assert(G == 8 && V <= 3, "lane-group shuffles of width 8; root_value() has three entries");
  const uint32_t gtid = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t slot = gtid / G, lane = gtid % G;
  if (slot >= n) return;
  float* rv = raw_v + static_cast<size_t>(slot) * V;
  float* rp = raw_pi + static_cast<size_t>(slot) * M;
  double* o = out + static_cast<size_t>(slot) * 3;
  if (!valid[slot]) { sb_net_metrics_nan(lane, G, M, V, rv, rp, o); return; }
  float* f = q_f + static_cast<size_t>(slot) * stride_f;
  uint32_t* u = q_u + static_cast<size_t>(slot) * stride_u;
  mcts_query_slot<GM>(ep, ar, slot, lane, kQCounts, 0.0f, 0u, f, u);
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");      // the slot state lane 0 stored is loaded again by every lane
  mcts_query_slot<GM>(ep, ar, slot, lane, kQRootValue, 0.0f, 0u, f, u);
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");      // the rows written by single lanes are read by all of them
  sb_net_metrics_row<G>(lane, M, V, u, f, rv, rp, o);
}

template <class GM>
__global__ __launch_bounds__(64) void k_sb_big_net_metrics(EngineParams ep, EngineArrays ar, uint32_t n, const uint8_t* valid, float* raw_v, float* raw_pi,
                                                           double* out, float* q_f, uint32_t stride_f, uint32_t* q_u, uint32_t stride_u) {
  __shared__ BigScratch<GM> sm;
  constexpr uint32_t V = GM::P + 1, M = GM::M;
  static_assert(V <= 3, "root_value() has three entries");
  const uint32_t slot = blockIdx.x, lane = threadIdx.x;
  if (slot >= n) return;
  float* rv = raw_v + static_cast<size_t>(slot) * V;
  float* rp = raw_pi + static_cast<size_t>(slot) * M;
  double* o = out + static_cast<size_t>(slot) * 3;
  if (!valid[slot]) { sb_net_metrics_nan(lane, 64u, M, V, rv, rp, o); return; }
  float* f = q_f + static_cast<size_t>(slot) * stride_f;
  uint32_t* u = q_u + static_cast<size_t>(slot) * stride_u;
  mcts_big_query_slot<GM>(ep, ar, sm, slot, lane, kQCounts, 0.0f, 0u, f, u);
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  mcts_big_query_slot<GM>(ep, ar, sm, slot, lane, kQRootValue, 0.0f, 0u, f, u);
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  sb_net_metrics_row<64>(lane, M, V, u, f, rv, rp, o);
}

}  // namespace azmi
