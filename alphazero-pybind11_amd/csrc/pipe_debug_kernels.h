// Kernels of the pipeline's diagnostic entry points (pipeline_debug.hip): the lane-group primitives of the descent and expand_node on
// their own, and the synthetic requests that let the net side drain a ring alone.  Included by pipeline.hip alone, last.
#pragma once
#include "pipe_tree_kernels.h"

// ---- diagnostics: the lane-group primitives of the descent, one wavefront (eight groups) per row ------------------------------------
namespace azmi {
__global__ __launch_bounds__(64) void k_debug_group_select(const uint32_t* k8, const uint32_t* n64, const float* q64, const float* p64, const float* vpar8,
                                                           const uint32_t* npar8, const float* fpu8, const float* cpuct8, const unsigned long long* pred,
                                                           float* sum64, uint32_t* best64, uint32_t* all64) {
  const uint32_t wlane = threadIdx.x & 63u, row = blockIdx.x;
  const size_t li = static_cast<size_t>(row) * 64u + wlane, gi = static_cast<size_t>(row) * 8u + (wlane >> 3);
  EngineParams ep{};
  EngineArrays ar{};
  ep.cpuct = cpuct8[gi];
  SlotCtx<Connect4> c(ep, ar, 0u, wlane & 7u);
  const uint32_t k = k8[gi], n_l = n64[li];
  const float q_l = q64[li], p_l = p64[li];
  sum64[li] = c.seqsum8((c.lane < k && n_l > 0u) ? p_l : 0.0f);
  best64[li] = c.select_child(k, n_l, q_l, p_l, vpar8[gi], npar8[gi], fpu8[gi]);
  const bool mine = (pred[row] >> wlane) & 1ull;
  all64[li] = (c.group_all(mine) ? 1u : 0u) | (c.group_any(mine) ? 2u : 0u);
}
}  // namespace azmi

// ---- diagnostics: expand_node on its own, one wavefront (eight groups) per row, `reps` positions per group one after the other ------
namespace azmi {
template <bool LANE_PACK>
__global__ __launch_bounds__(64) void k_debug_group_expand(uint32_t reps, uint32_t cap, NodeRec* nodes, Control* ctl, const uint64_t* bb0, const uint64_t* bb1,
                                                           const uint32_t* player, const uint64_t* rng_in, uint32_t* words, uint64_t* rng_out) {
  const uint32_t wlane = threadIdx.x & 63u, grp = wlane >> 3, lane = wlane & 7u;
  const uint32_t slot = blockIdx.x * 8u + grp;
  EngineParams ep{};
  EngineArrays ar{};
  ep.S = gridDim.x * 8u; ep.cap = cap;
  ar.nodes = nodes; ar.ctl = ctl;
  SlotCtx<Connect4> c(ep, ar, slot, lane);
  c.t_bump[0] = reps; c.t_bump[1] = 0u;       // (tree 0 of the slot: nodes 0 .. reps-1 are the parents, the children follow)
  for (uint32_t r = 0; r < reps; ++r) {
    const size_t pi = static_cast<size_t>(slot) * reps + r;
    Connect4::State st{{bb0[pi], bb1[pi]}, 0u, player[pi]};
    c.rng.state = rng_in[pi];
    uint32_t c0 = 0xFFFFFFFFu, k = 0xFFFFFFFFu, mv = 0xFFFFFFFFu;
    const bool ok = c.template expand_node<LANE_PACK>(0u, r, st, meta_pack(0, 0, r & 7u, st.player, 0), c0, k, &mv);
    const size_t o = pi * 8u + lane;
    words[o * 4u + 0u] = mv; words[o * 4u + 1u] = c0; words[o * 4u + 2u] = k; words[o * 4u + 3u] = ok ? 1u : 0u;
    rng_out[o] = c.rng.state;
    if (!ok) break;
  }
}
}  // namespace azmi

// ---- diagnostics: the net side alone -----------------------------------------------------------------------------------------
namespace azmi {
__global__ void k_pipe_fill(PipeArrays pa, uint32_t n, uint32_t S, uint64_t seed) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) { pa.ep->stop = 1u; }
  if (i >= n) return;
  const uint32_t pos = pa.ctl->tail + i;
  // a random legal-looking position: stones dropped column by column
  uint64_t x = mix64(seed + i);
  uint64_t b0 = 0, b1 = 0;
  uint32_t player = 0;
  for (uint32_t w = 0; w < 7; ++w) {
    const uint32_t hgt = static_cast<uint32_t>(x % 5u); x = mix64(x);
    for (uint32_t j = 0; j < hgt; ++j) {
      const uint64_t bit = 1ull << ((5u - j) * 7u + w);
      if (x & 1ull) b0 |= bit; else b1 |= bit;
      x >>= 1; player ^= 1u;
    }
  }
  unsigned long long* e = pa.ring + static_cast<size_t>(pos & (kPipeRing - 1u)) * kReqGranules;
  const unsigned long long tag = pipe_lap_tag(pos) << 48;
  e[0] = tag | b0; e[1] = tag | b1; e[2] = tag | (i % S) | (static_cast<unsigned long long>(player & 1u) << 16); e[3] = tag | (i + 1u);
}
__global__ void k_pipe_fill_done(PipeArrays pa, uint32_t n) { pa.ctl->tail += n; }
__global__ void k_pipe_head_reset(PipeArrays pa) { pa.ctl->head = pa.ctl->tail; for (uint32_t w = 0; w < pa.n_tree_wgs; ++w) pa.wg[w].rhead = pa.wg[w].rtail; }
}  // namespace azmi
