// Net side of the asynchronous tree / net pipeline and what runs between two epochs: the persistent net kernel (k_pipe_net over the
// tiles of leafnet_c4.h), the settle and cache-insert kernels of the epoch boundary, and the two one-thread kernels that find out
// whether two streams run side by side.  Included by pipeline.hip alone, behind pipe_tree_kernels.h.
#pragma once
#include "leafnet_c4.h"
#include "pipe_tree_kernels.h"

namespace azmi {

// ---- net side -----------------------------------------------------------------------------------------------------------------------
// A persistent workgroup of the leaf net (leafnet_c4.h: 4 waves, one tile of boards through the whole tower): claim up to six
// requests, read their granules, build the input planes from the packed positions (connect4_gs.cc:131-149: planes 0 / 1 the
// stones, plane 2 + player all ones), run the 3- or the 6-board tile, write the (v, pi) granules of every board, again.
// Leaves when the epoch is over: stop is up, every tree workgroup has left and the ring is empty.
constexpr uint32_t kPipeXs = 512;      // bytes of claim scratch behind the tile's LDS
// MODE 0: the 3- and the 6-board tile (by what the claim brought), 1: the 6-board tile only, 2: the 3-board tile only
// X3: the bf16x3 tier's tiles (Tile<.., SPLIT>: weights and activations as bf16 high + low parts, three MFMAs per product - the north
// star's 1e-5 on the matrix cores); 16 activation planes, so ONE workgroup per CU, beside which a tree workgroup still fits
// Two model groups (play_past: one net per group): np1 = the weights of group 1's net; a workgroup serves ONE group's ring for the
// whole epoch (its index's parity when both groups have a net behind them, pa.net_groups).
template <int MODE, bool X3 = false>
__global__ __launch_bounds__(256, 2) void k_pipe_net(azmi_net_dev::NetDesc nd, azmi_net_dev::NetPtrs np, azmi_net_dev::NetPtrs np1, PipeArrays pa) {
  constexpr uint32_t kMaxTake = MODE == 2 ? 3u : 6u;
  constexpr uint64_t kPatienceTicks = 150;       // 1.5 us: how long a request that is there waits for the rest of its window
  using namespace azmi_net_dev;
  using TBig = std::conditional_t<X3, c4::TileBigX3, c4::TileBig>;
  using TSmall = std::conditional_t<X3, c4::TileSmallX3, c4::TileSmall>;
  extern __shared__ __attribute__((aligned(16))) uint8_t lds_pipe[];
  // claim scratch: [0] boards claimed (0 = leave), [1] first ring position; [8..14) slot, [16..22) sequence number,
  // [24..30) player, then as u64: [0..6) stones of player 0, [8..14) stones of player 1
  uint32_t* const xs = reinterpret_cast<uint32_t*>(lds_pipe + TBig::LDS_BYTES);
  static_assert(TBig::LDS_BYTES >= TSmall::LDS_BYTES && (X3 ? 1 : 2) * (TBig::LDS_BYTES + kPipeXs) <= 160 * 1024, "two workgroups per CU (X3: one)");
  const uint32_t tid0 = threadIdx.x;
  uint64_t t_start = wall_clock64(), t_last = t_start;      // (wave 0's copy moves by what a freeze takes)
  PipeCtl* const pc = pa.ctl;
  PipeEpoch* const pe = pa.ep;
  const uint32_t mg = pa.net_groups == 3u ? (blockIdx.x & 1u) : (pa.net_groups == 2u ? 1u : 0u);      // this workgroup's model group
  uint32_t* const q_head = pipe_head_of(pc, mg);
  uint32_t* const q_tail = pipe_tail_of(pc, mg);
  const unsigned long long* const q_ring = pipe_ring_of(pa, mg);
  if (tid0 == 0) {
    unsigned long long t0 = atomicCAS(&pe->t0, 0ull, static_cast<unsigned long long>(t_start));
    if (t0 == 0ull) t0 = t_start;
    atomicMax(&pe->net_late, static_cast<uint32_t>(t_start > t0 ? t_start - t0 : 0ull));
    atomicAdd(&pe->net_arrived, 1u);
    if (pa.census_hold != 0u && t_start > t0 && t_start - t0 >= pa.census_hold) atomicAdd(&pe->net_late_n, 1u);      // calibration launch: see k_pipe_tree
  }
  if (pa.census_hold != 0u) {
    __syncthreads();
    const unsigned long long t0 = g_ld(&pe->t0);
    while (wall_clock64() < t0 + pa.census_hold) __builtin_amdgcn_s_sleep(32);
    return;
  }
  // The workgroup's WINDOW: kMaxTake consecutive ring positions drawn with ONE fetch-add on `head` (a compare-and-swap claim
  // of "what is there" serialises every workgroup of the chip on one word: a claim then costs a memory round trip per
  // contender).  The window's positions are this workgroup's to serve, whenever their requests arrive: it waits until the
  // rest of the window is there - or, when a request is waiting, for a short patience only -, runs a tile over what
  // arrived, and draws a new window once this one is used up.  head therefore runs ahead of tail.
  uint32_t w0 = 0, wn = 0, wdone = 0;        // window start, size, positions served (wave 0 keeps them; uniform)
  bool prev_full = false, first_look = false; // the last window drawn was complete when first looked at (a backlog); the next look is a window's first
  uint64_t pf_wait = 0, pf_tile = 0, pf_mark = wall_clock64();
  for (;;) {
    uint32_t tid = tid0;      // (opaque per tile, as k_pipe_tree's lane number: per-thread addresses are not hoisted out of the epoch's loop)
    asm volatile("" : "+v"(tid));
    __syncthreads();
    { const uint64_t nowp = wall_clock64(); pf_tile += nowp - pf_mark; pf_mark = nowp; }
    if (tid < 64) {        // wave 0 runs the claim; lanes 0..7 look at one ring entry each
      uint32_t n = 0;
      uint32_t sl = 0xFFFFFFFFu, sq = 0, pl = 0;
      unsigned long long b0 = 0, b1 = 0;
      uint64_t t_first = 0;                  // when the first request of this pass was seen
      uint32_t final_looks = 0;              // empty looks at the window after the tree side had left
      uint64_t t_empty = 0;                  // when this claim first found nothing at its position
      uint32_t empty_looks = 0;              // looks that found nothing (lane 0 counts)
      unsigned long long sims_seen = 0; uint64_t t_prog = 0;     // a surplus workgroup's view of the tree side's progress (its slow poll)
      for (;;) {
        if (wdone == wn) {
          // the window's size follows the load (MODE 0): with a backlog of requests the 6-board tile (capacity: 28 M evaluations/s on
          // the chip's net places), with none - this workgroup is idle, and so are others - the 3-board tile (latency: 39 us alone
          // against 60; the slots, not the matrix cores, are what is short then)
          // (round 4 asked the ring: 6 when at least big_at = 96 requests waited, from a load of head and one of tail per claim.  Those
          // are the two hottest words of the pipeline - every request is a returning add on tail - and the two loads alone cost 2.7 % of
          // the headline (always-3 with them against always-3 without).  Round 5: a workgroup whose LAST window was complete when it
          // first looked at it has met a backlog itself - 6; one that had to wait for its requests - 3.  No load at all: +3.4 % on one
          // box, profiles/r5_window_rule_ab.txt.  AZMI_PIPE_BIG_AT >= 2 brings the ring's count back as a second condition.)
          uint32_t h = 0, take = kMaxTake;
          if (MODE == 0 && pa.big_at != 0u) {
            if (!prev_full) take = 3u;
            else if (pa.big_at >= 2u) {
              uint32_t hd = 0, tl = 0;
              if (tid == 0) { hd = g_ld(q_head); tl = g_ld(q_tail); }
              const int32_t backlog = static_cast<int32_t>(__builtin_amdgcn_readfirstlane(tl) - __builtin_amdgcn_readfirstlane(hd));
              if (backlog < static_cast<int32_t>(pa.big_at)) take = 3u;
            }
          }
          first_look = true;
          if (tid == 0) h = atomicAdd(q_head, take);
          w0 = __builtin_amdgcn_readfirstlane(h); wn = take; wdone = 0;
        }
        const uint32_t left = wn - wdone;
        bool here = false;
        if (tid < left) {
          const uint32_t pos = w0 + wdone + tid;
          const unsigned long long want = pipe_lap_tag(pos);
          const unsigned long long* e = q_ring + static_cast<size_t>(pos & (kPipeRing - 1u)) * kReqGranules;
          const unsigned long long a0 = g_ld(e), a1 = g_ld(e + 1), a2 = g_ld(e + 2), a3 = g_ld(e + 3);
          here = (a0 >> 48) == want && (a1 >> 48) == want && (a2 >> 48) == want && (a3 >> 48) == want;
          if (here) {
            b0 = a0 & kMask48; b1 = a1 & kMask48;
            sl = static_cast<uint32_t>(a2 & 0xFFFFull); pl = static_cast<uint32_t>((a2 >> 16) & 1ull);
            sq = static_cast<uint32_t>(a3);
          }
        }
        const uint32_t hm = static_cast<uint32_t>(__ballot(here)) & 0xFFu;
        const uint32_t k = static_cast<uint32_t>(__builtin_ctz(~hm));          // arrived prefix of the window's rest
        if (first_look) { prev_full = k == left; first_look = false; }
        const uint64_t now = wall_clock64();
        pipe_freeze_credit(pc, now, t_last, t_start, tid == 0);
        if (k == left) { n = k; break; }
        if (k != 0u) {
          if (t_first == 0) t_first = now;
          if (now - t_first > kPatienceTicks) { n = k; break; }
          continue;
        }
        // nothing there: is the epoch over?  stop is up (no tree workgroup that arrives from now on sends anything) and every
        // tree workgroup that did arrive has left: tail is final, and what lies at or beyond it never comes
        uint32_t over = 0, stale = 0, idle = 0, leave = 0;
        if (tid == 0) {
          // A position more than half a ring BEHIND the tail will never show this lap's tag again: its request was overwritten a lap
          // later before this workgroup could look (seen once in ~1e10 requests: the workgroup sat 2 laps behind - it had been
          // switched out).  Give the window up; the slot stays unanswered and k_pipe_settle sends its request again.
          // (looked at only once this position has been empty for 0.5 ms: `tail` is the hottest word of the pipeline - every request
          // is a returning add on it - and 384 idle workgroups reading it on every poll slowed every request: the headline lost 12 %)
          if (t_empty == 0) t_empty = now;
          if (now - t_empty > 2000ull) idle = 1;          // nothing for 20 us: poll slowly from here on (below)
          if (now - t_empty > 50000ull && static_cast<int32_t>(g_ld(q_tail) - (w0 + wdone)) > static_cast<int32_t>(kPipeRing / 2u)) stale = 1;
          // (err and stop are looked at on every eighth empty look only - ~4 us: they matter when the epoch ends, the window's own
          // ring entries, read above on every look, are what a request's latency depends on)
          if (idle == 0u && (empty_looks++ & 7u) != 0u) { /* not this time */ }      // (a workgroup in its slow poll looks every time: 14 us apart)
          else if (g_ld(&pc->err)) over = 1;
          else if (g_ld(&pe->stop) != 0u && g_ld(&pe->tree_done) >= g_ld(&pe->tree_arrived)) {
            const uint32_t t2 = g_ld(q_tail);
            if (static_cast<int32_t>(t2 - (w0 + wdone)) <= 0) over = 1;
            // every writer has left (and drained its stores before it was counted done): a position below the final tail that is
            // still not there on the second look after that will never be - given up like a stale one
            else if (++final_looks >= 2u) stale = 1;
          }
          // the stall detector: cap x 1.25 once the tree side is there; while no tree workgroup has started yet (the host was held up
          // between the two launches, the tree kernel waits for a place) four caps - long enough for any scheduling hiccup, short
          // enough that a launch that never comes is an error and not a hang
          // (round 5: FORTY caps = 10 s.  The cap is the tree side's stall detector; the net side only waits for the tree side, and the
          // tree kernel's wavefronts were seen to stand still for 0.3 s (profiles/r5_repro_generic_freeze_credit.txt) and for more than
          // 2 s (r5_repro_generic_8xcap.txt) while this kernel kept running: they credit such a freeze and finish normally, this side
          // must outwait it; a tree kernel that never comes is still an error after 10 s, not a hang)
          // (round 6, ADVICE r5: what round 5's captures showed is that tree wavefronts can stand still for as long as HUNDREDS of idle
          // net workgroups stay resident beside them, and run on the moment those leave.  An epoch launches no more net workgroups than
          // its slots can keep busy (net_launch), so this only arises under AZMI_PIPE_NET_ALL; there a workgroup the slots do not need
          // (index >= net_needed) that has been idle, in its slow poll, beside a tree side that HAS arrived and whose simulation count
          // has not moved for 1.25 caps gives its place back instead of outwaiting the freeze: its window is given up like a stale one
          // (k_pipe_settle sends a request that still lands there again), no error.  The needed workgroups keep the long patience.)
          if (idle != 0u && !over && blockIdx.x >= pa.net_needed) {
            const unsigned long long s_now = g_ld(&pe->sims);
            if (s_now != sims_seen || t_prog == 0) { sims_seen = s_now; t_prog = now; }
            else if (g_ld(&pe->tree_arrived) != 0u && now - t_prog > pa.cap_ticks + (pa.cap_ticks >> 2)) { stale = 1; leave = 1; }
          }
          if (!over && now - t_start > 40u * pa.cap_ticks) {
            // (what the stalled workgroup saw, for the error message: dbg[8..14) = stop, tree workgroups done / arrived, ring tail,
            // the window position it waits at, 10 us units since its start)
            if (atomicAdd(&pc->dbg[7], 1u) == 0u) {
              pc->dbg[8] = g_ld(&pe->stop); pc->dbg[9] = g_ld(&pe->tree_done); pc->dbg[10] = g_ld(&pe->tree_arrived);
              pc->dbg[11] = g_ld(q_tail); pc->dbg[12] = w0 + wdone; pc->dbg[13] = static_cast<uint32_t>((now - t_start) / 1000u);
            }
            atomicOr(&pc->err, static_cast<uint32_t>(kPipeErrNetTimeout)); g_st(&pe->stop, 1u); over = 1;
          }
        }
        if (__builtin_amdgcn_readfirstlane(over)) { n = 0; break; }
        if (__builtin_amdgcn_readfirstlane(stale)) {
          if (tid == 0) { atomicAdd(&pe->lost, left); atomicAdd(&pc->lost_total, left); }
          wdone = wn;          // (the next turn of the loop draws a new window)
          if (__builtin_amdgcn_readfirstlane(leave)) { n = 0; break; }      // a surplus workgroup gives its place back
          continue;
        }
        // A workgroup that has found nothing for 20 us polls every ~14 us instead of every 0.5 us (7 us more latency for a request that
        // arrives into an idle chip): idle persistent workgroups are not free - their polls share the control lines and the fabric with
        // the tree side.  (Round 5: this alone did NOT end the seconds-long stalls of the tree wavefronts seen beside ~500 idle net
        // workgroups - not launching them did: net_launch.)
        if (__builtin_amdgcn_readfirstlane(idle)) {
          __builtin_amdgcn_s_sleep(127); __builtin_amdgcn_s_sleep(127); __builtin_amdgcn_s_sleep(127); __builtin_amdgcn_s_sleep(127);
        } else {
          __builtin_amdgcn_s_sleep(16);
        }
      }
      if (tid < 8) {
        const bool mine = tid < n;
        xs[8 + tid] = mine ? sl : 0xFFFFFFFFu; xs[16 + tid] = sq; xs[24 + tid] = pl;
        unsigned long long* xb = reinterpret_cast<unsigned long long*>(xs + 32);
        xb[tid] = mine ? b0 : 0ull; xb[8 + tid] = mine ? b1 : 0ull;
        if (pa.l0) {       // the position's cache key (Connect4::key: stones and the player to move) for the in-epoch answer table
          Connect4::State ps_; ps_.bb[0] = b0; ps_.bb[1] = b1; ps_.player = pl; ps_.turn = 0;
          const unsigned long long k64 = Connect4::key(ps_) ^ (mg ? kPipeGroupSalt : 0ull);
          xb[16 + tid] = k64;
          xs[96 + tid] = pipe_l0_entry(k64, pa.l0_mask);
        }
      }
      if (tid == 0) xs[0] = n;
      wdone += n;
    }
    __syncthreads();
    { const uint64_t nowp = wall_clock64(); pf_wait += nowp - pf_mark; pf_mark = nowp; }
    const uint32_t n = xs[0];
    if (n == 0) break;
    if (tid == 0) { atomicAdd(&pc->tiles, 1ull); atomicAdd(&pc->tile_boards, static_cast<unsigned long long>(n)); atomicAdd(&pc->tile_hist[(n - 1u) % 6u], 1ull); }
    __syncthreads();
    c4::PipeIO pio{pa.res, xs + 8, xs + 16, kResStride, kResV, pa.l0, xs + 96, reinterpret_cast<const unsigned long long*>(xs + 32) + 16,
                   reinterpret_cast<const unsigned long long*>(xs + 32), xs + 24};
    // the weight pointers are made opaque per pass: otherwise the tile's loads of its (pass-invariant) head weights are
    // hoisted out of this loop and sit in ~120 registers for the whole tile (spills)
    NetPtrs npi = mg ? np1 : np;
    asm volatile("" : "+s"(npi.stem_w), "+s"(npi.stem_b), "+s"(npi.blocks), "+s"(npi.head_w), "+s"(npi.head_b), "+s"(npi.v_fc1_w));
    asm volatile("" : "+s"(npi.v_fc1_b), "+s"(npi.v_fc2_w), "+s"(npi.v_fc2_b), "+s"(npi.pi_fc_w), "+s"(npi.pi_fc_b));
    if (MODE == 2 || (MODE == 0 && n <= static_cast<uint32_t>(TSmall::TBW))) {
      if constexpr (MODE != 1) {
        c4::tile<TSmall, 4, 4, 16, 0, true>(nd, npi, nullptr, nullptr, nullptr, TSmall::TBW, nullptr, nullptr, 0u, lds_pipe, &pio);
      }
    } else {
      if constexpr (MODE != 2) {
        c4::tile<TBig, 4, 4, 16, 0, true>(nd, npi, nullptr, nullptr, nullptr, TBig::TBW, nullptr, nullptr, 0u, lds_pipe, &pio);
      }
    }
    // READY tokens of the answered slots (the tree wavefront that draws one checks the granules' tags itself, so the tokens
    // need no ordering behind the tile's stores)
    // (each into the ring of its slot's home workgroup: one ticket per board, drawn side by side)
    if (tid < n) {
      const uint32_t sl = xs[8 + tid];
      const uint32_t home = sl % pa.n_tree_wgs;
      const uint32_t pos = atomicAdd(&pa.wg[home].rtail, 1u);
      pipe_push_token(pa, home, pos, static_cast<unsigned long long>(sl) | (static_cast<unsigned long long>(xs[16 + tid]) << 16));
    }
  }
  if (tid0 == 0) { atomicAdd(&pc->prof[7], pf_wait); atomicAdd(&pc->prof[8], pf_tile); }
}

// (the net kernel's time accounting is added by its thread 0 when it leaves)
// ---- between epochs -----------------------------------------------------------------------------------------------------------------
// Requests that were still out when the epoch ended have been answered by now (the net workgroups drain the ring before they
// leave): their answers move from the granules into the slots' (v, pi) rows - the lock-step form of a pending answer - and
// into the insert log.
__global__ void k_pipe_settle(EngineParams ep, EngineArrays ar, PipeArrays pa) {
  const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
  // the net workgroups left with unused window positions (head ran ahead of tail): the next epoch's windows start at tail; tokens
  // that were still in a READY ring when the epoch ended are dropped (their slots are whole in HBM: k_pipe_seed sends new ones)
  if (slot == 0) { pa.ctl->head = pa.ctl->tail; pa.ctl->head1 = pa.ctl->tail1; pa.ctl->sims_total += pa.ep->sims; }
  if (slot < pa.n_tree_wgs) pa.wg[slot].rhead = pa.wg[slot].rtail;
  if (slot >= ep.S) return;
  // slots the epoch listed for the move step and did not get to (listed as it ended): the boundary's move step
  if (ar.flags[slot] & kFlagListed) ar.mover_list[atomicAdd(&ar.ctl->mover_count, 1u)] = slot;
  else { const uint8_t s0 = ar.sstate[slot]; if (s0 == kSlotFresh || s0 == kSlotRestart) ar.mover_list[atomicAdd(&ar.ctl->mover_count, 1u)] = slot; }
  const uint8_t f = ar.flags[slot];
  if (!(f & kFlagReqOut)) return;
  const uint32_t seq = ar.req_seq[slot];
  constexpr int M = Connect4::M, P1 = Connect4::P + 1;
  float val[M + P1];
  bool bad = false;
#pragma unroll
  for (int i = 0; i < M + P1; ++i) {
    const unsigned long long g = pa.res[static_cast<size_t>(slot) * kResStride + i];
    bad = bad || static_cast<uint32_t>(g >> 32) != seq;
    val[i] = __uint_as_float(static_cast<uint32_t>(g));
  }
  if (bad) {
    // the request was never answered - the net side left early (a pipeline error: time cap, engine stop) or gave a ring position up
    // (PipeEpoch::lost).  The slot goes back
    // to the form the move step leaves a leaf in (kSlotQueued: planes + packed position written, no request out), so the next epoch
    // sends the request again and a lock-step round lists it: the engine stays usable after the error has been reported.
    if (g_ld(&pa.ctl->err) == 0u && ar.ctl->stop == 0u && pa.ep->lost == 0u) { atomicOr(&pa.ctl->err, static_cast<uint32_t>(kPipeErrTag)); return; }
    Connect4::State leaf;
    leaf.bb[0] = ar.leaf_pos[0 * static_cast<size_t>(ep.S) + slot];
    leaf.bb[1] = ar.leaf_pos[1 * static_cast<size_t>(ep.S) + slot];
    leaf.player = static_cast<uint32_t>(ar.leaf_pos[2 * static_cast<size_t>(ep.S) + slot]) & 1u;
    leaf.turn = static_cast<uint32_t>(__popcll(leaf.bb[0] | leaf.bb[1]));
    float* row = ar.canon + static_cast<size_t>(slot) * Connect4::CANON;
    for (uint32_t e = 0; e < static_cast<uint32_t>(Connect4::CANON); ++e) row[e] = Connect4::canonical_at(leaf, e);
    ar.flags[slot] = f & static_cast<uint8_t>(~kFlagReqOut);
    ar.sstate[slot] = kSlotQueued;
    return;
  }
#pragma unroll
  for (int i = 0; i < M; ++i) ar.pi[static_cast<size_t>(slot) * M + i] = val[i];
#pragma unroll
  for (int i = 0; i < P1; ++i) ar.v[static_cast<size_t>(slot) * P1 + i] = val[kResV + i];
  ar.flags[slot] = f & static_cast<uint8_t>(~kFlagReqOut);
  if (ep.cache_on) {
    const uint32_t idx = atomicAdd(&pa.ep->ins_count, 1u);
    if (idx < pa.ins_cap) {
      pa.ins_key[idx] = ar.leaf_key[slot];
      if (pa.ins_grp) pa.ins_grp[idx] = ar.leaf_group[slot];
#pragma unroll
      for (int i = 0; i < M; ++i) pa.ins_pi[static_cast<size_t>(idx) * M + i] = val[i];
#pragma unroll
      for (int i = 0; i < P1; ++i) pa.ins_v[static_cast<size_t>(idx) * P1 + i] = val[kResV + i];
    }
    // (a full log only loses cache entries, never answers: the epoch's quota bounds it, k_pipe_tree stops filling it at its end)
  }
}

// The epoch's answers go into the position cache (PlayManager::update_inferences -> insert_many, play_manager.cc:631-640): one
// wavefront per log entry, under the shard's insert lock (dev_cache.h).  The order of the inserts is the order the
// wavefronts get there - the reference's is the order its threads get the mutex.
// Two launches per epoch: `late` = 0 right behind the tree kernel - the log holds every answer a tree wavefront consumed - while
// the net side is still finishing its last tiles (it does not touch the cache); `late` = 1 after k_pipe_settle for the few answers
// that arrived when the tree side had left.
__global__ __launch_bounds__(256) void k_pipe_cache_insert(EngineArrays ar, PipeArrays pa, uint32_t late) {
  const uint32_t n = min(pa.ep->ins_count, pa.ins_cap);
  const uint32_t from = late ? min(pa.ep->ins_done, n) : 0u;
  if (!late && blockIdx.x == 0 && threadIdx.x == 0) pa.ep->ins_done = n;     // (read by the second launch only; the log does not grow before k_pipe_settle)
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
  const uint32_t waves = gridDim.x * (blockDim.x >> 6);
  constexpr uint32_t M = Connect4::M, P1 = Connect4::P + 1;
  for (uint32_t i = from + wave; i < n; i += waves) {
    const uint64_t key = pa.ins_key[i];
    const float p = lane < M ? pa.ins_pi[static_cast<size_t>(i) * M + lane] : 0.0f;
    const float v = lane < P1 ? pa.ins_v[static_cast<size_t>(i) * P1 + lane] : 0.0f;
    const uint32_t g = pa.ins_grp ? (pa.ins_grp[i] & 1u) : 0u;           // (one S3-FIFO per model group, play_manager.cc:195-203)
    const bool ok = g ? wave_shard_insert_locked<false>(ar.caches[1], pa.locks + pa.lock_base1, key, p, v, lane)
                      : wave_shard_insert_locked<false>(ar.cache, pa.locks, key, p, v, lane);
    if (!ok && lane == 0) atomicOr(&pa.ctl->err, static_cast<uint32_t>(kPipeErrLock));
  }
}
// ---- do two streams run side by side? -------------------------------------------------------------------------------------------
// The runtime multiplexes streams onto a few hardware queues (4 by default): two streams that share a queue run their kernels
// one after the other, and an epoch's tree and net kernels, each waiting for the other, would then sit there until the time cap.
// k_pair_wait (launched first, on the tree side's stream) waits up to 2 ms for the word k_pair_set (net side's stream) writes.
__global__ void k_pair_wait(uint32_t* flag) {
  const uint64_t t0 = wall_clock64();
  while (g_ld(flag) == 0u) {
    if (wall_clock64() - t0 > 200000ull) { g_st(flag + 1, 1u); return; }     // 2 ms: the partner never started
    __builtin_amdgcn_s_sleep(32);
  }
}
__global__ void k_pair_set(uint32_t* flag) { g_st(flag, 1u); }

}  // namespace azmi
