// Tree side of the asynchronous tree / net pipeline (pipe_types.h has the structure and the hand-off protocol): the polling and
// freeze primitives every pipeline kernel uses, the epoch's seed kernel, the move step inside an epoch and the two persistent tree
// kernels - k_pipe_tree (the fast one: its plain, profiled, two-group and Gumbel builds) and k_pipe_tree_generic (every step through
// the lock-step engine's move-step function: the cross-check).  One kernel family; included by pipeline.hip alone, which launches it.
#pragma once
#include "engine_kernels.h"
#include "pipe_types.h"

namespace azmi {

__device__ __forceinline__ unsigned long long g_ld(const unsigned long long* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ uint32_t g_ld(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void g_st(unsigned long long* p, unsigned long long v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void g_st(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }


enum : uint32_t { kGrpIdle = 0, kGrpReady = 1, kGrpWait = 2, kGrpPush = 3 };
// A FREEZE: two looks at the wall clock by one polling wavefront more than 2 ms apart.  No iteration of a polling loop takes that
// long on its own - the loops load a few words and sleep a microsecond -: the wavefront, and with it the chip, stood still (round 5:
// the stall-cap error of round 4, one in ~30,000 epochs, was every wavefront of both kernels spanning > 190 ms in ONE iteration - the
// GPU's own scheduler had switched the process's queues out, profiles/r5_repro_generic.txt).  The time caps are stall detectors for
// THIS code's protocol, so a freeze is credited: the wavefront's start time moves by the gap, the freeze is counted
// (PipeCtl::freezes, longest gap in PipeCtl::freeze_max) and reported with the call's statistics, not as an error.  Only a gap INSIDE
// a poll loop counts: the first look after a pass (a slow pass is not a freeze) only sets the mark.
constexpr uint64_t kFreezeTicks = 200000ull;
__device__ __forceinline__ void pipe_freeze_credit(PipeCtl* pc, uint64_t now, uint64_t& t_last, uint64_t& t_start, bool leader) {
  const uint64_t gap = now - t_last;
  if (gap > kFreezeTicks) {
    t_start += gap;
    if (leader) { atomicAdd(&pc->freezes, 1ull); atomicMax(&pc->freeze_max, static_cast<unsigned long long>(gap)); }
  }
  t_last = now;
}
constexpr uint64_t kMask48 = (1ull << 48) - 1;
constexpr uint32_t kNoSlot = 0xFFFFFFFFu;

// one struct = the whole kernarg segment of k_pipe_tree: the move step (a function of its own, below) reads its arguments from
// there instead of from copies on the stack
struct PipeKernArgs { EngineParams ep; EngineArrays ar; PipeArrays pa; };

// ---- tree side ---------------------------------------------------------------------------------------------------------------------
// Every slot has a HOME workgroup (slot % tree workgroups).  A slot that can take its next step sits, as a token, in its home
// workgroup's READY ring (seeded by k_pipe_seed when the epoch starts, refilled by the net workgroups with the slots they have
// answered and by the workgroup's own wavefronts with slots whose next answer is already at hand or whose next step is the move
// step's).  A tree wavefront works in PASSES: look at the ring's head | tail word, draw what is there (at most eight tokens: one
// fetch-add), load the slots - one 8-lane group each -, back the pending simulations up and descend again until each group's new
// leaf needs the net (k_sim's body, engine_kernels.h: the path in registers, level i in lane i), store the slots, hand the leaves
// to the request ring.  A slot's state and trees are plain memory that only ever moves between the wavefronts of ONE workgroup =
// one CU = one vector L1: a pass drains its stores (s_waitcnt vmcnt(0)) before its tokens go out and that is all (round 3 let
// slots wander between CUs and paid an agent-scope acquire + release, ~10 us, per pass).

__device__ __forceinline__ void pipe_push_token(const PipeArrays& pa, uint32_t home, uint32_t pos, unsigned long long payload) {
  g_st(pa.rring + ((static_cast<size_t>(home) << pa.rshift) + (pos & ((1u << pa.rshift) - 1u))), (pipe_lap_tag_r(pos, pa.rshift) << 48) | payload);
}

// request ring of model group g (0 or 1): its tail / head words and its entries
__device__ __forceinline__ uint32_t* pipe_tail_of(PipeCtl* pc, uint32_t g) { return g ? &pc->tail1 : &pc->tail; }
__device__ __forceinline__ uint32_t* pipe_head_of(PipeCtl* pc, uint32_t g) { return g ? &pc->head1 : &pc->head; }
__device__ __forceinline__ unsigned long long* pipe_ring_of(const PipeArrays& pa, uint32_t g) { return g ? pa.ring1 : pa.ring; }

// The epoch's first tokens: one thread per slot.  A slot whose leaf was left by the move step (kSlotQueued) sends its request, a
// slot with its answer in the (v, pi) rows gets a READY token, a slot whose game has to start a READY token with the move bit.
__global__ void k_pipe_seed(EngineParams ep, EngineArrays ar, PipeArrays pa) {
  const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= ep.S) return;
  PipeCtl* const pc = pa.ctl;
  PipeEpoch* const pe = pa.ep;
  if (ar.ctl->stop != 0 || pc->err != 0) { atomicAdd(&pe->dead, 1u); return; }
  const uint8_t sst = ar.sstate[slot];
  if (sst == kSlotDone || sst == kSlotEnded) { atomicAdd(&pe->dead, 1u); return; }
  const uint32_t home = slot % pa.n_tree_wgs;
  const uint8_t f = ar.flags[slot];
  if ((sst != kSlotWaitEval && sst != kSlotQueued) || (f & kFlagListed)) {       // kSlotFresh / kSlotRestart: a game start is the move step's
    const uint32_t pos = atomicAdd(&pa.wg[home].rtail, 1u);
    pipe_push_token(pa, home, pos, static_cast<unsigned long long>(slot) | kTokMove);
    return;
  }
  if (f & kFlagReqOut) { atomicOr(&pc->err, static_cast<uint32_t>(kPipeErrTag)); return; }      // (every request was settled)
  if (sst == kSlotQueued) {
    const uint32_t grp_ = pa.n_groups > 1u ? (ar.leaf_group[slot] & 1u) : 0u;
    const uint32_t pos = atomicAdd(pipe_tail_of(pc, grp_), 1u);
    uint32_t seq = ar.req_seq[slot] + 1u;
    if (seq == 0u) seq = 1u;
    ar.req_seq[slot] = seq;
    const unsigned long long tag = pipe_lap_tag(pos) << 48;
    unsigned long long* e = pipe_ring_of(pa, grp_) + static_cast<size_t>(pos & (kPipeRing - 1u)) * kReqGranules;
    g_st(e + 0, tag | (ar.leaf_pos[0 * static_cast<size_t>(ep.S) + slot] & kMask48));
    g_st(e + 1, tag | (ar.leaf_pos[1 * static_cast<size_t>(ep.S) + slot] & kMask48));
    g_st(e + 2, tag | static_cast<unsigned long long>(slot) | ((ar.leaf_pos[2 * static_cast<size_t>(ep.S) + slot] & 1ull) << 16));
    g_st(e + 3, tag | static_cast<unsigned long long>(seq));
    ar.flags[slot] = f | kFlagReqOut;
    ar.sstate[slot] = kSlotWaitEval;
    return;
  }
  const uint32_t pos = atomicAdd(&pa.wg[home].rtail, 1u);
  pipe_push_token(pa, home, pos, static_cast<unsigned long long>(slot));     // (answers no request: sequence field 0)
}

// ---- the move step inside the epoch ---------------------------------------------------------------------------------------------
// A slot a tree wavefront lists (its next backup completes a search, or its leaf is the root) and a slot whose game has to start
// come back to their home workgroup as tokens with the move bit; the wavefront that draws them runs the lock-step engine's own
// move step (round_slot<kMover>: backup, move, history row, re-rooting, game step / game end, first descent of the next search)
// for those groups before the pass proper.  What a group gets back: kSlotWaitEval - the next answer is at hand, the group goes on
// into the pass like any READY slot; kSlotQueued - the new leaf is a request now (sent here), the group sits this pass out;
// kSlotEnded / kSlotDone - the game is over, the slot waits for the boundary's k_assign.
// A function of its own, NOT inlined: inside k_pipe_tree its 244 registers pushed the tree loop into scratch (pass 50 -> 73 us).
// Its arguments are references into the kernel's kernarg segment (PipeKernArgs), not into copies.
template <class GM>
__device__ __attribute__((noinline)) uint32_t pipe_move_groups(const EngineParams& ep, const EngineArrays& ar, const PipeArrays& pa, const uint32_t my_slot) {
  const uint32_t wlane = threadIdx.x & 63u, grp = wlane >> 3, lane = wlane & 7u;
  PipeCtl* const pc = pa.ctl;
  PipeEpoch* const pe = pa.ep;
  const bool on = my_slot != kNoSlot;
  const uint32_t slot = on ? my_slot : 0u;
  uint32_t res_state = 0xFFu, seq = 0, was_sim = 0;
  if (on) {
    was_sim = ar.sstate[slot] == kSlotWaitEval ? 1u : 0u;        // (a listed slot's step finishes a simulation; a game start does not)
    res_state = round_slot<GM, false, true>(ep, ar, slot, lane);
  }
  if (on && res_state == kSlotQueued && lane == 0) {
    // the leaf goes to the net: the slot takes the form of a slot with a request out (k_pipe_seed does the same between epochs)
    seq = g_ld(ar.req_seq + slot) + 1u;
    if (seq == 0u) seq = 1u;
    ar.flags[slot] = ar.flags[slot] | kFlagReqOut;
    ar.sstate[slot] = kSlotWaitEval;
  }
  seq = __shfl(seq, static_cast<int>(grp * 8), 64);
  // everything the move steps wrote is in L2 before a request of theirs is out (its answer's token may be drawn by another
  // wavefront of this workgroup)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (on && res_state == kSlotQueued) {
    if (lane == 0) g_st(ar.req_seq + slot, seq);
    const uint32_t mg = pa.n_groups > 1u ? (ar.leaf_group[slot] & 1u) : 0u;       // the leaf's model group: its net's ring
    uint32_t pos = 0;
    if (lane == 0) pos = atomicAdd(pipe_tail_of(pc, mg), 1u);
    pos = __shfl(pos, static_cast<int>(grp * 8), 64);
    const size_t S_ = static_cast<size_t>(ep.S);
    const uint64_t payload = lane == 0 ? ar.leaf_pos[0 * S_ + slot] : lane == 1 ? ar.leaf_pos[1 * S_ + slot]
                           : lane == 2 ? (static_cast<uint64_t>(slot) | ((ar.leaf_pos[2 * S_ + slot] & 1ull) << 16)) : static_cast<uint64_t>(seq);
    if (lane < kReqGranules)
      g_st(pipe_ring_of(pa, mg) + static_cast<size_t>(pos & (kPipeRing - 1u)) * kReqGranules + lane, (pipe_lap_tag(pos) << 48) | (payload & kMask48));
  }
  {
    const unsigned long long em = __ballot(on && lane == 0 && res_state == kSlotEnded);
    const unsigned long long dm = __ballot(on && lane == 0 && (res_state == kSlotDone || res_state == 0xFFu));
    const unsigned long long om = __ballot(on && lane == 0);
    const unsigned long long sm = __ballot(on && lane == 0 && was_sim != 0u);
    if (wlane == 0) {
      if (em) atomicAdd(&pe->ended, static_cast<uint32_t>(__popcll(em)));
      if (dm) atomicAdd(&pe->dead, static_cast<uint32_t>(__popcll(dm)));
      if (sm) atomicAdd(&pe->sims, static_cast<unsigned long long>(__popcll(sm)));
      atomicAdd(&pe->moved, static_cast<uint32_t>(__popcll(om)));
    }
  }
  return res_state;
}

// NT: threads per workgroup (256: four wavefronts beside one net workgroup on a CU)
// PROF: the time accounting of AZMI_PIPE_PROF (a build of its own: the counters cost a dozen registers of a kernel that has none to spare)
// TWO: two model groups (play_past: a leaf goes to the S3-FIFO, the answer table lines and the request ring of the group its seat belongs
// to) - a build of its own for the same reason
// GUM: Gumbel seats (mcts.cc:233-342).  A search differs from plain PUCT in the choice at the root (the sequential-halving schedule,
// gumbel_next_root_child) and - gumbel_full - at interior nodes (gumbel_interior_select): both are SlotCtx's own functions, called
// from the descent below; the Gumbel state of a search (g, survivors, phase) is initialised by the move step's first descent
// (find_leaf's lazy init), so a search whose state is not there yet is handed to the move step.  Built with TWO.
#ifndef AZMI_TREE_MINB
#define AZMI_TREE_MINB 2          // workgroups of k_pipe_tree per CU the register budget is set for (experiment builds: 3, 4)
#endif
template <class GM, int NT, bool PROF, bool TWO = false, bool GUM = false>
__global__ __launch_bounds__(NT, AZMI_TREE_MINB) void k_pipe_tree(PipeKernArgs ka) {
  constexpr int G = GM::GROUP;
  constexpr int P = GM::P;
  static_assert(P == 2 && G == 8 && GM::M == 7, "written for Connect4's 8-lane groups");
  const EngineParams& ep = ka.ep;
  const EngineArrays& ar = ka.ar;
  const PipeArrays& pa = ka.pa;
  const uint32_t wlane = threadIdx.x & 63u, grp = wlane >> 3, lane0 = wlane & 7u;
  uint64_t t_start = wall_clock64(), t_last = t_start;      // (t_start moves by what a freeze takes: pipe_freeze_credit)
  PipeCtl* const pc = pa.ctl;
  PipeEpoch* const pe = pa.ep;
  PipeWg* const wc = pa.wg + blockIdx.x;
  const uint32_t rmask = (1u << pa.rshift) - 1u;
  unsigned long long* const myring = pa.rring + (static_cast<size_t>(blockIdx.x) << pa.rshift);
  // census first, then the epoch's stop word: a workgroup that only gets a place on the chip after the epoch has ended (the net
  // side, which leaves when every ARRIVED tree workgroup is done, may be gone by then) must not send requests any more
  if (threadIdx.x == 0) {
    unsigned long long t0 = atomicCAS(&pe->t0, 0ull, static_cast<unsigned long long>(t_start));
    if (t0 == 0ull) t0 = t_start;
    atomicMax(&pe->tree_late, static_cast<uint32_t>(t_start > t0 ? t_start - t0 : 0ull));
    const uint32_t before = atomicAdd(&pe->tree_arrived, 1u);
    asm volatile("s_waitcnt vmcnt(0)" :: "v"(before) : "memory");
  }
  __syncthreads();
  if (pa.census_hold != 0u) {
    // calibration launch (pipe_calibrate): hold the place until census_hold ticks after the epoch's first workgroup started, do
    // nothing else.  A workgroup the chip had no place for starts when the others have left: it finds itself late and is counted.
    // (EVERY wavefront holds: a wavefront that ends gives its registers back, and a workgroup of one live wavefront would let a
    // third workgroup onto the CU - the measurement would admit more than an epoch can hold)
    const unsigned long long t0 = g_ld(&pe->t0);
    if (threadIdx.x == 0 && t_start > t0 && t_start - t0 >= pa.census_hold) atomicAdd(&pe->tree_late_n, 1u);
    while (wall_clock64() < t0 + pa.census_hold) __builtin_amdgcn_s_sleep(32);
    return;
  }
  bool go = g_ld(&ar.ctl->stop) == 0 && g_ld(&pc->err) == 0 && g_ld(&pe->stop) == 0;
  // The ring's HEAD lives in LDS for the epoch: this workgroup's four wavefronts are its only consumers, so a draw is one look at the
  // ring (eight token loads side by side) and a compare-and-swap in LDS - no head | tail word, no fetch-add in HBM, no window that
  // can reach past the tail (round 4, second half: three dependent round trips per pass became one).
  __shared__ uint32_t s_head;
  if (threadIdx.x == 0) s_head = wc->rhead;
  __syncthreads();
  uint64_t pf_pass = 0, pf_idle = 0, pf_n = 0, pf_act = 0, pf_polls = 0, pf_io = 0, pf_lvls = 0, pf_mv = 0;
  uint64_t pf_ph[5] = {0, 0, 0, 0, 0};     // per group (lane 0 counts): ticks in backup / descent / expansion / probe, simulations
  SlotCtx<GM> c(ep, ar, 0u, lane0);

  while (go) {
    const uint64_t pf_t0 = PROF ? wall_clock64() : 0;
    // (the lane number, opaque per pass: per-lane addresses - base + lane x stride of a dozen arrays - are then computed where they
    // are used instead of being hoisted out of the epoch's loop into 64-bit registers that live for ever, and spill)
    uint32_t lane = lane0;
    asm volatile("" : "+v"(lane));
    c.lane = lane;
    // ---- tokens for this pass: the arrived prefix of the eight ring positions at the head
    uint32_t my_slot = kNoSlot, tok_seq = 0, tok_move = 0, n_tok = 0, empty_polls = 0, ctl_word = 0;
    uint64_t t_seen = 0;
    bool fresh_pass = true;
    for (;;) {
      const uint32_t h = __builtin_amdgcn_readfirstlane(*const_cast<volatile uint32_t*>(&s_head));
      unsigned long long tok = 0;
      bool here = false;
      if (lane == 0) {
        const uint32_t pos = h + grp;
        tok = g_ld(myring + (pos & rmask));
        here = (tok >> 48) == pipe_lap_tag_r(pos, pa.rshift);
      }
      // the epoch's end: stop word / error, the quota, games that ended, the engine's own stop word.  (Looked at on the first poll
      // of a pass and on every fourth poll of a wavefront that finds nothing: idle wavefronts must not hammer hot lines)
      if ((empty_polls & 3u) == 0u) {
        ctl_word = 0;
        if (wlane == 7) ctl_word = g_ld(&pe->stop) | g_ld(&pc->err) | g_ld(&ar.ctl->stop);
        else if (wlane == 15) ctl_word = g_ld(&pe->sims) >= pa.quota ? 1u : 0u;
        else if (wlane == 23) ctl_word = g_ld(&pe->ended);
        else if (wlane == 31) ctl_word = g_ld(&pe->dead);
      }
      uint32_t stop_seen = __builtin_amdgcn_readlane(ctl_word, 7) | __builtin_amdgcn_readlane(ctl_word, 15);
      {
        const uint32_t w = __builtin_amdgcn_readlane(ctl_word, 23), d = __builtin_amdgcn_readlane(ctl_word, 31);
        const uint32_t with_game = ep.S > d ? ep.S - d : 0u;
        const uint32_t thr = max(1u, static_cast<uint32_t>((static_cast<unsigned long long>(with_game) * pa.idle_num) >> 10));
        if (w >= thr || w + d >= ep.S) stop_seen = 1u;
      }
      const uint64_t now = wall_clock64();
      if (fresh_pass) { t_last = now; fresh_pass = false; }      // (the pass before this look is work, not a freeze)
      else pipe_freeze_credit(pc, now, t_last, t_start, wlane == 0);
      // an epoch that runs long (a cold cache sends every leaf to the net: 16384 slots x 256 simulations take > 200 ms then) simply
      // ends at a quarter of the cap; the cap itself is the stall detector
      if (now - t_start > pa.soft_ticks) stop_seen = 1u;
      if (now - t_start > pa.cap_ticks) {
        if (wlane == 0) { atomicOr(&pc->err, static_cast<uint32_t>(kPipeErrTimeout)); pc->dbg[16] = __builtin_amdgcn_readlane(ctl_word, 23); pc->dbg[17] = __builtin_amdgcn_readlane(ctl_word, 31); }
        stop_seen = 1u;
      }
      if (stop_seen) {          // (tokens still in the ring are dropped: their slots are whole in HBM, the next epoch seeds them again)
        if (wlane == 0) g_st(&pe->stop, 1u);
        go = false;
        break;
      }
      if constexpr (PROF) pf_polls += 1;
      const unsigned long long hm = __ballot(here);
      // group g's token is bit 8 g: the arrived prefix in group order
      uint32_t k = 0;
      while (k < kTreeWindow && ((hm >> (8 * k)) & 1ull)) ++k;
      if (k == 0u) { ++empty_polls; __builtin_amdgcn_s_sleep(16); continue; }
      // fewer than a window: a short wait gathers what is on its way (AZMI_PIPE_TAKE_WAIT; 0 = take what is there)
      if (k < kTreeWindow && pa.take_wait != 0u) {
        if (t_seen == 0) t_seen = now;
        if (now - t_seen <= pa.take_wait) { __builtin_amdgcn_s_sleep(2); continue; }
      }
      // claim [h, h + k): another wavefront of this workgroup may have been faster - then look again from the new head
      uint32_t won = 0;
      if (wlane == 0) won = atomicCAS(&s_head, h, h + k) == h ? 1u : 0u;
      if (__builtin_amdgcn_readfirstlane(won) == 0u) continue;
      n_tok = k;
      {
        const uint32_t sl = static_cast<uint32_t>(__shfl(static_cast<uint32_t>(tok & 0xFFFFull), static_cast<int>(grp * 8), 64));
        const uint32_t sq = static_cast<uint32_t>(__shfl(static_cast<uint32_t>((tok >> 16) & 0xFFFFFFFFull), static_cast<int>(grp * 8), 64));
        if (grp < k) { my_slot = sl & static_cast<uint32_t>(kTokSlotMask); tok_move = (sl >> 15) & 1u; tok_seq = sq; }
      }
      break;
    }
    if (!go) break;
    const uint64_t pf_t1 = PROF ? wall_clock64() : 0;
    if constexpr (PROF) { pf_idle += pf_t1 - pf_t0; pf_n += 1; pf_act += n_tok; }

    // ---- the move step for the groups whose token carries the move bit (pipe_move_groups); a group whose next answer is at
    // hand afterwards goes on into the pass like any READY slot
    if (__ballot(tok_move != 0u) != 0ull) {
      const PipeKernArgs* const kargs = reinterpret_cast<const PipeKernArgs*>(reinterpret_cast<uintptr_t>(__builtin_amdgcn_kernarg_segment_ptr()));
      const uint32_t rs = pipe_move_groups<GM>(kargs->ep, kargs->ar, kargs->pa, tok_move != 0u ? my_slot : kNoSlot);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (tok_move != 0u) { if (rs == kSlotWaitEval) tok_seq = 0u; else my_slot = kNoSlot; }
      if constexpr (PROF) pf_mv += wall_clock64() - pf_t1;
    }

    // ---- the pass.  A token that answers a request (its sequence field is not 0) may be here before the wavefront that sent
    // the request - early, in the middle of its own pass - has put the slot back: req_seq[slot] is written last, behind that
    // pass's drained stores, so the slot is whole once it shows the token's sequence number.  (Same CU, same L1: no acquire.)
    // Everything the pass needs of its slots is asked for in ONE batch - the publication word, the answer's granules (speculatively:
    // they are where the token says), the slot's state, its path image, the leaf's key - and checked afterwards; only a slot that
    // turns out not to be back yet (rare) costs a second round (round 4, second half: four dependent round trips became two).
    const uint32_t slot = my_slot != kNoSlot ? my_slot : 0u;
    c.slot = slot;
    uint32_t st = kGrpIdle;
    uint8_t final_state = kSlotWaitEval;
    uint32_t cp = 0, root = 0, goal = 0, seq = 0, mg = 0, gum_active = 0, gum_full = 0;
    bool gum_defer = false;
    size_t tb = 0;
    float fpu_root = 0.0f;
    uint32_t* const path = ar.path + static_cast<size_t>(slot) * ep.max_depth;
    unsigned long long* const res = pa.res + static_cast<size_t>(slot) * kResStride;
    float reg_pi = 0.0f, reg_v = 0.0f;
    uint32_t root_n = 0; float root_v = 0.0f; uint64_t root_meta = 0;
    uint32_t lv_node = 0, lv_n = 0, lv_pp = 0;
    float lv_q = 0.0f, lv_d = 0.0f, lv_v = 0.0f;
    uint64_t lf_meta = 0;
    uint32_t lf_mv = 0, lf_c0 = 0, lf_k = 0, lf_term = 0, lf_player = 0;
    bool fw = false;
    uint32_t fw_node = 0, fw_n = 0, fw_plen = 0;
    float fw_q = 0.0f, fw_d = 0.0f, fw_v = 0.0f;
    uint32_t fl_node = 0xFFFFFFFFu, fl_mv = 0;
    uint64_t fl_meta = 0;
    float fl_pr = 0.0f;
    uint32_t sims_done = 0, sims_mem = 0, l0_hits = 0;
    bool rec_ok = true, answered = false;
    uint64_t cur_key = 0;
    unsigned long long g0 = 0, g1 = 0;
    PendRec pr_in{};
    uint32_t seq_now = 0;
    // (the publication word is looked at BEFORE the slot's plain loads are issued, not in one batch with them: the word
    // comes from L2 (sc1), the plain loads may hit this CU's L1 earlier in time - a holder that published in between would have had its
    // new sequence number accepted beside lines read before its stores.  One more round trip per pass, ~0.5 us of ~120.)
    if (my_slot != kNoSlot) {
      seq_now = g_ld(ar.req_seq + slot);
      if (tok_seq != 0u) {
        while (seq_now != tok_seq) {      // the slot's last holder is still storing it: wait for the publication (rare)
          if (wall_clock64() - t_start > pa.cap_ticks) {
            if (lane == 0 && atomicAdd(&pc->dbg[0], 1u) == 0u) { pc->dbg[1] = slot; pc->dbg[2] = tok_seq; pc->dbg[3] = seq_now; pc->dbg[4] = 0xEEEEu; pc->dbg[14] = blockIdx.x; pc->dbg[15] = static_cast<uint32_t>((wall_clock64() - t_start) / 100u); }
            if (lane == 0) atomicOr(&pc->err, static_cast<uint32_t>(kPipeErrTimeout));
            my_slot = kNoSlot;      // (its other holder is still at work: the slot is not touched; k_pipe_settle takes its answer over)
            break;
          }
          __builtin_amdgcn_s_sleep(2);
          seq_now = g_ld(ar.req_seq + slot);
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");      // (no instruction: the loads below stay below the poll)
    if (my_slot != kNoSlot) {
      if (tok_seq != 0u) {
        if (lane < static_cast<uint32_t>(GM::M)) g0 = g_ld(res + lane);
        if (lane <= static_cast<uint32_t>(P)) g1 = g_ld(res + kResV + lane);
      }
      pr_in = ar.pend[static_cast<size_t>(slot) * G + lane];
      cur_key = ar.leaf_key[slot];
      c.load();
    }
    const bool on = my_slot != kNoSlot;
    if (on) {
      cp = c.gs.player;
      if constexpr (TWO) mg = c.seat_group(cp) & 1u;        // (no move inside a pass: one player to move, one model group, also for the answer the pass starts with)
      tb = c.tree_base(cp);
      root = AZMI_SEL(c.t_root, cp);
      goal = (c.flags & kFlagCapped) ? c.seat_cap_visits(cp) : c.seat_visits(cp);
      fpu_root = c.seat_fpu_zero(cp) ? 0.0f : ep.fpu_reduction;
      seq = seq_now;
      rec_ok = (c.flags & kFlagPendRec) != 0;
      st = kGrpReady;
      if constexpr (GUM) {
        if (c.seat_gumbel(cp)) {
          const uint32_t* const gst = c.gum_state(cp);
          gum_active = gst[SlotCtx<GM>::kGumInit];
          gum_defer = gum_active == 0u && gst[SlotCtx<GM>::kGumTarget] > 0u;      // (not initialised yet: find_leaf's lazy init is the move step's)
          gum_full = c.seat_gumbel_full(cp) ? 1u : 0u;
        }
      }
      { const NodeRec* rr = ar.nodes + tb + root; root_n = rr->n; root_v = rr->v; root_meta = rr->meta; }
      lv_node = pr_in.node; lv_n = pr_in.n; lv_pp = pr_in.pp_mv & 0xFFu;
      lv_q = pr_in.q; lv_d = pr_in.d; lv_v = pr_in.v;
      lf_meta = pr_in.leaf_meta;
      lf_mv = pr_in.pp_mv >> 8;
      lf_c0 = meta_ch0(lf_meta); lf_k = meta_nch(lf_meta); lf_term = meta_term(lf_meta); lf_player = meta_player(lf_meta);
      if (c.flags & kFlagReqOut) {
        // the answer of the slot's request: its granules (asked for with the batch above; on their way at the latest - the net
        // workgroup sent the token after them -, so a granule that is not there yet is simply asked for again)
        for (uint32_t spins = 0;; ++spins) {
          if (spins != 0u || tok_seq == 0u) {
            if (lane < static_cast<uint32_t>(GM::M)) g0 = g_ld(res + lane);
            if (lane <= static_cast<uint32_t>(P)) g1 = g_ld(res + kResV + lane);
          }
          const bool ok = (lane >= static_cast<uint32_t>(GM::M) || static_cast<uint32_t>(g0 >> 32) == seq) &&
                          (lane > static_cast<uint32_t>(P) || static_cast<uint32_t>(g1 >> 32) == seq);
          // (all eight lanes of the group agree: the group's byte of the wavefront's ballot, no LDS traffic)
          if (c.group_all(ok)) break;
          if (wall_clock64() - t_start > pa.cap_ticks) {
            if (lane == 0 && atomicAdd(&pc->dbg[0], 1u) == 0u) { pc->dbg[1] = slot; pc->dbg[2] = seq; pc->dbg[3] = c.flags; pc->dbg[4] = static_cast<uint32_t>(g1 >> 32); pc->dbg[5] = static_cast<uint32_t>(g0 >> 32); }
            if (lane == 0) atomicOr(&pc->err, static_cast<uint32_t>(kPipeErrTimeout));
            st = kGrpIdle;
            break;
          }
          __builtin_amdgcn_s_sleep(2);
        }
        if (st == kGrpReady) {
          reg_pi = lane < static_cast<uint32_t>(GM::M) ? __uint_as_float(static_cast<uint32_t>(g0)) : 0.0f;
          reg_v = lane <= static_cast<uint32_t>(P) ? __uint_as_float(static_cast<uint32_t>(g1)) : 0.0f;
          // the rows keep the pending answer, as they do for the lock-step kernels (the move step reads them)
          if (lane < static_cast<uint32_t>(GM::M)) ar.pi[static_cast<size_t>(slot) * GM::M + lane] = reg_pi;
          if (lane <= static_cast<uint32_t>(P)) ar.v[static_cast<size_t>(slot) * (P + 1) + lane] = reg_v;
          c.flags &= ~kFlagReqOut;
          answered = true;
        }
      } else if (c.flags & kFlagLeafNeedsNet) {
        if (lane < static_cast<uint32_t>(GM::M)) reg_pi = ar.pi[static_cast<size_t>(slot) * GM::M + lane];
        if (lane <= static_cast<uint32_t>(P)) reg_v = ar.v[static_cast<size_t>(slot) * (P + 1) + lane];
      }
    }
    if (ep.cache_on) {        // PlayManager::update_inferences -> insert_many (play_manager.cc:631-640): logged, applied after the epoch
      const unsigned long long am = __ballot(answered && lane == 0);
      if (am) {
        uint32_t base = 0;
        if (wlane == 0) base = atomicAdd(&pe->ins_count, static_cast<uint32_t>(__popcll(am)));
        base = __builtin_amdgcn_readfirstlane(base);
        if (answered) {
          const uint32_t idx = base + static_cast<uint32_t>(__popcll(am & ((1ull << (grp * 8)) - 1ull)));
          if (idx < pa.ins_cap) {
            if (lane == 0) pa.ins_key[idx] = cur_key;
            if constexpr (TWO) { if (lane == 1 && pa.ins_grp) pa.ins_grp[idx] = static_cast<uint8_t>(mg); }
            if (lane < static_cast<uint32_t>(GM::M)) pa.ins_pi[static_cast<size_t>(idx) * GM::M + lane] = reg_pi;
            if (lane <= static_cast<uint32_t>(P)) pa.ins_v[static_cast<size_t>(idx) * (P + 1) + lane] = reg_v;
          } else if (lane == 0) {
            g_st(&pe->stop, 1u);      // the log is full: this answer is not cached (nothing else is lost) and the epoch ends here
          }
        }
      }
    }
    const uint64_t pf_t2 = PROF ? wall_clock64() : 0;
    if constexpr (PROF) pf_io += pf_t2 - pf_t1;

    // ---- simulations (k_sim's body)
    bool listed = false;
    if (st == kGrpReady) {
      uint32_t inline_sims = 0;
      // (read once per pass: the level loop would otherwise fetch them from the kernel's arguments, a scalar load and its wait - which
      // is also a wait for every LDS permute in flight - in the middle of each level's divide chain)
      float cpuct = ep.cpuct, fpu_red = ep.fpu_reduction;
      asm volatile("" : "+s"(cpuct), "+s"(fpu_red));
      for (;;) {
        if (AZMI_SEL(c.t_depth, cp) + 1 >= goal || c.cur == root || (GUM && gum_defer)) {
          // the next backup completes the search (a move follows) or the evaluated leaf is the root (temperature, noise): the move step's
          c.flags |= kFlagListed;
          listed = true;
          st = kGrpIdle;
          break;
        }
        const uint64_t ph0 = PROF ? wall_clock64() : 0;
        if (!rec_ok) {
          // a path deeper than the 8 levels of the lane image: the backup walks MCTS::path_ in memory (the lock-step engine hands
          // these to the move step; here that would park the slot until the epoch ends)
          const bool from_net = (c.flags & kFlagLeafNeedsNet) != 0;
          c.template process_result<true>(cp, from_net, false, from_net, reg_pi, reg_v);     // (counts the simulation in c_sims itself)
          root_n += 1;
          sims_mem += 1;
          fw = false; fl_node = 0xFFFFFFFFu;
        } else {
          // ---- MCTS::process_result (mcts.cc:500-555) on the lane-resident path
          const bool from_net = (c.flags & kFlagLeafNeedsNet) != 0;
          float val[P + 1];
          if (lf_term != 0) {
#pragma unroll
            for (int i = 0; i <= P; ++i) val[i] = (static_cast<int>(lf_term) - 1 == i) ? 1.0f : 0.0f;
          } else {
            float p = 0.0f;
            if (from_net) {
              val[0] = c.template bcast_lane<0>(reg_v); val[1] = c.template bcast_lane<1>(reg_v); val[2] = c.template bcast_lane<2>(reg_v);
              p = c.bcast(reg_pi, static_cast<int>(lf_mv));
              if (lane >= lf_k) p = 0.0f;
            } else {                  // dumb_eval: uniform over legal moves, u8 sum wraps (game_state.h:160-173)
#pragma unroll
              for (int i = 0; i <= P; ++i) val[i] = static_cast<float>(1.0 / (P + 1));
              const float ksum = static_cast<float>(lf_k & 0xFFu);
              if (lane < lf_k) p = (ksum == 0.0f) ? 0.0f : 1.0f / ksum;
            }
            const float sum = c.seqsum8(lane < lf_k ? p : 0.0f);
            p = p / sum;
            if (lane < lf_k) ar.nodes[tb + lf_c0 + lane].pr = p;
            fl_pr = p;
          }
          fl_node = c.cur; fl_mv = lf_mv; fl_meta = lf_meta;
          const float draw_share = val[P] / static_cast<int32_t>(P);
          const uint32_t plen = c.plen;
          float nq = 0.0f, nd = 0.0f, nv = lv_v;
          if (lane < plen) {
            const float vv = ((lv_pp == 0) ? val[0] : val[1]) + draw_share;
            nq = (lv_q * static_cast<float>(lv_n) + vv) / static_cast<float>(lv_n + 1);
            nd = (lv_d * static_cast<float>(lv_n) + val[P]) / static_cast<float>(lv_n + 1);
            NodeRec* nr = ar.nodes + tb + lv_node;
            nr->q = nq; nr->d = nd;
            if (lv_n == 0) { nv = ((lf_player == 0) ? val[0] : val[1]) + draw_share; nr->v = nv; }   // only the leaf can be a first visit
            nr->n = lv_n + 1;
          }
          fw_node = lv_node; fw_n = lv_n + 1; fw_q = nq; fw_d = nd; fw_v = nv; fw_plen = plen; fw = true;
          root_n += 1;
          if (lane == 0) ar.nodes[tb + root].n = root_n;
#pragma unroll
          for (int p = 0; p < P; ++p) if (static_cast<uint32_t>(p) == cp) c.t_depth[p] += 1;
          sims_done += 1;
        }
        // ---- MCTS::find_leaf (mcts.cc:462-498), plain PUCT, with the forwarded values patched in
        const uint64_t ph1 = PROF ? wall_clock64() : 0;
        typename GM::State leaf = c.gs;
        uint32_t cur = root, plen = 0, n = root_n;
        uint64_t meta = root_meta;
        float v_cur = root_v;
        bool prefix = true, failed = false;
        while (n > 0 && meta_term(meta) == 0) {
          if (plen >= ep.max_depth) { failed = true; break; }
          if (lane == 0) path[plen] = cur;
          uint32_t k = meta_nch(meta); const uint32_t c0 = meta_ch0(meta);
          if (k == 0) { failed = true; break; }
          // the node the last backup updated at this level: asked for here, with the child records, and used twice below (the patch
          // and the prefix test) - one permute and no round trip of its own behind the winner's
          const uint32_t t_node = c.bcast(fw_node, static_cast<int>(plen & 7u));
          // Every lane asks for a child record (the lanes past the children for the last child's, and a group whose children are all
          // in registers - the leaf evaluated a moment ago - for records it will not use): the loads stand in no exec-mask region, so
          // nothing has to wait for them where they are issued, and the parent's share of the select runs while they are on their way.
          const bool in_regs = cur == fl_node;
          const NodeRec* const cr = ar.nodes + tb + c0 + (lane < k ? lane : k - 1u);
          uint32_t n_l = cr->n; float q_l = cr->q, p_l = cr->pr, d_l = cr->d, v_l = cr->v; uint64_t m_l = cr->meta;
          float sqrt_n = SlotCtx<GM>::select_parent(n);
          // (the selects below read k as this statement leaves it, so they - and the wait for the records in front of them - stay
          // behind the square root instead of being scheduled ahead of it)
          asm volatile("" : "+v"(sqrt_n), "+v"(k));
          {
            const bool have = lane < k, mem = have && !in_regs;
            n_l = mem ? n_l : 0u; q_l = mem ? q_l : 0.0f; d_l = mem ? d_l : 0.0f; v_l = mem ? v_l : 0.0f;
            p_l = mem ? p_l : have ? fl_pr : 0.0f;
            m_l = mem ? m_l : have ? meta_pack(0, 0, fl_mv, 0, 0) : 0ull;
          }
          if (!in_regs) {
            if (fw && prefix && plen < fw_plen && plen < 8u) {   // one child of this node was updated by the last backup
              const uint32_t t_n = c.bcast(fw_n, static_cast<int>(plen));
              const float t_q = c.bcast(fw_q, static_cast<int>(plen)), t_d = c.bcast(fw_d, static_cast<int>(plen)), t_v = c.bcast(fw_v, static_cast<int>(plen));
              if (c0 + lane == t_node) { n_l = t_n; q_l = t_q; d_l = t_d; v_l = t_v; if (t_node == fl_node) m_l = fl_meta; }
            }
          }
          const float fpu = (cur == root) ? fpu_root : fpu_red;
          uint32_t best;
          if constexpr (GUM) {
            if (gum_active != 0u && cur == root) best = c.gumbel_next_root_child(cp, k, n_l, q_l, p_l);
            else if (gum_active != 0u && gum_full != 0u) best = c.gumbel_interior_select(cp, k, n_l, q_l, p_l, v_cur);
            else best = c.select_among(k, n_l, q_l, p_l, v_cur, sqrt_n, cpuct, fpu);
          } else {
            best = c.select_among(k, n_l, q_l, p_l, v_cur, sqrt_n, cpuct, fpu);
          }
          const uint32_t nxt = c0 + best;
          const uint32_t s_n = c.bcast(n_l, static_cast<int>(best));
          const float s_q = c.bcast(q_l, static_cast<int>(best)), s_d = c.bcast(d_l, static_cast<int>(best)), s_v = c.bcast(v_l, static_cast<int>(best));
          const uint64_t s_m = c.bcast(m_l, static_cast<int>(best));
          if (plen < 8u) {
            if (lane == plen) { lv_node = nxt; lv_n = s_n; lv_q = s_q; lv_d = s_d; lv_v = s_v; lv_pp = meta_player(meta); }
            prefix = prefix && plen < fw_plen && nxt == t_node;
          } else {
            prefix = false;
          }
          cur = nxt; n = s_n; meta = s_m; v_cur = s_v;
          GM::play(leaf, meta_mv(meta));
          ++plen;
        }
        if (failed) { c.raise(8u); final_state = kSlotDone; st = kGrpIdle; break; }
        const uint64_t ph2 = PROF ? wall_clock64() : 0;
        if constexpr (PROF) pf_lvls += plen;
        c.cur = cur; c.plen = plen;
        rec_ok = plen <= 8u;
#pragma unroll
        for (int p = 0; p < P; ++p) if (static_cast<uint32_t>(p) == cp) c.t_tld[p] += plen;
        uint32_t term = meta_term(meta);
        lf_k = meta_nch(meta); lf_c0 = meta_ch0(meta); lf_mv = 0; lf_meta = meta;
        if (n == 0) {
          term = GM::terminal(leaf);
          const uint64_t keep = meta_pack(0, 0, meta_mv(meta), leaf.player, term);
          if (!c.template expand_node<true>(cp, cur, leaf, keep, lf_c0, lf_k, &lf_mv)) { final_state = kSlotDone; st = kGrpIdle; break; }
          lf_meta = meta_pack(lf_c0, lf_k, meta_mv(meta), leaf.player, term);
        }
        lf_term = term; lf_player = leaf.player;
        const uint64_t ph3 = PROF ? wall_clock64() : 0;
        const bool needs_net = term == 0 && !c.seat_eval_random(cp);
        c.flags = needs_net ? (c.flags | kFlagLeafNeedsNet) : (c.flags & ~kFlagLeafNeedsNet);
        if (needs_net) {
          const uint64_t key = GM::key(leaf);
          // the answer table's granules are asked for inside the lookup, right behind the S3-FIFO shard's key loads (one round trip for
          // both); when they are valid - all ten carry this key's tags - the answer is there and the shard's payload round trip is
          // skipped; a shard hit the table did not have is copied into it (ten granule stores, nothing waits for them)
          unsigned long long l0a = 0, l0b = 0;
          const uint64_t lkey = TWO ? key ^ (mg ? kPipeGroupSalt : 0ull) : key;        // the answer table is one: group 1's lines under a salted key
          const unsigned long long* const le = pa.l0 + static_cast<size_t>(pipe_l0_entry(lkey, pa.l0_mask)) * kResStride;
          const bool hit = ep.cache_on && c.cache_lookup(key, mg, reg_pi, reg_v,
            [&]() {
              if (pa.l0) {
                if (lane < static_cast<uint32_t>(GM::M)) l0a = g_ld(le + lane);
                if (lane <= static_cast<uint32_t>(P)) l0b = g_ld(le + kResV + lane);
              }
            },
            [&](int cslot, float& o_pi, float& o_v) -> bool {
              if (!pa.l0) return false;
              const bool okl = (lane >= static_cast<uint32_t>(GM::M) || static_cast<uint32_t>(l0a >> 32) == pipe_l0_tag(lkey, lane)) &&
                               (lane > static_cast<uint32_t>(P) || static_cast<uint32_t>(l0b >> 32) == pipe_l0_tag(lkey, kResV + lane));
              if (!c.group_all(okl)) return false;
              o_pi = lane < static_cast<uint32_t>(GM::M) ? __uint_as_float(static_cast<uint32_t>(l0a)) : 0.0f;
              o_v = lane <= static_cast<uint32_t>(P) ? __uint_as_float(static_cast<uint32_t>(l0b)) : 0.0f;
              if (cslot < 0) l0_hits += 1;          // (the shard counted a miss: the host moves these to the hits)
              return true;
            },
            [&](float h_pi, float h_v) {
              if (pa.l0 && pa.l0_wb) {
                unsigned long long* const we = pa.l0 + static_cast<size_t>(pipe_l0_entry(lkey, pa.l0_mask)) * kResStride;
                if (lane < static_cast<uint32_t>(GM::M)) g_st(we + lane, (static_cast<unsigned long long>(pipe_l0_tag(lkey, lane)) << 32) | __float_as_uint(h_pi));
                if (lane <= static_cast<uint32_t>(P)) g_st(we + kResV + lane, (static_cast<unsigned long long>(pipe_l0_tag(lkey, kResV + lane)) << 32) | __float_as_uint(h_v));
              }
            });
          if (!hit) {
            // the request goes out NOW, not when the pass ends (its slowest group may run two more simulations): the net's
            // answer and this pass's tail overlap.  Nobody can take the slot before it is back: see the pass start.
            cur_key = key;
            seq = seq + 1u == 0u ? 1u : seq + 1u;
            uint32_t pos = 0;
            if (lane == 0) pos = atomicAdd(TWO ? pipe_tail_of(pc, mg) : &pc->tail, 1u);
            pos = c.template bcast_lane<0>(pos);
            const uint64_t payload = lane == 0 ? leaf.bb[0] : lane == 1 ? leaf.bb[1] : lane == 2 ? (static_cast<uint64_t>(slot) | (static_cast<uint64_t>(leaf.player) << 16))
                                                                                                  : static_cast<uint64_t>(seq);
            // (test hook, AZMI_PIPE_TEST_DROP = n: the request at ring position n goes out with a foreign lap tag - what an entry looks
            // like that was overwritten before its net workgroup could read it; tests/test_gpu_pipeline.py)
            const unsigned long long rtag = (pa.test_drop != 0u && pos == pa.test_drop) ? pipe_lap_tag(pos + kPipeRing) : pipe_lap_tag(pos);
            if (lane < kReqGranules)
              g_st((TWO ? pipe_ring_of(pa, mg) : pa.ring) + static_cast<size_t>(pos & (kPipeRing - 1u)) * kReqGranules + lane, (rtag << 48) | (payload & kMask48));
            // (the packed position stays with the slot: a request dropped by a pipeline error is sent again from there)
            if (lane < 3u) ar.leaf_pos[static_cast<size_t>(lane) * ep.S + slot] = lane == 2u ? static_cast<uint64_t>(leaf.player) : payload;
            if constexpr (TWO) { if (lane == 3u) ar.leaf_group[slot] = static_cast<uint8_t>(mg); }
            st = kGrpPush;
          }
        }
        if constexpr (PROF) {
          const uint64_t ph4 = wall_clock64();
          pf_ph[0] += ph1 - ph0; pf_ph[1] += ph2 - ph1; pf_ph[2] += ph3 - ph2; pf_ph[3] += ph4 - ph3; pf_ph[4] += 1;
        }
        if (st == kGrpPush) break;
        // the answer of this leaf is at hand (terminal, RANDOM evaluator, cache hit): the group goes on, a few times - the
        // pass ends with its slowest group
        if (++inline_sims >= pa.max_inline) break;
        // (the groups still here all have their next answer at hand; when only a few are left the other lanes of the wavefront idle:
        // the stragglers re-queue as READY instead and the pass ends)
        if (static_cast<uint32_t>(__popcll(__ballot(lane == 0))) < pa.min_active) break;
      }
    }
    const uint64_t pf_t3 = PROF ? wall_clock64() : 0;
    if constexpr (PROF) pf_pass += pf_t3 - pf_t2;


    // ---- the slots go back to HBM (k_sim's exit); the request's sequence number is drawn here, its flag is part of the state
    if (on) {
      if (st == kGrpPush) c.flags |= kFlagReqOut;
      if (lane == 0) {
        if (sims_done) ar.c_sims[slot] += sims_done;
        if (st == kGrpPush) { ar.c_evals[slot] += 1; ar.leaf_key[slot] = cur_key; }
      }
      if (rec_ok) {
        PathRegs r;
        r.node = lv_node; r.n = lv_n; r.q = lv_q; r.d = lv_d; r.v = lv_v; r.pp = lv_pp; r.mv = lf_mv; r.leaf_meta = lf_meta;
        c.store_pend(r);
        c.flags |= kFlagPendRec;
      } else {
        c.flags &= ~kFlagPendRec;
      }
      c.store(final_state);
    }
    // ---- tokens out, into this workgroup's own ring: READY tokens for the slots whose next answer is at hand (the requests went
    // out when their leaves were found), READY tokens with the move bit for the slots whose next step is the move step's.  The
    // ring TICKET is drawn before the stores have drained (it only reserves positions: its round trip and the drain overlap); the
    // tokens themselves go out behind the drain.
    {
      const bool tok_out = on && lane == 0 && (st == kGrpReady || listed);
      const unsigned long long rm = __ballot(tok_out);
      uint32_t base = 0;
      if (rm && wlane == 0) base = atomicAdd(&wc->rtail, static_cast<uint32_t>(__popcll(rm)));
      // everything this pass wrote is in L2 before any of its tokens is out (workgroup scope: the slots stay on this CU)
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      // the slot is whole: publish it (the word a token's taker waits for)
      if (on && lane == 0) g_st(ar.req_seq + slot, seq);
      if (rm) {
        base = __builtin_amdgcn_readfirstlane(base);
        if (tok_out) {
          const uint32_t pos = base + static_cast<uint32_t>(__popcll(rm & ((1ull << (grp * 8)) - 1ull)));
          g_st(myring + (pos & rmask), (pipe_lap_tag_r(pos, pa.rshift) << 48) | static_cast<unsigned long long>(slot) | (listed ? kTokMove : 0ull));
        }
      }
    }
    // ---- the epoch's counts: simulations (the quota ends it), slots lost to an engine error
    {
      uint32_t x = lane == 0 ? sims_done + sims_mem : 0u;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
      if (wlane == 0 && x) atomicAdd(&pe->sims, static_cast<unsigned long long>(x));
      if (pa.l0) {
        uint32_t y = lane == 0 ? l0_hits : 0u;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) y += __shfl_xor(y, off, 64);
        if (wlane == 0 && y) atomicAdd(&pc->l0_hits, static_cast<unsigned long long>(y));
      }
      const unsigned long long fm = __ballot(on && lane == 0 && final_state == kSlotDone);
      if (wlane == 0 && fm) atomicAdd(&pe->dead, static_cast<uint32_t>(__popcll(fm)));
    }
    if constexpr (PROF) pf_io += wall_clock64() - pf_t3;
  }

  if (wlane == 0) g_st(&pe->stop, 1u);       // a tree wavefront leaves: the epoch is over (also when it never began: engine stopped, error)
  if (PROF && wlane == 0) {
    atomicAdd(&pc->prof[0], pf_pass); atomicAdd(&pc->prof[1], pf_idle); atomicAdd(&pc->prof[2], pf_n); atomicAdd(&pc->prof[3], pf_act);
    atomicAdd(&pc->prof[4], pf_polls); atomicAdd(&pc->prof[5], pf_io);
    atomicAdd(&pc->prof[9], pf_ph[0]); atomicAdd(&pc->prof[10], pf_ph[1]); atomicAdd(&pc->prof[11], pf_ph[2]); atomicAdd(&pc->prof[12], pf_ph[3]);
    atomicAdd(&pc->prof[13], pf_ph[4]); atomicAdd(&pc->prof[14], pf_lvls); atomicAdd(&pc->prof[15], pf_mv); atomicAdd(&pc->prof[6], static_cast<unsigned long long>(wall_clock64() - t_start));
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) { wc->rhead = s_head; atomicAdd(&pe->tree_done, 1u); }
}

// ---- the generic tree kernel: every search variant, two model groups -----------------------------------------------------------
// Engines the fast kernel above does not drive - Gumbel seats (k_sim is plain PUCT), two model groups (play_past: a leaf goes to the
// net of its seat's group) - run EVERY step through the lock-step engine's own round_slot<kMover> (pipe_move_groups): a pass = the
// tokens that have arrived, for an answer token first the answer (granules -> the slot's (v, pi) rows, the insert log), then one
// step per slot (backup, a move if the search is complete, descent to the next leaf, cache probe), then a request (sent by
// pipe_move_groups, into the ring of the leaf's group) or - when the answer is at hand - the slot's token back into the ring.  One
// simulation per slot and pass instead of the fast kernel's several, but no round barrier: a slot waits for its own answer only.
// Same rings, granules, home workgroups, epoch boundaries and exit conditions as k_pipe_tree.
// DIAG (AZMI_PIPE_DIAG=1, a build of its own): round 5's instrumentation of the stall hunt - phase stamps, segment clocks, the longest
// interval between two looks - written into PipeWg::pad (the line of rtail, the word net workgroups add to: hence not on by default,
// ADVICE r5) with s_waitcnt fences around the poll loop's loads so that each segment can be clocked.
template <class GM, int NT, bool DIAG = false>
__global__ __launch_bounds__(NT, 2) void k_pipe_tree_generic(PipeKernArgs ka) {
  constexpr int P = GM::P;
  const EngineParams& ep = ka.ep;
  const EngineArrays& ar = ka.ar;
  const PipeArrays& pa = ka.pa;
  const uint32_t wlane = threadIdx.x & 63u, grp = wlane >> 3, lane = wlane & 7u;
  uint64_t t_start = wall_clock64(), t_last = t_start;
  PipeCtl* const pc = pa.ctl;
  PipeEpoch* const pe = pa.ep;
  PipeWg* const wc = pa.wg + blockIdx.x;
  // where every wavefront of this workgroup is (diagnostics of the rare stall-cap error): PipeWg::pad[2 + wave] =
  // phase | units of 10 us since the wave started << 8; the host prints the words of every tree workgroup with a pipeline error
  uint32_t* const phase_word = &wc->pad[2 + (threadIdx.x >> 6)];
  // (an epoch that starts with the error word already set - the epochs of a call that were enqueued behind the failing one - leaves
  // the diagnostics of the failing epoch alone)
  const bool diag_on = DIAG && g_ld(&pc->err) == 0u;
#define AZMI_GEN_PHASE(x) do { if (DIAG && wlane == 0 && diag_on) g_st(phase_word, static_cast<uint32_t>(x) | (static_cast<uint32_t>((wall_clock64() - t_start) / 1000u) << 8)); } while (0)
  AZMI_GEN_PHASE(1);
  // (when each wavefront of the workgroup ENTERED the kernel: the raw clock, low 32 bits - do the four start together?)
  if (DIAG && wlane == 0 && diag_on) g_st(&wc->pad[6 + (threadIdx.x >> 6)], static_cast<uint32_t>(t_start));
  const uint32_t rmask = (1u << pa.rshift) - 1u;
  unsigned long long* const myring = pa.rring + (static_cast<size_t>(blockIdx.x) << pa.rshift);
  if (threadIdx.x == 0) {
    unsigned long long t0 = atomicCAS(&pe->t0, 0ull, static_cast<unsigned long long>(t_start));
    if (t0 == 0ull) t0 = t_start;
    atomicMax(&pe->tree_late, static_cast<uint32_t>(t_start > t0 ? t_start - t0 : 0ull));
    const uint32_t before = atomicAdd(&pe->tree_arrived, 1u);
    asm volatile("s_waitcnt vmcnt(0)" :: "v"(before) : "memory");
  }
  __syncthreads();
  AZMI_GEN_PHASE(2);
  if (pa.census_hold != 0u) {        // calibration launch: see k_pipe_tree
    const unsigned long long t0 = g_ld(&pe->t0);
    if (threadIdx.x == 0 && t_start > t0 && t_start - t0 >= pa.census_hold) atomicAdd(&pe->tree_late_n, 1u);
    while (wall_clock64() < t0 + pa.census_hold) __builtin_amdgcn_s_sleep(32);
    return;
  }
  bool go = g_ld(&ar.ctl->stop) == 0 && g_ld(&pc->err) == 0 && g_ld(&pe->stop) == 0;
  __shared__ uint32_t s_head;
  if (threadIdx.x == 0) s_head = wc->rhead;
  __syncthreads();
  const PipeKernArgs* const kargs = reinterpret_cast<const PipeKernArgs*>(reinterpret_cast<uintptr_t>(__builtin_amdgcn_kernarg_segment_ptr()));
  uint64_t seg_max[3] = {0, 0, 0}, sg_prev = DIAG ? __builtin_amdgcn_s_memtime() : 0ull;
  uint64_t ph_max[5] = {0, 0, 0, 0, 0};
  uint64_t gap_rt = 0, gap_sq = 0, sq_last = DIAG ? __builtin_amdgcn_s_memtime() : 0ull;
  uint32_t gap_where = 0, did_pass = 0, gap_polls = 0, total_polls = 0;
  while (go) {
    AZMI_GEN_PHASE(3);
    // ---- tokens (as k_pipe_tree: the arrived prefix of the eight ring positions at the LDS head)
    uint32_t my_slot = kNoSlot, tok_seq = 0, empty_polls = 0, ctl_word = 0;
    bool fresh_pass = true;
    for (;;) {
      const uint64_t sg0 = DIAG ? __builtin_amdgcn_s_memtime() : 0ull;
      const uint32_t h = __builtin_amdgcn_readfirstlane(*const_cast<volatile uint32_t*>(&s_head));
      unsigned long long tok = 0;
      bool here = false;
      if (lane == 0) {
        const uint32_t pos = h + grp;
        tok = g_ld(myring + (pos & rmask));
        here = (tok >> 48) == pipe_lap_tag_r(pos, pa.rshift);
      }
      uint64_t sg1 = 0;
      if constexpr (DIAG) {
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" :: "v"(tok) : "memory");
        sg1 = __builtin_amdgcn_s_memtime();
        if (sg1 - sg0 > seg_max[0]) seg_max[0] = sg1 - sg0;          // (diagnostics: LDS head + the token load)
      }
      if ((empty_polls & 3u) == 0u) {
        ctl_word = 0;
        if (wlane == 7) ctl_word = g_ld(&pe->stop) | g_ld(&pc->err) | g_ld(&ar.ctl->stop);
        else if (wlane == 15) ctl_word = g_ld(&pe->sims) >= pa.quota ? 1u : 0u;
        else if (wlane == 23) ctl_word = g_ld(&pe->ended);
        else if (wlane == 31) ctl_word = g_ld(&pe->dead);
      }
      if constexpr (DIAG) {
        asm volatile("s_waitcnt vmcnt(0)" :: "v"(ctl_word) : "memory");
        const uint64_t sg2 = __builtin_amdgcn_s_memtime();
        if (sg2 - sg1 > seg_max[1]) seg_max[1] = sg2 - sg1;          // (the control words)
        if (sg0 - sg_prev > seg_max[2]) seg_max[2] = sg0 - sg_prev;  // (from the last look's control words to this look's start: the sleep, a pass)
        sg_prev = sg2;
      }
      uint32_t stop_seen = __builtin_amdgcn_readlane(ctl_word, 7) | __builtin_amdgcn_readlane(ctl_word, 15);
      {
        const uint32_t w = __builtin_amdgcn_readlane(ctl_word, 23), d = __builtin_amdgcn_readlane(ctl_word, 31);
        const uint32_t with_game = ep.S > d ? ep.S - d : 0u;
        const uint32_t thr = max(1u, static_cast<uint32_t>((static_cast<unsigned long long>(with_game) * pa.idle_num) >> 10));
        if (w >= thr || w + d >= ep.S) stop_seen = 1u;
      }
      const uint64_t now = wall_clock64();
      if constexpr (DIAG) {   // diagnostics: the longest interval between two looks of this wavefront by the 100 MHz wall clock, the same interval by the SQ's
          // own counter (s_memtime), and where the wavefront was in between (0: only this poll loop, 1: a pass)
        const uint64_t sq_now = __builtin_amdgcn_s_memtime();
        if (now - t_last > gap_rt) { gap_rt = now - t_last; gap_sq = sq_now - sq_last; gap_where = did_pass; gap_polls = total_polls; }
        sq_last = sq_now; did_pass = 0u; ++total_polls;
      }
      if (fresh_pass) { t_last = now; fresh_pass = false; }
      else pipe_freeze_credit(pc, now, t_last, t_start, wlane == 0);
      if (now - t_start > pa.soft_ticks) stop_seen = 1u;
      if (now - t_start > pa.cap_ticks) {
        if (wlane == 0) {
          atomicOr(&pc->err, static_cast<uint32_t>(kPipeErrTimeout));
          if (atomicAdd(&pc->dbg[0], 1u) == 0u) { pc->dbg[1] = blockIdx.x; pc->dbg[2] = empty_polls; pc->dbg[3] = h; pc->dbg[4] = 0xCCCCu; pc->dbg[5] = wc->rtail; pc->dbg[6] = static_cast<uint32_t>(pa.soft_ticks / 1000u); }
        }
        stop_seen = 1u;
      }
      if (stop_seen) { if (wlane == 0) g_st(&pe->stop, 1u); go = false; break; }
      const unsigned long long hm = __ballot(here);
      uint32_t k = 0;
      while (k < kTreeWindow && ((hm >> (8 * k)) & 1ull)) ++k;
      if (k == 0u) { ++empty_polls; __builtin_amdgcn_s_sleep(16); continue; }
      uint32_t won = 0;
      if (wlane == 0) won = atomicCAS(&s_head, h, h + k) == h ? 1u : 0u;
      if (__builtin_amdgcn_readfirstlane(won) == 0u) continue;
      const uint32_t sl = static_cast<uint32_t>(__shfl(static_cast<uint32_t>(tok & 0xFFFFull), static_cast<int>(grp * 8), 64));
      const uint32_t sq = static_cast<uint32_t>(__shfl(static_cast<uint32_t>((tok >> 16) & 0xFFFFFFFFull), static_cast<int>(grp * 8), 64));
      if (grp < k) { my_slot = sl & static_cast<uint32_t>(kTokSlotMask); tok_seq = sq; }
      break;
    }
    if (!go) break;
    did_pass = 1u;
    uint64_t ph_t = DIAG ? __builtin_amdgcn_s_memtime() : 0ull;
#define AZMI_GEN_SEG(i) do { if constexpr (DIAG) { const uint64_t t_ = __builtin_amdgcn_s_memtime(); if (t_ - ph_t > ph_max[i]) ph_max[i] = t_ - ph_t; ph_t = t_; } } while (0)
    AZMI_GEN_PHASE(4);
    // ---- an answer token: the slot is back once req_seq shows the token's number; its granules become the slot's (v, pi) rows
    if (my_slot != kNoSlot && tok_seq != 0u) {
      while (g_ld(ar.req_seq + my_slot) != tok_seq) {
        if (wall_clock64() - t_start > pa.cap_ticks) {
          if (lane == 0 && atomicAdd(&pc->dbg[0], 1u) == 0u) { pc->dbg[1] = my_slot; pc->dbg[2] = tok_seq; pc->dbg[3] = g_ld(ar.req_seq + my_slot); pc->dbg[4] = 0xAAAAu; pc->dbg[5] = ar.sstate[my_slot]; pc->dbg[6] = ar.flags[my_slot]; }
          if (lane == 0) atomicOr(&pc->err, static_cast<uint32_t>(kPipeErrTimeout));
          my_slot = kNoSlot; break;
        }
        __builtin_amdgcn_s_sleep(2);
      }
    }
    bool answered = false;
    float reg_pi = 0.0f, reg_v = 0.0f;
    AZMI_GEN_SEG(0);      // the wait for the slot's publication word
    AZMI_GEN_PHASE(5);
    if (my_slot != kNoSlot && tok_seq != 0u) {
      const unsigned long long* const res = pa.res + static_cast<size_t>(my_slot) * kResStride;
      unsigned long long g0 = 0, g1 = 0;
      for (;;) {
        if (lane < static_cast<uint32_t>(GM::M)) g0 = g_ld(res + lane);
        if (lane <= static_cast<uint32_t>(P)) g1 = g_ld(res + kResV + lane);
        const bool okl = (lane >= static_cast<uint32_t>(GM::M) || static_cast<uint32_t>(g0 >> 32) == tok_seq) &&
                         (lane > static_cast<uint32_t>(P) || static_cast<uint32_t>(g1 >> 32) == tok_seq);
        if (((__ballot(okl) >> (grp * 8u)) & 0xFFull) == 0xFFull) { answered = true; break; }      // (the group's byte of the ballot: all eight agree)
        if (wall_clock64() - t_start > pa.cap_ticks) {
          if (lane == 0 && atomicAdd(&pc->dbg[0], 1u) == 0u) { pc->dbg[1] = my_slot; pc->dbg[2] = tok_seq; pc->dbg[3] = static_cast<uint32_t>(g0 >> 32); pc->dbg[4] = 0xBBBBu; pc->dbg[5] = static_cast<uint32_t>(g1 >> 32); pc->dbg[6] = g_ld(ar.req_seq + my_slot); }
          if (lane == 0) atomicOr(&pc->err, static_cast<uint32_t>(kPipeErrTimeout));
          my_slot = kNoSlot; break;
        }
        __builtin_amdgcn_s_sleep(2);
      }
      if (answered) {
        reg_pi = lane < static_cast<uint32_t>(GM::M) ? __uint_as_float(static_cast<uint32_t>(g0)) : 0.0f;
        reg_v = lane <= static_cast<uint32_t>(P) ? __uint_as_float(static_cast<uint32_t>(g1)) : 0.0f;
        if (lane < static_cast<uint32_t>(GM::M)) ar.pi[static_cast<size_t>(my_slot) * GM::M + lane] = reg_pi;
        if (lane <= static_cast<uint32_t>(P)) ar.v[static_cast<size_t>(my_slot) * (P + 1) + lane] = reg_v;
        if (lane == 0) ar.flags[my_slot] = ar.flags[my_slot] & static_cast<uint8_t>(~kFlagReqOut);
      }
    }
    AZMI_GEN_SEG(1);      // the answer's granules
    if (ep.cache_on) {        // PlayManager::update_inferences -> insert_many: logged with the leaf's group, applied after the epoch
      const unsigned long long am = __ballot(answered && lane == 0);
      if (am) {
        uint32_t base = 0;
        if (wlane == 0) base = atomicAdd(&pe->ins_count, static_cast<uint32_t>(__popcll(am)));
        base = __builtin_amdgcn_readfirstlane(base);
        if (answered) {
          const uint32_t idx = base + static_cast<uint32_t>(__popcll(am & ((1ull << (grp * 8)) - 1ull)));
          if (idx < pa.ins_cap) {
            if (lane == 0) { pa.ins_key[idx] = ar.leaf_key[my_slot]; if (pa.ins_grp) pa.ins_grp[idx] = ar.leaf_group[my_slot]; }
            if (lane < static_cast<uint32_t>(GM::M)) pa.ins_pi[static_cast<size_t>(idx) * GM::M + lane] = reg_pi;
            if (lane <= static_cast<uint32_t>(P)) pa.ins_v[static_cast<size_t>(idx) * (P + 1) + lane] = reg_v;
          } else if (lane == 0) {
            g_st(&pe->stop, 1u);
          }
        }
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the rows are in place before the step reads them
    AZMI_GEN_SEG(2);      // the insert-log ticket and the drain
    AZMI_GEN_PHASE(6);
    // ---- one step of every slot of the pass (requests leave inside)
    const uint32_t rs = pipe_move_groups<GM>(kargs->ep, kargs->ar, kargs->pa, my_slot);
    AZMI_GEN_SEG(3);      // the steps themselves (round_slot, the requests)
    AZMI_GEN_PHASE(7);
    // ---- a slot whose next answer is at hand (cache hit, terminal leaf, RANDOM seat) goes straight back into the ring
    {
      const bool tok_out = my_slot != kNoSlot && lane == 0 && rs == kSlotWaitEval;
      const unsigned long long rm = __ballot(tok_out);
      uint32_t base = 0;
      if (rm && wlane == 0) base = atomicAdd(&wc->rtail, static_cast<uint32_t>(__popcll(rm)));
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (rm) {
        base = __builtin_amdgcn_readfirstlane(base);
        if (tok_out) {
          const uint32_t pos = base + static_cast<uint32_t>(__popcll(rm & ((1ull << (grp * 8)) - 1ull)));
          g_st(myring + (pos & rmask), (pipe_lap_tag_r(pos, pa.rshift) << 48) | static_cast<unsigned long long>(my_slot));
        }
      }
    }
    AZMI_GEN_SEG(4);      // the READY tokens
#undef AZMI_GEN_SEG
  }
  AZMI_GEN_PHASE(8);
  if (wlane == 0) g_st(&pe->stop, 1u);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  AZMI_GEN_PHASE(9);
  if (DIAG && threadIdx.x == 0 && diag_on) {      // (wavefront 0's longest interval between two looks: 10 us units by the wall clock | by the SQ clock, raw ticks >> 10 | where | after how many polls)
    for (int i = 0; i < 5; ++i) wc->pad[18 + i] = static_cast<uint32_t>(ph_max[i] >> 10);
    wc->pad[15] = static_cast<uint32_t>(seg_max[0] >> 10); wc->pad[16] = static_cast<uint32_t>(seg_max[1] >> 10); wc->pad[17] = static_cast<uint32_t>(seg_max[2] >> 10);
    wc->pad[10] = static_cast<uint32_t>(gap_rt / 1000u); wc->pad[11] = static_cast<uint32_t>(gap_sq >> 10); wc->pad[12] = gap_where; wc->pad[13] = gap_polls; wc->pad[14] = total_polls;
  }
  if (threadIdx.x == 0) { wc->rhead = s_head; atomicAdd(&pe->tree_done, 1u); }
#undef AZMI_GEN_PHASE
}

}  // namespace azmi
