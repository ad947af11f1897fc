// Plain-data views and constants of the batched position search that its host side (search_batch*.hip, search_batch_host.h) and
// its kernels (the four search_*_kernels.h) share, and the layouts of the device blocks that hold several arrays in one allocation
// (block_cut.h: one function per block is both its size and its carving).  What each array means is told where its kernels are.
// Plain C++: a host-only unit, or a program built without HIP, can include this.
#pragma once
#include <cstddef>
#include <cstdint>

#include "block_cut.h"

namespace azmi {

// WU-UCT batched API state (mcts.cc:752-851): Node::n_in_flight per arena node + the in_flight_ list.  Every kernel of the
// object that can create nodes clears the marks of the nodes it created, so the array always describes live nodes.
// (mcts_object_kernels.h's; it sits here because SbWuArrays holds one)
struct WuArrays {
  uint32_t* nif;        // [trees * cap] Node::n_in_flight
  uint32_t* ifl_path;   // [ifl_cap][max_depth] InFlightLeaf::path
  uint32_t* ifl_plen;   // [ifl_cap]
  uint32_t* ifl_cur;    // [ifl_cap] InFlightLeaf::leaf
};

// the read-out kinds of azmi_mcts_query / azmi_search_query (mcts_object_kernels.h's too; here so that host-only units can name them)
enum MctsQuery : uint32_t {
  kQCounts = 0, kQProbs = 1, kQProbsPruned = 2, kQRootValue = 3, kQRootQ = 4, kQScalars = 5, kQGumbelPolicy = 6,
  kQGumbelFinal = 7, kQAddRootNoise = 8, kQApplyRootTemp = 9, kQPickMove = 10, kQPrincipalVariation = 11, kQSetGumbelSims = 12, kQRootChildren = 13
};

// ---- search_batch_kernels.h ------------------------------------------------------------------------------------------------------
enum SbPend : uint8_t {
  kPendNone = 0,    // nothing to back up: terminal leaf (backed up by the find kernel), or a stopped tree
  kPendRow = 1,     // the leaf's planes are in the slot's canonical row: the evaluator's answer is awaited
  kPendCached = 2,  // a cache hit: the answer is already in the slot's (v, pi) rows
  kPendRandom = 3,  // EvalType::RANDOM: process_result synthesises dumb_eval
  kPendRollout = 4  // EvalType::PLAYOUT: the answer of the leaf's rollout is (Connect4: will be, behind k_sb_rollout) in the slot's (v, pi) rows
};
enum SbStatus : int32_t {
  kSbFinished = 1,     // the game is over
  kSbPaused = 2,       // the tree has reached its target of the running search_to call: set and cleared by the checkpoint kernels alone
  kSbBadStart = -1,    // bad start position
  kSbFindFailed = -2,  // find_leaf failed: arena / path capacity
  kSbBadMove = -3,     // update_root was given a move the root does not have
  kSbNoVisits = -4,    // a move was asked of a root without visits
  kSbBadState = -5     // the root state did not take a move its tree has
};
constexpr uint32_t kNoRow = 0xFFFFFFFFu;

struct SbArrays {
  uint8_t* pend;       // [N]
  int32_t* status;     // [N]
  uint32_t* row_of;    // [N]
  uint32_t* rows;      // [N]
  uint32_t* n_rows;    // [1]
  uint32_t* n_term;    // [N] simulations that ended in a terminal leaf since the last reset
};

struct SbWuArrays {
  WuArrays wu;         // nif [N * P * cap]; in-flight records [K * N]: ifl_path[max_depth], ifl_plen, ifl_cur
  uint8_t* pend;       // [K * N] SbPend of descent k of tree i (kPendRow or kPendNone: everything else is backed up by the find kernel)
  uint32_t* row_of;    // [K * N] compacted row of the entry (kNoRow = none)
  uint32_t* rows;      // [K * N] entry of compacted row r: the net's row list
  uint32_t* tree_of;   // [K * N] tree of compacted row r (ascending, with repeats)
  float* canon;        // [K * N, C, H, W]
  float* v;            // [K * N, P + 1]
  float* pi;           // [K * N, M]
  uint64_t* keys;      // [K * N] cache keys of the evaluated entries (0 = none)
};

struct SbPlayArrays {
  int32_t* move;       // [N]
  int32_t* log;        // [N, log_cap]
  uint32_t* log_len;   // [N]
  float* final;        // [N, P + 1]
  uint32_t log_cap;
};

struct SbRollArrays {
  uint64_t* seeds;     // [N] rollout_seeds
  uint32_t* count;     // [N] rollouts of tree i since the last reset: the j of its next one
  uint8_t* states;     // [N] GM::State (Connect4, K == 1): the leaf that awaits k_sb_rollout
};

constexpr uint32_t kSbMaxCheckpoints = 32;

struct SbSweepArrays {
  uint32_t* target;     // [N]
  uint32_t* cps;        // [kSbMaxCheckpoints]
  uint32_t* taken;      // [N]
  uint32_t* root_n;     // [N, J]
  uint32_t* counts;     // [N, J, M]
  float* probs;         // [N, J, M]
  float* root_values;   // [N, J, 3]
  float* root_q;        // [N, J, M]
  uint32_t n_cp;        // J
};

struct SbDlArrays {
  uint32_t* todo;       // [N]
  uint32_t* todo_max;   // [2]
};

// ---- search_pool_kernels.h -------------------------------------------------------------------------------------------------------
//   key[i][p], player[i][p], variant[i][p]   the root of tree i when it had played p moves since reset (p < log_cap)
//   len[i]                                   1 + the largest ply captured of tree i since reset
struct SbCaptureArrays {
  uint64_t* key;       // [N, log_cap]
  uint8_t* player;     // [N, log_cap]
  int8_t* variant;     // [N, log_cap]  -1 for a game without variants
  uint32_t* len;       // [N]
};

constexpr uint32_t kPoolEmpty = 0xFFFFFFFFu;
constexpr uint32_t kPoolMaxRecords = 1u << 30;      // 2 n slots indexed by 32 bits

// ---- search_frontier_kernels.h ---------------------------------------------------------------------------------------------------
//   reach[i], temp[i]       the caller's reach probability and sampling temperature of tree i
//   kind[i]                 0 a searched live root, 1 a terminal root (value = its scores, no children), 2 the tree takes no part
//                           (finished, stopped or reach == 0: zero rows)
//   keep[i][a]              move a of tree i is kept; kept[i] = how many are
//   record r of tree i      first_child[i] <= r < first_child[i + 1], ascending action; r >= max_children is not written
struct SbFrontierArrays {
  const double* reach;     // [N]
  const double* temp;      // [N]
  uint8_t* kind;           // [N]
  uint64_t* key;           // [N]
  double* raw_pi;          // [N, M]
  double* samp_pi;         // [N, M]
  uint8_t* keep;           // [N, M]
  double* entropy;         // [N]
  double* value;           // [N, 3]
  uint32_t* kept;          // [N]
  uint32_t* first_child;   // [N + 1]
  uint32_t* total;         // [1]
  uint32_t* parent;        // [max_children] ...
  uint32_t* action;
  double* child_reach;
  uint64_t* child_key;
  uint8_t* child_player;
  int8_t* child_variant;   // -1 for a game without variants
  uint8_t* child_terminal;
  float* child_scores;     // [max_children, P + 1]
  uint32_t max_children;
};

// ---- search_sweep_metrics_kernels.h ----------------------------------------------------------------------------------------------
// the columns of a row, in the order of azmi_search_sweep_metrics' out_rows
enum SweepCol : uint32_t {
  kSwJsd = 0, kSwTv, kSwHellinger, kSwTop1, kSwTop3, kSwTop9,      // the six of azmi_policy_divergences, in its order
  kSwReward, kSwRegret, kSwPressure, kSwBenefit, kSwEntropy, kSwValueGap, kSwAbsErr, kSwCloserAnchor, kSwCloserRaw,
  kSweepCols
};
constexpr uint32_t kPolicyCols = 6;
constexpr uint32_t kSweepMeanThreads = 256;

// the output block of azmi_search_sweep_metrics for the J checkpoints of the current snapshot set
struct SweepMetricsOut {
  double *rows, *ceiling, *mean, *outcomes;
  uint32_t* count;
  uint8_t* valid;
};

// ---- the blocks: N trees, M moves, V = P + 1 scores; the arrays in descending element size, so no take pads ------------------------
// The snapshots of azmi_search_run_to with room for `cap` checkpoints: [taken | root_n | counts | probs | root_values | root_q]
// (cleared by every call) and [target | cps] behind them (uploaded by every call).  Rows are indexed with the call's own J, so a
// block cut for more checkpoints serves fewer.  Returns the bytes of the leading part: the offset at which `target` starts
inline size_t sb_cut_sweep(BlockCut& c, SbSweepArrays& sw, size_t N, size_t M, size_t cap) {
  sw.taken = c.take<uint32_t>(N);
  sw.root_n = c.take<uint32_t>(N * cap);
  sw.counts = c.take<uint32_t>(N * cap * M);
  sw.probs = c.take<float>(N * cap * M);
  sw.root_values = c.take<float>(N * cap * 3);
  sw.root_q = c.take<float>(N * cap * M);
  const size_t clear_bytes = c.off;
  sw.target = c.take<uint32_t>(N);
  sw.cps = c.take<uint32_t>(kSbMaxCheckpoints);
  return clear_bytes;
}

// the per-tree arrays of azmi_search_expand (reach | temp are neighbours: one upload fills both)
inline void sb_cut_frontier_trees(BlockCut& c, SbFrontierArrays& fr, size_t N, size_t M) {
  fr.reach = c.take<double>(N);
  fr.temp = c.take<double>(N);
  fr.raw_pi = c.take<double>(N * M);
  fr.samp_pi = c.take<double>(N * M);
  fr.entropy = c.take<double>(N);
  fr.value = c.take<double>(3 * N);
  fr.key = c.take<uint64_t>(N);
  fr.kept = c.take<uint32_t>(N);
  fr.first_child = c.take<uint32_t>(N + 1);
  fr.total = c.take<uint32_t>(1);
  fr.kind = c.take<uint8_t>(N);
  fr.keep = c.take<uint8_t>(N * M);
}

// its per-record arrays with room for `cap` records
inline void sb_cut_frontier_records(BlockCut& c, SbFrontierArrays& fr, size_t cap, size_t V) {
  fr.child_reach = c.take<double>(cap);
  fr.child_key = c.take<uint64_t>(cap);
  fr.parent = c.take<uint32_t>(cap);
  fr.action = c.take<uint32_t>(cap);
  fr.child_scores = c.take<float>(cap * V);
  fr.child_player = c.take<uint8_t>(cap);
  fr.child_variant = c.take<int8_t>(cap);
  fr.child_terminal = c.take<uint8_t>(cap);
}

// rows [N, cap, 15] | ceiling [N] | mean [cap, 15] | outcomes [N] f64, count [cap, 15] u32, valid [N, cap] u8
inline void sb_cut_sweep_metrics(BlockCut& c, SweepMetricsOut& o, size_t N, size_t cap) {
  o.rows = c.take<double>(N * cap * kSweepCols);
  o.ceiling = c.take<double>(N);
  o.mean = c.take<double>(cap * kSweepCols);
  o.outcomes = c.take<double>(N);
  o.count = c.take<uint32_t>(cap * kSweepCols);
  o.valid = c.take<uint8_t>(N * cap);
}

}  // namespace azmi
