// Host-side state of one batched position search and what the translation units behind azmi_search_* share:
//   search_batch.hip           the one device module of the four search_*_kernels.h (a kernel's code depends on its module-mates
//                              and on the order they are instantiated in, DESIGN.md sections 1 and 8.3): every launch function
//                              below and nothing else
//   search_batch_create.hip    azmi_search_create / destroy / set_leaves_per_step / set_descents_per_step / host_reads / reset /
//                              set_rollout_seeds
//   search_batch_steps.hip     the sb_begin_* / sb_check_* checks, sb_search_args, sb_enqueue_step / search; azmi_search_find_leaves /
//                              leaves_to_host / process_results* / run*
//   search_batch_moves.hip     azmi_search_pick_moves / update_roots / root_prior / play*, game_state / query / sync / stats
//   search_batch_sweep.hip     azmi_search_run_to / checkpoints / sweep_metrics, azmi_policy_divergences
//   search_batch_pool.hip      azmi_search_set_capture / capture_roots / captured / net_metrics, azmi_pool_unique
//   search_batch_frontier.hip  azmi_search_expand / frontier
// All but the first are host code only: no kernel header, no launch of their own, no device code in their objects.
// The engine behind a search is a PlayManager engine with N slots built from the MCTS constructor's arguments (azmi_host_mcts_params,
// as azmi_mcts_create does for its one slot); the engine's own game loop never runs on it.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/azmi.h"
#include "engine_host.h"
#include "search_batch_types.h"

#define SB_FAIL azmi_host_fail
#define SB_TRY AZMI_HIP_TRY

struct azmi_search {
  azmi_pm* pm = nullptr;
  uint32_t n = 0, max_sims = 0;
  uint32_t sims_done = 0;      // descents that count against max_sims: since reset (Connect4), since the last update_roots (wide games)
  bool flat_arena = false;     // Connect4: the arena never reclaims.  Wide games: two halves, compacted behind update_roots
  float root_temp = 1.0f;
  azmi::SbPlayArrays pl{};
  int32_t* d_moves_in = nullptr;  // [N] a caller's moves for update_roots
  uint32_t chw = 0, vec_f = 0, vec_u = 0;
  bool ready = false;          // reset() has given every tree a position
  bool step_pending = false;   // find_leaves() without its process_results()
  bool gumbel = false;
  uint32_t step_rows = 0;
  azmi::SbArrays sb{};
  uint64_t* d_keys = nullptr;     // [N] ar.cache_keys of a search with a cache attached
  float* d_batch = nullptr;       // [N, C, H, W] compacted leaf batch of the step API
  float* d_vrows = nullptr;       // [N, P+1] / [N, M]: host evaluator answers staged for the step API
  float* d_pirows = nullptr;
  float* d_qf = nullptr;          // [N, vec_f] / [N, vec_u] read-out buffers
  uint32_t* d_qu = nullptr;
  uint64_t launches = 0, net_calls = 0, steps = 0;
  // several leaves in flight per tree and step (azmi_search_set_leaves_per_step): allocated only when K > 1
  uint32_t k_leaves = 1;
  uint32_t step_k = 0;            // descents of the pending find_leaves step
  azmi::SbWuArrays wu{};
  float* d_batch_wu = nullptr;    // [K * N, ...] the step API's buffers of a K > 1 step (d_batch, d_vrows, d_pirows hold N rows)
  float* d_vrows_wu = nullptr;
  float* d_pirows_wu = nullptr;
  std::vector<void*> wu_allocs;
  // EvalType::PLAYOUT: the rollout seed and rollout count of every tree, the parked leaf states of a Connect4 K == 1 step
  azmi::SbRollArrays ro{};
  std::vector<uint64_t> tree_seeds;   // seeds of the last reset: the default rollout seeds derive from them
  // search to targets (azmi_search_run_to): allocated by the first call, regrown when it brings more checkpoints
  azmi::SbSweepArrays sw{};
  DevBlock sw_block;                  // one allocation behind every sw pointer (sb_cut_sweep)
  size_t sw_clear_bytes = 0;          // its leading part that every call clears: taken masks and snapshot rows
  uint32_t sw_cap = 0;                // checkpoints the block has room for
  bool sw_valid = false;              // a run_to call has defined the snapshot set
  std::vector<uint32_t> sw_upload;    // targets [N] + checkpoints [32]: the host side of the call's upload (kept until the next call)
  // descents_per_step (azmi_search_set_descents_per_step): up to L descents of a tree per step while its leaves need no evaluator
  uint32_t dl_L = 1;
  azmi::SbDlArrays dl{};              // todo [N], todo_max [2]
  uint32_t dl_parity = 0;             // parity of the next step of the running search: the todo_max word it raises
  uint64_t host_reads = 0;            // 4-byte reads of todo_max since creation
  // root capture (azmi_search_set_capture): allocated by the first call that turns it on
  bool capture = false;
  azmi::SbCaptureArrays cp{};
  // net versus search (azmi_search_net_metrics): allocated by the first call
  double* d_nm_out = nullptr;         // [N, 3]
  uint8_t* d_nm_valid = nullptr;      // [N]
  // opening-tree frontier (azmi_search_expand): allocated by the first call, the records regrown when max_children grows
  azmi::SbFrontierArrays fr{};
  void* fr_trees = nullptr;           // one allocation behind every per-tree pointer of fr (sb_cut_frontier_trees)
  DevBlock fr_records;                // one behind the per-record pointers (sb_cut_frontier_records)
  uint32_t fr_cap = 0;                // records fr_records has room for
  double* fr_host = nullptr;          // pinned [2 N]: reach | temp of the last call, the host side of its upload
  hipEvent_t fr_uploaded = nullptr;   // behind that upload
  bool fr_valid = false;              // an expand call has defined the frontier
  // sweep metrics (azmi_search_sweep_metrics): allocated by the first call, regrown when a sweep brings more checkpoints
  DevBlock sm_block;                  // sb_cut_sweep_metrics
  uint32_t sm_cap = 0;                // checkpoints the block has room for
  // the step API's leaf keys (azmi_search_leaf_keys): allocated by the first call, regrown when leaves_per_step grows
  DevBlock leaf_keys_block;
  uint64_t* d_leaf_keys = nullptr;    // [K * N] the keys of the pending step's rows, in row order
};

// ---- defined in search_batch_steps.hip -----------------------------------------------------------------------------------------------
// the checks an entry point starts with: the trees have positions (begin_step); a NULL handle on a machine without a device
// repeats the no-device failure of its create (begin_read); no find_leaves step is pending (begin_move: the calls that change the trees)
int sb_begin_step(azmi_search* s, const char* what);
int sb_begin_read(azmi_search* s, const char* what);
int sb_begin_move(azmi_search* s, const char* what);
// why `more` descents do not fit into max_simulations (0: they do)
int sb_check_budget(const azmi_search* s, const char* what, uint64_t more);
// synchronises `st` and turns a stopped tree / a raised overflow bit into an error that names the tree
int sb_check_device(azmi_search* s, hipStream_t st);

// the engine parameters and arrays of a search() with this net and cache
struct SbSearchArgs {
  azmi::EngineParams ep;
  azmi::EngineArrays ar;
  azmi_net* net = nullptr;
  bool playout = false;
};
int sb_search_args(azmi_search* s, const char* what, int eval_type, azmi_net* net, azmi_cache* cache, SbSearchArgs* out);
// one step of every live tree on `st`: `kk` descents each, the evaluator, the back-up; the steps of search(visits), nothing read back
int sb_enqueue_step(azmi_search* s, const SbSearchArgs& a, uint32_t kk, uint32_t rn, hipStream_t st);
int sb_enqueue_search(azmi_search* s, const SbSearchArgs& a, uint32_t visits, uint32_t rn, hipStream_t st);

// ---- defined in search_batch.hip -----------------------------------------------------------------------------------------------------
// One launch function per kernel family, on `st`, each counted in s->launches; arguments as the kernels take them.
void sb_launch_find(azmi_search* s, const azmi::EngineParams& ep, const azmi::EngineArrays& ar, uint32_t eval_random, hipStream_t st);
void sb_launch_process(azmi_search* s, const azmi::EngineParams& ep, const azmi::EngineArrays& ar, uint32_t root_noise, const float* v_rows,
                       const float* pi_rows, hipStream_t st);
void sb_launch_query(azmi_search* s, uint32_t kind, float temp, uint32_t arg, hipStream_t st);
void sb_launch_query_scalars(azmi_search* s, hipStream_t st);      // kind kQScalars (enum MctsQuery, search_batch_types.h)
void sb_launch_cache_insert(azmi_search* s, const azmi::EngineParams& ep, const azmi::EngineArrays& ar, uint32_t total, hipStream_t st);
void sb_launch_find_wu(azmi_search* s, const azmi::EngineParams& ep, const azmi::EngineArrays& ar, uint32_t kk, uint32_t eval_random, uint32_t root_noise,
                       hipStream_t st);
void sb_launch_process_wu(azmi_search* s, const azmi::EngineParams& ep, const azmi::EngineArrays& ar, uint32_t kk, uint32_t root_noise,
                          const float* v_rows, const float* pi_rows, hipStream_t st);
void sb_launch_pick(azmi_search* s, float temp, hipStream_t st);
void sb_launch_update_root(azmi_search* s, const int32_t* moves, hipStream_t st);
void sb_launch_root_prior(azmi_search* s, uint32_t apply_temp, uint32_t noise, hipStream_t st);
// reset: every tree's position from the uploaded start rows and game records; the step API: the step's kk * N (K > 1) or N rows into one batch
void sb_launch_seed(azmi_search* s, const uint8_t* d_init, uint32_t init_stride, const int32_t* d_moves, const uint32_t* d_offs, const uint64_t* d_seeds,
                    hipStream_t st);
void sb_launch_gather(azmi_search* s, uint32_t kk, hipStream_t st);
// EvalType::PLAYOUT steps
void sb_launch_step_playout(azmi_search* s, const azmi::EngineParams& ep, const azmi::EngineArrays& ar, uint32_t root_noise, hipStream_t st);
void sb_launch_step_playout_wu(azmi_search* s, const azmi::EngineParams& ep, const azmi::EngineArrays& ar, uint32_t kk, uint32_t root_noise, hipStream_t st);
// the checkpoint kernel of azmi_search_run_to
void sb_launch_checkpoint(azmi_search* s, float temp, uint32_t pruned, uint32_t resume, hipStream_t st);
// descents_per_step > 1: the counter launch of a search, the find launch(es) of a step
void sb_launch_todo_set(azmi_search* s, uint32_t visits, hipStream_t st);
void sb_launch_find_dl(azmi_search* s, const azmi::EngineParams& ep, const azmi::EngineArrays& ar, uint32_t parity, uint32_t eval_random,
                       uint32_t root_noise, hipStream_t st);
void sb_launch_find_dl_playout(azmi_search* s, const azmi::EngineParams& ep, const azmi::EngineArrays& ar, uint32_t parity, hipStream_t st);
// root capture: the record of every live tree's root at its current ply; net versus search: the roots' planes into d_batch, then
// the raw rows of d_vrows / d_pirows against the searches
void sb_launch_capture(azmi_search* s, hipStream_t st);
void sb_launch_root_canon(azmi_search* s, hipStream_t st);
void sb_launch_net_metrics(azmi_search* s, hipStream_t st);
// first occurrence of every key (azmi_pool_unique; no search object: nothing is counted)
void sb_launch_pool_claim(const uint64_t* d_keys, const uint8_t* d_valid, uint32_t n, uint32_t mask, uint32_t* d_owner, uint32_t* d_first,
                          uint32_t* d_slot_of, hipStream_t st);
void sb_launch_pool_compact(const uint8_t* d_valid, uint32_t n, const uint32_t* d_first, const uint32_t* d_slot_of, uint32_t* d_out, uint32_t* d_counts,
                            hipStream_t st);
// opening-tree frontier: policy, scan, emit over s->fr
void sb_launch_frontier_policy(azmi_search* s, double min_reach, hipStream_t st);
void sb_launch_frontier_scan(azmi_search* s, hipStream_t st);
void sb_launch_frontier_emit(azmi_search* s, hipStream_t st);
// sweep metrics: the rows of s->sw against ref->sw, the per-checkpoint means; the row function over any [rows, M] pair of policies
void sb_launch_sweep_metrics(azmi_search* s, const azmi_search* ref, uint32_t anchor, int32_t raw, const double* d_outcomes,
                             const azmi::SweepMetricsOut& o, hipStream_t st);
void sb_launch_sweep_mean(azmi_search* s, uint32_t J, const azmi::SweepMetricsOut& o, hipStream_t st);
// the step API's leaf keys into s->d_leaf_keys, in row order
void sb_launch_leaf_keys(azmi_search* s, hipStream_t st);
void sb_launch_policy_divergences(const float* d_p, const float* d_q, uint32_t rows, uint32_t M, double* d_out, hipStream_t st);
