// Host-side state of one PlayManager engine and the host helpers shared by the translation units of libazmi.so that launch
// kernels on it:
//   engine.hip          the ONE device module of the engine, MCTS-object and replay kernels (the code of a kernel depends on the
//                       kernels it shares a module with and on the order they are instantiated in, DESIGN.md sections 1 and 8.3):
//                       the kernel headers, k_assign / k_seed / k_net_move / k_delay, the azmi_host_launch_* functions below and
//                       nothing else
//   engine_create.hip   the error text (azmi_host_fail, azmi_last_error), the defaults, the description of a game, the seat
//                       tables, azmi_pm_create* / azmi_pm_destroy
//   engine_rounds.hip   the lock-step round loop: azmi_pm_round*, azmi_run_rounds* and their hipGraph, azmi_pm_net_forward*,
//                       azmi_pm_play, azmi_pm_poll, azmi_host_read_ctl
//   engine_results.hip  the read-outs: scores, statistics, counters, slot state, the history ring, the move log, debug reads
//   engine_hostbuf.hip  the host-buffer compatibility path: azmi_pm_build_batch*, azmi_pm_update_inferences
//   mcts_object.hip     the stand-alone MCTS object (azmi_mcts_*) on a one-slot engine
//   replay.hip          rules replay, playout evaluation, StarGambit images and the RNG probe
//                       The last six are host code only: they launch through engine.hip, and an edit to them cannot move a kernel.
//                       The four engine_* units include no kernel header and their objects carry no device code.
//   pipeline.hip      the asynchronous tree / net pipeline: the one device module of the three pipe_*_kernels.h and their launch
//                     functions; pipeline_state.hip, pipeline_run.hip and pipeline_debug.hip are its host code (pipeline_host.h)
//   search_batch.hip  the batched position search (azmi_search_*): the one device module of the four search_*_kernels.h and every
//                     launch of them.  search_batch_create.hip, search_batch_steps.hip and search_batch_moves.hip hold the core
//                     entry points, search_batch_sweep.hip, search_batch_pool.hip and search_batch_frontier.hip those of their
//                     three families; host code only, they launch through search_batch.hip (search_batch_host.h)
//   samples.hip       per-row losses, resample plan and metrics (azmi_sample_*, azmi_resample_*); DevBlock only
// DevTemps are the device buffers of one call, DevBlock one that is kept between calls and grown.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <deque>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/azmi.h"
#include "engine_types.h"

// sets the thread's azmi_last_error() text and returns `code` (defined in engine_create.hip)
int azmi_host_fail(int code, const char* fmt, ...);
#define AZMI_HIP_TRY(expr)                                                                \
  do {                                                                                    \
    hipError_t e_ = (expr);                                                               \
    if (e_ != hipSuccess)                                                                 \
      return azmi_host_fail(e_ == hipErrorOutOfMemory ? AZMI_ERR_OOM : AZMI_ERR_NO_DEVICE, "%s: %s", #expr, \
                            hipGetErrorString(e_));                                       \
  } while (0)

// calls that stage temporary device buffers (DevTemps below) report every HIP error as AZMI_ERR_NO_DEVICE
#define AZMI_HIP_TRY_NODEV(expr)                                                          \
  do {                                                                                    \
    hipError_t e_ = (expr);                                                               \
    if (e_ != hipSuccess) return azmi_host_fail(AZMI_ERR_NO_DEVICE, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

// the PlayParams of the engine behind MCTS(...) constructor arguments with room for `sims` simulations per tree
// (mcts_object.hip; shared with search_batch.hip)
extern "C" int azmi_host_mcts_params(int game, const azmi_mcts_config* cfg, uint32_t sims, azmi_play_params* out_p);
// the host-side check of a batch of serialized start positions (replay.hip)
extern "C" int azmi_host_check_init_rows(int game, const uint8_t* init, uint32_t init_stride, uint32_t n, uint32_t* extra_reps);

// Temporary device buffers of one host call, freed when the call returns.  A buffer is never smaller than min_bytes.
struct DevTemps {
  explicit DevTemps(size_t min_bytes = 4) : min_bytes_(min_bytes) {}
  DevTemps(const DevTemps&) = delete;
  DevTemps& operator=(const DevTemps&) = delete;
  ~DevTemps() { for (void* q : bufs_) (void)hipFree(q); }
  template <class T>
  hipError_t alloc(T*& p, size_t count) {
    void* q = nullptr;
    const hipError_t e = hipMalloc(&q, std::max(count * sizeof(T), min_bytes_));
    if (e == hipSuccess) { bufs_.push_back(q); p = static_cast<T*>(q); }
    return e;
  }
  // alloc + copy of `count` elements from the host: blocking, or queued on `st`
  template <class T>
  hipError_t upload(T*& p, const T* host, size_t count) {
    const hipError_t e = alloc(p, count);
    return e != hipSuccess || count == 0 ? e : hipMemcpy(p, host, count * sizeof(T), hipMemcpyHostToDevice);
  }
  template <class T>
  hipError_t upload_async(T*& p, const T* host, size_t count, hipStream_t st) {
    const hipError_t e = alloc(p, count);
    return e != hipSuccess || count == 0 ? e : hipMemcpyAsync(p, host, count * sizeof(T), hipMemcpyHostToDevice, st);
  }
 private:
  size_t min_bytes_;
  std::vector<void*> bufs_;
};

// A device block that outlives the call: kept by its owner between calls, grown when a call needs more, never shrunk.  What
// the old block held is gone after a growth (the layouts of block_cut.h are cut again on the new one); the owner frees `p`.
struct DevBlock {
  void* p = nullptr;
  size_t bytes = 0;
  hipError_t reserve(size_t need) {
    if (p && need <= bytes) return hipSuccess;
    void* q = nullptr;
    const hipError_t e = hipMalloc(&q, need);
    if (e != hipSuccess) return e;      // (the old block stays)
    if (p) (void)hipFree(p);            // (waits for the device)
    p = q; bytes = need;
    return hipSuccess;
  }
};

namespace azmi {
struct GameInfo {
  uint32_t P, M, C, H, W, maxk, max_turns, state_words;
  uint32_t cap_branch;  // children per expansion the tree arena is sized for (== maxk when that is affordable)
};

// the asynchronous pipeline's own HBM (pipeline_host.h), created on first use
struct PipeState;
void pipe_state_free(PipeState* p);
}  // namespace azmi

struct azmi_pm {
  int game = 0;
  int device = 0;
  azmi::GameInfo gi{};
  azmi_play_params params{};
  azmi::EngineParams ep{};
  azmi::EngineArrays ar{};
  std::vector<void*> allocs;
  size_t bytes = 0;
  hipStream_t stream = nullptr;  // engine-owned stream (AZMI_STREAM_ENGINE)
  hipStream_t last = nullptr;    // stream of the most recent round: result queries order themselves behind it
  hipStream_t pick(void* s) { last = (s == AZMI_STREAM_ENGINE) ? stream : static_cast<hipStream_t>(s); return last; }
  unsigned long long hist_read = 0;
  uint32_t cache_shards = 0;
  std::vector<azmi::CacheView> group_caches;   // host copies of the per-model-group cache views
  std::vector<uint8_t> group_cache_counted;  // 0: stand-in for a `None` entry of an external cache list (not in the statistics)
  bool all_random = false;               // no seat needs a net (EvalType::RANDOM / PLAYOUT everywhere)
  bool any_playout = false;              // some seat uses EvalType::PLAYOUT
  uint32_t nn_groups = 0;                // bit g: a seat of model group g evaluates with the net
  bool big_split = false;                // wide games, no PLAYOUT seats: k_round_big_sim (StarGambit: k_round_big_sim1) + k_round_big_move instead of the one-kernel round (engine_kernels_big.h)
  bool split_rounds = false;             // Connect4, plain PUCT seats: k_sim + move step instead of the one k_round (engine_kernels.h)
  bool max_inline_explicit = false;      // azmi_pm_options.max_inline was given (the pipeline then keeps it instead of its own default)
  std::vector<std::deque<uint32_t>> pending_g;   // host-buffer path: pending leaves per model group
  // hipGraph of kGraphRounds x (round kernels + net) for azmi_run_rounds: one graph launch instead of
  // ~5 kernel launches per round keeps the host ahead of the GPU
  hipGraphExec_t graph_exec = nullptr;
  hipStream_t graph_stream = nullptr;
  azmi_net* graph_net = nullptr;
  // host-buffer compatibility path
  std::deque<uint32_t> pending;        // slots whose leaf waits for the net
  std::vector<float> host_v, host_pi;  // mirrors of the slot-indexed rows
  uint32_t outstanding = 0;
  std::atomic<bool> stopped{false};
  // The reference's callers reach one PlayManager from several Python threads (mcts_workers x play(), batcher threads with
  // build_batch / update_inferences, the main thread with counters): every entry point that touches the engine's host state
  // takes this lock, so such callers are serialised instead of racing.  (Recursive: entry points call each other.)
  azmi::PipeState* pipe = nullptr;   // the asynchronous tree / net pipeline (pipeline_host.h), created by its first run
  std::recursive_mutex mu;    // PlayManager::stop(), play_manager.h:177 (may be set from another thread)

  template <class T>
  int alloc(T*& p, size_t n, bool zero) {
    void* q = nullptr;
    const size_t sz = std::max<size_t>(n, 1) * sizeof(T);
    AZMI_HIP_TRY(hipMalloc(&q, sz));
    allocs.push_back(q);
    bytes += sz;
    if (zero) {     // (hipMemset is asynchronous to the host, on the null stream: nothing on another stream may run ahead of it)
      AZMI_HIP_TRY(hipMemset(q, 0, sz));
      AZMI_HIP_TRY(hipStreamSynchronize(nullptr));
    }
    p = static_cast<T*>(q);
    return AZMI_OK;
  }
  ~azmi_pm() {
    if (pipe) azmi::pipe_state_free(pipe);
    if (graph_exec) (void)hipGraphExecDestroy(graph_exec);
    for (void* q : allocs) (void)hipFree(q);
    if (stream) (void)hipStreamDestroy(stream);
  }
};

namespace azmi {
// `n` elements of a device array into `dst`, behind everything queued on `st`
template <class T>
int d2h(std::vector<T>& dst, const T* src, size_t n, hipStream_t st) {
  dst.resize(n);
  AZMI_HIP_TRY(hipMemcpyAsync(dst.data(), src, n * sizeof(T), hipMemcpyDeviceToHost, st));
  AZMI_HIP_TRY(hipStreamSynchronize(st));
  return AZMI_OK;
}
}  // namespace azmi

// the static description of a game id (false: unknown id; engine_create.hip), and the engine's Control block read back on `st` -
// after a settling k_assign when `settle` - with a raised overflow mask turned into AZMI_ERR_OVERFLOW (engine_rounds.hip)
bool azmi_host_game_info(int game, azmi::GameInfo* gi);
int azmi_host_read_ctl(azmi_pm* pm, hipStream_t st, azmi::Control* out, bool settle);

// ---- defined in engine.hip, the device module: one launch each, arguments as the kernels take them ------------------------------------
// A round of the engine's game on `st`: cache insert + restart / retire bookkeeping, then the tree kernels.  defer_moves (split
// rounds only) leaves the move step to the azmi_host_launch_net_move that follows: the tiles of the round's eval list through the
// net of `view` and the move step, in one launch.
struct azmi_net_c4_view;
int azmi_host_launch_round(azmi_pm* pm, hipStream_t st, bool defer_moves = false);
int azmi_host_launch_net_move(azmi_pm* pm, const azmi_net_c4_view& view, hipStream_t st);
// the two between-epoch steps of the pipeline: the move step of a split round as a launch of its own, and k_assign
int azmi_host_launch_move_step(azmi_pm* pm, hipStream_t st);
int azmi_host_launch_assign(azmi_pm* pm, hipStream_t st, uint32_t count_round);
// k_assign that counts no round, unchecked: the read-back behind it reports (azmi_host_read_ctl)
void azmi_host_launch_settle(azmi_pm* pm, hipStream_t st);
// the three RNG streams of every slot from `seed`, on the engine's own stream
void azmi_host_launch_seed(azmi_pm* pm, uint64_t seed);
// one wavefront that holds `st` for about `us` microseconds
void azmi_host_launch_delay(uint32_t us, hipStream_t st);
// Replay family: on the null stream, grids sized by n.
void azmi_host_launch_replay(int game, const uint8_t* d_init, uint32_t init_stride, const int32_t* d_moves, uint32_t n, uint32_t len, uint64_t* d_rep,
                             uint32_t stride, uint8_t* d_valid, float* d_scores, float* d_canon, uint32_t* d_player, uint32_t* d_turn, uint64_t* d_key,
                             int32_t* d_status, uint32_t flags);
void azmi_host_launch_playout(int game, const uint8_t* d_init, uint32_t init_stride, const int32_t* d_moves, uint32_t n, uint32_t len, uint64_t* d_rep,
                              uint32_t stride, const uint64_t* d_seeds, float* d_v, float* d_pi, int32_t* d_status);
void azmi_host_launch_sg_image(const uint8_t* d_init, uint32_t init_stride, const int32_t* d_moves, uint32_t n, uint32_t len, uint64_t* d_rep, uint32_t stride,
                               uint8_t* d_out, uint32_t out_stride, uint32_t* d_len, int32_t* d_status, uint32_t flags);
void azmi_host_launch_rng_probe(int kind, uint64_t seed, float param, uint32_t n, uint32_t reps, uint32_t* out_u, float* out_f);
// MCTS object: one wavefront on the engine's slot 0, on `st`
namespace azmi { struct WuArrays; }
void azmi_host_launch_mcts_find_leaf(azmi_pm* pm, hipStream_t st, uint32_t* nif, const uint8_t* di, uint32_t init_bytes, const int32_t* d_moves, uint32_t len,
                                     int32_t* d_out_moves, uint32_t* d_len, int32_t* d_status);
void azmi_host_launch_mcts_process_result(azmi_pm* pm, hipStream_t st, uint32_t rn, float* d_f);
void azmi_host_launch_mcts_find_leaf_batched(azmi_pm* pm, hipStream_t st, const azmi::WuArrays& wu, uint32_t idx, const uint8_t* di, uint32_t init_bytes,
                                             const int32_t* d_moves, uint32_t len, int32_t* d_out_moves, uint32_t* d_len, int32_t* d_status);
void azmi_host_launch_mcts_process_result_batched(azmi_pm* pm, hipStream_t st, const azmi::WuArrays& wu, uint32_t leaf_index, uint32_t rn, float* d_f);
void azmi_host_launch_mcts_update_root(azmi_pm* pm, hipStream_t st, uint32_t* nif, const uint8_t* di, uint32_t init_bytes, const int32_t* d_moves, uint32_t len,
                                       uint32_t move, int32_t* d_status);
void azmi_host_launch_mcts_query(azmi_pm* pm, hipStream_t st, uint32_t kind, float temp, uint32_t arg, float* d_f, uint32_t* d_u);
// k_compact over the first `trees` trees of the engine on `st` (nif: the in-flight marks that move with the nodes, or NULL); no-op for Connect4
void azmi_host_launch_compact(azmi_pm* pm, hipStream_t st, uint32_t trees, uint32_t* nif);
