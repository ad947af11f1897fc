// The read-outs of one PlayManager engine: model groups and per-permutation scores, stop / queue counts, one slot's state, scores,
// statistics, counters, the finished-sample ring, the move log and the debug reads.  Host code only: copies from the engine's HBM
// behind the stream of its most recent round, no launch but the settling k_assign of azmi_host_read_ctl (engine_host.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/azmi.h"
#include "engine_host.h"

using namespace azmi;

unsigned long long azmi_host_pipe_l0_hits(azmi_pm* pm, hipStream_t st);    // pipeline_state.hip

extern "C" {

int azmi_pm_groups(azmi_pm* pm, uint32_t* num_model_groups, uint32_t* num_seat_perms) {
  if (!pm) return azmi_host_fail(AZMI_ERR_INVALID, "null pm");
  if (num_model_groups) *num_model_groups = pm->ep.num_groups;
  if (num_seat_perms) *num_seat_perms = pm->ep.num_perms;
  return AZMI_OK;
}

int azmi_pm_perm_scores(azmi_pm* pm, uint32_t perm, float* out_scores, uint32_t* games_completed) {
  if (!pm) return azmi_host_fail(AZMI_ERR_INVALID, "null pm");
  std::lock_guard<std::recursive_mutex> lock_(pm->mu);
  if (perm >= pm->ep.num_perms) return azmi_host_fail(AZMI_ERR_INVALID, "seat permutation %u out of range", perm);
  const uint32_t S = pm->ep.S, V = pm->gi.P + 1, NP = pm->ep.num_perms;
  std::vector<float> a; std::vector<uint32_t> g;
  int rc = d2h(a, pm->ar.a_perm_scores, static_cast<size_t>(S) * NP * V, pm->last); if (rc) return rc;
  rc = d2h(g, pm->ar.a_perm_games, static_cast<size_t>(S) * NP, pm->last); if (rc) return rc;
  if (out_scores) {
    for (uint32_t i = 0; i < V; ++i) out_scores[i] = 0.0f;
    for (uint32_t s = 0; s < S; ++s) for (uint32_t i = 0; i < V; ++i) out_scores[i] += a[(static_cast<size_t>(s) * NP + perm) * V + i];
  }
  if (games_completed) { uint32_t n = 0; for (uint32_t s = 0; s < S; ++s) n += g[static_cast<size_t>(s) * NP + perm]; *games_completed = n; }
  return AZMI_OK;
}

int azmi_pm_io_buffers(azmi_pm* pm, float** dev_canonical, float** dev_v, float** dev_pi) {
  if (!pm) return azmi_host_fail(AZMI_ERR_INVALID, "null pm");
  if (dev_canonical) *dev_canonical = pm->ar.canon;
  if (dev_v) *dev_v = pm->ar.v;
  if (dev_pi) *dev_pi = pm->ar.pi;
  return AZMI_OK;
}

// ---- PlayManager::stop / stopped / queue sizes / one slot's GameState (play_manager.h:177-186, 285-324) ----------
int azmi_pm_stop(azmi_pm* pm) {
  if (!pm) return azmi_host_fail(AZMI_ERR_INVALID, "null pm");
  pm->stopped.store(true, std::memory_order_relaxed);
  return AZMI_OK;
}
int azmi_pm_stopped(azmi_pm* pm, int* out) {
  if (!pm || !out) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  *out = pm->stopped.load(std::memory_order_relaxed) ? 1 : 0;
  return AZMI_OK;
}
// awaiting_inference_count(): leaves waiting to be handed out by build_batch / pop_games; awaiting_mcts_count(): live
// slots that hold their answer (or need none) and wait for the next round
int azmi_pm_queue_counts(azmi_pm* pm, uint32_t* awaiting_inference, uint32_t* awaiting_mcts) {
  if (!pm) return azmi_host_fail(AZMI_ERR_INVALID, "null pm");
  std::lock_guard<std::recursive_mutex> lock_(pm->mu);
  Control c;
  const int rc = azmi_host_read_ctl(pm, pm->last, &c, true);
  if (rc != AZMI_OK) return rc;
  uint32_t pend = 0;
  for (auto& q : pm->pending_g) pend += static_cast<uint32_t>(q.size());
  const uint32_t live = c.stop ? 0u : c.live_slots;
  if (awaiting_inference) *awaiting_inference = pend;
  if (awaiting_mcts) *awaiting_mcts = live > pend + pm->outstanding ? live - pend - pm->outstanding : 0u;
  return AZMI_OK;
}
// game_data(i).gs: the packed state words of slot `slot` (Connect4: stones of player 0, stones of player 1,
// turn | player << 32; Tafl family: defenders lo/hi, attackers lo/hi, king | turn << 8 | player << 24 | repetitions << 32)
int azmi_pm_slot_state(azmi_pm* pm, uint32_t slot, uint64_t* words, uint32_t cap, uint32_t* n) {
  if (!pm || !words || !n) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  std::lock_guard<std::recursive_mutex> lock_(pm->mu);
  if (slot >= pm->ep.S) return azmi_host_fail(AZMI_ERR_RANGE, "game index %u out of range", slot);
  const uint32_t W = pm->gi.state_words;
  if (cap < W + 1) return azmi_host_fail(AZMI_ERR_INVALID, "words too small");
  AZMI_HIP_TRY(hipStreamSynchronize(pm->last));
  for (uint32_t w = 0; w < W; ++w)
    AZMI_HIP_TRY(hipMemcpy(words + w, pm->ar.gs_words + static_cast<size_t>(w) * pm->ep.S + slot, 8, hipMemcpyDeviceToHost));
  uint32_t perm = 0;
  AZMI_HIP_TRY(hipMemcpy(&perm, pm->ar.perm + slot, 4, hipMemcpyDeviceToHost));
  words[W] = perm;      // GameData::perm_index, play_manager.h:41
  *n = W + 1;
  return AZMI_OK;
}

// game_data(i).gs of a game with a position history (StarGambit: position_history_, star_gambit_gs.h:745): the slot's
// history entries (the reference's own position hashes since the last deploy)
int azmi_pm_slot_history(azmi_pm* pm, uint32_t slot, uint64_t* out, uint32_t cap, uint32_t* n) {
  if (!pm || !out || !n) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  std::lock_guard<std::recursive_mutex> lock_(pm->mu);
  if (slot >= pm->ep.S) return azmi_host_fail(AZMI_ERR_RANGE, "game index %u out of range", slot);
  if (pm->game == AZMI_GAME_CONNECT4) { *n = 0; return AZMI_OK; }
  AZMI_HIP_TRY(hipStreamSynchronize(pm->last));
  uint32_t len = 0;
  AZMI_HIP_TRY(hipMemcpy(&len, pm->ar.rep_len + slot, 4, hipMemcpyDeviceToHost));
  if (len > cap) return azmi_host_fail(AZMI_ERR_INVALID, "history of %u entries does not fit %u", len, cap);
  if (len) AZMI_HIP_TRY(hipMemcpy(out, pm->ar.rep_list + static_cast<size_t>(slot) * (pm->gi.max_turns + 2), static_cast<size_t>(len) * 8, hipMemcpyDeviceToHost));
  *n = len;
  return AZMI_OK;
}

// game_data(i).canonical(): the planes of the leaf slot `slot` is waiting on (host array [C,H,W])
int azmi_pm_slot_canonical(azmi_pm* pm, uint32_t slot, float* out) {
  if (!pm || !out) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  std::lock_guard<std::recursive_mutex> lock_(pm->mu);
  if (slot >= pm->ep.S) return azmi_host_fail(AZMI_ERR_RANGE, "game index %u out of range", slot);
  const size_t CANON = static_cast<size_t>(pm->gi.C) * pm->gi.H * pm->gi.W;
  AZMI_HIP_TRY(hipStreamSynchronize(pm->last));
  AZMI_HIP_TRY(hipMemcpy(out, pm->ar.canon + slot * CANON, CANON * 4, hipMemcpyDeviceToHost));
  return AZMI_OK;
}

int azmi_pm_scores(azmi_pm* pm, float* out) {
  if (!pm || !out) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  std::lock_guard<std::recursive_mutex> lock_(pm->mu);
  std::vector<float> a;
  const uint32_t V = pm->gi.P + 1;
  const int rc = d2h(a, pm->ar.a_scores, static_cast<size_t>(pm->ep.S) * V, pm->last);
  if (rc != AZMI_OK) return rc;
  for (uint32_t i = 0; i < V; ++i) out[i] = 0.0f;
  for (uint32_t s = 0; s < pm->ep.S; ++s) for (uint32_t i = 0; i < V; ++i) out[i] += a[static_cast<size_t>(s) * V + i];
  return AZMI_OK;
}
int azmi_pm_resign_scores(azmi_pm* pm, float* out) {
  if (!pm || !out) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  std::lock_guard<std::recursive_mutex> lock_(pm->mu);
  std::vector<float> a;
  const uint32_t V = pm->gi.P + 1;
  const int rc = d2h(a, pm->ar.a_resign, static_cast<size_t>(pm->ep.S) * V, pm->last);
  if (rc != AZMI_OK) return rc;
  for (uint32_t i = 0; i < V; ++i) out[i] = 0.0f;
  for (uint32_t s = 0; s < pm->ep.S; ++s) for (uint32_t i = 0; i < V; ++i) out[i] += a[static_cast<size_t>(s) * V + i];
  return AZMI_OK;
}

// the sums behind azmi_pm_stats, for callers that combine several engines (shards / ranks) into one set of averages:
// out[10] = game_length, games completed, total / full / fast move counts, leaf depth, entropy, fast leaf depth,
//           fast entropy, valid moves (the accumulators of play_manager.h:398-424)
int azmi_pm_stat_sums(azmi_pm* pm, double* out) {
  if (!pm || !out) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  std::lock_guard<std::recursive_mutex> lock_(pm->mu);
  const uint32_t S = pm->ep.S;
  std::vector<uint64_t> len, cnt; std::vector<double> ds; std::vector<uint32_t> games;
  int rc = d2h(len, pm->ar.a_len, S, pm->last); if (rc) return rc;
  rc = d2h(cnt, pm->ar.a_cnt, 3 * static_cast<size_t>(S), pm->last); if (rc) return rc;
  rc = d2h(ds, pm->ar.a_dsum, 5 * static_cast<size_t>(S), pm->last); if (rc) return rc;
  rc = d2h(games, pm->ar.slot_games, S, pm->last); if (rc) return rc;
  for (int i = 0; i < 10; ++i) out[i] = 0.0;
  for (uint32_t s = 0; s < S; ++s) {
    out[0] += static_cast<double>(len[s]); out[1] += games[s];
    for (int j = 0; j < 3; ++j) out[2 + j] += static_cast<double>(cnt[static_cast<size_t>(j) * S + s]);
    for (int j = 0; j < 5; ++j) out[5 + j] += ds[static_cast<size_t>(j) * S + s];
  }
  return AZMI_OK;
}

uint32_t azmi_pm_num_variants(azmi_pm* pm) { return pm && pm->game == AZMI_GAME_STARGAMBIT ? 4u : 0u; }   // num_variants(), star_gambit_gs.h:863
int azmi_pm_variant_sums(azmi_pm* pm, uint32_t variant, float* perm_scores, uint32_t* perm_games, double* sums) {
  if (!pm || !perm_scores || !perm_games || !sums) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  if (variant >= azmi_pm_num_variants(pm)) return azmi_host_fail(AZMI_ERR_RANGE, "variant %u out of range", variant);
  std::lock_guard<std::recursive_mutex> lock_(pm->mu);
  const uint32_t S = pm->ep.S, NP = pm->ep.num_perms, V = pm->gi.P + 1;
  std::vector<float> sc; std::vector<uint32_t> gm; std::vector<uint64_t> len, cnt; std::vector<double> ds;
  int rc = d2h(sc, pm->ar.a_var_scores, static_cast<size_t>(S) * 4 * NP * V, pm->last); if (rc) return rc;
  rc = d2h(gm, pm->ar.a_var_games, static_cast<size_t>(S) * 4 * NP, pm->last); if (rc) return rc;
  rc = d2h(len, pm->ar.a_var_len, static_cast<size_t>(S) * 4, pm->last); if (rc) return rc;
  rc = d2h(ds, pm->ar.a_var_dsum, static_cast<size_t>(S) * 4 * 5, pm->last); if (rc) return rc;
  rc = d2h(cnt, pm->ar.a_var_cnt, static_cast<size_t>(S) * 4 * 3, pm->last); if (rc) return rc;
  for (uint32_t i = 0; i < NP * V; ++i) perm_scores[i] = 0.0f;
  for (uint32_t i = 0; i < NP; ++i) perm_games[i] = 0;
  for (int i = 0; i < 10; ++i) sums[i] = 0.0;
  for (uint32_t s = 0; s < S; ++s) {      // slot order: a deterministic sum
    const size_t sv = static_cast<size_t>(s) * 4 + variant;
    for (uint32_t q = 0; q < NP; ++q) {
      for (uint32_t i = 0; i < V; ++i) perm_scores[q * V + i] += sc[(sv * NP + q) * V + i];
      perm_games[q] += gm[sv * NP + q];
      sums[1] += gm[sv * NP + q];
    }
    sums[0] += static_cast<double>(len[sv]);
    for (int j = 0; j < 3; ++j) sums[2 + j] += static_cast<double>(cnt[sv * 3 + j]);
    for (int j = 0; j < 5; ++j) sums[5 + j] += ds[sv * 5 + j];
  }
  return AZMI_OK;
}

int azmi_pm_stats(azmi_pm* pm, float* out) {  // play_manager.h:288-315
  if (!pm || !out) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  std::lock_guard<std::recursive_mutex> lock_(pm->mu);
  const uint32_t S = pm->ep.S;
  std::vector<uint64_t> len, cnt; std::vector<double> ds; std::vector<uint32_t> games;
  int rc = d2h(len, pm->ar.a_len, S, pm->last); if (rc) return rc;
  rc = d2h(cnt, pm->ar.a_cnt, 3 * static_cast<size_t>(S), pm->last); if (rc) return rc;
  rc = d2h(ds, pm->ar.a_dsum, 5 * static_cast<size_t>(S), pm->last); if (rc) return rc;
  rc = d2h(games, pm->ar.slot_games, S, pm->last); if (rc) return rc;
  uint64_t game_length = 0, mc[3] = {0, 0, 0}, completed = 0; double d[5] = {0, 0, 0, 0, 0};
  for (uint32_t s = 0; s < S; ++s) {
    game_length += len[s]; completed += games[s];
    for (int j = 0; j < 3; ++j) mc[j] += cnt[static_cast<size_t>(j) * S + s];
    for (int j = 0; j < 5; ++j) d[j] += ds[static_cast<size_t>(j) * S + s];
  }
  out[0] = static_cast<float>(game_length) / static_cast<float>(completed);
  out[1] = mc[1] == 0 ? 0.0f : static_cast<float>(d[0] / static_cast<double>(mc[1]));
  out[2] = mc[1] == 0 ? 0.0f : static_cast<float>(d[1] / static_cast<double>(mc[1]));
  out[3] = mc[2] == 0 ? 0.0f : static_cast<float>(d[2] / static_cast<double>(mc[2]));
  out[4] = mc[2] == 0 ? 0.0f : static_cast<float>(d[3] / static_cast<double>(mc[2]));
  out[5] = game_length == 0 ? 0.0f : static_cast<float>(mc[0]) / static_cast<float>(game_length);
  out[6] = mc[0] == 0 ? 0.0f : static_cast<float>(d[4] / static_cast<double>(mc[0]));
  return AZMI_OK;
}

// cache_hits / misses / evictions / reinserts / size / max_size summed over the model groups' caches (play_manager.h:325-366)
int azmi_pm_cache_stats(azmi_pm* pm, uint64_t out[6]) {
  if (!pm || !out) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  std::lock_guard<std::recursive_mutex> lock_(pm->mu);
  for (int i = 0; i < 6; ++i) out[i] = 0;
  if (!pm->ep.cache_on) return AZMI_OK;
  for (uint32_t g = 0; g < pm->ep.num_groups; ++g) {
    if (!pm->group_cache_counted[g]) continue;
    const CacheView& c = pm->group_caches[g];
    std::vector<unsigned long long> st; std::vector<uint32_t> state;
    int rc = d2h(st, c.stats, static_cast<size_t>(c.shards) * 4, pm->last); if (rc) return rc;
    rc = d2h(state, c.state, static_cast<size_t>(c.shards) * 8, pm->last); if (rc) return rc;
    for (uint32_t s = 0; s < c.shards; ++s) {
      for (int j = 0; j < 4; ++j) out[j] += st[static_cast<size_t>(s) * 4 + j];
      out[4] += state[static_cast<size_t>(s) * 8 + kSize];
    }
    out[5] += static_cast<uint64_t>(c.cap) * c.shards;
  }
  // the pipeline's in-epoch answer table answers probes the S3-FIFO shard counted as misses (pipe_types.h)
  const unsigned long long l0 = azmi_host_pipe_l0_hits(pm, pm->last);
  out[0] += l0; out[1] -= std::min<uint64_t>(out[1], l0);
  return AZMI_OK;
}

int azmi_pm_counters(azmi_pm* pm, uint64_t* out) {
  if (!pm || !out) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  std::lock_guard<std::recursive_mutex> lock_(pm->mu);
  const uint32_t S = pm->ep.S;
  std::vector<uint64_t> sims, evals;
  int rc = d2h(sims, pm->ar.c_sims, S, pm->last); if (rc) return rc;
  rc = d2h(evals, pm->ar.c_evals, S, pm->last); if (rc) return rc;
  Control c;
  rc = azmi_host_read_ctl(pm, pm->last, &c, true); if (rc) return rc;
  out[0] = out[1] = 0;
  for (uint32_t s = 0; s < S; ++s) { out[0] += sims[s]; out[1] += evals[s]; }
  uint64_t cs[6];
  rc = azmi_pm_cache_stats(pm, cs); if (rc) return rc;
  out[2] = cs[0]; out[3] = cs[1];
  out[4] = c.hist_rows - pm->hist_read;   // free-running 64-bit counters: the difference is the live row count
  out[5] = c.rounds;
  return AZMI_OK;
}

namespace {
// tells the device how far the host has consumed the finished-sample ring (ordered behind the rounds already queued)
int publish_hist_read(azmi_pm* pm) {
  AZMI_HIP_TRY(hipMemcpyAsync(&pm->ar.ctl->hist_read, &pm->hist_read, sizeof(pm->hist_read), hipMemcpyHostToDevice, pm->last));
  AZMI_HIP_TRY(hipStreamSynchronize(pm->last));
  return AZMI_OK;
}
}  // namespace

int azmi_pm_pop_history(azmi_pm* pm, float* canonical, float* v, float* pi, uint32_t cap, uint32_t* n) {
  if (!pm || !n) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  std::lock_guard<std::recursive_mutex> lock_(pm->mu);
  Control c;
  int rc = azmi_host_read_ctl(pm, pm->last, &c, true); if (rc) return rc;
  const uint32_t avail = static_cast<uint32_t>(c.hist_rows - pm->hist_read);
  const uint32_t take = std::min(avail, cap);
  const uint32_t CANON = pm->gi.C * pm->gi.H * pm->gi.W, V = pm->gi.P + 1, M = pm->gi.M;
  if (take) {
    const uint32_t first = static_cast<uint32_t>(pm->hist_read % pm->ep.hist_cap);
    const uint32_t n1 = std::min(take, pm->ep.hist_cap - first);
    for (int seg = 0; seg < 2; ++seg) {     // the window may wrap around the end of the ring
      const size_t r0 = seg == 0 ? first : 0, nr = seg == 0 ? n1 : take - n1, o = seg == 0 ? 0 : n1;
      if (!nr) continue;
      AZMI_HIP_TRY(hipMemcpy(canonical + o * CANON, pm->ar.h_canon + r0 * CANON, nr * CANON * 4, hipMemcpyDeviceToHost));
      AZMI_HIP_TRY(hipMemcpy(v + o * V, pm->ar.h_v + r0 * V, nr * V * 4, hipMemcpyDeviceToHost));
      AZMI_HIP_TRY(hipMemcpy(pi + o * M, pm->ar.h_pi + r0 * M, nr * M * 4, hipMemcpyDeviceToHost));
    }
    pm->hist_read += take;
    rc = publish_hist_read(pm); if (rc) return rc;
  }
  *n = take;
  return AZMI_OK;
}

int azmi_pm_history_device(azmi_pm* pm, float** dev_canonical, float** dev_v, float** dev_pi, uint32_t** dev_meta,
                           uint32_t* rows) {
  if (!pm) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  std::lock_guard<std::recursive_mutex> lock_(pm->mu);
  Control c;
  int rc = azmi_host_read_ctl(pm, pm->last, &c, true); if (rc) return rc;
  if (dev_canonical) *dev_canonical = pm->ar.h_canon;
  if (dev_v) *dev_v = pm->ar.h_v;
  if (dev_pi) *dev_pi = pm->ar.h_pi;
  if (dev_meta) *dev_meta = pm->ar.h_meta;
  if (rows) *rows = static_cast<uint32_t>(std::min<unsigned long long>(c.hist_rows, pm->ep.hist_cap));   // rows of the run while nothing has wrapped; use the window call for a ring
  return AZMI_OK;
}

int azmi_pm_history_window(azmi_pm* pm, uint32_t* first_row, uint32_t* rows, uint32_t* capacity) {
  if (!pm) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  std::lock_guard<std::recursive_mutex> lock_(pm->mu);
  Control c;
  int rc = azmi_host_read_ctl(pm, pm->last, &c, true); if (rc) return rc;
  if (first_row) *first_row = pm->ep.hist_cap ? static_cast<uint32_t>(pm->hist_read % pm->ep.hist_cap) : 0;
  if (rows) *rows = static_cast<uint32_t>(c.hist_rows - pm->hist_read);
  if (capacity) *capacity = pm->ep.hist_cap;
  return AZMI_OK;
}

int azmi_pm_history_consume(azmi_pm* pm, uint32_t rows) {
  if (!pm) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  std::lock_guard<std::recursive_mutex> lock_(pm->mu);
  Control c;
  int rc = azmi_host_read_ctl(pm, pm->last, &c, true); if (rc) return rc;
  if (rows > c.hist_rows - pm->hist_read) return azmi_host_fail(AZMI_ERR_INVALID, "history_consume: %u rows asked, %u unread", rows, static_cast<uint32_t>(c.hist_rows - pm->hist_read));
  pm->hist_read += rows;
  return publish_hist_read(pm);
}

int azmi_pm_move_log(azmi_pm* pm, uint32_t* rows, uint32_t* counts, uint32_t cap, uint32_t* n) {
  if (!pm || !n) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  std::lock_guard<std::recursive_mutex> lock_(pm->mu);
  if (!pm->ep.log_moves) return azmi_host_fail(AZMI_ERR_STATE, "move log was not enabled (azmi_engine_opts.log_moves)");
  Control c;
  int rc = azmi_host_read_ctl(pm, pm->last, &c, true); if (rc) return rc;
  const uint32_t take = std::min(std::min(c.log_rows, pm->ep.log_cap), cap);
  if (take && rows) AZMI_HIP_TRY(hipMemcpy(rows, pm->ar.log_rows, static_cast<size_t>(take) * 8 * 4, hipMemcpyDeviceToHost));
  if (take && counts) AZMI_HIP_TRY(hipMemcpy(counts, pm->ar.log_counts, static_cast<size_t>(take) * pm->gi.M * 4, hipMemcpyDeviceToHost));
  *n = take;
  return AZMI_OK;
}

// debug: keys of the leaves the last round sent to the net (0 = none), one per slot
int azmi_debug_eval_keys(azmi_pm* pm, uint64_t* out, uint32_t cap, uint32_t* n) {
  if (!pm || !out || !n) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  if (!pm->ep.cache_on) return azmi_host_fail(AZMI_ERR_STATE, "cache is off");
  std::vector<uint64_t> k;
  const int rc = d2h(k, pm->ar.cache_keys, pm->ep.S, pm->last);
  if (rc) return rc;
  const uint32_t cnt = std::min<uint32_t>(cap, pm->ep.S);
  std::memcpy(out, k.data(), static_cast<size_t>(cnt) * 8);
  *n = cnt;
  return AZMI_OK;
}

int azmi_debug_trace(azmi_pm* pm, uint64_t* out, uint32_t cap, uint32_t* n) {
  std::vector<uint64_t> t;
  const int rc = d2h(t, pm->ar.trace, 2 * static_cast<size_t>(pm->ep.trace_cap), pm->last);
  if (rc) return rc;
  const uint32_t cnt = static_cast<uint32_t>(std::min<uint64_t>(t[0], cap));
  std::memcpy(out, t.data() + 2, static_cast<size_t>(cnt) * 16);
  *n = cnt;
  return AZMI_OK;
}

int azmi_pm_slot_games(azmi_pm* pm, uint32_t* out) {
  if (!pm || !out) return azmi_host_fail(AZMI_ERR_INVALID, "null argument");
  std::lock_guard<std::recursive_mutex> lock_(pm->mu);
  std::vector<uint32_t> g;
  const int rc = d2h(g, pm->ar.slot_games, pm->ep.S, pm->last);
  if (rc) return rc;
  std::memcpy(out, g.data(), g.size() * 4);
  return AZMI_OK;
}

}  // extern "C"
