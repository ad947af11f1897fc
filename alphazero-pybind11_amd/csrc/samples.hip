// Per-row surprise loss, resample plan and row gather on the device: the host side of samples_kernels.h.
// azmi_sample_loss / azmi_resample_plan / azmi_resample_gather take DEVICE pointers and a stream; only the plan synchronises,
// once, to hand back its record (the caller needs rows_out to size the gather's outputs).
// Likewise the per-row diagnostics of sample_metrics_kernels.h: azmi_sample_metrics and azmi_sample_plane_argmax are one
// asynchronous launch each, azmi_sample_metrics_reduce synchronises once for its record.
// And the history window and the reservoir of samples_window_kernels.h: azmi_samples_reservoir_keys and
// azmi_samples_window_gather are one asynchronous launch each, azmi_samples_select_top synchronises once for its record.
// And the participation ratio of feature_rank_kernels.h: azmi_samples_feature_rank is five launches and synchronises once for its
// record.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <mutex>
#include <string>

#include "../../include/azmi.h"
#include "engine_host.h"
#include "host_error.h"
#include "samples_kernels.h"
#include "sample_metrics_kernels.h"
#include "samples_window_kernels.h"
#include "feature_rank_kernels.h"
#include "samples_layout.h"

namespace {
using namespace azmi;

static_assert(sizeof(ResampleRecord) == sizeof(azmi_resample_record), "azmi_resample_record is the device record");
static_assert(sizeof(SampleMetricsRecord) == sizeof(azmi_sample_metrics_record), "azmi_sample_metrics_record is the device record");
static_assert(kSampleMetricColumns == AZMI_SAMPLE_METRIC_COLUMNS && kMetricMaxBuckets == AZMI_SAMPLE_METRIC_MAX_BUCKETS, "the header's sizes");
static_assert(offsetof(SelectState, prefix) == sizeof(azmi_select_record), "azmi_select_record is the head of the device state");
static_assert(kWindowMaxSegments == AZMI_WINDOW_MAX_SEGMENTS, "the header's sizes");
static_assert(sizeof(FeatureRankRecord) == sizeof(azmi_feature_rank_record), "azmi_feature_rank_record is the device record");
static_assert(kRankMaxChannels == AZMI_FEATURE_RANK_MAX_CHANNELS, "the header's sizes");

thread_local std::string g_samples_err;

int sfail(int code, const char* fmt, ...) {
  AZMI_FORMAT_ERROR(g_samples_err, fmt);
  return code;
}

int hip_fail(const char* what, hipError_t e) {
  return sfail(e == hipErrorOutOfMemory ? AZMI_ERR_OOM : AZMI_ERR_NO_DEVICE, "%s: %s", what, hipGetErrorString(e));
}

// selects `device` for one call and puts the thread's current device back when the call ends
struct DeviceScope {
  int prev = -1;
  ~DeviceScope() { if (prev >= 0) (void)hipSetDevice(prev); }
  int enter(const char* what, int device) {
    int ndev = 0, cur = -1;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return sfail(AZMI_ERR_NO_DEVICE, "%s: no HIP device: libazmi has no CPU path", what);
    if (device < 0 || device >= ndev) return sfail(AZMI_ERR_INVALID, "%s: device %d out of range", what, device);
    if (hipGetDevice(&cur) != hipSuccess) cur = -1;
    if (cur == device) return AZMI_OK;
    const hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return hip_fail(what, e);
    prev = cur;
    return AZMI_OK;
  }
};

// The plan's scratch block, one per device, kept between calls and grown when a call needs more.  A call holds the mutex up to
// its synchronisation, so two calls never use a block at once, and in the steady state no call allocates or frees (hipFree waits
// for the whole device, not for the call's stream).
constexpr int kPlanMaxDevices = 64;
std::mutex g_plan_mutex;
DevBlock g_plan_scratch[kPlanMaxDevices];

DevBlock g_metrics_scratch[kPlanMaxDevices];      // the same for azmi_sample_metrics_reduce, under the same mutex
DevBlock g_select_scratch[kPlanMaxDevices];       // and for azmi_samples_select_top
DevBlock g_rank_scratch[kPlanMaxDevices];         // and for azmi_samples_feature_rank

uint32_t tiles_of(uint32_t n) { return (n + kPlanBlock - 1) / kPlanBlock; }

// the lane group k_sample_loss gives a row of `entries` entries
int lanes_of(uint32_t entries) { return entries <= 8 ? 8 : entries <= 16 ? 16 : entries <= 32 ? 32 : 64; }

}  // namespace

extern "C" {

const char* azmi_samples_last_error(void) { return g_samples_err.c_str(); }

int azmi_sample_loss(const float* dev_target, const float* dev_p, uint32_t n, uint32_t M, double scale, double* dev_loss_out, int device,
                     void* stream) {
  if (n > kPlanMaxRows || M == 0 || M > (1u << 20))
    return sfail(AZMI_ERR_INVALID, "azmi_sample_loss: n = %u, M = %u: at most %u rows of 1 to %u entries", n, M, kPlanMaxRows, 1u << 20);
  if (n == 0) return AZMI_OK;
  if (!dev_target || !dev_p || !dev_loss_out) return sfail(AZMI_ERR_INVALID, "azmi_sample_loss: null argument");
  DeviceScope scope;
  int rc = scope.enter("azmi_sample_loss", device); if (rc) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  // the lane group of a row: 8 lanes for M <= 8, then 16, 32, and one wavefront striding m from M = 33 on
  if (M <= 8) k_sample_loss<8><<<(n + 31u) / 32u, kLossThreads, 0, st>>>(dev_target, dev_p, n, M, scale, dev_loss_out);
  else if (M <= 16) k_sample_loss<16><<<(n + 15u) / 16u, kLossThreads, 0, st>>>(dev_target, dev_p, n, M, scale, dev_loss_out);
  else if (M <= 32) k_sample_loss<32><<<(n + 7u) / 8u, kLossThreads, 0, st>>>(dev_target, dev_p, n, M, scale, dev_loss_out);
  else k_sample_loss<64><<<(n + 3u) / 4u, kLossThreads, 0, st>>>(dev_target, dev_p, n, M, scale, dev_loss_out);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? AZMI_OK : hip_fail("k_sample_loss", e);
}

int azmi_resample_plan(const double* dev_loss, uint32_t n, uint64_t seed, uint32_t* dev_copies, uint64_t* dev_offsets,
                       azmi_resample_record* host_record_out, int device, void* stream) {
  if (!host_record_out) return sfail(AZMI_ERR_INVALID, "azmi_resample_plan: null argument");
  *host_record_out = azmi_resample_record{0.0, 0, 0, kPlanNone};
  if (n > kPlanMaxRows) return sfail(AZMI_ERR_INVALID, "azmi_resample_plan: n = %u: at most %u rows", n, kPlanMaxRows);
  if (n == 0) return AZMI_OK;
  if (!dev_loss || (dev_copies == nullptr) != (dev_offsets == nullptr))
    return sfail(AZMI_ERR_INVALID, "azmi_resample_plan: null argument (dev_copies and dev_offsets: both, or neither for the sums alone)");
  if (device >= kPlanMaxDevices) return sfail(AZMI_ERR_INVALID, "azmi_resample_plan: device %d: at most %d devices", device, kPlanMaxDevices);
  DeviceScope scope;
  int rc = scope.enter("azmi_resample_plan", device); if (rc) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  // one block: the record | the tile sums of the three levels (f64) | the tile totals of the scan's upper levels (u64)
  const uint32_t t0 = tiles_of(n), t1 = tiles_of(t0);      // t1 <= 1024: the level above it is one tile
  PlanScratch<ResampleRecord> ps;
  BlockCut size;
  cut_plan_scratch(size, ps, t0, t1);
  std::lock_guard<std::mutex> lock(g_plan_mutex);
  DevBlock& sc = g_plan_scratch[device];
  hipError_t e = sc.reserve(size.off);      // allocates on the first call on this device, or for a larger n than any before
  if (e != hipSuccess) return hip_fail("azmi_resample_plan", e);
  BlockCut cut(sc.p);
  cut_plan_scratch(cut, ps, t0, t1);
  ResampleRecord* rec = ps.rec;
  double *sum0 = ps.sum0, *sum1 = ps.sum1;
  uint64_t *tot0 = ps.tot0, *tot1 = ps.tot1;
  e = hipMemsetAsync(rec, 0, sizeof *rec, st);
  if (e == hipSuccess) e = hipMemsetAsync(&rec->first_nonfinite, 0xFF, 4, st);
  if (e == hipSuccess) {
    // the total: a tree over tiles of kPlanBlock, whose top writes the record
    k_plan_sum<true><<<t0, kPlanBlock, 0, st>>>(dev_loss, n, t0 == 1 ? &rec->total_loss : sum0, rec);
    if (t0 > 1) k_plan_sum<false><<<t1, kPlanBlock, 0, st>>>(sum0, t0, t1 == 1 ? &rec->total_loss : sum1, rec);
    if (t1 > 1) k_plan_sum<false><<<1, kPlanBlock, 0, st>>>(sum1, t1, &rec->total_loss, rec);
    if (dev_copies) {
      // the counts and their scan inside a tile, the tile totals scanned level by level, the bases handed down again
      k_plan_copies<<<t0, kPlanBlock, 0, st>>>(dev_loss, n, seed, &rec->total_loss, dev_copies, dev_offsets, t0 == 1 ? &rec->rows_out : tot0);
      if (t0 > 1) k_plan_scan<<<t1, kPlanBlock, 0, st>>>(tot0, t0, t1 == 1 ? &rec->rows_out : tot1);
      if (t1 > 1) {
        k_plan_scan<<<1, kPlanBlock, 0, st>>>(tot1, t1, &rec->rows_out);
        k_plan_add<<<t1, kPlanBlock, 0, st>>>(tot0, t0, tot1);
      }
      if (t0 > 1) k_plan_add<<<t0, kPlanBlock, 0, st>>>(dev_offsets, n, tot0);
    }
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(host_record_out, rec, sizeof *rec, hipMemcpyDeviceToHost, st);
  const hipError_t es = hipStreamSynchronize(st);      // the one synchronisation; always: what was queued uses the block the next call reuses
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return hip_fail("azmi_resample_plan", e);
  return AZMI_OK;
}

int azmi_resample_gather(const uint32_t* dev_copies, const uint64_t* dev_offsets, uint32_t n, uint32_t n_arrays, const void* const* dev_in,
                         void* const* dev_out, const uint32_t* row_bytes, int device, void* stream) {
  if (n > kPlanMaxRows) return sfail(AZMI_ERR_INVALID, "azmi_resample_gather: n = %u: at most %u rows", n, kPlanMaxRows);
  if (n_arrays > kGatherMaxArrays) return sfail(AZMI_ERR_INVALID, "azmi_resample_gather: %u arrays: at most %u per call", n_arrays, kGatherMaxArrays);
  if (n_arrays && (!dev_in || !dev_out || !row_bytes)) return sfail(AZMI_ERR_INVALID, "azmi_resample_gather: null argument");
  GatherArrays a{};
  for (uint32_t k = 0; k < n_arrays; ++k) {
    const uint32_t rb = row_bytes[k];
    if (rb == 0 || rb % 4u) return sfail(AZMI_ERR_INVALID, "azmi_resample_gather: array %u: a row of %u bytes: rows are whole dwords", k, rb);
    if (n && (!dev_in[k] || !dev_out[k])) return sfail(AZMI_ERR_INVALID, "azmi_resample_gather: array %u: null argument", k);
    if (reinterpret_cast<uintptr_t>(dev_in[k]) % 4u || reinterpret_cast<uintptr_t>(dev_out[k]) % 4u)
      return sfail(AZMI_ERR_INVALID, "azmi_resample_gather: array %u: the arrays are dword-aligned", k);
    // the 16-byte path needs every row of both arrays on a 16-byte boundary
    const bool vec = rb % 16u == 0 && reinterpret_cast<uintptr_t>(dev_in[k]) % 16u == 0 && reinterpret_cast<uintptr_t>(dev_out[k]) % 16u == 0;
    a.in[k] = dev_in[k]; a.out[k] = dev_out[k];
    a.vec[k] = vec ? 1 : 0;
    a.units[k] = vec ? rb / 16u : rb / 4u;
    uint32_t lanes = 1;
    while (lanes < 64u && lanes < a.units[k]) lanes <<= 1;
    a.lanes[k] = lanes;
  }
  if (n == 0 || n_arrays == 0) return AZMI_OK;
  if (!dev_copies || !dev_offsets) return sfail(AZMI_ERR_INVALID, "azmi_resample_gather: null argument");
  DeviceScope scope;
  int rc = scope.enter("azmi_resample_gather", device); if (rc) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  // grid.x covers the array with the widest groups (the fewest rows per workgroup); the others leave early
  uint32_t max_lanes = 1;
  for (uint32_t k = 0; k < n_arrays; ++k) max_lanes = a.lanes[k] > max_lanes ? a.lanes[k] : max_lanes;
  const uint32_t rows_per_wg = kGatherThreads / max_lanes;
  k_resample_gather<<<dim3((n + rows_per_wg - 1) / rows_per_wg, n_arrays), kGatherThreads, 0, st>>>(a, n, dev_copies, dev_offsets);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? AZMI_OK : hip_fail("k_resample_gather", e);
}

int azmi_sample_metrics(const float* dev_target_pi, const float* dev_p_pi, const float* dev_target_v, const float* dev_p_v, uint32_t n,
                        uint32_t M, uint32_t V, double cv, double* dev_cols_out, uint64_t col_stride, uint32_t* dev_mcts_argmax_out,
                        uint32_t* dev_net_argmax_out, int device, void* stream) {
  if (n > kPlanMaxRows || M == 0 || M > (1u << 20) || V == 0 || V > (1u << 20))
    return sfail(AZMI_ERR_INVALID, "azmi_sample_metrics: n = %u, M = %u, V = %u: at most %u rows of 1 to %u entries", n, M, V, kPlanMaxRows,
                 1u << 20);
  if (col_stride < n)
    return sfail(AZMI_ERR_INVALID, "azmi_sample_metrics: col_stride = %llu: a column holds at least n = %u rows",
                 static_cast<unsigned long long>(col_stride), n);
  if (n == 0) return AZMI_OK;
  if (!dev_target_pi || !dev_p_pi || !dev_target_v || !dev_p_v || !dev_cols_out || !dev_mcts_argmax_out || !dev_net_argmax_out)
    return sfail(AZMI_ERR_INVALID, "azmi_sample_metrics: null argument");
  DeviceScope scope;
  int rc = scope.enter("azmi_sample_metrics", device); if (rc) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  // a row's group: the larger of the groups k_sample_loss gives the policy row and the value row
  const int lm = lanes_of(M), lv = lanes_of(V), g = lm > lv ? lm : lv;
#define AZMI_METRICS_LAUNCH(G)                                                                                                          \
  k_sample_metrics<G><<<(n + kMetricThreads / G - 1) / (kMetricThreads / G), kMetricThreads, 0, st>>>(                                  \
      dev_target_pi, dev_p_pi, dev_target_v, dev_p_v, n, M, V, lm, lv, cv, dev_cols_out, col_stride, dev_mcts_argmax_out, dev_net_argmax_out)
  if (g == 8) AZMI_METRICS_LAUNCH(8);
  else if (g == 16) AZMI_METRICS_LAUNCH(16);
  else if (g == 32) AZMI_METRICS_LAUNCH(32);
  else AZMI_METRICS_LAUNCH(64);
#undef AZMI_METRICS_LAUNCH
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? AZMI_OK : hip_fail("k_sample_metrics", e);
}

int azmi_sample_plane_argmax(const float* dev_canonical, uint32_t n, uint32_t C, uint32_t H, uint32_t W, uint32_t first_plane,
                             uint32_t n_planes, uint32_t row, uint32_t col, uint8_t* dev_out, int device, void* stream) {
  if (n > kPlanMaxRows) return sfail(AZMI_ERR_INVALID, "azmi_sample_plane_argmax: n = %u: at most %u rows", n, kPlanMaxRows);
  if (C == 0 || H == 0 || W == 0 || uint64_t(C) * H * W >= (1ull << 30))
    return sfail(AZMI_ERR_INVALID, "azmi_sample_plane_argmax: a row of %u x %u x %u: rows hold 1 to 2^30 - 1 float32", C, H, W);
  if (n_planes == 0 || n_planes > 16 || first_plane >= C || n_planes > C - first_plane)
    return sfail(AZMI_ERR_INVALID, "azmi_sample_plane_argmax: planes %u .. %u + %u of %u: 1 to 16 planes inside the row", first_plane,
                 first_plane, n_planes, C);
  if (row >= H || col >= W) return sfail(AZMI_ERR_INVALID, "azmi_sample_plane_argmax: cell (%u, %u) outside the %u x %u board", row, col, H, W);
  if (n == 0) return AZMI_OK;
  if (!dev_canonical || !dev_out) return sfail(AZMI_ERR_INVALID, "azmi_sample_plane_argmax: null argument");
  DeviceScope scope;
  int rc = scope.enter("azmi_sample_plane_argmax", device); if (rc) return rc;
  const uint64_t plane = uint64_t(H) * W;
  k_sample_plane_argmax<<<(n + kMetricThreads - 1) / kMetricThreads, kMetricThreads, 0, static_cast<hipStream_t>(stream)>>>(
      dev_canonical, n, plane * C, plane, plane * first_plane + uint64_t(row) * W + col, n_planes, dev_out);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? AZMI_OK : hip_fail("k_sample_plane_argmax", e);
}

int azmi_sample_metrics_reduce(const double* dev_cols, uint64_t col_stride, uint32_t n, const uint8_t* dev_bucket, uint32_t n_buckets,
                               azmi_sample_metrics_record* host_record_out, int device, void* stream) {
  if (!host_record_out) return sfail(AZMI_ERR_INVALID, "azmi_sample_metrics_reduce: null argument");
  *host_record_out = azmi_sample_metrics_record{};
  host_record_out->first_nonfinite = kPlanNone;
  if (n > kPlanMaxRows) return sfail(AZMI_ERR_INVALID, "azmi_sample_metrics_reduce: n = %u: at most %u rows", n, kPlanMaxRows);
  if (n_buckets == 0 || n_buckets > kMetricMaxBuckets)
    return sfail(AZMI_ERR_INVALID, "azmi_sample_metrics_reduce: n_buckets = %u: 1 to %u buckets", n_buckets, kMetricMaxBuckets);
  if (!dev_bucket && n_buckets != 1)
    return sfail(AZMI_ERR_INVALID, "azmi_sample_metrics_reduce: n_buckets = %u without a bucket array: every row is in bucket 0", n_buckets);
  if (col_stride < n)
    return sfail(AZMI_ERR_INVALID, "azmi_sample_metrics_reduce: col_stride = %llu: a column holds at least n = %u rows",
                 static_cast<unsigned long long>(col_stride), n);
  if (n == 0) return AZMI_OK;
  if (!dev_cols) return sfail(AZMI_ERR_INVALID, "azmi_sample_metrics_reduce: null argument");
  if (device >= kPlanMaxDevices) return sfail(AZMI_ERR_INVALID, "azmi_sample_metrics_reduce: device %d: at most %d devices", device, kPlanMaxDevices);
  DeviceScope scope;
  int rc = scope.enter("azmi_sample_metrics_reduce", device); if (rc) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  // one block: the record | per (bucket, column) pair the tile sums of the first and of the second level
  const bool has_all = dev_bucket != nullptr;
  const uint32_t pairs = (n_buckets + (has_all ? 1u : 0u)) * kSampleMetricColumns;
  const uint32_t t0 = tiles_of(n), t1 = tiles_of(t0);      // t1 <= 1024: the level above it is one tile
  MetricsScratch<SampleMetricsRecord> ms;
  BlockCut size;
  cut_metrics_scratch(size, ms, pairs, t0, t1);
  std::lock_guard<std::mutex> lock(g_plan_mutex);
  DevBlock& sc = g_metrics_scratch[device];
  hipError_t e = sc.reserve(size.off);      // allocates on the first call on this device, or for a larger one than any before
  if (e != hipSuccess) return hip_fail("azmi_sample_metrics_reduce", e);
  BlockCut cut(sc.p);
  cut_metrics_scratch(cut, ms, pairs, t0, t1);
  SampleMetricsRecord* rec = ms.rec;
  double *sum0 = ms.sum0, *sum1 = ms.sum1;
  e = hipMemsetAsync(rec, 0, sizeof *rec, st);
  if (e == hipSuccess) e = hipMemsetAsync(&rec->first_nonfinite, 0xFF, 4, st);
  if (e == hipSuccess) {
    k_metrics_sum<<<dim3(t0, pairs), kPlanBlock, 0, st>>>(dev_cols, col_stride, n, dev_bucket, n_buckets, sum0, rec);
    if (t0 > 1) k_metrics_sum_up<<<dim3(t1, pairs), kPlanBlock, 0, st>>>(sum0, t0, n_buckets, has_all, sum1, rec);
    if (t1 > 1) k_metrics_sum_up<<<dim3(1, pairs), kPlanBlock, 0, st>>>(sum1, t1, n_buckets, has_all, nullptr, rec);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(host_record_out, rec, sizeof *rec, hipMemcpyDeviceToHost, st);
  const hipError_t es = hipStreamSynchronize(st);      // the one synchronisation; always: what was queued uses the block the next call reuses
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return hip_fail("azmi_sample_metrics_reduce", e);
  if (!has_all) {      // one bucket of every row: it is the overall figure too
    for (uint32_t c = 0; c < kSampleMetricColumns; ++c) host_record_out->total[c] = host_record_out->sum[0][c];
  }
  return AZMI_OK;
}

// ---- the history window and the reservoir (samples_window_kernels.h) --------------------------------------------------------------
int azmi_samples_reservoir_keys(const int32_t* dev_iters, const uint64_t* dev_row_ids, uint32_t n, double iteration, double decay,
                                uint64_t seed, double* dev_keys_out, uint64_t* dev_bits_out, int device, void* stream) {
  if (n > kPlanMaxRows) return sfail(AZMI_ERR_INVALID, "azmi_samples_reservoir_keys: n = %u: at most %u rows", n, kPlanMaxRows);
  if (!std::isfinite(iteration)) return sfail(AZMI_ERR_INVALID, "azmi_samples_reservoir_keys: iteration must be finite, got %g", iteration);
  if (!(decay > 0.0 && decay <= 1.0)) return sfail(AZMI_ERR_INVALID, "azmi_samples_reservoir_keys: decay must be in (0, 1], got %g", decay);
  if (n == 0) return AZMI_OK;
  if (!dev_iters || !dev_keys_out) return sfail(AZMI_ERR_INVALID, "azmi_samples_reservoir_keys: null argument");
  DeviceScope scope;
  int rc = scope.enter("azmi_samples_reservoir_keys", device); if (rc) return rc;
  k_reservoir_keys<<<(n + kKeyThreads - 1) / kKeyThreads, kKeyThreads, 0, static_cast<hipStream_t>(stream)>>>(
      dev_iters, dev_row_ids, n, iteration, decay, seed, dev_keys_out, dev_bits_out);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? AZMI_OK : hip_fail("k_reservoir_keys", e);
}

int azmi_samples_select_top(const double* dev_keys, uint32_t n, uint32_t k, int64_t* dev_index_out, azmi_select_record* host_record_out,
                            int device, void* stream) {
  if (!host_record_out) return sfail(AZMI_ERR_INVALID, "azmi_samples_select_top: null argument");
  *host_record_out = azmi_select_record{0.0, 0, 0, kPlanNone};
  if (n > kPlanMaxRows) return sfail(AZMI_ERR_INVALID, "azmi_samples_select_top: n = %u: at most %u rows", n, kPlanMaxRows);
  if (k > n) return sfail(AZMI_ERR_INVALID, "azmi_samples_select_top: k = %u of n = %u keys", k, n);
  if (k == 0) return AZMI_OK;
  if (!dev_keys || !dev_index_out) return sfail(AZMI_ERR_INVALID, "azmi_samples_select_top: null argument");
  if (device >= kPlanMaxDevices) return sfail(AZMI_ERR_INVALID, "azmi_samples_select_top: device %d: at most %d devices", device, kPlanMaxDevices);
  DeviceScope scope;
  int rc = scope.enter("azmi_samples_select_top", device); if (rc) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const uint32_t t0 = tiles_of(n), t1 = tiles_of(t0);      // t1 <= 1024: the level above it is one tile
  SelectScratch<SelectState> ss;
  BlockCut size;
  cut_select_scratch(size, ss, t0, t1);
  std::lock_guard<std::mutex> lock(g_plan_mutex);
  DevBlock& sc = g_select_scratch[device];
  hipError_t e = sc.reserve(size.off);      // allocates on the first call on this device, or for a larger n than any before
  if (e != hipSuccess) return hip_fail("azmi_samples_select_top", e);
  BlockCut cut(sc.p);
  cut_select_scratch(cut, ss, t0, t1);
  e = hipMemsetAsync(ss.st, 0, sizeof *ss.st, st);
  if (e == hipSuccess) e = hipMemsetAsync(&ss.st->first_bad_row, 0xFF, 4, st);
  if (e == hipSuccess) {
    uint32_t blocks = (n + kSelectThreads - 1) / kSelectThreads;
    blocks = blocks < kSelectMaxBlocks ? blocks : kSelectMaxBlocks;
    for (uint32_t pass = 0; pass < kSelectPasses; ++pass) {
      k_select_hist<<<blocks, kSelectThreads, 0, st>>>(dev_keys, n, ss.st, pass);
      k_select_pick<<<1, 64, 0, st>>>(ss.st, pass, k);
    }
    // the chosen rows in ascending order: the tile counts, their scan level by level (as the plan's offsets), the write
    if (t0 > 1) {
      k_select_tiles<<<t0, kPlanBlock, 0, st>>>(dev_keys, n, ss.st, ss.tot0);
      k_plan_scan<<<t1, kPlanBlock, 0, st>>>(ss.tot0, t0, t1 == 1 ? ss.top : ss.tot1);
      if (t1 > 1) {
        k_plan_scan<<<1, kPlanBlock, 0, st>>>(ss.tot1, t1, ss.top);
        k_plan_add<<<t1, kPlanBlock, 0, st>>>(ss.tot0, t0, ss.tot1);
      }
    }
    k_select_write<<<t0, kPlanBlock, 0, st>>>(dev_keys, n, ss.st, t0 > 1 ? ss.tot0 : nullptr, k, dev_index_out);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(host_record_out, ss.st, sizeof *host_record_out, hipMemcpyDeviceToHost, st);
  const hipError_t es = hipStreamSynchronize(st);      // the one synchronisation; always: what was queued uses the block the next call reuses
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return hip_fail("azmi_samples_select_top", e);
  return AZMI_OK;
}

int azmi_samples_window_gather(const void* const* dev_segments, const uint64_t* segment_rows, uint32_t n_segments, uint32_t row_bytes,
                               const int64_t* dev_index, uint64_t seed, uint64_t pass_index, uint64_t first, uint32_t rows, void* dev_out,
                               int device, void* stream) {
  const char* what = "azmi_samples_window_gather";
  if (n_segments == 0 || n_segments > kWindowMaxSegments)
    return sfail(AZMI_ERR_INVALID, "%s: %u segments: 1 to %u per call", what, n_segments, kWindowMaxSegments);
  if (!dev_segments || !segment_rows) return sfail(AZMI_ERR_INVALID, "%s: null argument", what);
  if (row_bytes == 0 || row_bytes % 4u || row_bytes >= (1u << 26))
    return sfail(AZMI_ERR_INVALID, "%s: a row of %u bytes: rows are whole dwords below 64 MiB", what, row_bytes);
  if (rows > kPlanMaxRows) return sfail(AZMI_ERR_INVALID, "%s: rows = %u: at most %u rows per call", what, rows, kPlanMaxRows);
  WindowSegments seg{};
  WindowPerm pm{};
  bool vec = row_bytes % 16u == 0 && reinterpret_cast<uintptr_t>(dev_out) % 16u == 0;
  uint64_t total = 0;
  for (uint32_t s = 0; s < n_segments; ++s) {
    if (segment_rows[s] > (1ull << 40) || total + segment_rows[s] > (1ull << 40))
      return sfail(AZMI_ERR_INVALID, "%s: segment %u: the window holds at most 2^40 rows", what, s);
    if (segment_rows[s] && !dev_segments[s]) return sfail(AZMI_ERR_INVALID, "%s: segment %u: null argument", what, s);
    if (reinterpret_cast<uintptr_t>(dev_segments[s]) % 4u) return sfail(AZMI_ERR_INVALID, "%s: segment %u: the arrays are dword-aligned", what, s);
    if (segment_rows[s] && reinterpret_cast<uintptr_t>(dev_segments[s]) % 16u) vec = false;
    seg.base[s] = dev_segments[s];
    seg.start[s] = total;
    total += segment_rows[s];
  }
  seg.count = n_segments;
  if (first > total || rows > total - first)
    return sfail(AZMI_ERR_INVALID, "%s: rows %llu .. %llu + %u of a window of %llu rows", what, static_cast<unsigned long long>(first),
                 static_cast<unsigned long long>(first), rows, static_cast<unsigned long long>(total));
  if (rows == 0) return AZMI_OK;
  if (!dev_out || reinterpret_cast<uintptr_t>(dev_out) % 4u) return sfail(AZMI_ERR_INVALID, "%s: dev_out: null or not dword-aligned", what);
  pm.total = total;
  pm.bits = 2;
  while (pm.bits < 41 && (1ull << pm.bits) < total) ++pm.bits;
  const uint64_t k0 = mix64(seed + 0x9E3779B97F4A7C15ULL * (pass_index + 1));
  for (uint32_t r = 0; r < kFeistelRounds; ++r) pm.key[r] = mix64(k0 + 0x9E3779B97F4A7C15ULL * (r + 1));
  DeviceScope scope;
  int rc = scope.enter(what, device); if (rc) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const uint32_t grid = (rows + kWindowThreads - 1) / kWindowThreads;
  if (vec) k_window_gather<uint4><<<grid, kWindowThreads, 0, st>>>(seg, pm, dev_index, first, rows, row_bytes / 16u, static_cast<uint4*>(dev_out));
  else k_window_gather<uint32_t><<<grid, kWindowThreads, 0, st>>>(seg, pm, dev_index, first, rows, row_bytes / 4u, static_cast<uint32_t*>(dev_out));
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? AZMI_OK : hip_fail("k_window_gather", e);
}

// ---- the participation ratio of a feature matrix (feature_rank_kernels.h) ------------------------------------------------------------
int azmi_samples_feature_rank(const float* dev_features, uint32_t n, uint32_t C, double* dev_mean_out, double* dev_gram_out,
                              azmi_feature_rank_record* host_record_out, int device, void* stream) {
  const char* what = "azmi_samples_feature_rank";
  if (!host_record_out) return sfail(AZMI_ERR_INVALID, "%s: null argument", what);
  *host_record_out = azmi_feature_rank_record{0.0, 0.0, std::nan(""), n, C};
  if (n > kPlanMaxRows) return sfail(AZMI_ERR_INVALID, "%s: n = %u: at most %u rows", what, n, kPlanMaxRows);
  if (C == 0 || C > kRankMaxChannels) return sfail(AZMI_ERR_INVALID, "%s: C = %u: 1 to %u channels", what, C, kRankMaxChannels);
  if (n == 0) return AZMI_OK;      // (the reference: nan on an empty batch)
  if (!dev_features) return sfail(AZMI_ERR_INVALID, "%s: null argument", what);
  if (reinterpret_cast<uintptr_t>(dev_features) % 4u || reinterpret_cast<uintptr_t>(dev_mean_out) % 8u || reinterpret_cast<uintptr_t>(dev_gram_out) % 8u)
    return sfail(AZMI_ERR_INVALID, "%s: the features are dword-aligned, the float64 outputs 8-byte aligned", what);
  if (device >= kPlanMaxDevices) return sfail(AZMI_ERR_INVALID, "%s: device %d: at most %d devices", what, device, kPlanMaxDevices);
  DeviceScope scope;
  int rc = scope.enter(what, device); if (rc) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const RankPlan plan = rank_plan(n, C);
  const uint32_t blocks = plan.pairs * (kRankTileCells / kRankThreads);
  RankScratch<FeatureRankRecord> rs;
  BlockCut size;
  cut_rank_scratch(size, rs, C, plan.sum_slabs, size_t(plan.slabs) * plan.pairs * kRankTileCells, blocks);
  std::lock_guard<std::mutex> lock(g_plan_mutex);
  DevBlock& sc = g_rank_scratch[device];
  hipError_t e = sc.reserve(size.off);      // allocates on the first call on this device, or for a larger one than any before
  if (e != hipSuccess) return hip_fail(what, e);
  BlockCut cut(sc.p);
  cut_rank_scratch(cut, rs, C, plan.sum_slabs, size_t(plan.slabs) * plan.pairs * kRankTileCells, blocks);
  // pass one, the column means; pass two, the centred products per (tile pair, slab); the slabs summed, the trace and the norm
  k_rank_colsum<<<dim3((C + 63) / 64, plan.sum_slabs), 64, 0, st>>>(dev_features, n, C, plan.sum_slab_rows, rs.col_part);
  k_rank_mean<<<(C + kRankThreads - 1) / kRankThreads, kRankThreads, 0, st>>>(rs.col_part, plan.sum_slabs, C, n, rs.mean, dev_mean_out);
  k_rank_gram<<<dim3(plan.pairs, plan.slabs), kRankThreads, 0, st>>>(dev_features, n, C, rs.mean, plan.tiles, plan.slab_rows, rs.gram_part);
  k_rank_reduce<<<dim3(kRankTileCells / kRankThreads, plan.pairs), kRankThreads, 0, st>>>(rs.gram_part, plan.slabs, C, plan.tiles, dev_gram_out,
                                                                                          rs.block_trace, rs.block_frob2);
  k_rank_final<<<1, kRankThreads, 0, st>>>(rs.block_trace, rs.block_frob2, blocks, n, C, rs.rec);
  e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(host_record_out, rs.rec, sizeof *host_record_out, hipMemcpyDeviceToHost, st);
  const hipError_t es = hipStreamSynchronize(st);      // the one synchronisation; always: what was queued uses the block the next call reuses
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return hip_fail(what, e);
  return AZMI_OK;
}

}  // extern "C"
