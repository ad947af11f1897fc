// Batched position search, frozen_eval.py's capture loop and metric extraction (csrc/search_pool_kernels.h): root records before
// every move's search (azmi_search_set_capture / capture_roots / captured), first-occurrence dedup of keys (azmi_pool_unique),
// the net's raw forward of the roots against their searches (azmi_search_net_metrics).  Host code only: the kernels and their
// launch functions are in search_batch.hip's device module (search_batch_host.h).
#include <hip/hip_runtime.h>

#include <vector>

#include "search_batch_host.h"

using namespace azmi;

extern "C" {

int azmi_search_set_capture(azmi_search* s, int on) {
  if (!s) return SB_FAIL(AZMI_ERR_INVALID, "null argument");
  if (on && !s->cp.key) {
    azmi_pm* pm = s->pm;
    SB_TRY(hipSetDevice(pm->device));
    const size_t rows = static_cast<size_t>(s->n) * s->pl.log_cap;
    SbCaptureArrays cp{};
    int rc = pm->alloc(cp.key, rows, true);
    if (rc == AZMI_OK) rc = pm->alloc(cp.player, rows, true);
    if (rc == AZMI_OK) rc = pm->alloc(cp.variant, rows, true);
    if (rc == AZMI_OK) rc = pm->alloc(cp.len, s->n, true);
    if (rc != AZMI_OK) return rc;      // (what was allocated stays with the engine and is freed with it)
    s->cp = cp;
  }
  s->capture = on != 0;
  return AZMI_OK;
}

int azmi_search_capture_roots(azmi_search* s, void* stream) {
  int rc = sb_begin_move(s, "capture_roots"); if (rc) return rc;
  if (!s->capture) return SB_FAIL(AZMI_ERR_STATE, "capture_roots: capture is off; call set_capture(true) first");
  azmi_pm* pm = s->pm;
  SB_TRY(hipSetDevice(pm->device));
  sb_launch_capture(s, pm->pick(stream));
  SB_TRY(hipGetLastError());
  return AZMI_OK;
}

int azmi_search_captured(azmi_search* s, uint64_t* key, uint8_t* player, int8_t* variant, uint32_t* len) {
  int rc = sb_begin_read(s, "captured"); if (rc) return rc;
  if (!s->cp.key) return SB_FAIL(AZMI_ERR_STATE, "captured: capture was never on for this batch; call set_capture(true) before playing");
  azmi_pm* pm = s->pm;
  SB_TRY(hipSetDevice(pm->device));
  rc = sb_check_device(s, pm->last); if (rc) return rc;      // (synchronises)
  const size_t rows = static_cast<size_t>(s->n) * s->pl.log_cap;
  if (key) SB_TRY(hipMemcpy(key, s->cp.key, rows * 8, hipMemcpyDeviceToHost));
  if (player) SB_TRY(hipMemcpy(player, s->cp.player, rows, hipMemcpyDeviceToHost));
  if (variant) SB_TRY(hipMemcpy(variant, s->cp.variant, rows, hipMemcpyDeviceToHost));
  if (len) SB_TRY(hipMemcpy(len, s->cp.len, static_cast<size_t>(s->n) * 4, hipMemcpyDeviceToHost));
  return AZMI_OK;
}

int azmi_search_net_metrics(azmi_search* s, azmi_net* net, double* out, float* raw_v, float* raw_pi, uint8_t* valid, void* stream) {
  int rc = sb_begin_move(s, "net_vs_search"); if (rc) return rc;
  if (!net) return SB_FAIL(AZMI_ERR_INVALID, "net_vs_search: needs a net");
  azmi_pm* pm = s->pm;
  SB_TRY(hipSetDevice(pm->device));
  if (!s->d_nm_out) {
    rc = pm->alloc(s->d_nm_valid, s->n, true); if (rc) return rc;
    rc = pm->alloc(s->d_nm_out, static_cast<size_t>(s->n) * 3, true); if (rc) return rc;
  }
  hipStream_t st = pm->pick(stream);
  const size_t N = s->n, V = pm->gi.P + 1, M = pm->gi.M;
  // the step API's staging buffers are free (no step is pending): the roots' planes, the net's raw rows
  sb_launch_root_canon(s, st);
  rc = azmi_net_forward(net, s->d_batch, s->d_vrows, s->d_pirows, s->n, st);
  if (rc != AZMI_OK) return SB_FAIL(rc, "leaf net: %s", azmi_net_last_error());
  s->net_calls += 1;
  sb_launch_net_metrics(s, st);
  SB_TRY(hipGetLastError());
  if (out) SB_TRY(hipMemcpyAsync(out, s->d_nm_out, N * 3 * 8, hipMemcpyDeviceToHost, st));
  if (raw_v) SB_TRY(hipMemcpyAsync(raw_v, s->d_vrows, N * V * 4, hipMemcpyDeviceToHost, st));
  if (raw_pi) SB_TRY(hipMemcpyAsync(raw_pi, s->d_pirows, N * M * 4, hipMemcpyDeviceToHost, st));
  if (valid) SB_TRY(hipMemcpyAsync(valid, s->d_nm_valid, N, hipMemcpyDeviceToHost, st));
  return sb_check_device(s, st);      // the one synchronisation
}

int azmi_pool_unique(const uint64_t* keys, const uint8_t* valid, uint32_t n, uint32_t* first_index_out, uint32_t* n_unique, uint32_t* n_duplicates,
                     int device, void* stream) {
  if (n > kPoolMaxRecords)
    return SB_FAIL(AZMI_ERR_INVALID, "azmi_pool_unique: n = %u records: the table takes a power of two of at least 2 n slots indexed by 32 bits, "
                   "at most %u records", n, kPoolMaxRecords);
  if (!n_unique || !n_duplicates || (n && (!keys || !first_index_out))) return SB_FAIL(AZMI_ERR_INVALID, "azmi_pool_unique: null argument");
  *n_unique = 0; *n_duplicates = 0;
  if (n == 0) return AZMI_OK;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return SB_FAIL(AZMI_ERR_NO_DEVICE, "no HIP device: libazmi has no CPU path");
  if (device < 0 || device >= ndev) return SB_FAIL(AZMI_ERR_INVALID, "device %d out of range", device);
  SB_TRY(hipSetDevice(device));
  hipStream_t st = stream == AZMI_STREAM_ENGINE ? nullptr : static_cast<hipStream_t>(stream);
  uint32_t slots = 64;
  while (slots < 2u * n) slots <<= 1;
  DevTemps tmp;
  uint64_t* d_keys = nullptr; uint8_t* d_valid = nullptr; uint32_t *d_owner = nullptr, *d_first = nullptr, *d_slot_of = nullptr, *d_out = nullptr, *d_counts = nullptr;
  std::vector<uint8_t> all;
  if (!valid) { all.assign(n, 1); valid = all.data(); }
  AZMI_HIP_TRY_NODEV(tmp.upload_async(d_keys, keys, n, st));
  hipError_t e = tmp.upload_async(d_valid, valid, n, st);
  if (e == hipSuccess) e = tmp.alloc(d_owner, slots);
  if (e == hipSuccess) e = tmp.alloc(d_first, slots);
  if (e == hipSuccess) e = tmp.alloc(d_slot_of, n);
  if (e == hipSuccess) e = tmp.alloc(d_out, n);
  if (e == hipSuccess) e = tmp.alloc(d_counts, 2);
  if (e == hipSuccess) e = hipMemsetAsync(d_owner, 0xFF, static_cast<size_t>(slots) * 4, st);      // kPoolEmpty
  if (e == hipSuccess) e = hipMemsetAsync(d_first, 0xFF, static_cast<size_t>(slots) * 4, st);
  if (e == hipSuccess) {
    sb_launch_pool_claim(d_keys, d_valid, n, slots - 1u, d_owner, d_first, d_slot_of, st);
    sb_launch_pool_compact(d_valid, n, d_first, d_slot_of, d_out, d_counts, st);
    e = hipGetLastError();
  }
  uint32_t counts[2] = {0, 0};
  if (e == hipSuccess) e = hipMemcpyAsync(counts, d_counts, 8, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(first_index_out, d_out, static_cast<size_t>(n) * 4, hipMemcpyDeviceToHost, st);
  const hipError_t es = hipStreamSynchronize(st);      // always: what was queued reads the buffers tmp is about to free
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return SB_FAIL(e == hipErrorOutOfMemory ? AZMI_ERR_OOM : AZMI_ERR_NO_DEVICE, "azmi_pool_unique: %s", hipGetErrorString(e));
  *n_unique = counts[0]; *n_duplicates = counts[1];
  return AZMI_OK;
}

}  // extern "C"
