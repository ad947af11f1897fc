// Stand-alone C ABI of the device S3-FIFO cache: the counterpart of the reference's
// `S3FIFOCache` / `ShardedS3FIFOCache` Python classes (py_wrapper.cc:222-259) — used by the parity
// tests against the oracle's restatement of s3fifo_cache.h and available to callers such as
// cache_utils.cached_inference.  The PlayManager engine embeds the same structure (engine.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/azmi.h"
#include "cache_host.h"
#include "cache_rows_kernels.h"
#include "host_error.h"
#include "leafnet_host.h"

using namespace azmi;

namespace {
thread_local std::string g_cache_err;
int cfail(int code, const char* fmt, ...) {
  AZMI_FORMAT_ERROR(g_cache_err, fmt);
  return code;
}

// one lane per shard, batch order preserved inside a shard (s3fifo_cache.h:259-286)
__global__ void k_cache_insert_many(CacheView c, const uint64_t* hashes, const float* policy, const float* value, uint32_t n) {
  const uint32_t sh = blockIdx.x * blockDim.x + threadIdx.x;
  if (sh >= c.shards) return;
  ShardCtx ctx(c, sh);
  for (uint32_t i = 0; i < n; ++i) {
    const uint64_t h = hashes[i];
    if (shard_of(c, h) != sh) continue;
    const int slot = ctx.insert(h);
    if (slot < 0) continue;
    float* dp = c.policy + (static_cast<size_t>(sh) * c.cap + slot) * c.np;
    float* dv = c.value + (static_cast<size_t>(sh) * c.cap + slot) * c.nv;
    for (uint32_t j = 0; j < c.np; ++j) dp[j] = policy[static_cast<size_t>(i) * c.np + j];
    for (uint32_t j = 0; j < c.nv; ++j) dv[j] = value[static_cast<size_t>(i) * c.nv + j];
  }
}

__global__ __launch_bounds__(256) void k_cache_apply_wave(CacheView c, const uint64_t* keys, const float* policy, const float* value, uint32_t n) {
  __shared__ uint32_t s_sid[kApplyMax];
  cache_apply_batch<true>(c, keys, policy, value, n, s_sid);      // hash 0 is a key here (s3fifo_cache.h has no reserved key)
}

// G lanes per query: the lane-group shapes the engines use (GM::GROUP: 8 = the DPP reduction, 64 = the shuffle reduction).  The
// stand-alone cache probes with 8; azmi_debug_cache_find_group chooses
template <int G>
__global__ void k_cache_find_wave(CacheView c, const uint64_t* hashes, uint32_t n, uint8_t* hit, float* policy, float* value) {
  const uint32_t gtid = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t i = gtid / G, gl = gtid % G;
  if (i >= n) return;
  uint32_t sh;
  const int slot = wave_shard_find<G>(c, hashes[i], gl, &sh);
  if (gl == 0) { wave_shard_find_account(c, hashes[i], sh, slot); hit[i] = slot >= 0; }
  if (slot < 0) return;
  const float* sp = c.policy + (static_cast<size_t>(sh) * kWaveCap + slot) * c.np;
  const float* sv = c.value + (static_cast<size_t>(sh) * kWaveCap + slot) * c.nv;
  for (uint32_t j = gl; j < c.np; j += G) policy[static_cast<size_t>(i) * c.np + j] = sp[j];
  for (uint32_t j = gl; j < c.nv; j += G) value[static_cast<size_t>(i) * c.nv + j] = sv[j];
}

__global__ void k_cache_find_many(CacheView c, const uint64_t* hashes, uint32_t n, uint8_t* hit, float* policy, float* value) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t sh;
  const int slot = cache_find(c, hashes[i], &sh);
  cache_find_account(c, hashes[i], sh, slot);
  hit[i] = slot >= 0;
  if (slot < 0) return;
  const float* sp = c.policy + (static_cast<size_t>(sh) * c.cap + slot) * c.np;
  const float* sv = c.value + (static_cast<size_t>(sh) * c.cap + slot) * c.nv;
  for (uint32_t j = 0; j < c.np; ++j) policy[static_cast<size_t>(i) * c.np + j] = sp[j];
  for (uint32_t j = 0; j < c.nv; ++j) value[static_cast<size_t>(i) * c.nv + j] = sv[j];
}

// k_pipe_cache_insert's shape (pipe_net_kernels.h) on host-given entries: `waves` wavefronts stride over the n entries, each entry
// under its shard's insert lock
__global__ __launch_bounds__(256) void k_debug_insert_locked(CacheView c, uint32_t* locks, const uint64_t* keys, const float* policy,
                                                             const float* value, uint32_t n, uint32_t waves, uint32_t* failed) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
  if (wave >= waves) return;
  for (uint32_t i = wave; i < n; i += waves) {
    const float p = lane < c.np ? policy[static_cast<size_t>(i) * c.np + lane] : 0.0f;
    const float v = lane < c.nv ? value[static_cast<size_t>(i) * c.nv + lane] : 0.0f;
    const bool ok = wave_shard_insert_locked<false>(c, locks, keys[i], p, v, lane);
    if (!ok && lane == 0) atomicAdd(failed, 1u);
  }
}

// shard_of as the device compiles it, one hash per thread
__global__ void k_debug_shard_index(uint32_t shards, uint64_t mul, const uint64_t* hashes, uint32_t n, uint32_t* out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = shard_of(hashes[i], shards, mul);
}

// the finds of one call: host arrays in, host arrays out.  group_lanes = 0: the generic tables, one lane per query
int find_many(azmi_cache* c, uint32_t group_lanes, const uint64_t* hashes, uint32_t n, uint8_t* hit, float* policy, float* value) {
  (void)hipSetDevice(c->device);
  uint64_t* dh = nullptr; uint8_t* dhit = nullptr; float *dp = nullptr, *dv = nullptr;
  hipError_t e = hipMalloc(&dh, n * 8ULL);
  if (e == hipSuccess) e = hipMalloc(&dhit, n);
  if (e == hipSuccess) e = hipMalloc(&dp, static_cast<size_t>(n) * c->c.np * 4);
  if (e == hipSuccess) e = hipMalloc(&dv, static_cast<size_t>(n) * c->c.nv * 4);
  if (e == hipSuccess) e = hipMemcpy(dh, hashes, n * 8ULL, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(dp, 0, static_cast<size_t>(n) * c->c.np * 4);
  if (e == hipSuccess) e = hipMemset(dv, 0, static_cast<size_t>(n) * c->c.nv * 4);
  if (e == hipSuccess) {
    const uint32_t blocks = static_cast<uint32_t>((static_cast<uint64_t>(n) * (group_lanes ? group_lanes : 1u) + 255u) / 256u);
    if (group_lanes == 8u) k_cache_find_wave<8><<<blocks, 256>>>(c->c, dh, n, dhit, dp, dv);
    else if (group_lanes == 64u) k_cache_find_wave<64><<<blocks, 256>>>(c->c, dh, n, dhit, dp, dv);
    else k_cache_find_many<<<blocks, 256>>>(c->c, dh, n, dhit, dp, dv);
    e = hipDeviceSynchronize();
  }
  if (e == hipSuccess) e = hipMemcpy(hit, dhit, n, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(policy, dp, static_cast<size_t>(n) * c->c.np * 4, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(value, dv, static_cast<size_t>(n) * c->c.nv * 4, hipMemcpyDeviceToHost);
  (void)hipFree(dh); (void)hipFree(dhit); (void)hipFree(dp); (void)hipFree(dv);
  return e == hipSuccess ? AZMI_OK : cfail(AZMI_ERR_NO_DEVICE, "cache find: %s", hipGetErrorString(e));
}

// ---- the device-pointer entries: scratch and launches (cache_rows_kernels.h) -----------------------------------------------------
// the scratch of `n` rows: the first call and a larger n only (synchronous, outside the steady state, like the leaf nets'
// per-stream staging); every other call finds it there
int rows_reserve(azmi_cache* c, uint32_t n) {
  if (c->rows_scratch && n <= c->rows_cap) return AZMI_OK;
  (void)hipDeviceSynchronize();      // an earlier call may still be using the old block
  if (c->rows_scratch) (void)hipFree(c->rows_scratch);
  c->rows_scratch = nullptr; c->rows_cap = 0;
  const size_t words = 1 + static_cast<size_t>(n) + rows_groups(n);
  if (hipMalloc(reinterpret_cast<void**>(&c->rows_scratch), words * 4) != hipSuccess) return cfail(AZMI_ERR_OOM, "hipMalloc(cache row scratch) failed");
  c->rows_cap = n;
  return AZMI_OK;
}
uint32_t* rows_miss_count(azmi_cache* c) { return c->rows_scratch; }
uint32_t* rows_miss_rows(azmi_cache* c) { return c->rows_scratch + 1; }
uint32_t* rows_offs(azmi_cache* c) { return c->rows_scratch + 1 + c->rows_cap; }

// find (+ the ordered miss list when miss_rows is given) enqueued on st; arguments checked by the callers
int enqueue_find_rows(azmi_cache* c, const uint64_t* keys, uint32_t n, uint8_t* hit, float* pi, float* v, uint32_t* miss_rows, uint32_t* miss_count,
                      hipStream_t st) {
  if (wave_layout(c->c)) k_cache_find_rows<true><<<(n + 31u) / 32u, 256, 0, st>>>(c->c, keys, n, hit, pi, v);
  else k_cache_find_rows<false><<<(n + 255u) / 256u, 256, 0, st>>>(c->c, keys, n, hit, pi, v);
  if (miss_rows) {
    k_cache_miss_scan<<<1, kRowsScanThreads, 0, st>>>(hit, n, rows_offs(c), miss_count);
    k_cache_miss_scatter<<<(n + 255u) / 256u, 256, 0, st>>>(hit, n, rows_offs(c), miss_rows);
  }
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? AZMI_OK : cfail(AZMI_ERR_NO_DEVICE, "cache find_rows launch: %s", hipGetErrorString(e));
}

int enqueue_insert_rows(azmi_cache* c, const uint64_t* keys, const float* pi, const float* v, const uint32_t* rows, const uint32_t* row_count,
                        uint32_t n_max, hipStream_t st) {
  if (wave_layout(c->c)) {
    const uint32_t chunks = rows_chunks(n_max, kApplyMax);      // in order on the one stream; a chunk behind *row_count exits at once
    for (uint32_t k = 0; k < chunks; ++k) {
      const uint32_t m = std::min<uint32_t>(kApplyMax, n_max - k * kApplyMax);
      k_cache_insert_rows_wave<<<(m + 3) / 4, 256, 0, st>>>(c->c, keys, pi, v, rows, row_count, n_max, k);
    }
  } else {
    k_cache_insert_rows<<<(c->c.shards + 63) / 64, 64, 0, st>>>(c->c, keys, pi, v, rows, row_count, n_max);
  }
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? AZMI_OK : cfail(AZMI_ERR_NO_DEVICE, "cache insert_rows launch: %s", hipGetErrorString(e));
}

}  // namespace


extern "C" {

const char* azmi_cache_last_error(void) { return g_cache_err.c_str(); }

int azmi_cache_create(uint32_t max_size, uint32_t shards, uint32_t ghost_size, uint32_t num_policy, uint32_t num_value,
                      int device, azmi_cache** out) {
  if (!out || shards == 0) return cfail(AZMI_ERR_INVALID, "bad cache arguments");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return cfail(AZMI_ERR_NO_DEVICE, "no HIP device: libazmi has no CPU path");
  if (hipSetDevice(device) != hipSuccess) return cfail(AZMI_ERR_NO_DEVICE, "hipSetDevice failed");
  auto* c = new azmi_cache();
  c->device = device;
  c->max_size = (max_size / shards) * shards;
  if (cache_alloc(c->c, c->allocs, max_size, shards, ghost_size, num_policy, num_value) != hipSuccess) {
    delete c;
    return cfail(AZMI_ERR_OOM, "cache allocation failed");
  }
  (void)hipDeviceSynchronize();
  *out = c;
  return AZMI_OK;
}
void azmi_cache_destroy(azmi_cache* c) { delete c; }

int azmi_cache_insert_many(azmi_cache* c, const uint64_t* hashes, const float* policy, const float* value, uint32_t n) {
  if (!c || (n && (!hashes || !policy || !value))) return cfail(AZMI_ERR_INVALID, "null argument");
  if (n == 0) return AZMI_OK;
  (void)hipSetDevice(c->device);
  uint64_t* dh = nullptr; float *dp = nullptr, *dv = nullptr;
  hipError_t e = hipMalloc(&dh, n * 8ULL);
  if (e == hipSuccess) e = hipMalloc(&dp, static_cast<size_t>(n) * c->c.np * 4);
  if (e == hipSuccess) e = hipMalloc(&dv, static_cast<size_t>(n) * c->c.nv * 4);
  if (e == hipSuccess) e = hipMemcpy(dh, hashes, n * 8ULL, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dp, policy, static_cast<size_t>(n) * c->c.np * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dv, value, static_cast<size_t>(n) * c->c.nv * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    if (wave_layout(c->c)) {
      for (uint32_t off = 0; off < n && e == hipSuccess; off += kApplyMax) {  // chunks keep batch order
        const uint32_t m = std::min<uint32_t>(kApplyMax, n - off);
        k_cache_apply_wave<<<(m + 3) / 4, 256>>>(c->c, dh + off, dp + static_cast<size_t>(off) * c->c.np, dv + static_cast<size_t>(off) * c->c.nv, m);
        e = hipDeviceSynchronize();
      }
    } else {
      k_cache_insert_many<<<(c->c.shards + 63) / 64, 64>>>(c->c, dh, dp, dv, n);
      e = hipDeviceSynchronize();
    }
  }
  (void)hipFree(dh); (void)hipFree(dp); (void)hipFree(dv);
  return e == hipSuccess ? AZMI_OK : cfail(AZMI_ERR_NO_DEVICE, "cache insert: %s", hipGetErrorString(e));
}

int azmi_cache_find_many(azmi_cache* c, const uint64_t* hashes, uint32_t n, uint8_t* hit, float* policy, float* value) {
  if (!c || (n && (!hashes || !hit || !policy || !value))) return cfail(AZMI_ERR_INVALID, "null argument");
  if (n == 0) return AZMI_OK;
  return find_many(c, wave_layout(c->c) ? 8u : 0u, hashes, n, hit, policy, value);
}

int azmi_cache_find_rows(azmi_cache* c, const uint64_t* d_keys, uint32_t n, uint8_t* d_hit, float* d_pi, float* d_v, uint32_t* d_miss_rows,
                         uint32_t* d_miss_count, void* stream) {
  if (!c) return cfail(AZMI_ERR_INVALID, "azmi_cache_find_rows: null argument: cache");
  if (n == 0) return AZMI_OK;
  if (!d_keys) return cfail(AZMI_ERR_INVALID, "azmi_cache_find_rows: null argument: d_keys");
  if (!d_hit) return cfail(AZMI_ERR_INVALID, "azmi_cache_find_rows: null argument: d_hit");
  if (!d_pi) return cfail(AZMI_ERR_INVALID, "azmi_cache_find_rows: null argument: d_pi");
  if (!d_v) return cfail(AZMI_ERR_INVALID, "azmi_cache_find_rows: null argument: d_v");
  if (!d_miss_rows != !d_miss_count)
    return cfail(AZMI_ERR_INVALID, "azmi_cache_find_rows: d_miss_rows and d_miss_count go together (both, or neither for no compaction)");
  if (n > kRowsMax) return cfail(AZMI_ERR_INVALID, "azmi_cache_find_rows: n = %u, at most 2^30 rows per call", n);
  if (hipSetDevice(c->device) != hipSuccess) return cfail(AZMI_ERR_NO_DEVICE, "hipSetDevice failed");
  if (d_miss_rows) { const int rc = rows_reserve(c, n); if (rc != AZMI_OK) return rc; }
  return enqueue_find_rows(c, d_keys, n, d_hit, d_pi, d_v, d_miss_rows, d_miss_count, static_cast<hipStream_t>(stream));
}

int azmi_cache_insert_rows(azmi_cache* c, const uint64_t* d_keys, const float* d_pi, const float* d_v, const uint32_t* d_rows,
                           const uint32_t* d_row_count, uint32_t n_max, void* stream) {
  if (!c) return cfail(AZMI_ERR_INVALID, "azmi_cache_insert_rows: null argument: cache");
  if (n_max == 0) return AZMI_OK;
  if (!d_keys) return cfail(AZMI_ERR_INVALID, "azmi_cache_insert_rows: null argument: d_keys");
  if (!d_pi) return cfail(AZMI_ERR_INVALID, "azmi_cache_insert_rows: null argument: d_pi");
  if (!d_v) return cfail(AZMI_ERR_INVALID, "azmi_cache_insert_rows: null argument: d_v");
  if (n_max > kRowsMax) return cfail(AZMI_ERR_INVALID, "azmi_cache_insert_rows: n_max = %u, at most 2^30 rows per call", n_max);
  if (hipSetDevice(c->device) != hipSuccess) return cfail(AZMI_ERR_NO_DEVICE, "hipSetDevice failed");
  return enqueue_insert_rows(c, d_keys, d_pi, d_v, d_rows, d_row_count, n_max, static_cast<hipStream_t>(stream));
}

int azmi_net_forward_cached(azmi_net* net, azmi_cache* c, const float* d_canon, const uint64_t* d_keys, uint32_t n, float* d_v, float* d_pi,
                            uint8_t* d_hit, void* stream) {
  if (!net) return cfail(AZMI_ERR_INVALID, "azmi_net_forward_cached: null argument: net");
  if (!c) return cfail(AZMI_ERR_INVALID, "azmi_net_forward_cached: null argument: cache");
  if (n == 0) return AZMI_OK;
  if (!d_canon) return cfail(AZMI_ERR_INVALID, "azmi_net_forward_cached: null argument: d_canon");
  if (!d_keys) return cfail(AZMI_ERR_INVALID, "azmi_net_forward_cached: null argument: d_keys");
  if (!d_v) return cfail(AZMI_ERR_INVALID, "azmi_net_forward_cached: null argument: d_v");
  if (!d_pi) return cfail(AZMI_ERR_INVALID, "azmi_net_forward_cached: null argument: d_pi");
  if (!d_hit) return cfail(AZMI_ERR_INVALID, "azmi_net_forward_cached: null argument: d_hit");
  if (n > kRowsMax) return cfail(AZMI_ERR_INVALID, "azmi_net_forward_cached: n = %u, at most 2^30 rows per call", n);
  uint32_t chw, p1, m;
  net->family->dims(&chw, &p1, &m);
  if (c->c.np != m || c->c.nv != p1)
    return cfail(AZMI_ERR_INVALID, "azmi_net_forward_cached: cache: num_policy = %u, num_value = %u, but the net answers %u moves and %u values",
                 c->c.np, c->c.nv, m, p1);
  if (c->device != net->device)
    return cfail(AZMI_ERR_INVALID, "azmi_net_forward_cached: cache: it lives on device %d, the net on device %d", c->device, net->device);
  if (hipSetDevice(c->device) != hipSuccess) return cfail(AZMI_ERR_NO_DEVICE, "hipSetDevice failed");
  int rc = rows_reserve(c, n); if (rc != AZMI_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  rc = enqueue_find_rows(c, d_keys, n, d_hit, d_pi, d_v, rows_miss_rows(c), rows_miss_count(c), st); if (rc != AZMI_OK) return rc;
  rc = azmi_net_forward_rows(net, d_canon, d_v, d_pi, rows_miss_rows(c), rows_miss_count(c), n, stream);
  if (rc != AZMI_OK) return cfail(rc, "azmi_net_forward_cached: leaf net: %s", azmi_net_last_error());
  return enqueue_insert_rows(c, d_keys, d_pi, d_v, rows_miss_rows(c), rows_miss_count(c), n, st);
}

int azmi_debug_cache_find_group(azmi_cache* c, uint32_t group_lanes, const uint64_t* hashes, uint32_t n, uint8_t* hit, float* policy, float* value) {
  if (!c || (n && (!hashes || !hit || !policy || !value))) return cfail(AZMI_ERR_INVALID, "azmi_debug_cache_find_group: null argument");
  if (group_lanes != 8u && group_lanes != 64u)
    return cfail(AZMI_ERR_INVALID, "azmi_debug_cache_find_group: group_lanes %u is not a lane group of the engines (8 or 64)", group_lanes);
  if (n == 0) return AZMI_OK;
  if (!wave_layout(c->c))
    return cfail(AZMI_ERR_INVALID, "azmi_debug_cache_find_group: not a cache of 64-entry wave shards (max_size / shards = %u, ghost_size / shards = %u)",
                 c->c.cap, c->c.ghost_cap);
  return find_many(c, group_lanes, hashes, n, hit, policy, value);
}

int azmi_debug_cache_insert_locked(azmi_cache* c, const uint64_t* hashes, const float* policy, const float* value, uint32_t n, uint32_t waves,
                                   uint32_t* failed_out) {
  if (!c || !failed_out || (n && (!hashes || !policy || !value))) return cfail(AZMI_ERR_INVALID, "azmi_debug_cache_insert_locked: null argument");
  if (waves == 0u || waves > 8192u) return cfail(AZMI_ERR_INVALID, "azmi_debug_cache_insert_locked: waves must be 1 .. 8192");
  *failed_out = 0;
  if (n == 0) return AZMI_OK;
  if (!wave_layout(c->c))
    return cfail(AZMI_ERR_INVALID, "azmi_debug_cache_insert_locked: not a cache of 64-entry wave shards (max_size / shards = %u, ghost_size / shards = %u)",
                 c->c.cap, c->c.ghost_cap);
  if (c->c.np > 64u || c->c.nv > 64u)
    return cfail(AZMI_ERR_INVALID, "azmi_debug_cache_insert_locked: a lane carries one entry of each row: num_policy and num_value must be <= 64 (%u, %u)",
                 c->c.np, c->c.nv);
  (void)hipSetDevice(c->device);
  const size_t np = c->c.np, nv = c->c.nv;
  uint64_t* dh = nullptr; float *dp = nullptr, *dv = nullptr; uint32_t* dl = nullptr;      // dl: [shards] lock words, then the failure count
  hipError_t e = hipMalloc(&dh, n * 8ULL);
  if (e == hipSuccess) e = hipMalloc(&dp, n * np * 4);
  if (e == hipSuccess) e = hipMalloc(&dv, n * nv * 4);
  if (e == hipSuccess) e = hipMalloc(&dl, (static_cast<size_t>(c->c.shards) + 1) * 4);
  if (e == hipSuccess) e = hipMemcpy(dh, hashes, n * 8ULL, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dp, policy, n * np * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dv, value, n * nv * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(dl, 0, (static_cast<size_t>(c->c.shards) + 1) * 4);
  if (e == hipSuccess) {
    if (waves == 1u) k_debug_insert_locked<<<1, 64>>>(c->c, dl, dh, dp, dv, n, waves, dl + c->c.shards);
    else k_debug_insert_locked<<<(waves + 3) / 4, 256>>>(c->c, dl, dh, dp, dv, n, waves, dl + c->c.shards);
    e = hipDeviceSynchronize();
  }
  if (e == hipSuccess) e = hipMemcpy(failed_out, dl + c->c.shards, 4, hipMemcpyDeviceToHost);
  (void)hipFree(dh); (void)hipFree(dp); (void)hipFree(dv); (void)hipFree(dl);
  return e == hipSuccess ? AZMI_OK : cfail(AZMI_ERR_NO_DEVICE, "azmi_debug_cache_insert_locked: %s", hipGetErrorString(e));
}

int azmi_debug_shard_index(int device, uint32_t shards, const uint64_t* hashes, uint32_t n, uint32_t* out) {
  if (shards == 0u) return cfail(AZMI_ERR_INVALID, "azmi_debug_shard_index: shards must be at least 1");
  if (n && (!hashes || !out)) return cfail(AZMI_ERR_INVALID, "azmi_debug_shard_index: null argument");
  if (n == 0) return AZMI_OK;
  const uint64_t mul = shard_multiplier(shards);
  if (device < 0) {      // the host's compilation of shard_of: what cache_alloc's callers and the insert logs' readers would run
    for (uint32_t i = 0; i < n; ++i) out[i] = shard_of(hashes[i], shards, mul);
    return AZMI_OK;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return cfail(AZMI_ERR_NO_DEVICE, "no HIP device: libazmi has no CPU path");
  if (hipSetDevice(device) != hipSuccess) return cfail(AZMI_ERR_NO_DEVICE, "hipSetDevice failed");
  uint64_t* dh = nullptr; uint32_t* dout = nullptr;
  hipError_t e = hipMalloc(&dh, n * 8ULL);
  if (e == hipSuccess) e = hipMalloc(&dout, n * 4ULL);
  if (e == hipSuccess) e = hipMemcpy(dh, hashes, n * 8ULL, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    k_debug_shard_index<<<(n + 255u) / 256u, 256>>>(shards, mul, dh, n, dout);
    e = hipDeviceSynchronize();
  }
  if (e == hipSuccess) e = hipMemcpy(out, dout, n * 4ULL, hipMemcpyDeviceToHost);
  (void)hipFree(dh); (void)hipFree(dout);
  return e == hipSuccess ? AZMI_OK : cfail(AZMI_ERR_NO_DEVICE, "azmi_debug_shard_index: %s", hipGetErrorString(e));
}

int azmi_cache_stats(azmi_cache* c, uint64_t out[6]) {
  if (!c || !out) return cfail(AZMI_ERR_INVALID, "null argument");
  (void)hipSetDevice(c->device);
  (void)hipDeviceSynchronize();      // the device-pointer entries run on the caller's streams: read behind all of them
  std::vector<unsigned long long> st(static_cast<size_t>(c->c.shards) * 4);
  std::vector<uint32_t> state(static_cast<size_t>(c->c.shards) * 8);
  if (hipMemcpy(st.data(), c->c.stats, st.size() * 8, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(state.data(), c->c.state, state.size() * 4, hipMemcpyDeviceToHost) != hipSuccess)
    return cfail(AZMI_ERR_NO_DEVICE, "cache stats copy failed");
  for (int i = 0; i < 6; ++i) out[i] = 0;
  for (uint32_t s = 0; s < c->c.shards; ++s) {
    for (int j = 0; j < 4; ++j) out[j] += st[static_cast<size_t>(s) * 4 + j];
    out[4] += state[static_cast<size_t>(s) * 8 + kSize];
  }
  out[5] = static_cast<uint64_t>(c->c.cap) * c->c.shards;
  return AZMI_OK;
}

}  // extern "C"
