// Host side of the leaf nets, shared by leafnet.hip (the C entries behind azmi_net_*) and the family units
// (leafnet_c4_host.hip, leafnet_sp_host.hip, leafnet_dense_host.hip, leafnet_dense_sp_host.hip):
//   * Family     - what a net does behind its handle: one record per net, built by its family's `make`;
//   * FamilyDef  - what a family unit registers: its bounds, its weight image and `make`;
//   * BlobCursor - the one statement of a weight image: a walk over its sections that sizes it or hands out device pointers;
//   * azmi_net   - what every net shares: device, weight image, per-stream scratch, the record.
// No device code: the kernels stay in their headers and are included by their family unit alone.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <map>
#include <mutex>
#include <string>

#include "../../include/azmi.h"
#include "host_error.h"
#include "leafnet_c4_types.h"
#include "leafnet_refresh_types.h"

namespace azmi_net_host {

// the error text behind azmi_net_last_error (thread-local, leafnet.hip): sets it and returns `code`
int nfail(int code, const char* fmt, ...);
// a refusal text with arguments (std::string: empty = inside the bounds), cut like every error text of the library
inline std::string textf(const char* fmt, ...) {
  std::string s;
  AZMI_FORMAT_ERROR(s, fmt);
  return s;
}

struct Family {
  virtual ~Family() = default;      // frees what the family owns beside the weight image and the per-stream scratch
  // rows == nullptr: a dense batch of rows_max rows; else the eval list rows[0 .. *row_count), rows that are not listed untouched
  virtual int forward(const float* canon, float* v, float* pi, uint32_t rows_max, const uint32_t* rows, const uint32_t* row_count,
                      void* stream) = 0;
  // false: forward takes dense batches only and azmi_net_forward_rows stages the list for it (gather, forward, scatter)
  virtual bool takes_rows() const { return true; }
  virtual void dims(uint32_t* chw, uint32_t* p1, uint32_t* m) const = 0;      // floats per canonical row, P+1, M
  virtual int reserve_stream(void* stream, uint32_t max_rows) { return AZMI_OK; }      // nothing per stream
  virtual int c4_view(azmi_net_c4_view* out) const { return 0; }      // only the Connect4 tile is launched through a view
  // the trunk read-out: refused (leafnet.hip, kTrunkOnTile) unless the family keeps its trunk's output in memory
  virtual int trunk_channels(uint32_t* cf);
  virtual int trunk_features(const float* canon, float* features, uint32_t batch, void* stream);
  // azmi_net_refresh: the family's parameter list and the region map of its image; false = refresh is not built for this family
  virtual bool refresh_plan(azmi_refresh::Plan* plan) const { return false; }
};
// what azmi_net_refresh keeps per net from its first call on (leafnet_refresh.hip): plan, table, scratch, staging image
struct RefreshState;
void free_refresh(RefreshState* state);

// A matrix-core family, registered once (leafnet.hip, resolve / resolve2 name the records).  azmi_net_create* calls refusal,
// compares the blob with blob_bytes - both before the device is touched - uploads the image and calls make.
struct FamilyDef {
  std::string (*refusal)(const azmi_net_desc* d);      // empty when `d` is inside the family's bounds, else what is outside
  size_t (*blob_bytes)(const azmi_net_desc* d);        // the final offset of the family's layout; answers without validating
  int (*make)(const azmi_net_desc* d, azmi_net* net);  // net->blob holds the image: sets net->family, or fails through nfail
};
// (functions, not objects: a record of host function pointers must not be emitted into the device code of its unit)
const FamilyDef& c4_family();
const FamilyDef& spatial_family();
const FamilyDef& dense_family();
const FamilyDef& dense_layer_family();
const FamilyDef& dense_sp_family();

// A family states its image once, as calls in section order: with base == nullptr the walk only adds up (off = blob_bytes at the
// end), with the device pointer it yields the sections
struct BlobCursor {
  const uint8_t* base = nullptr;
  size_t off = 0;
  const uint8_t* bytes(size_t n) {
    const uint8_t* p = base ? base + off : nullptr;
    off += n;
    return p;
  }
  const float* f32(size_t count) { return reinterpret_cast<const float*>(bytes(count * 4)); }
};

}  // namespace azmi_net_host

struct azmi_net {
  int device = 0;
  void* blob = nullptr;      // the weight image on the device (the fp32 tier keeps its own: leafnet_f32.hip)
  size_t blob_bytes = 0;
  azmi_net_host::Family* family = nullptr;
  std::mutex refresh_mu;
  azmi_net_host::RefreshState* refresh = nullptr;
  // Scratch between the kernels of one forward: PER STREAM - engines on different streams share one net object and run
  // their forwards concurrently (round 1 kept one buffer per net: the value heads of concurrent shards read each other's
  // pooled features)
  struct StreamScratch {
    float* pool = nullptr;     // [2][pool_rows][64] pooled value-head / policy-head features between k_leafnet_sp and k_heads_fc_a,
    uint32_t pool_rows = 0;    // [pool_rows][32] global-action logits and [pool_rows][hidden] last hidden layer between _a and _b
    uint32_t pool_hidden = 0;
    float *g_canon = nullptr, *g_v = nullptr, *g_pi = nullptr;   // row-list staging for a family that takes dense batches only
    uint32_t g_rows = 0;
  };
  std::mutex scratch_mu;
  std::map<void*, StreamScratch> scratch;
  StreamScratch& scratch_of(void* stream) { std::lock_guard<std::mutex> l(scratch_mu); return scratch[stream]; }
  void free_scratch() {
    for (auto& kv : scratch) {
      StreamScratch& sc = kv.second;
      if (sc.pool) (void)hipFree(sc.pool);
      if (sc.g_canon) (void)hipFree(sc.g_canon);
      if (sc.g_v) (void)hipFree(sc.g_v);
      if (sc.g_pi) (void)hipFree(sc.g_pi);
    }
    scratch.clear();
  }
};
