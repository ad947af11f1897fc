// azmi_net_refresh (include/azmi.h): the weight image of a live matrix-core leaf net rewritten in place from the trained model's
// parameters, on a stream.  The family states what its image is made of (Family::refresh_plan: the ordered parameter list and
// the region map, leafnet_refresh_types.h); this unit checks the caller's table against it, launches the three kernels of
// leafnet_refresh_kernels.h into a staging image and moves that into the live one with one device-to-device copy on the same
// stream: work enqueued on the stream before the call reads the old weights whole, work enqueued after it the new ones whole.
// Its own translation unit: the device modules of the leaf-net and pipeline units stay what they were.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <utility>

#include "leafnet_host.h"
#include "leafnet_refresh_kernels.h"

namespace azmi_net_host {

using namespace azmi_refresh;

struct RefreshState {
  Plan plan;
  Bn* bns = nullptr;            // the plan on the device
  Frag* frags = nullptr;
  F32* f32s = nullptr;
  Param* table = nullptr;       // the caller's table: device copy and its pinned source
  Param* table_host = nullptr;
  double* scratch = nullptr;    // [BatchNorm][a, b][BN_STRIDE]
  uint8_t* staging = nullptr;   // the image being written
  hipEvent_t done = nullptr;    // behind the last refresh: the next one reuses table_host and staging
  bool pending = false;
  uint32_t frag_blocks = 1, f32_blocks = 1;
};

void free_refresh(RefreshState* st) {
  if (!st) return;
  if (st->pending) (void)hipEventSynchronize(st->done);
  if (st->done) (void)hipEventDestroy(st->done);
  (void)hipFree(st->bns); (void)hipFree(st->frags); (void)hipFree(st->f32s); (void)hipFree(st->table);
  (void)hipFree(st->scratch); (void)hipFree(st->staging);
  if (st->table_host) (void)hipHostFree(st->table_host);
  delete st;
}

}  // namespace azmi_net_host

namespace {

using namespace azmi_net_host;
using namespace azmi_refresh;

// The plan against itself and against the image: every index inside its table, no zero divisor, and the regions tile
// [0, blob_bytes) exactly - so every store of the kernels lands inside the staging image and every byte of it is written
const char* plan_fault(const Plan& p, size_t blob_bytes) {
  const uint32_t np = static_cast<uint32_t>(p.params.size()), nb = static_cast<uint32_t>(p.bns.size());
  if (np == 0) return "no parameters";
  for (const Bn& b : p.bns)
    if (b.w >= np || b.b >= np || b.mean >= np || b.var >= np || b.channels > BN_STRIDE) return "a BatchNorm record is out of range";
  std::vector<std::pair<uint64_t, uint64_t>> spans;
  for (const Frag& f : p.frags) {
    if (!f.mt || !f.kspc || !f.npass || !f.kc || f.npass > 32) return "a fragment region has a zero size";
    for (int s = 0; s < 2; ++s)
      if (f.src[s] >= np || (f.bn[s] != NO_BN && (f.bn[s] >= nb || f.rows[s] > p.bns[f.bn[s]].channels))) return "a fragment region is out of range";
    spans.emplace_back(f.dst, static_cast<uint64_t>(f.units) * 16);
  }
  for (const F32& r : p.f32s) {
    const bool bn = r.kind == F32_BN_A || r.kind == F32_BN_B;
    if (bn ? (r.src >= nb || r.valid > p.bns[r.src].channels) : r.src >= np) return "a float32 region is out of range";
    if (r.kind == F32_FRAG && (r.k < 16 || r.k % 16 || r.count % (16 * r.k))) return "a float32 fragment region has a bad shape";
    if (r.kind > F32_FRAG || r.valid > r.count) return "a float32 region is malformed";
    spans.emplace_back(r.dst, static_cast<uint64_t>(r.count) * 4);
  }
  std::sort(spans.begin(), spans.end());
  uint64_t at = 0;
  for (const auto& s : spans) {
    if (s.first != at) return "the regions do not tile the weight image";
    at += s.second;
  }
  return at == blob_bytes ? nullptr : "the regions do not end where the weight image ends";
}

template <class T>
bool to_device(T** dst, const std::vector<T>& src) {
  if (src.empty()) return true;
  return hipMalloc(reinterpret_cast<void**>(dst), src.size() * sizeof(T)) == hipSuccess &&
         hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess;
}

// first refresh of a net: the plan, its device copy, the table, the scratch and the staging image (synchronous, once)
int prepare(azmi_net* net) {
  auto st = new RefreshState();
  if (!net->blob || !net->family->refresh_plan(&st->plan)) {
    delete st;
    return nfail(AZMI_ERR_INVALID, "refresh is not built for this family: build a new HipLeafNet from the model (azmi_net_create*)");
  }
  if (const char* why = plan_fault(st->plan, net->blob_bytes)) {
    delete st;
    return nfail(AZMI_ERR_STATE, "azmi_net_refresh: %s", why);
  }
  uint32_t frag_units = 1, f32_count = 1;
  for (const Frag& f : st->plan.frags) frag_units = std::max(frag_units, f.units);
  for (const F32& r : st->plan.f32s) f32_count = std::max(f32_count, r.count);
  st->frag_blocks = std::min<uint32_t>((frag_units + NTH - 1) / NTH, 64);
  st->f32_blocks = std::min<uint32_t>((f32_count + NTH - 1) / NTH, 64);
  const size_t n = st->plan.params.size();
  const bool ok = to_device(&st->bns, st->plan.bns) && to_device(&st->frags, st->plan.frags) && to_device(&st->f32s, st->plan.f32s) &&
                  hipMalloc(reinterpret_cast<void**>(&st->table), n * sizeof(Param)) == hipSuccess &&
                  hipHostMalloc(reinterpret_cast<void**>(&st->table_host), n * sizeof(Param), hipHostMallocDefault) == hipSuccess &&
                  hipMalloc(reinterpret_cast<void**>(&st->scratch), std::max<size_t>(st->plan.bns.size(), 1) * 2 * BN_STRIDE * sizeof(double)) == hipSuccess &&
                  hipMalloc(reinterpret_cast<void**>(&st->staging), net->blob_bytes) == hipSuccess &&
                  hipEventCreateWithFlags(&st->done, hipEventDisableTiming) == hipSuccess;
  if (!ok) {
    free_refresh(st);
    return nfail(AZMI_ERR_OOM, "azmi_net_refresh: allocating the table, scratch and staging image failed");
  }
  net->refresh = st;
  return AZMI_OK;
}

}  // namespace

extern "C" int azmi_net_refresh(azmi_net* net, const azmi_net_param* params, uint32_t n_params, void* stream) {
  if (!net || !params) return nfail(AZMI_ERR_INVALID, "null argument");
  std::lock_guard<std::mutex> lock(net->refresh_mu);
  if (hipSetDevice(net->device) != hipSuccess) return nfail(AZMI_ERR_NO_DEVICE, "hipSetDevice failed");
  if (!net->refresh) {
    const int rc = prepare(net);
    if (rc != AZMI_OK) return rc;
  }
  RefreshState& st = *net->refresh;
  // the table against the family's list, before anything is enqueued: a refusal leaves the weights as they were
  const std::vector<ParamSpec>& want = st.plan.params;
  if (n_params != want.size())
    return nfail(AZMI_ERR_INVALID, "azmi_net_refresh: %u parameters given, this net's family reads %zu (the first is %s)", n_params, want.size(),
                 want[0].name.c_str());
  for (uint32_t i = 0; i < n_params; ++i) {
    const azmi_net_param& p = params[i];
    const char* name = want[i].name.c_str();
    if (p.kind != want[i].kind) return nfail(AZMI_ERR_INVALID, "azmi_net_refresh: parameter %u (%s) has kind %u, expected %u", i, name, p.kind, want[i].kind);
    if (p.count != want[i].count)
      return nfail(AZMI_ERR_INVALID, "azmi_net_refresh: %s has %llu elements, this net was built with %llu", name,
                   static_cast<unsigned long long>(p.count), static_cast<unsigned long long>(want[i].count));
    if (!p.data) return nfail(AZMI_ERR_INVALID, "azmi_net_refresh: %s has a null pointer", name);
    if (p.reserved != 0) return nfail(AZMI_ERR_INVALID, "azmi_net_refresh: %s: the reserved word must be zero", name);
    if (p.kind == AZMI_PARAM_BN_VAR && !(p.eps >= 0.0)) return nfail(AZMI_ERR_INVALID, "azmi_net_refresh: %s: eps must be >= 0", name);
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p.data) != hipSuccess || at.type != hipMemoryTypeDevice || at.device != net->device) {
      (void)hipGetLastError();
      return nfail(AZMI_ERR_INVALID, "azmi_net_refresh: %s is not device memory of device %d", name, net->device);
    }
  }
  if (st.pending && hipEventSynchronize(st.done) != hipSuccess) return nfail(AZMI_ERR_NO_DEVICE, "azmi_net_refresh: the previous refresh failed");
  st.pending = false;
  for (uint32_t i = 0; i < n_params; ++i) st.table_host[i] = Param{static_cast<const float*>(params[i].data), params[i].count, params[i].eps};
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (hipMemcpyAsync(st.table, st.table_host, n_params * sizeof(Param), hipMemcpyHostToDevice, s) != hipSuccess)
    return nfail(AZMI_ERR_NO_DEVICE, "azmi_net_refresh: table upload failed");
  const uint32_t nb = static_cast<uint32_t>(st.plan.bns.size()), nf = static_cast<uint32_t>(st.plan.frags.size()),
                 n32 = static_cast<uint32_t>(st.plan.f32s.size());
  if (nb) k_refresh_bn<<<dim3(1, nb), NTH, 0, s>>>(st.table, st.bns, st.scratch);
  if (nf) k_refresh_frags<<<dim3(st.frag_blocks, nf), NTH, 0, s>>>(st.table, st.frags, st.scratch, st.staging);
  if (n32) k_refresh_f32<<<dim3(st.f32_blocks, n32), NTH, 0, s>>>(st.table, st.f32s, st.scratch, st.staging);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(net->blob, st.staging, net->blob_bytes, hipMemcpyDeviceToDevice, s);
  // (recorded even after a failed launch: the pinned table may be in flight)
  st.pending = hipEventRecord(st.done, s) == hipSuccess;
  if (e != hipSuccess) return nfail(AZMI_ERR_NO_DEVICE, "azmi_net_refresh: %s", hipGetErrorString(e));
  return AZMI_OK;
}
