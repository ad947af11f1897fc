// Leaf policy/value network on gfx950 matrix cores — the one dense contraction of the path.
//
// Restates the inference forward of the reference's ResNet-mode NNArch
// (/root/reference/src/neural_net.py:233-263 ResidualBlock, :448-510 NNArch.forward) and the
// probability output of NNWrapper.process (:800-823) for the trunk width the BASELINE configs
// use (64 channels, 3x3 convolutions, value head with average pool, flat policy head), with
// inference BatchNorms folded on the host (alphazero/hip_net.py):
//     stem   s  = conv3x3(x) + b0                         (bn1 folded)
//     block  t  = relu(a1 * s + b1)                       (bn1 of the block: affine on the stream)
//            u  = relu(conv3x3(t) + c1)                   (bn2 folded into conv1)
//            s  = s + conv3x3(u)
//     heads  h  = relu(conv1x1(s) + bh)                   (v_bn / pi_bn folded; 32 + 32 channels)
//            v  = softmax(W2 relu(W1 avgpool(h_v) + b1) + b2),  pi = softmax(Wp flatten(h_pi) + bp)
//
// Two kernels, one machine (a workgroup of 4 waves carries a tile of boards through the WHOLE net; weights stream from L2
// into an LDS ring by DMA; the residual stream stays in fp32 MFMA accumulators):
//   * leafnet_c4.h - the Connect4-family net (flat policy head), also launched fused with the engine's move step;
//   * leafnet_sp.h - the spatial-policy-head nets (Tafl family, StarGambit).
// and a third for the reference's DEFAULT trunk (dense_net, azmi_net_create2):
//   * leafnet_dense.h - the dense Connect4 family (6x7, 3x3 / 5x5, flat policy head): one wavefront per board, every raw
//     feature in LDS;
//   * leafnet_dense_sp.h - the dense spatial-head family (7x7 / 11x11 / 13x13, the single-variant StarGambit configs): one
//     workgroup per board.
// Each family's host side - bounds, weight image, kernel instances, launches - is its own unit (leafnet_c4_host.hip,
// leafnet_sp_host.hip, leafnet_dense_host.hip, leafnet_dense_sp_host.hip) behind one record (leafnet_host.h, Family).  This file
// is what they share behind azmi_net_* (include/azmi.h): the resolver from a descriptor to a family, the upload of the weight
// image, the C entries, the row-list staging for a family that takes dense batches only, and the adapter of the one such
// family, the fp32 correctness path (leafnet_f32.hip).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../include/azmi.h"
#include "leafnet_f32.h"
#include "leafnet_host.h"

namespace azmi_net_host {

static thread_local std::string g_net_err;
int nfail(int code, const char* fmt, ...) {
  AZMI_FORMAT_ERROR(g_net_err, fmt);
  return code;
}

// The trunk read-out exists where the trunk's output does: in the fp32 tier's activation buffer.  The matrix-core tiles keep
// theirs in LDS and registers and are not touched
static const char* kTrunkOnTile = "the trunk read-out (trunk_channels, trunk_features) runs on the fp32 tier only: the matrix-core tiles keep "
                                  "their trunk activations on chip; build the net with precision='fp32'";
int Family::trunk_channels(uint32_t*) { return nfail(AZMI_ERR_INVALID, "%s", kTrunkOnTile); }
int Family::trunk_features(const float*, float*, uint32_t, void*) { return nfail(AZMI_ERR_INVALID, "%s", kTrunkOnTile); }

}  // namespace azmi_net_host

namespace {

using namespace azmi_net_host;

// compact[i] = canon[rows[i]] for i < *count, zeros behind (those rows are evaluated and dropped)
__global__ void k_gather_rows(const float* __restrict__ canon, const uint32_t* __restrict__ rows, const uint32_t* __restrict__ count,
                              uint32_t max_rows, uint32_t chw, float* __restrict__ compact) {
  const uint32_t i = blockIdx.x;
  if (i >= max_rows) return;
  const bool on = i < *count;
  const float* src = canon + static_cast<size_t>(on ? rows[i] : 0u) * chw;
  float* dst = compact + static_cast<size_t>(i) * chw;
  for (uint32_t e = threadIdx.x; e < chw; e += blockDim.x) dst[e] = on ? src[e] : 0.0f;
}
// v[rows[i]] = v_c[i], pi[rows[i]] = pi_c[i] for i < *count: rows that are not listed are left untouched
__global__ void k_scatter_rows(const float* __restrict__ v_c, const float* __restrict__ pi_c, const uint32_t* __restrict__ rows,
                               const uint32_t* __restrict__ count, uint32_t p1, uint32_t m, float* __restrict__ v, float* __restrict__ pi) {
  const uint32_t i = blockIdx.x;
  if (i >= *count) return;
  const uint32_t r = rows[i];
  for (uint32_t e = threadIdx.x; e < p1; e += blockDim.x) v[static_cast<size_t>(r) * p1 + e] = v_c[static_cast<size_t>(i) * p1 + e];
  for (uint32_t e = threadIdx.x; e < m; e += blockDim.x) pi[static_cast<size_t>(r) * m + e] = pi_c[static_cast<size_t>(i) * m + e];
}

// The fp32 tier (azmi_f32::*, leafnet_f32.hip) behind the record.  It owns its weight image and keeps ONE set of activation
// buffers per net: a forward on another stream first waits for the previous one (a correctness path, not a throughput path)
struct F32Family : Family {
  void* impl = nullptr;
  void* last_stream = nullptr;
  bool last_stream_set = false;

  ~F32Family() override { azmi_f32::destroy(impl); }
  void take_buffers(void* stream) {
    if (last_stream_set && last_stream != stream) (void)hipStreamSynchronize(static_cast<hipStream_t>(last_stream));
    last_stream = stream; last_stream_set = true;
  }
  bool takes_rows() const override { return false; }
  int forward(const float* canon, float* v, float* pi, uint32_t batch, const uint32_t*, const uint32_t*, void* stream) override {
    take_buffers(stream);
    const char* msg = "";
    const int rc = azmi_f32::forward(impl, canon, v, pi, batch, stream, &msg);
    return rc == AZMI_OK ? rc : nfail(rc, "%s", msg);
  }
  void dims(uint32_t* chw, uint32_t* p1, uint32_t* m) const override { azmi_f32::dims(impl, chw, p1, m); }
  int trunk_channels(uint32_t* cf) override { *cf = azmi_f32::trunk_channels(impl); return AZMI_OK; }
  int trunk_features(const float* canon, float* features, uint32_t batch, void* stream) override {
    if (batch == 0) return AZMI_OK;
    if (!canon || !features) return nfail(AZMI_ERR_INVALID, "null argument");
    take_buffers(stream);
    const char* msg = "";
    const int rc = azmi_f32::trunk_features(impl, canon, features, batch, stream, &msg);
    return rc == AZMI_OK ? rc : nfail(rc, "%s", msg);
  }
};

// What a descriptor asks for: a refusal, the first descriptor's entries (azmi_net_desc2 with nothing set behind `base`), the fp32
// tier, or a matrix-core family - whose own bounds (FamilyDef::refusal) are checked where it is sized or created
struct Resolved {
  enum { REFUSED, FIRST, FP32, TILE } to = REFUSED;
  const char* why = nullptr;
  const FamilyDef* tile = nullptr;
  bool f32_dense = false;
  azmi_f32::Variant var;
};
Resolved refused(const char* why) { Resolved r; r.why = why; return r; }
Resolved to_tile(const FamilyDef& f) { Resolved r; r.to = Resolved::TILE; r.tile = &f; return r; }
Resolved to_f32(bool dense, azmi_f32::Variant var = azmi_f32::Variant{}) { Resolved r; r.to = Resolved::FP32; r.f32_dense = dense; r.var = var; return r; }

// the ResNet tile of a first descriptor, whatever else it says
const FamilyDef& resnet_tile(const azmi_net_desc* d) { return d->policy_channels > 0 ? spatial_family() : c4_family(); }
Resolved resolve(const azmi_net_desc* d) {
  if (d->precision == 1) return to_f32(false);      // (a ResNet trunk: 3x3 only, azmi_f32::create)
  if (d->precision != 0 && d->precision != 2) return refused("precision must be 0 (bf16 MFMA), 1 (fp32) or 2 (bf16x3: split bf16 MFMA)");
  return to_tile(resnet_tile(d));
}

bool reserved_zero(const azmi_net_desc2* d) {
  for (int32_t r : d->reserved) if (r != 0) return false;
  return true;
}
// The words behind dense_net: NULL when they are in range, else what is not
const char* variant_refusal(const azmi_net_desc2* d) {
  if (d->trunk_norm != 0 && d->trunk_norm != 1) return "azmi_net_desc2: trunk_norm must be 0 (batch) or 1 (layer)";
  if (d->trunk_act != 0 && d->trunk_act != 1) return "azmi_net_desc2: trunk_act must be 0 (relu) or 1 (crelu)";
  if (d->pi_fc_layers < 0) return "azmi_net_desc2: pi_fc_layers must be >= 0";
  if (d->pi_fc_layers > 0 && d->base.policy_channels > 0) return "azmi_net_desc2: pi_fc_layers > 0 is the flat policy head's FC stack (policy_channels must be 0)";
  if (d->pi_fc_layers > 0 && d->base.pi_hidden < 1) return "azmi_net_desc2: pi_fc_layers > 0 needs pi_hidden (the stack's width)";
  return nullptr;
}
bool is_variant(const azmi_net_desc2* d) { return d->trunk_norm != 0 || d->trunk_act != 0 || d->pi_fc_layers != 0; }
azmi_f32::Variant f32_variant(const azmi_net_desc2* d) {
  azmi_f32::Variant v;
  v.trunk_norm = d->trunk_norm; v.trunk_act = d->trunk_act; v.pi_fc_layers = d->pi_fc_layers;
  return v;
}
// The one variant a matrix-core tile takes: the dense tile's layer-norm instance (trunk_act relu, no policy FC stack).  The ResNet
// tiles are tuned around the folded BatchNorms, the dense tile's LDS plan has no room for crelu's doubled K, and no tile has
// the policy FC stack
bool tile_layer(const azmi_net_desc2* d) {
  return d->dense_net == 1 && d->base.precision == 0 && d->trunk_norm == 1 && d->trunk_act == 0 && d->pi_fc_layers == 0;
}
const char* kVariantOnTile = "the matrix-core tiles cover trunk_act='relu' and pi_fc_layers=0, with trunk_norm='batch' or, on the dense "
                             "Connect4 tile (precision 'bf16'), 'layer'; use precision='fp32' for the other layer-norm nets, crelu and "
                             "the policy FC stack";
const char* kLayerOnDenseSp = "dense spatial leaf net kernel: trunk_norm='batch' only (the layer-norm instance is the dense Connect4 tile's); "
                              "use precision='fp32' for layer-norm nets";
// Which dense tile a bf16 descriptor is for: the spatial one takes every spatial head off the 6x7 board (a spatial head ON 6x7 is
// refused by the Connect4 tile's own words, as it always was)
bool is_dense_spatial(const azmi_net_desc* d) { return d->policy_channels > 0 && !(d->height == 6 && d->width == 7); }

// The decision tree of the second descriptor, for azmi_net_create2 and azmi_net_blob_bytes2 alike
Resolved resolve2(const azmi_net_desc2* d2) {
  if (!reserved_zero(d2)) return refused("azmi_net_desc2: reserved words must be zero");
  if (d2->dense_net != 0 && d2->dense_net != 1) return refused("azmi_net_desc2: dense_net must be 0 or 1");
  if (const char* why = variant_refusal(d2)) return refused(why);
  const azmi_net_desc* d = &d2->base;
  const bool layer = tile_layer(d2);
  if (is_variant(d2) && !layer)      // either trunk, the fp32 tier
    return d->precision == 1 ? to_f32(d2->dense_net == 1, f32_variant(d2)) : refused(kVariantOnTile);
  if (!d2->dense_net) { Resolved r; r.to = Resolved::FIRST; return r; }      // the old entries, with everything they refuse
  if (d->precision == 1) return to_f32(true);
  if (d->precision == 2) return refused("dense leaf net: no bf16x3 tier; the 1e-5 tier of dense nets is precision='fp32'");
  if (d->precision != 0) return refused("precision must be 0 (bf16 MFMA) or 1 (fp32) for a dense net");
  if (is_dense_spatial(d)) return layer ? refused(kLayerOnDenseSp) : to_tile(dense_sp_family());
  return to_tile(layer ? dense_layer_family() : dense_family());
}

// The weight image on the device and the net object around it: AZMI_OK and *out, or nothing left behind
int upload(const void* blob, size_t blob_bytes, int device, azmi_net** out) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return nfail(AZMI_ERR_NO_DEVICE, "no HIP device: libazmi has no CPU path");
  if (hipSetDevice(device) != hipSuccess) return nfail(AZMI_ERR_NO_DEVICE, "hipSetDevice failed");
  auto net = new azmi_net();
  net->device = device;
  if (hipMalloc(&net->blob, blob_bytes) != hipSuccess) { delete net; return nfail(AZMI_ERR_OOM, "hipMalloc(weights) failed"); }
  if (hipMemcpy(net->blob, blob, blob_bytes, hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(net->blob); delete net;
    return nfail(AZMI_ERR_NO_DEVICE, "weight upload failed");
  }
  net->blob_bytes = blob_bytes;
  *out = net;
  return AZMI_OK;
}
// the one way out of a net, finished or not: the record, the weight image, the per-stream scratch
void release(azmi_net* net) {
  (void)hipSetDevice(net->device);
  delete net->family;
  free_refresh(net->refresh);
  (void)hipFree(net->blob);
  net->free_scratch();
  delete net;
}

int create(const Resolved& r, const azmi_net_desc* d, const void* blob, size_t blob_bytes, int device, azmi_net** out) {
  if (r.to == Resolved::REFUSED) return nfail(AZMI_ERR_INVALID, "%s", r.why);
  if (r.to == Resolved::FP32) {
    const char* msg = "";
    void* impl = nullptr;
    const int rc = azmi_f32::create(d, r.f32_dense, blob, blob_bytes, device, &impl, &msg, r.var);
    if (rc != AZMI_OK) return nfail(rc, "%s", msg);
    auto f = new F32Family();
    f->impl = impl;
    auto net = new azmi_net();
    net->device = device; net->family = f;
    *out = net;
    return AZMI_OK;
  }
  // a matrix-core family: every refusal and the size of the image before the device is touched
  const std::string why = r.tile->refusal(d);
  if (!why.empty()) return nfail(AZMI_ERR_INVALID, "%s", why.c_str());
  const size_t want = r.tile->blob_bytes(d);
  if (blob_bytes != want) return nfail(AZMI_ERR_INVALID, "weight blob is %zu bytes, expected %zu", blob_bytes, want);
  azmi_net* net = nullptr;
  int rc = upload(blob, blob_bytes, device, &net);
  if (rc != AZMI_OK) return rc;
  rc = r.tile->make(d, net);
  if (rc != AZMI_OK) { release(net); return rc; }
  *out = net;
  return AZMI_OK;
}

}  // namespace

extern "C" {

const char* azmi_net_last_error(void) { return g_net_err.c_str(); }

size_t azmi_net_blob_bytes(const azmi_net_desc* d) {      // answers without validating
  if (!d) return 0;
  if (d->precision == 1) return azmi_f32::blob_bytes(d, false);
  return resnet_tile(d).blob_bytes(d);
}

int azmi_net_create(const azmi_net_desc* d, const void* blob, size_t blob_bytes, int device, azmi_net** out) {
  if (!d || !blob || !out) return nfail(AZMI_ERR_INVALID, "null argument");
  return create(resolve(d), d, blob, blob_bytes, device, out);
}

size_t azmi_net_blob_bytes2(const azmi_net_desc2* d2) {
  if (!d2) return 0;
  // 0 exactly where azmi_net_create2 refuses - but for a dense_net word outside 0 / 1 on a descriptor without variant words,
  // which this entry has always sized as a dense net (tests/golden/leafnet_descriptor_table.json pins it)
  azmi_net_desc2 s = *d2;
  if (s.dense_net != 0 && !is_variant(&s)) s.dense_net = 1;
  const Resolved r = resolve2(&s);
  const azmi_net_desc* d = &s.base;
  if (r.to == Resolved::FIRST) return azmi_net_blob_bytes(d);
  if (r.to == Resolved::FP32) return azmi_f32::blob_bytes(d, r.f32_dense, r.var);
  if (r.to == Resolved::TILE) return r.tile->refusal(d).empty() ? r.tile->blob_bytes(d) : 0;
  return 0;
}

int azmi_net_create2(const azmi_net_desc2* d2, const void* blob, size_t blob_bytes, int device, azmi_net** out) {
  if (!d2 || !blob || !out) return nfail(AZMI_ERR_INVALID, "null argument");
  const Resolved r = resolve2(d2);
  if (r.to == Resolved::FIRST) return azmi_net_create(&d2->base, blob, blob_bytes, device, out);
  return create(r, &d2->base, blob, blob_bytes, device, out);
}

void azmi_net_destroy(azmi_net* net) {
  if (net) release(net);
}

int azmi_net_reserve_stream(azmi_net* net, void* stream, uint32_t max_rows) {
  if (!net) return nfail(AZMI_ERR_INVALID, "null argument");
  return net->family->reserve_stream(stream, max_rows);
}

int azmi_net_forward(azmi_net* net, const float* dev_canonical, float* dev_v, float* dev_pi, uint32_t batch, void* stream) {
  if (!net || !dev_canonical || !dev_v || !dev_pi) return nfail(AZMI_ERR_INVALID, "null argument");
  if (batch == 0) return AZMI_OK;
  return net->family->forward(dev_canonical, dev_v, dev_pi, batch, nullptr, nullptr, stream);
}

int azmi_net_trunk_channels(azmi_net* net, uint32_t* cf) {
  if (!net || !cf) return nfail(AZMI_ERR_INVALID, "null argument");
  return net->family->trunk_channels(cf);
}
int azmi_net_trunk_features(azmi_net* net, const float* dev_canonical, float* dev_features, uint32_t batch, void* stream) {
  if (!net) return nfail(AZMI_ERR_INVALID, "null argument");
  return net->family->trunk_features(dev_canonical, dev_features, batch, stream);
}

int azmi_net_forward_rows(azmi_net* net, const float* dev_canonical, float* dev_v, float* dev_pi, const uint32_t* dev_rows,
                          const uint32_t* dev_row_count, uint32_t max_rows, void* stream) {
  if (!net || !dev_canonical || !dev_v || !dev_pi || !dev_rows || !dev_row_count) return nfail(AZMI_ERR_INVALID, "null argument");
  if (max_rows == 0) return AZMI_OK;
  // Rows that are not listed are NOT touched (another model group's answers, cache hits already delivered: ADVICE r1,
  // play_manager.cc:577-597).  The MFMA kernels read and write through the list themselves; workgroups past the count exit.
  if (net->family->takes_rows()) return net->family->forward(dev_canonical, dev_v, dev_pi, max_rows, dev_rows, dev_row_count, stream);
  // a family of dense batches (the fp32 kernels): gather the listed rows, evaluate, scatter the answers back
  uint32_t chw, p1, m;
  net->family->dims(&chw, &p1, &m);
  hipStream_t st = static_cast<hipStream_t>(stream);
  azmi_net::StreamScratch& sc = net->scratch_of(stream);
  if (max_rows > sc.g_rows) {      // first use of this stream / a larger engine only (synchronous, outside the steady state)
    (void)hipSetDevice(net->device);
    (void)hipDeviceSynchronize();
    if (sc.g_canon) (void)hipFree(sc.g_canon);
    if (sc.g_v) (void)hipFree(sc.g_v);
    if (sc.g_pi) (void)hipFree(sc.g_pi);
    sc.g_canon = sc.g_v = sc.g_pi = nullptr; sc.g_rows = 0;
    if (hipMalloc(reinterpret_cast<void**>(&sc.g_canon), static_cast<size_t>(max_rows) * chw * 4) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&sc.g_v), static_cast<size_t>(max_rows) * p1 * 4) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&sc.g_pi), static_cast<size_t>(max_rows) * m * 4) != hipSuccess)
      return nfail(AZMI_ERR_OOM, "hipMalloc(row-list staging) failed");
    sc.g_rows = max_rows;
  }
  k_gather_rows<<<max_rows, 256, 0, st>>>(dev_canonical, dev_rows, dev_row_count, max_rows, chw, sc.g_canon);
  const int rc = net->family->forward(sc.g_canon, sc.g_v, sc.g_pi, max_rows, nullptr, nullptr, stream);
  if (rc != AZMI_OK) return rc;
  k_scatter_rows<<<max_rows, 64, 0, st>>>(sc.g_v, sc.g_pi, dev_rows, dev_row_count, p1, m, dev_v, dev_pi);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return nfail(AZMI_ERR_NO_DEVICE, "row-list gather/scatter launch: %s", hipGetErrorString(e));
  return AZMI_OK;
}

namespace {
struct HostEvalCtx {          // per calling thread: its own stream and staging buffers
  int device = -1;
  hipStream_t st = nullptr;
  float *c = nullptr, *v = nullptr, *pi = nullptr;
  uint32_t rows = 0, chw = 0, p1 = 0, m = 0;
  ~HostEvalCtx() {
    if (device < 0) return;
    (void)hipSetDevice(device);
    if (c) (void)hipFree(c); if (v) (void)hipFree(v); if (pi) (void)hipFree(pi);
    if (st) (void)hipStreamDestroy(st);
  }
};
}  // namespace

void azmi_net_eval_host(const float* canonical, uint32_t n, float* v, float* pi, void* net_v) {
  azmi_net* net = static_cast<azmi_net*>(net_v);
  if (!net || !canonical || !v || !pi || n == 0) return;
  uint32_t chw, p1, m;
  net->family->dims(&chw, &p1, &m);
  auto poison = [&]() {
    for (size_t i = 0; i < static_cast<size_t>(n) * p1; ++i) v[i] = __builtin_nanf("");
    for (size_t i = 0; i < static_cast<size_t>(n) * m; ++i) pi[i] = __builtin_nanf("");
  };
  thread_local HostEvalCtx ctx;
  if (hipSetDevice(net->device) != hipSuccess) { poison(); return; }
  if (ctx.device != net->device || ctx.rows < n || ctx.chw != chw || ctx.p1 != p1 || ctx.m != m) {
    if (ctx.c) (void)hipFree(ctx.c); if (ctx.v) (void)hipFree(ctx.v); if (ctx.pi) (void)hipFree(ctx.pi);
    ctx.c = ctx.v = ctx.pi = nullptr;
    if (!ctx.st && hipStreamCreateWithFlags(&ctx.st, hipStreamNonBlocking) != hipSuccess) { poison(); return; }
    const uint32_t rows = n < 256 ? 256 : n;
    if (hipMalloc(reinterpret_cast<void**>(&ctx.c), static_cast<size_t>(rows) * chw * 4) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&ctx.v), static_cast<size_t>(rows) * p1 * 4) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&ctx.pi), static_cast<size_t>(rows) * m * 4) != hipSuccess) { poison(); return; }
    ctx.device = net->device; ctx.rows = rows; ctx.chw = chw; ctx.p1 = p1; ctx.m = m;
  }
  bool ok = hipMemcpyAsync(ctx.c, canonical, static_cast<size_t>(n) * chw * 4, hipMemcpyHostToDevice, ctx.st) == hipSuccess;
  ok = ok && azmi_net_forward(net, ctx.c, ctx.v, ctx.pi, n, ctx.st) == AZMI_OK;
  ok = ok && hipMemcpyAsync(v, ctx.v, static_cast<size_t>(n) * p1 * 4, hipMemcpyDeviceToHost, ctx.st) == hipSuccess;
  ok = ok && hipMemcpyAsync(pi, ctx.pi, static_cast<size_t>(n) * m * 4, hipMemcpyDeviceToHost, ctx.st) == hipSuccess;
  ok = ok && hipStreamSynchronize(ctx.st) == hipSuccess;
  if (!ok) poison();
}

int azmi_net_blob_read(azmi_net* net, void* host_out, size_t bytes) {
  if (!net || !host_out) return nfail(AZMI_ERR_INVALID, "null argument");
  if (!net->blob) return nfail(AZMI_ERR_INVALID, "azmi_net_blob_read: the fp32 tier keeps its weight image to itself");
  if (bytes != net->blob_bytes) return nfail(AZMI_ERR_INVALID, "azmi_net_blob_read: %zu bytes asked for, the weight image has %zu", bytes, net->blob_bytes);
  if (hipSetDevice(net->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
      hipMemcpy(host_out, net->blob, bytes, hipMemcpyDeviceToHost) != hipSuccess)
    return nfail(AZMI_ERR_NO_DEVICE, "azmi_net_blob_read: reading the weight image back failed");
  return AZMI_OK;
}

int azmi_net_c4_view_get(const azmi_net* net, azmi_net_c4_view* out) {
  if (!net || !out) return 0;
  return net->family->c4_view(out);
}

}  // extern "C"
