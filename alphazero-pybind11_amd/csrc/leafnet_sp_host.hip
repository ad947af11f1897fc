// Host side of the spatial-policy-head leaf nets (leafnet_sp.h: Tafl family 7x7 / 11x11, StarGambit 13x13; bf16 and bf16x3
// tiers): their bounds, their weight image (alphazero/hip_net.py fold_spatial), the six tile instances, the per-stream scratch
// between the tile and the heads' FC kernels, and the launches.  The one unit that includes leafnet_sp.h: k_heads_fc, k_heads_fc_a
// and k_heads_fc_b are no templates and are defined here alone.
#include "leafnet_sp.h"
#include "leafnet_host.h"

namespace {

using namespace azmi_net_dev;
using namespace azmi_net_host;

using SpKernel = void (*)(sp::SpDesc, sp::SpPtrs, const float*, float*, float*, float*, uint32_t, const uint32_t*, const uint32_t*);
struct SpInstance {
  int board;      // edge of the square board
  bool x3;        // the bf16x3 tier: Geo<.., SPLIT>, 16 activation planes, one workgroup per CU
  SpKernel kernel;
  int tbw;        // boards per workgroup
  size_t lds;
};
template <class G>
SpInstance instance() { return SpInstance{G::H, G::SPLIT != 0, &sp::k_leafnet_sp<G>, G::TBW, static_cast<size_t>(G::LDS_BYTES)}; }
const SpInstance kInstances[] = {instance<sp::Geo7>(),   instance<sp::Geo11>(),   instance<sp::Geo13>(),
                                 instance<sp::Geo7X3>(), instance<sp::Geo11X3>(), instance<sp::Geo13X3>()};
const SpInstance* instance_of(const azmi_net_desc* d) {
  for (const SpInstance& i : kInstances)
    if (d->height == i.board && d->width == i.board && (d->precision == 2) == i.x3) return &i;
  return nullptr;
}

int num_global(const azmi_net_desc* d) { return d->num_moves - d->policy_channels * d->height * d->width; }

std::string refusal(const azmi_net_desc* d) {
  if (d->channels != CH || d->head_channels != sp::HCS || d->kernel_size != 3 || d->v_head_convs != 1 || d->pi_head_convs != 1)
    return "spatial leaf net kernel covers 64 trunk / 64 head channels, 3x3 convs, one extra conv per head";
  const SpInstance* inst = instance_of(d);
  if (!inst) return textf("spatial leaf net kernel: board %dx%d not instantiated", d->height, d->width);
  if (d->policy_channels > 32 || num_global(d) < 0 || num_global(d) > 32) return "spatial head: policy channels <= 32, 0..32 global actions";
  if (num_global(d) > 0 && (d->pi_hidden < 64 || d->pi_hidden > 1024 || d->pi_hidden % 64))
    return "spatial head with global actions: pi_hidden must be a multiple of 64 in [64, 1024]";
  if (d->in_channels < 1 || d->in_channels > 64) return textf("spatial leaf net kernel: %d input planes not supported", d->in_channels);
  if (d->depth < 1 || d->depth > sp::MAXDEPTH) return textf("spatial leaf net kernel: 1..%d residual blocks", sp::MAXDEPTH);
  if (static_cast<size_t>(inst->tbw) * d->num_moves * 4 > sp::RING_BYTES) return "spatial head: logits do not fit the tile's LDS";
  if (d->v_hidden < 128 || d->v_hidden > 512 || d->v_hidden % 128 || d->v_fc_layers < 1 || d->num_players < 1 || d->num_players + 1 > 16)
    return "value head sizes out of range";
  return std::string();
}

// the chunk stream (bf16x3: every chunk three times) | the fp32 parameters of the tower and the heads | the value FC stack |
// pi_global: W1^T[64][Hp] b[Hp] W2^T[Hp][32] b[32] ln_g[32] ln_b[32]
sp::SpPtrs layout(const azmi_net_desc* d, BlobCursor& c) {
  const size_t Hd = d->v_hidden, L = d->v_fc_layers;
  sp::SpPtrs p{};
  p.stream = c.bytes(static_cast<size_t>(sp::stream_chunks(d->depth, d->in_channels, d->precision == 2)) * sp::CHUNK_BYTES);
  p.prm = c.f32(CH + static_cast<size_t>(d->depth) * 3 * CH + 2 * sp::HCS + sp::HCS + sp::HCS + 32);
  p.fc1_w = c.f32(64 * Hd); p.fc1_b = c.f32(Hd);
  p.fcx_w = c.f32((L - 1) * Hd * Hd); p.fcx_b = c.f32((L - 1) * Hd);
  p.fc2_w = c.f32(Hd * 16); p.fc2_b = c.f32(16);
  if (num_global(d) > 0) {
    const size_t Hp = d->pi_hidden;
    p.pg1_w = c.f32(64 * Hp); p.pg1_b = c.f32(Hp); p.pg2_w = c.f32(Hp * 32); p.pg2_b = c.f32(32); p.pg_ln_g = c.f32(32); p.pg_ln_b = c.f32(32);
  }
  return p;
}
size_t blob_bytes(const azmi_net_desc* d) {
  BlobCursor c;
  layout(d, c);
  return c.off;
}

struct SpFamily : Family {
  azmi_net* net = nullptr;      // the per-stream scratch lives with the net
  sp::SpDesc sd{};
  sp::SpPtrs sp{};
  const SpInstance* inst = nullptr;
  size_t fc_lds = 0;         // dynamic LDS of k_heads_fc
  bool fc_split = false;     // the heads' FC step as k_heads_fc_a + _b (big FC stacks) instead of the one k_heads_fc

  int reserve_stream(void* stream, uint32_t batch) override {
    azmi_net::StreamScratch& sc = net->scratch_of(stream);
    const uint32_t Hd = static_cast<uint32_t>(sd.v_hidden);
    if (batch <= sc.pool_rows && sc.pool_hidden == Hd) return AZMI_OK;
    // first use of this stream / a larger batch only (synchronous, outside the steady state and outside stream capture)
    (void)hipSetDevice(net->device);
    if (sc.pool) { (void)hipDeviceSynchronize(); (void)hipFree(sc.pool); sc.pool = nullptr; sc.pool_rows = 0; }
    const uint32_t want = ((batch < 4096u ? 4096u : batch) + 15u) / 16u * 16u;
    if (hipMalloc(reinterpret_cast<void**>(&sc.pool), static_cast<size_t>(want) * (2 * 64 + 32 + Hd) * sizeof(float)) != hipSuccess)
      return nfail(AZMI_ERR_OOM, "hipMalloc(head scratch) failed");
    sc.pool_rows = want; sc.pool_hidden = Hd;
    return AZMI_OK;
  }
  // the tiles (tower, both heads up to their pooled features / spatial logits), then the heads' FC parts batched (two small launches)
  int forward(const float* canon, float* v, float* pi, uint32_t batch, const uint32_t* rows, const uint32_t* row_count, void* stream) override {
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int rrc = reserve_stream(stream, batch);
    if (rrc != AZMI_OK) return rrc;
    azmi_net::StreamScratch& sc = net->scratch_of(stream);
    float* vpool = sc.pool;
    float* ppool = sc.pool + static_cast<size_t>(sc.pool_rows) * 64;
    float* glob = sc.pool + static_cast<size_t>(sc.pool_rows) * 128;
    float* hidden = sc.pool + static_cast<size_t>(sc.pool_rows) * 160;
    const uint32_t tiles = (batch + inst->tbw - 1) / inst->tbw;
    inst->kernel<<<tiles, sp::NTH, inst->lds, st>>>(sd, sp, canon, vpool, ppool, pi, batch, rows, row_count);
    const uint32_t groups = (batch + 15) / 16;
    const uint32_t parts = static_cast<uint32_t>(sd.v_hidden / sp::HFC_SLICE) + (sd.num_global > 0 ? 1u : 0u);
    if (fc_split) {
      const int hmax = sd.v_hidden > sd.pi_hidden || sd.num_global == 0 ? sd.v_hidden : sd.pi_hidden;
      sp::k_heads_fc_a<<<groups * parts, sp::HFC_THREADS, sp::heads_fc_a_lds(hmax, sd.v_fc_layers), st>>>(sd, sp, vpool, ppool, hidden, glob, batch, row_count);
      sp::k_heads_fc_b<<<groups, sp::HFC_THREADS, sp::heads_fc_b_lds(sd.v_hidden), st>>>(sd, sp, hidden, glob, v, pi, batch, rows, row_count);
    } else {
      sp::k_heads_fc<<<groups, sp::HFC_THREADS, fc_lds, st>>>(sd, sp, vpool, ppool, v, pi, batch, rows, row_count);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return nfail(AZMI_ERR_NO_DEVICE, "k_leafnet_sp launch: %s", hipGetErrorString(e));
    return AZMI_OK;
  }
  void dims(uint32_t* chw, uint32_t* p1, uint32_t* m) const override { *chw = sd.C_in * sd.H * sd.W; *p1 = sd.num_players + 1; *m = sd.num_moves; }
};

int make(const azmi_net_desc* d, azmi_net* net) {
  auto f = new SpFamily();
  net->family = f;
  f->net = net;
  const int ng = num_global(d);
  f->sd = sp::SpDesc{d->in_channels, d->height, d->width, d->depth, d->num_moves, d->num_players, d->v_hidden, d->v_fc_layers, d->policy_channels,
                     ng, ng > 0 ? d->pi_hidden : 0};
  BlobCursor c{static_cast<const uint8_t*>(net->blob)};
  f->sp = layout(d, c);
  f->inst = instance_of(d);
  f->fc_split = d->v_hidden > 256 || ng > 0;   // more than ~0.4 MB of FC weights per group
  f->fc_lds = sp::heads_fc_lds(d->v_hidden > d->pi_hidden || ng == 0 ? d->v_hidden : d->pi_hidden);
  // The FC kernels are shared by every spatial net of the process: the attribute is set to the most any descriptor this
  // library accepts can ask for (v_hidden / pi_hidden <= 1024), never to this net's own need - a later, smaller net must
  // not lower it under an earlier, larger one
  const int fc_max = static_cast<int>(sp::heads_fc_lds(1024));
  if (f->fc_lds > static_cast<size_t>(fc_max)) return nfail(AZMI_ERR_INVALID, "v_hidden / pi_hidden above 1024");
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(f->inst->kernel), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(f->inst->lds)) != hipSuccess ||
      hipFuncSetAttribute(reinterpret_cast<const void*>(&sp::k_heads_fc), hipFuncAttributeMaxDynamicSharedMemorySize, fc_max) != hipSuccess ||
      hipFuncSetAttribute(reinterpret_cast<const void*>(&sp::k_heads_fc_a), hipFuncAttributeMaxDynamicSharedMemorySize, fc_max) != hipSuccess ||
      hipFuncSetAttribute(reinterpret_cast<const void*>(&sp::k_heads_fc_b), hipFuncAttributeMaxDynamicSharedMemorySize, fc_max) != hipSuccess)
    return nfail(AZMI_ERR_NO_DEVICE, "cannot reserve LDS for the spatial leaf net");
  return AZMI_OK;
}

}  // namespace

namespace azmi_net_host {
const FamilyDef& spatial_family() {
  static const FamilyDef f = {refusal, blob_bytes, make};
  return f;
}
}
