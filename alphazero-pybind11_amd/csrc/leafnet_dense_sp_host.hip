// Host side of the dense spatial-head family (leafnet_dense_sp.h: DenseNet trunk on 7x7 / 11x11 / 13x13, 3x3 / 5x5, the
// single-variant StarGambit configs): its bounds, its weight image (alphazero/hip_net.py fold_dense_spatial) and its six
// instances (board x kernel size).
#include "leafnet_dense_sp.h"
#include "leafnet_host.h"

namespace {

using namespace azmi_net_dev;
using namespace azmi_net_host;

using DspKernel = void (*)(dsp::DspDesc, dsp::DspPtrs, const float*, float*, float*, uint32_t, const uint32_t*, const uint32_t*);
struct DspInstance {
  int board, k;      // board edge (7 / 11 / 13) and kernel size (3 / 5)
  DspKernel kernel;
  size_t (*lds)(int cfp);
};
template <class GEO, int K>
DspInstance instance() { return DspInstance{GEO::B, K, &dsp::k_leafnet_dense_sp<GEO, K>, &GEO::lds_bytes}; }
const DspInstance kInstances[] = {instance<dsp::Geo7, 3>(),  instance<dsp::Geo7, 5>(),  instance<dsp::Geo11, 3>(),
                                  instance<dsp::Geo11, 5>(), instance<dsp::Geo13, 3>(), instance<dsp::Geo13, 5>()};
const DspInstance* instance_of(const azmi_net_desc* d) {
  for (const DspInstance& i : kInstances)
    if (d->height == i.board && d->width == i.board && d->kernel_size == i.k) return &i;
  return nullptr;
}

int num_global(const azmi_net_desc* d) { return d->num_moves - d->policy_channels * d->height * d->width; }
// the trunk is the dense Connect4 tile's (block_bytes)
dn::DnDesc trunk_desc(const azmi_net_desc* d) {
  const int cf = d->in_channels + d->channels * d->depth;
  return dn::DnDesc{d->in_channels, d->channels, d->depth, d->kernel_size, cf, dn::round_up(cf, 32), d->num_moves, d->num_players, d->v_hidden};
}
dsp::DspDesc dense_sp_desc(const azmi_net_desc* d) {
  const int cf = d->in_channels + d->channels * d->depth, ng = num_global(d);
  return dsp::DspDesc{d->in_channels, d->channels, d->depth, cf, dn::round_up(cf, 32), d->num_moves, d->num_players, d->v_hidden,
                      d->policy_channels, ng, ng > 0 ? d->pi_hidden : 0};
}

// The bounds of the dense spatial tile (leafnet_dense_sp.h), stated once
std::string refusal(const azmi_net_desc* d) {
  const bool board = d->height == d->width && (d->height == 7 || d->height == 11 || d->height == 13);
  if (!board) return "dense spatial leaf net kernel covers 7x7, 11x11 and 13x13 boards; use precision='fp32' for other shapes";
  if (d->kernel_size != 3 && d->kernel_size != 5) return "dense spatial leaf net kernel: kernel_size 3 or 5; use precision='fp32' for other shapes";
  if (d->channels < 1 || d->channels > dn::MAX_G) return "dense spatial leaf net kernel: growth rate (channels) 1..16; use precision='fp32' for other shapes";
  if (d->depth < 1 || d->in_channels < 1) return "dense spatial leaf net kernel: at least one block and one input plane; use precision='fp32' for other shapes";
  if (static_cast<long long>(d->in_channels) + static_cast<long long>(d->channels) * d->depth > dn::MAX_CF)
    return "dense spatial leaf net kernel: in_channels + channels * depth <= 128; use precision='fp32' for other shapes";
  if (d->head_channels != dsp::HC1 || d->v_head_convs != 0 || d->pi_head_convs != 0 || d->v_fc_layers != 1)
    return "dense spatial leaf net kernel: 32 head channels, no extra head convolutions, one value FC layer; use precision='fp32' for other shapes";
  if (d->policy_channels < 1 || d->policy_channels > dsp::MAX_PC || num_global(d) < 0 || num_global(d) > dsp::MAX_NG)
    return "dense spatial leaf net kernel: policy channels 1..32, 0..32 global actions; use precision='fp32' for other shapes";
  if (num_global(d) > 0 && (d->pi_hidden < 16 || d->pi_hidden > dsp::MAX_HID || d->pi_hidden % 16))
    return "dense spatial leaf net kernel: pi_hidden must be a multiple of 16 in 16..256 with global actions; use precision='fp32' for other shapes";
  if (d->v_hidden < 16 || d->v_hidden > dsp::MAX_HID || d->v_hidden % 16 || d->num_players < 1 || d->num_players > 3)
    return "dense spatial leaf net kernel: head sizes out of range (v_hidden: a multiple of 16, at most 256; 1..3 players); use precision='fp32' for other shapes";
  return std::string();
}

// the blocks | head bias, head 1x1 fragments (high and low parts) | value FC | policy 1x1 (padded to MAX_PC) | pi_global
dsp::DspPtrs layout(const azmi_net_desc* d, BlobCursor& c) {
  const dn::DnDesc dd = trunk_desc(d);
  const size_t Hd = d->v_hidden, P1 = d->num_players + 1, ng = num_global(d), Hp = d->pi_hidden;
  dsp::DspPtrs p{};
  p.blocks = c.bytes(0);
  for (int i = 0; i < dd.depth; ++i) c.bytes(dn::block_bytes(dd, i));
  p.head_b = c.f32(dsp::HEADCH);
  p.head_w = c.bytes(2 * static_cast<size_t>(dd.CFP / 32) * 4 * WFRAG_BYTES);
  p.v_fc1_w = c.f32(Hd * dsp::HC1); p.v_fc1_b = c.f32(Hd);
  p.v_fc2_w = c.f32(P1 * Hd); p.v_fc2_b = c.f32(P1);
  p.pol_w = c.f32(static_cast<size_t>(dsp::MAX_PC) * dsp::HC1); p.pol_b = c.f32(dsp::MAX_PC);
  if (num_global(d) > 0) {
    p.pg1_w = c.f32(Hp * dsp::HC1); p.pg1_b = c.f32(Hp);
    p.pg2_w = c.f32(ng * Hp); p.pg2_b = c.f32(ng);
    p.pg_ln_g = c.f32(ng); p.pg_ln_b = c.f32(ng);
  }
  return p;
}
size_t blob_bytes(const azmi_net_desc* d) {
  BlobCursor c;
  layout(d, c);
  return c.off;
}

struct DenseSpFamily : Family {
  dsp::DspDesc xd{};
  dsp::DspPtrs xp{};
  int board = 0;
  DspKernel kernel = nullptr;
  size_t lds = 0;

  int forward(const float* canon, float* v, float* pi, uint32_t rows_max, const uint32_t* rows, const uint32_t* row_count, void* stream) override {
    const uint32_t tiles = (rows_max + dsp::TBW - 1) / dsp::TBW;
    kernel<<<tiles, dsp::NTH, lds, static_cast<hipStream_t>(stream)>>>(xd, xp, canon, v, pi, rows_max, rows, row_count);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return nfail(AZMI_ERR_NO_DEVICE, "k_leafnet_dense_sp launch: %s", hipGetErrorString(e));
    return AZMI_OK;
  }
  void dims(uint32_t* chw, uint32_t* p1, uint32_t* m) const override { *chw = xd.C_in * board * board; *p1 = xd.num_players + 1; *m = xd.num_moves; }
};

int make(const azmi_net_desc* d, azmi_net* net) {
  auto f = new DenseSpFamily();
  net->family = f;
  f->xd = dense_sp_desc(d);
  BlobCursor c{static_cast<const uint8_t*>(net->blob)};
  f->xp = layout(d, c);
  const DspInstance* inst = instance_of(d);
  f->board = inst->board;
  f->kernel = inst->kernel;
  f->lds = inst->lds(f->xd.CFP);
  // an instance is shared by every net of its board and kernel size: the attribute is what the widest accepted net asks for
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(f->kernel), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(inst->lds(dn::MAX_CF))) != hipSuccess)
    return nfail(AZMI_ERR_NO_DEVICE, "cannot reserve %zu bytes of LDS", f->lds);
  return AZMI_OK;
}

}  // namespace

namespace azmi_net_host {
const FamilyDef& dense_sp_family() {
  static const FamilyDef f = {refusal, blob_bytes, make};
  return f;
}
}
