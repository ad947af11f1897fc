// Host side of the dense Connect4 family (leafnet_dense.h: DenseNet trunk, 6x7 board, 3x3 / 5x5, flat policy head): its bounds,
// its weight image (alphazero/hip_net.py fold_dense) and the two instances - trunk_norm batch and layer - as two family records.
#include "leafnet_dense.h"
#include "leafnet_host.h"

namespace {

using namespace azmi_net_dev;
using namespace azmi_net_host;

using DnKernel = void (*)(dn::DnDesc, dn::DnPtrs, const float*, float*, float*, uint32_t, const uint32_t*, const uint32_t*);

dn::DnDesc dense_desc(const azmi_net_desc* d) {
  const int cf = d->in_channels + d->channels * d->depth;
  return dn::DnDesc{d->in_channels, d->channels, d->depth, d->kernel_size, cf, dn::round_up(cf, 32), d->num_moves, d->num_players, d->v_hidden};
}

// The bounds of the dense tile (leafnet_dense.h), stated once
std::string refusal(const azmi_net_desc* d) {
  if (d->policy_channels != 0 || d->height != dn::BH || d->width != dn::BW)
    return "dense leaf net kernel covers the 6x7 board with the flat policy head; use precision='fp32' for other shapes";
  if (d->kernel_size != 3 && d->kernel_size != 5) return "dense leaf net kernel: kernel_size 3 or 5; use precision='fp32' for other shapes";
  if (d->channels < 1 || d->channels > dn::MAX_G) return "dense leaf net kernel: growth rate (channels) 1..16; use precision='fp32' for other shapes";
  if (d->depth < 1 || d->in_channels < 1) return "dense leaf net kernel: at least one block and one input plane; use precision='fp32' for other shapes";
  if (static_cast<long long>(d->in_channels) + static_cast<long long>(d->channels) * d->depth > dn::MAX_CF)
    return "dense leaf net kernel: in_channels + channels * depth <= 128; use precision='fp32' for other shapes";
  if (d->head_channels != dn::HC1 || d->v_head_convs != 0 || d->pi_head_convs != 0 || d->v_fc_layers != 1)
    return "dense leaf net kernel: 32 head channels, no extra head convolutions, one value FC layer; use precision='fp32' for other shapes";
  if (d->v_hidden < 16 || d->v_hidden > 256 || d->v_hidden % 16 || d->num_players < 1 || d->num_players > 3 || d->num_moves < 1 || d->num_moves > 16)
    return "dense leaf net kernel: head sizes out of range (v_hidden: a multiple of 16, at most 256; 1..3 players; 1..16 moves); use precision='fp32' for other shapes";
  return std::string();
}

// the blocks (the layer instance: with their GroupNorm parameters) | head bias, head 1x1 fragments | value FC | policy FC
template <bool LAYER>
dn::DnPtrs layout(const azmi_net_desc* d, BlobCursor& c) {
  const dn::DnDesc dd = dense_desc(d);
  dn::DnPtrs p{};
  p.blocks = c.bytes(0);
  for (int i = 0; i < dd.depth; ++i) c.bytes(dn::block_bytes(dd, i, LAYER));
  p.head_b = c.f32(dn::HEADCH);
  p.head_w = c.bytes(static_cast<size_t>(dd.CFP / 32) * 4 * WFRAG_BYTES);
  p.v_fc1_w = c.f32(static_cast<size_t>(dd.v_hidden) * dn::HC1); p.v_fc1_b = c.f32(dd.v_hidden);
  p.v_fc2_w = c.f32(static_cast<size_t>(dd.num_players + 1) * dd.v_hidden); p.v_fc2_b = c.f32(dd.num_players + 1);
  p.pi_fc_w = c.f32(static_cast<size_t>(dd.num_moves) * dn::HC1 * dn::PIX); p.pi_fc_b = c.f32(dd.num_moves);
  return p;
}
template <bool LAYER>
size_t blob_bytes(const azmi_net_desc* d) {
  BlobCursor c;
  layout<LAYER>(d, c);
  return c.off;
}

struct DenseFamily : Family {
  dn::DnDesc dd{};
  dn::DnPtrs dp{};
  DnKernel kernel = nullptr;
  size_t lds = 0;

  int forward(const float* canon, float* v, float* pi, uint32_t rows_max, const uint32_t* rows, const uint32_t* row_count, void* stream) override {
    const uint32_t tiles = (rows_max + dn::TBW - 1) / dn::TBW;
    kernel<<<tiles, dn::NTH, lds, static_cast<hipStream_t>(stream)>>>(dd, dp, canon, v, pi, rows_max, rows, row_count);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return nfail(AZMI_ERR_NO_DEVICE, "k_leafnet_dense launch: %s", hipGetErrorString(e));
    return AZMI_OK;
  }
  void dims(uint32_t* chw, uint32_t* p1, uint32_t* m) const override { *chw = dd.C_in * dn::PIX; *p1 = dd.num_players + 1; *m = dd.num_moves; }
  // layout<false>() again, as what each section is made FROM (alphazero/hip_net.py fold_dense; the table order is
  // hip_net.refresh_names).  The layer-norm instance folds nothing and has no plan
  bool layer = false;
  bool refresh_plan(azmi_refresh::Plan* plan) const override {
    using namespace azmi_refresh;
    if (layer) return false;
    PlanBuilder b{*plan};
    const uint32_t g = dd.G, kk = dd.K * dd.K, cf = dd.CF, cfp = dd.CFP, hd = dd.v_hidden, p1 = dd.num_players + 1, m = dd.num_moves;
    const uint32_t m1 = dn::round_up(4 * dd.G, 16), k2 = dn::round_up(4 * dd.G, 32);
    for (int i = 0; i < dd.depth; ++i) {
      const std::string pre = "conv_layers." + std::to_string(i) + ".";
      const uint32_t ci = dd.C_in + dd.G * i, cip = dn::round_up(dd.C_in + dd.G * i, 32);
      const uint32_t n1 = b.bn(pre + "bn1", ci);
      const uint32_t w1 = b.param(pre + "conv1.weight", 4 * g * ci, AZMI_PARAM_CONV_W);
      const uint32_t n2 = b.bn(pre + "bn2", 4 * g);
      const uint32_t w2 = b.param(pre + "conv2.weight", g * 4 * g * kk, AZMI_PARAM_CONV_W);
      b.f32(F32_BN_A, n1, cfp, ci); b.f32(F32_BN_B, n1, cfp, ci); b.f32(F32_BN_B, n2, 64, 4 * g);
      b.frag(frag_of(w1, n2, 4 * g, m1 / 16, cip / 32, cip, 0, ci, 1), 1);      // rows = bn2-scaled conv1, k = input channel
      b.frag(frag_of(w2, NO_BN, g, 1, k2 / 32, k2, 1, 4 * g, kk), kk);           // per tap: rows = the G outputs, k = bottleneck channel
    }
    const uint32_t vc = b.param("v_conv.weight", dn::HC1 * cf, AZMI_PARAM_CONV_W);
    const uint32_t vb = b.bn("v_bn", dn::HC1);
    const uint32_t pc = b.param("pi_conv.weight", dn::HC1 * cf, AZMI_PARAM_CONV_W);
    const uint32_t pb = b.bn("pi_bn", dn::HC1);
    b.f32(F32_BN_B, vb, dn::HC1, dn::HC1); b.f32(F32_BN_B, pb, dn::HC1, dn::HC1);
    b.frag(head_frag(vc, vb, pc, pb, cfp / 32, cf), 1);
    b.f32(F32_COPY, b.param("v_fc1.weight", hd * dn::HC1, AZMI_PARAM_FC_W), hd * dn::HC1, hd * dn::HC1);
    b.f32(F32_COPY, b.param("v_fc1.bias", hd, AZMI_PARAM_FC_B), hd, hd);
    b.f32(F32_COPY, b.param("v_fc2.weight", p1 * hd, AZMI_PARAM_FC_W), p1 * hd, p1 * hd);
    b.f32(F32_COPY, b.param("v_fc2.bias", p1, AZMI_PARAM_FC_B), p1, p1);
    b.f32(F32_COPY, b.param("pi_fc1.weight", m * dn::HC1 * dn::PIX, AZMI_PARAM_FC_W), m * dn::HC1 * dn::PIX, m * dn::HC1 * dn::PIX);
    b.f32(F32_COPY, b.param("pi_fc1.bias", m, AZMI_PARAM_FC_B), m, m);
    return true;
  }
};

template <bool LAYER>
int make(const azmi_net_desc* d, azmi_net* net) {
  auto f = new DenseFamily();
  net->family = f;
  f->dd = dense_desc(d);
  BlobCursor c{static_cast<const uint8_t*>(net->blob)};
  f->dp = layout<LAYER>(d, c);
  f->layer = LAYER;
  f->kernel = &dn::k_leafnet_dense<LAYER>;
  f->lds = dn::lds_bytes(f->dd);
  // the kernel is shared by every dense net of the process: the attribute is what the widest accepted net asks for
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(f->kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                          static_cast<int>(dn::TBW * dn::board_lds(dn::MAX_CF))) != hipSuccess)
    return nfail(AZMI_ERR_NO_DEVICE, "cannot reserve %zu bytes of LDS", f->lds);
  return AZMI_OK;
}

}  // namespace

namespace azmi_net_host {
const FamilyDef& dense_family() {
  static const FamilyDef f = {refusal, blob_bytes<false>, make<false>};
  return f;
}
const FamilyDef& dense_layer_family() {
  static const FamilyDef f = {refusal, blob_bytes<true>, make<true>};
  return f;
}
}  // namespace azmi_net_host
