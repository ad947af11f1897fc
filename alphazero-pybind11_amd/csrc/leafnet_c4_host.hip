// Host side of the Connect4-family leaf net (leafnet_c4.h: 6x7 board, flat policy head; bf16 and bf16x3 tiers): its bounds, its
// weight image (alphazero/hip_net.py fold), the four tiles and the launch behind azmi_net_forward*.  The engine's fused launch
// and the pipeline run the same tiles through azmi_net_c4_view.
#include "leafnet_c4.h"
#include "leafnet_host.h"

namespace {

using namespace azmi_net_dev;
using namespace azmi_net_host;

using C4Kernel = void (*)(NetDesc, NetPtrs, const float*, float*, float*, uint32_t, const uint32_t*, const uint32_t*);
struct C4Tile {
  C4Kernel kernel;
  uint32_t tbw;      // boards per workgroup
  size_t lds;
};
template <class T>
C4Tile tile_of() { return C4Tile{&c4::k_leafnet_c4<T, 4, 4, 16>, static_cast<uint32_t>(T::TBW), static_cast<size_t>(T::LDS_BYTES)}; }
// 6-board tiles when the batch fills the chip's 512 workgroup slots with them, 3-board tiles below that (a launch of a few
// hundred rows is a LATENCY: leafnet_c4.h, Tile).  bf16x3 runs one workgroup per CU (16 activation planes): 6-board tiles once
// the 3-board ones would need a second pass over the chip
struct C4Tier {
  C4Tile small, big;
  uint32_t big_from;      // rows_max from which the big tile is launched
};
const C4Tier kTiers[2] = {
    {tile_of<c4::TileSmall>(), tile_of<c4::TileBig>(), 512u * c4::TileBig::TBW},
    {tile_of<c4::TileSmallX3>(), tile_of<c4::TileBigX3>(), 256u * c4::TileSmallX3::TBW + 1u},
};

std::string refusal(const azmi_net_desc* d) {
  if (d->channels != CH || d->head_channels != HC || d->kernel_size != 3) return "leaf net kernel covers 64 trunk channels, 32 head channels, 3x3 convs";
  if (!(d->height == 6 && d->width == 7)) return textf("leaf net kernel: board %dx%d not instantiated", d->height, d->width);
  if (d->in_channels != 4) return textf("leaf net kernel: %d input planes not instantiated (Connect4 has 4)", d->in_channels);
  if (d->depth < 1 || d->depth > c4::MAXDEPTH) return textf("leaf net kernel: 1..%d residual blocks", c4::MAXDEPTH);
  if (d->v_hidden < 16 || d->v_hidden > 256 || d->v_hidden % 16 || d->num_players < 1 || d->num_players + 1 > 4 || d->num_moves < 1 || d->num_moves > 16)
    return "head sizes out of range (v_hidden: a multiple of 16, at most 256)";
  return std::string();
}

// precision 2 (bf16x3): the stem's fragments twice (high, low parts), three chunks per tap and for the head 1x1 (leafnet_c4.h, SPLIT)
NetPtrs layout(const azmi_net_desc* d, BlobCursor& c) {
  const bool x3 = d->precision == 2;
  const size_t wconv = (x3 ? 3 : 1) * 18 * MT * WFRAG_BYTES, wsmall = 2 * MT * WFRAG_BYTES;
  NetPtrs np{};
  np.stem_w = c.bytes((x3 ? 2 : 1) * wsmall);
  np.stem_b = c.f32(CH);
  np.blocks = c.bytes(static_cast<size_t>(d->depth) * (3 * CH * 4 + 2 * wconv));
  np.head_w = c.bytes((x3 ? 3 : 1) * wsmall);
  np.head_b = c.f32(CH);
  np.v_fc1_w = c.f32(static_cast<size_t>(d->v_hidden) * HC);
  np.v_fc1_b = c.f32(static_cast<size_t>(d->v_hidden));
  np.v_fc2_w = c.f32(static_cast<size_t>(d->num_players + 1) * d->v_hidden);
  np.v_fc2_b = c.f32(static_cast<size_t>(d->num_players + 1));
  np.pi_fc_w = c.bytes(static_cast<size_t>(d->height) * d->width * 2 * WFRAG_BYTES);      // policy FC: bf16 hi / lo fragments per pixel position
  np.pi_fc_b = c.f32(static_cast<size_t>(d->num_moves));
  return np;
}
size_t blob_bytes(const azmi_net_desc* d) {
  BlobCursor c;
  layout(d, c);
  return c.off;
}

struct C4Family : Family {
  NetDesc nd{};
  NetPtrs np{};
  const C4Tier* tier = nullptr;
  bool x3 = false;

  int forward(const float* canon, float* v, float* pi, uint32_t rows_max, const uint32_t* rows, const uint32_t* row_count, void* stream) override {
    const C4Tile& t = rows_max >= tier->big_from ? tier->big : tier->small;
    t.kernel<<<(rows_max + t.tbw - 1) / t.tbw, c4::NTH, t.lds, static_cast<hipStream_t>(stream)>>>(nd, np, canon, v, pi, rows_max, rows, row_count);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return nfail(AZMI_ERR_NO_DEVICE, "k_leafnet launch: %s", hipGetErrorString(e));
    return AZMI_OK;
  }
  void dims(uint32_t* chw, uint32_t* p1, uint32_t* m) const override { *chw = nd.C_in * nd.H * nd.W; *p1 = nd.num_players + 1; *m = nd.num_moves; }
  int c4_view(azmi_net_c4_view* out) const override {
    out->nd = nd; out->np = np; out->x3 = x3 ? 1 : 0;
    out->lds_bytes = x3 ? tier->big.lds : tier->small.lds;   // (bf16: the engine's fused launch runs the small tile)
    return 1;
  }
  // layout() again, as what each section is made FROM (alphazero/hip_net.py fold; the table order is hip_net.refresh_names)
  bool refresh_plan(azmi_refresh::Plan* plan) const override {
    using namespace azmi_refresh;
    PlanBuilder b{*plan};
    const uint32_t cin = nd.C_in, pix = nd.H * nd.W, hd = nd.v_hidden, p1 = nd.num_players + 1, m = nd.num_moves;
    const uint32_t n3 = x3 ? 3 : 1, lo3 = x3 ? 4 : 0;      // trunk and heads: high, high, low parts; the stem: high, low
    const uint32_t conv1 = b.param("conv1.weight", CH * cin * 9, AZMI_PARAM_CONV_W);
    const uint32_t bn1 = b.bn("bn1", CH);
    b.frag(frag_of(conv1, bn1, CH, MT, 2, cin, 0, cin, 9, x3 ? 2 : 1, x3 ? 2 : 0), 1);      // k = tap * C_in + ci, zero behind 9 * C_in
    b.f32(F32_BN_B, bn1, CH, CH);
    for (int i = 0; i < nd.depth; ++i) {
      const std::string pre = "conv_layers." + std::to_string(i) + ".";
      const uint32_t n1 = b.bn(pre + "bn1", CH);
      const uint32_t w1 = b.param(pre + "conv1.weight", CH * CH * 9, AZMI_PARAM_CONV_W);
      const uint32_t n2 = b.bn(pre + "bn2", CH);
      const uint32_t w2 = b.param(pre + "conv2.weight", CH * CH * 9, AZMI_PARAM_CONV_W);
      b.f32(F32_BN_A, n1, CH, CH); b.f32(F32_BN_B, n1, CH, CH); b.f32(F32_BN_B, n2, CH, CH);
      b.frag(frag_of(w1, n2, CH, MT, 2, CH, 1, CH, 9, n3, lo3), 9);      // one chunk per tap: k = tap * 64 + ci
      b.frag(frag_of(w2, NO_BN, CH, MT, 2, CH, 1, CH, 9, n3, lo3), 9);
    }
    const uint32_t vc = b.param("v_conv.weight", HC * CH, AZMI_PARAM_CONV_W);
    const uint32_t vb = b.bn("v_bn", HC);
    const uint32_t pc = b.param("pi_conv.weight", HC * CH, AZMI_PARAM_CONV_W);
    const uint32_t pb = b.bn("pi_bn", HC);
    b.frag(head_frag(vc, vb, pc, pb, 2, CH, n3, lo3), 1);
    b.f32(F32_BN_B, vb, HC, HC); b.f32(F32_BN_B, pb, HC, HC);
    b.f32(F32_FRAG, b.param("v_fc1.weight", hd * HC, AZMI_PARAM_FC_W), hd * HC, hd * HC, HC);
    b.f32(F32_COPY, b.param("v_fc1.bias", hd, AZMI_PARAM_FC_B), hd, hd);
    b.f32(F32_COPY, b.param("v_fc2.weight", p1 * hd, AZMI_PARAM_FC_W), p1 * hd, p1 * hd);
    b.f32(F32_COPY, b.param("v_fc2.bias", p1, AZMI_PARAM_FC_B), p1, p1);
    // per pixel p the high parts of W_p[m][c] = W[m][c * HW + p], then the low parts: W as [m][32 channels][HW "taps"], chunk = p
    b.frag(frag_of(b.param("pi_fc1.weight", m * HC * pix, AZMI_PARAM_FC_W), NO_BN, m, 1, 1, HC, 1, HC, pix, 2, 2), pix);
    b.f32(F32_COPY, b.param("pi_fc1.bias", m, AZMI_PARAM_FC_B), m, m);
    return true;
  }
};

int make(const azmi_net_desc* d, azmi_net* net) {
  auto f = new C4Family();
  net->family = f;
  f->nd = NetDesc{d->in_channels, d->height, d->width, d->depth, d->num_moves, d->num_players, d->v_hidden};
  BlobCursor c{static_cast<const uint8_t*>(net->blob)};
  f->np = layout(d, c);
  f->x3 = d->precision == 2;
  f->tier = &kTiers[f->x3 ? 1 : 0];
  // the tiles are shared by every Connect4-family net of the process: each gets its own (fixed) LDS size
  for (const C4Tile* t : {&kTiers[0].big, &kTiers[0].small, &kTiers[1].big, &kTiers[1].small})
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(t->kernel), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(t->lds)) != hipSuccess)
      return nfail(AZMI_ERR_NO_DEVICE, "cannot reserve %zu bytes of LDS", f->tier->big.lds);
  return AZMI_OK;
}

}  // namespace

namespace azmi_net_host {
const FamilyDef& c4_family() {
  static const FamilyDef f = {refusal, blob_bytes, make};
  return f;
}
}
