// azmi_net_refresh (include/azmi.h): what a family states about its weight image so that the refresh kernels
// (leafnet_refresh_kernels.h) can write it from the trained model's parameters - the ordered parameter list and a region map.
// Plain records shared by host and device code; no device code here: the family units include this through leafnet_host.h.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/azmi.h"

namespace azmi_refresh {

constexpr uint32_t BN_STRIDE = 128;      // doubles per folded BatchNorm vector in the scratch (the dense tile's bn1 has up to 128 channels)
constexpr uint32_t NO_BN = 0xffffffffu;

// One tensor of the table, as the device sees it (the pointer and count of azmi_net_param; eps of a running_var record)
struct Param {
  const float* data;
  uint64_t count;
  double eps;
};

// BatchNorm l: a = w / sqrt(var + eps), b = bias - mean * a in float64 -> scratch[l][0][c], scratch[l][1][c], c < channels
struct Bn {
  uint32_t w, b, mean, var;      // table indices
  uint32_t channels;
};

// A run of bf16 MFMA A-fragments `frag` = [k-step][m-tile][64 lanes][8 bf16], element j of lane l = M[16*mt + (l & 15)][32*ks + 8*(l >> 4) + j],
// laid out as chunks of `kspc` k-steps, each chunk `npass` times (bit p of lo_mask: pass p holds the low parts x - bf16(x), else the
// high parts bf16(x); one plain pass is the bf16 image).  The matrix is a view of one or two convolution / FC weights W[row][ci][tap]:
//   k_in = k inside the chunk; tap = chunk * taps_per_chunk + k_in / kc, channel = k_in % kc;
//   rows below `split` come from src[0], the others (row - split) from src[1]; each scaled by its BatchNorm's `a` unless NO_BN;
//   a row >= rows[s], a channel >= ci or a tap >= taps is padding: exact zeros.
struct Frag {
  uint64_t dst;                  // byte offset in the image
  uint32_t units;                // 16-byte stores: chunks * npass * kspc * mt * 64
  uint32_t src[2], bn[2], rows[2];
  uint32_t split;
  uint32_t mt, kspc, npass, lo_mask;
  uint32_t kc, taps_per_chunk, ci, taps;
};

enum F32Kind : uint32_t {
  F32_COPY = 0,      // dst[i] = table[src][i], i < valid; zeros behind
  F32_BN_A = 1,      // dst[i] = float(a of BatchNorm src), i < valid; zeros behind
  F32_BN_B = 2,      // the same of b
  F32_FRAG = 3       // hip_net._f32_frags of table[src] = W[N][k]: [N/16][k/16][64 lanes][4], element j of lane l = W[16*t + (l & 15)][16*g + 4*j + (l >> 4)]
};
struct F32 {
  uint64_t dst;                  // byte offset in the image
  uint32_t count;                // floats written
  uint32_t kind, src, valid, k;
};

// Host side: the family's answer to Family::refresh_plan
struct ParamSpec {
  std::string name;              // the state_dict name (hip_net.refresh_names)
  uint64_t count;
  uint32_t kind;                 // AZMI_PARAM_*
};
struct Plan {
  std::vector<ParamSpec> params;
  std::vector<Bn> bns;
  std::vector<Frag> frags;
  std::vector<F32> f32s;
};

// A family writes its plan as it writes its BlobCursor walk: parameters in table order, regions in image order
struct PlanBuilder {
  Plan& plan;
  uint64_t off = 0;
  uint32_t param(const std::string& name, uint64_t count, uint32_t kind) {
    plan.params.push_back(ParamSpec{name, count, kind});
    return static_cast<uint32_t>(plan.params.size() - 1);
  }
  uint32_t bn(const std::string& prefix, uint32_t channels) {      // the four tensors of a BatchNorm2d; -> its index in the scratch
    Bn b{};
    b.w = param(prefix + ".weight", channels, AZMI_PARAM_BN_WEIGHT);
    b.b = param(prefix + ".bias", channels, AZMI_PARAM_BN_BIAS);
    b.mean = param(prefix + ".running_mean", channels, AZMI_PARAM_BN_MEAN);
    b.var = param(prefix + ".running_var", channels, AZMI_PARAM_BN_VAR);
    b.channels = channels;
    plan.bns.push_back(b);
    return static_cast<uint32_t>(plan.bns.size() - 1);
  }
  void frag(Frag f, uint32_t chunks) {
    f.dst = off;
    f.units = chunks * f.npass * f.kspc * f.mt * 64;
    off += static_cast<uint64_t>(f.units) * 16;
    plan.frags.push_back(f);
  }
  void f32(uint32_t kind, uint32_t src, uint32_t count, uint32_t valid, uint32_t k = 0) {
    plan.f32s.push_back(F32{off, count, kind, src, valid, k});
    off += static_cast<uint64_t>(count) * 4;
  }
};
// the fragments of one weight W[rows][ci][taps] (see Frag)
inline Frag frag_of(uint32_t src, uint32_t bn, uint32_t rows, uint32_t mt, uint32_t kspc, uint32_t kc, uint32_t taps_per_chunk, uint32_t ci,
                    uint32_t taps, uint32_t npass = 1, uint32_t lo_mask = 0) {
  Frag f{};
  f.src[0] = f.src[1] = src; f.bn[0] = f.bn[1] = bn; f.rows[0] = rows; f.rows[1] = 0;
  f.split = 0xffffffffu;
  f.mt = mt; f.kspc = kspc; f.npass = npass; f.lo_mask = lo_mask;
  f.kc = kc; f.taps_per_chunk = taps_per_chunk; f.ci = ci; f.taps = taps;
  return f;
}
// the heads' 1x1: rows 0-31 the value convolution, rows 32-63 the policy convolution, each through its own BatchNorm
inline Frag head_frag(uint32_t v_conv, uint32_t v_bn, uint32_t pi_conv, uint32_t pi_bn, uint32_t kspc, uint32_t ci, uint32_t npass = 1,
                      uint32_t lo_mask = 0) {
  Frag f = frag_of(v_conv, v_bn, 32, 4, kspc, 32 * kspc, 0, ci, 1, npass, lo_mask);
  f.src[1] = pi_conv; f.bn[1] = pi_bn; f.rows[1] = 32; f.split = 32;
  return f;
}

}  // namespace azmi_refresh
