// The kernels behind azmi_net_refresh: the weight image of a matrix-core leaf net written on the device from the trained model's
// float32 parameters, byte for byte what alphazero/hip_net.py fold() / fold_dense() lay out on the host.
//
// Three launches, one per kind of region (leafnet_refresh_types.h) and not per tensor; blockIdx.y names the region, x strides over it:
//   k_refresh_bn     a = w / sqrt(var + eps), b = bias - mean * a per BatchNorm in float64 (torch_net.bn_affine's expressions: IEEE
//                    double divide and sqrt, no contraction) into a float64 scratch [BatchNorm][a, b][BN_STRIDE];
//   k_refresh_frags  the bf16 MFMA fragments: an output element (chunk, pass, k-step, m-tile, lane, j) finds its source element
//                    W[row][channel][tap], reads it as double, multiplies by the row's `a` where fold does, and rounds double ->
//                    float32 -> bf16 (both to nearest even: hip_net._bf16_bits).  A low pass writes bf16(float(x - double(hi))).
//                    Padding is exact zeros.  One thread writes one lane's 8 values = 16 bytes, consecutive threads consecutive lanes:
//                    a wavefront stores one whole 1 KB fragment.  The flat policy head's per-pixel fragments are such a region too
//                    (chunk = pixel, passes high / low), so they need no kernel of their own;
//   k_refresh_f32    the float32 regions: folded `a` / `b` vectors, tensors in torch layout, the value FC's f32 A-fragments - one
//                    rounding double -> float32, 4 bytes per thread, consecutive threads consecutive floats.
// Every output element depends on one input element and at most one scale: no LDS, no cross-lane traffic.  Every index is
// bounded by the region's own sizes and by the tensor's element count; the host checks that the regions tile the image exactly.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "leafnet_refresh_types.h"

namespace azmi_refresh {

constexpr int NTH = 256;

// The element functions are __host__ __device__: the kernels below are loops around them, and a host program can run the same
// arithmetic over host pointers.

// float32 -> bf16 bits, round to nearest even (torch's float -> bfloat16)
__host__ __device__ inline uint32_t bf16_bits(float f) {
  const uint32_t u = __builtin_bit_cast(uint32_t, f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0u;
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}
__host__ __device__ inline float bf16_value(uint32_t bits) { return __builtin_bit_cast(float, bits << 16); }

struct __attribute__((aligned(4))) Store16 {      // (the policy fragments of the ResNet tile start behind 3 floats: 4-byte aligned only)
  uint32_t w[4];
};

// channel c of BatchNorm `bn`: torch_net.bn_affine's two expressions
__host__ __device__ inline void bn_fold(const Param* table, const Bn& bn, uint32_t c, double* a, double* b) {
#pragma clang fp contract(off)
  const Param var = table[bn.var];
  *a = static_cast<double>(table[bn.w].data[c]) / sqrt(static_cast<double>(var.data[c]) + var.eps);
  *b = static_cast<double>(table[bn.b].data[c]) - static_cast<double>(table[bn.mean].data[c]) * *a;
}

// store u of fragment region r: one lane's 8 bf16 values
__host__ __device__ inline Store16 frag_unit(const Param* table, const Frag& r, const double* scratch, uint32_t u) {
#pragma clang fp contract(off)
  const uint32_t per_pass = r.kspc * r.mt * 64, per_chunk = per_pass * r.npass;
  const uint32_t chunk = u / per_chunk, in_chunk = u % per_chunk;
  const uint32_t pass = in_chunk / per_pass, in_pass = in_chunk % per_pass;
  const uint32_t ks = in_pass / (r.mt * 64), mt = (in_pass >> 6) % r.mt, lane = in_pass & 63;
  const uint32_t row = 16 * mt + (lane & 15);
  const uint32_t s = row >= r.split ? 1u : 0u;
  const uint32_t rl = s ? row - r.split : row;
  const bool row_on = rl < r.rows[s];
  const bool lo = (r.lo_mask >> pass) & 1u;
  const Param p = table[r.src[s]];
  const bool scaled = r.bn[s] != NO_BN;
  const double scale = (scaled && row_on && rl < BN_STRIDE) ? scratch[(r.bn[s] * 2) * BN_STRIDE + rl] : 1.0;
  Store16 out = {{0u, 0u, 0u, 0u}};
  for (uint32_t j = 0; j < 8; ++j) {
    const uint32_t k_in = 32 * ks + 8 * (lane >> 4) + j;
    const uint32_t tap = chunk * r.taps_per_chunk + k_in / r.kc, ch = k_in % r.kc;
    uint32_t bits = 0;
    if (row_on && ch < r.ci && tap < r.taps) {
      const uint64_t idx = (static_cast<uint64_t>(rl) * r.ci + ch) * r.taps + tap;
      if (idx < p.count) {
        double x = static_cast<double>(p.data[idx]);
        if (scaled) x = x * scale;
        bits = bf16_bits(static_cast<float>(x));
        if (lo) bits = bf16_bits(static_cast<float>(x - static_cast<double>(bf16_value(bits))));
      }
    }
    out.w[j >> 1] |= bits << (16 * (j & 1));
  }
  return out;
}

// float i of float32 region r
__host__ __device__ inline float f32_value(const Param* table, const F32& r, const double* scratch, uint32_t i) {
  if (r.kind == F32_BN_A || r.kind == F32_BN_B)
    return (i < r.valid && i < BN_STRIDE) ? static_cast<float>(scratch[(r.src * 2 + (r.kind == F32_BN_B ? 1u : 0u)) * BN_STRIDE + i]) : 0.0f;
  const Param p = table[r.src];
  uint64_t idx = i;
  if (r.kind == F32_FRAG) {      // [N/16][k/16][64 lanes][4]
    const uint32_t j = i & 3, lane = (i >> 2) & 63, tg = i >> 8, groups = r.k / 16;
    idx = static_cast<uint64_t>(16 * (tg / groups) + (lane & 15)) * r.k + 16 * (tg % groups) + 4 * j + (lane >> 4);
  }
  return (i < r.valid && idx < p.count) ? p.data[idx] : 0.0f;
}

__global__ __launch_bounds__(NTH) void k_refresh_bn(const Param* __restrict__ table, const Bn* __restrict__ bns, double* __restrict__ scratch) {
  const Bn bn = bns[blockIdx.y];
  for (uint32_t c = blockIdx.x * NTH + threadIdx.x; c < BN_STRIDE; c += gridDim.x * NTH) {
    double a = 0.0, b = 0.0;
    if (c < bn.channels) bn_fold(table, bn, c, &a, &b);
    scratch[(blockIdx.y * 2 + 0) * BN_STRIDE + c] = a;
    scratch[(blockIdx.y * 2 + 1) * BN_STRIDE + c] = b;
  }
}

__global__ __launch_bounds__(NTH) void k_refresh_frags(const Param* __restrict__ table, const Frag* __restrict__ frags,
                                                       const double* __restrict__ scratch, uint8_t* __restrict__ image) {
  const Frag r = frags[blockIdx.y];
  for (uint32_t u = blockIdx.x * NTH + threadIdx.x; u < r.units; u += gridDim.x * NTH)
    *reinterpret_cast<Store16*>(image + r.dst + static_cast<uint64_t>(u) * 16) = frag_unit(table, r, scratch, u);
}

__global__ __launch_bounds__(NTH) void k_refresh_f32(const Param* __restrict__ table, const F32* __restrict__ regions,
                                                     const double* __restrict__ scratch, uint8_t* __restrict__ image) {
  const F32 r = regions[blockIdx.y];
  float* dst = reinterpret_cast<float*>(image + r.dst);
  for (uint32_t i = blockIdx.x * NTH + threadIdx.x; i < r.count; i += gridDim.x * NTH) dst[i] = f32_value(table, r, scratch, i);
}

}  // namespace azmi_refresh
