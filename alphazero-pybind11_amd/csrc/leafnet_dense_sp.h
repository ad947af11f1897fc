// The dense spatial-head leaf nets on the matrix cores: the reference's DenseNet-mode NNArch (neural_net.py:211-230 DenseBlock,
// :302-338) with the spatial policy head (:390-427, :448-510) on 7x7, 11x11 and 13x13 boards - the four single-variant StarGambit
// configs (configs/star_gambit_{skirmish,showdown,clash,battle}.yaml: growth 16, 4 blocks, 3x3, head_channels 32, 10 policy
// channels + 19 global actions) - from the canonical planes to (v, pi) in one kernel.
//
// The arithmetic and its numerics contract are those of the dense Connect4 tile (leafnet_dense.h); the geometry differs.  One
// WORKGROUP of four wavefronts carries one board: the PIX = 49 / 121 / 169 pixels are NT = 4 / 8 / 11 column tiles of 16, and
// wavefront w owns the tiles w, w + 4, w + 8 (NTW = 1 / 2 / 3 per wavefront; a tile index >= NT and the columns >= PIX of the
// last tile repeat pixel PIX - 1, are computed and dropped in front of every store: columns of a product do not mix).  LDS:
//   feat [PIX][CFP + 4] f32          every RAW feature, pixel-major (CFP = C_in + G*depth rounded up to 32; channels behind the
//                                    net's own stay 0); each wavefront reads and writes the rows of its own pixels only
//   mid  [(B + 4)^2 cells][72] bf16  the 4G-channel bottleneck relu(bn2(conv1x1(..))) with a zero halo of 2 cells; written by the
//                                    pixel's owner, read across wavefronts by the k x k: a workgroup barrier on either side
//   hbuf [64][PIX] f32               the heads' features relu(bn(conv1x1(feat))), rows 0-31 value, 32-63 policy; over mid (the
//                                    region is the larger of the two: at 13x13 hbuf is)
//   logit [pc*PIX + NG] f32          the policy logits in the reference's order (pixel-major, channel innermost, then the global
//                                    actions); over feat, which is dead behind the heads' 1x1 (pc*PIX + NG <= 32*PIX + 32 <= 36*PIX)
//   vec                              pooled[64] | value hidden[256] | pi_global hidden[256] | global logits[32] | value logits[4] |
//                                    reduction slots[8] | pi_conv2 W[32][32] b[32]
// Worst case (13x13, 128 features): 89,232 + 43,264 + 6,720 = 139,216 B of the CU's 160 KB; one workgroup per CU there and for
// the 11x11 configs (87,520 B), three and more at 7x7.
//
// Per block i (C_i = C_in + G*i), as in leafnet_dense.h:
//   1. B = bf16(relu(a1[c] * feat[p][c] + b1[c])), c < roundup32(C_i)
//   2. mid[p][m] = bf16(relu(W1 B + c1)), m < 16 * ceil(4G/16)                   | barrier
//   3. acc[g][p] = sum over taps, k: W2[tap][g][k] * mid[p + tap][k]
//   4. feat[p][C_i + g] = acc[g][p], g < G                                        | barrier
// Heads, fp32 from here on: hbuf = relu(Wh feat + bh) with SPLIT operands (feat and Wh as bf16 high + low parts, three MFMAs per
// product, the bf16x3 scheme of leafnet_c4.h: 2^-16 per product, where one bf16 rounding of feat and Wh is 2^-9 each and was,
// measured, the largest single error of the tile) | barrier | mean pool of all 64 rows; per pixel the pc logits of
// pi_conv2 (pi_bn2 folded) | barrier | v_fc1 + ReLU, pi_global[0] + ReLU | barrier | v_fc2, pi_global[2] | barrier |
// LayerNorm(globals, eps 1e-5, two passes) into the logits' tail | barrier | softmax over all num_moves logits (maximum
// subtracted; block-wide reductions in a fixed order: a row's bits do not depend on the batch) and over the value logits.
//
// Weight image (alphazero/hip_net.py fold_dense_spatial), `frag` as in leafnet_dense.h:
//   block i  a1[CFP] b1[CFP] c1[64] f32 | W1 frag[roundup32(C_i)/32 ks][ceil(4G/16) mt] | W2 frag[K*K taps][ceil(4G/32) ks]
//   heads    bh[64] f32 | Wh high parts frag[CFP/32 ks][4 mt] | Wh low parts (Wh - high) frag[CFP/32 ks][4 mt]
//   v_fc1 W[Hd][32] b[Hd] | v_fc2 W[P+1][Hd] b[P+1] | pi_conv2 W[32][32] b[32] (rows >= pc zero)                       (f32)
//   with global actions: pi_global.0 W[Hp][32] b[Hp] | pi_global.2 W[NG][Hp] b[NG] | LayerNorm g[NG] b[NG]              (f32)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "leafnet_dense.h"   // round_up, block_bytes, ldg_frag, MP, HALO; bf16x8 / f32x4

namespace azmi_net_dev {
namespace dsp {

constexpr int NTH = 256, WAVES = 4;        // threads; wavefronts of the one board of a workgroup
constexpr int TBW = 1;                     // boards per workgroup, every geometry
constexpr int HEADCH = 64, HC1 = 32, MAX_PC = 32, MAX_NG = 32, MAX_HID = 256;
// floats of `vec`: pooled | value hidden | pi_global hidden | global logits | value logits | reduction slots | pi_conv2 W, b
constexpr int V_POOL = 0, V_VHID = V_POOL + HEADCH, V_PHID = V_VHID + MAX_HID, V_GLOB = V_PHID + MAX_HID, V_VLOG = V_GLOB + MAX_NG,
              V_RED = V_VLOG + 4, V_WPI = V_RED + 8, V_BPI = V_WPI + MAX_PC * HC1, VEC_FLOATS = V_BPI + MAX_PC;

template <int B_>
struct Geo {
  static constexpr int B = B_, PIX = B * B, NT = (PIX + 15) / 16, NTW = (NT + WAVES - 1) / WAVES;
  static constexpr int MW = B + 2 * dn::HALO, MCELLS = MW * MW;
  static constexpr int MID_BYTES = MCELLS * dn::MP * 2, HBUF_BYTES = HEADCH * PIX * 4;
  static constexpr int REGION_BYTES = dn::round_up(MID_BYTES > HBUF_BYTES ? MID_BYTES : HBUF_BYTES, 16);
  static constexpr size_t lds_bytes(int cfp) { return static_cast<size_t>(PIX) * (cfp + 4) * 4 + REGION_BYTES + VEC_FLOATS * 4; }
};
using Geo7 = Geo<7>;
using Geo11 = Geo<11>;
using Geo13 = Geo<13>;

struct DspDesc {
  int C_in, G, depth, CF, CFP;             // CF = C_in + G*depth, CFP = CF rounded up to 32
  int num_moves, num_players, v_hidden, pc, num_global, pi_hidden;
};
struct DspPtrs {           // device pointers into the folded weight image
  const uint8_t* blocks;
  const float* head_b;     // [64]
  const uint8_t* head_w;   // frag[CFP/32][4] of the high parts, then of the low parts
  const float *v_fc1_w, *v_fc1_b, *v_fc2_w, *v_fc2_b, *pol_w, *pol_b;
  const float *pg1_w, *pg1_b, *pg2_w, *pg2_b, *pg_ln_g, *pg_ln_b;      // NULL without global actions
};

// rows / row_count (may be NULL): the eval list - workgroup g evaluates slot rows[g] while g < *row_count and nothing (no read,
// no store) from there on; without a list workgroup g is row g
template <typename GEO, int K>
__global__ __launch_bounds__(NTH) void k_leafnet_dense_sp(DspDesc d, DspPtrs w, const float* __restrict__ canon, float* __restrict__ v_out,
                                                          float* __restrict__ pi_out, uint32_t batch, const uint32_t* __restrict__ rows,
                                                          const uint32_t* __restrict__ row_count) {
  constexpr int PIX = GEO::PIX, NT = GEO::NT, NTW = GEO::NTW, MW = GEO::MW, MP = dn::MP, HALO = dn::HALO;
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t live = rows ? min(*row_count, batch) : batch;
  if (blockIdx.x >= live) return;                             // the whole workgroup (uniform), in front of every barrier
  const size_t row = rows ? rows[blockIdx.x] : blockIdx.x;
  const int FP = d.CFP + 4;
  float* feat = reinterpret_cast<float*>(lds);
  __bf16* mid = reinterpret_cast<__bf16*>(lds + static_cast<size_t>(PIX) * FP * 4);
  float* hbuf = reinterpret_cast<float*>(mid);
  float* vec = reinterpret_cast<float*>(lds + static_cast<size_t>(PIX) * FP * 4 + GEO::REGION_BYTES);
  float* logit = feat;

  for (int e = tid; e < PIX * FP; e += NTH) feat[e] = 0.0f;
  for (int e = tid; e < GEO::REGION_BYTES / 4; e += NTH) reinterpret_cast<uint32_t*>(mid)[e] = 0u;
  for (int e = tid; e < MAX_PC * HC1 + MAX_PC; e += NTH) vec[V_WPI + e] = w.pol_w[e];     // (b[32] follows W[32][32] in the image)
  __syncthreads();
  {
    const float* src = canon + row * static_cast<size_t>(d.C_in) * PIX;
    for (int e = tid; e < d.C_in * PIX; e += NTH) feat[(e % PIX) * FP + e / PIX] = src[e];
  }
  __syncthreads();

  const int q = lane >> 4, col = lane & 15;
  int px[NTW], cell[NTW];                                     // this lane's pixel in each of the wavefront's column tiles
  bool real[NTW];                                             // ... and whether the column is a pixel of the board
#pragma unroll
  for (int j = 0; j < NTW; ++j) {
    const int p = (wave + WAVES * j) * 16 + col;
    real[j] = wave + WAVES * j < NT && p < PIX;
    px[j] = min(p, PIX - 1);
    cell[j] = (px[j] / GEO::B + HALO) * MW + px[j] % GEO::B + HALO;
  }
  // B fragments of one k-step of a block's 1x1 over feat: channels 32*ks + 8*q .. + 7 of the lane's pixels through relu(a * x + b)
  auto feat_frags = [&](int ks, const float* a, const float* b, bf16x8* out) {
    const int c0 = 32 * ks + 8 * q;
    float sa[8], sb[8];
    const f32x4 a0 = *reinterpret_cast<const f32x4*>(a + c0), a1 = *reinterpret_cast<const f32x4*>(a + c0 + 4);
    const f32x4 b0 = *reinterpret_cast<const f32x4*>(b + c0), b1 = *reinterpret_cast<const f32x4*>(b + c0 + 4);
    for (int j = 0; j < 4; ++j) { sa[j] = a0[j]; sa[4 + j] = a1[j]; sb[j] = b0[j]; sb[4 + j] = b1[j]; }
#pragma unroll
    for (int nt = 0; nt < NTW; ++nt) {
      const float* f = feat + px[nt] * FP + c0;
      const f32x4 x0 = *reinterpret_cast<const f32x4*>(f), x1 = *reinterpret_cast<const f32x4*>(f + 4);
      for (int j = 0; j < 8; ++j) out[nt][j] = static_cast<__bf16>(fmaxf(sa[j] * (j < 4 ? x0[j] : x1[j - 4]) + sb[j], 0.0f));
    }
  };

  const dn::DnDesc bd{d.C_in, d.G, d.depth, K, d.CF, d.CFP, 0, 0, 0};      // (what block_bytes reads)
  const int MT1 = dn::round_up(4 * d.G, 16) / 16, KS2 = dn::round_up(4 * d.G, 32) / 32;
  constexpr int KK = K * K, half = K / 2;
  const uint8_t* blk = w.blocks;
  for (int i = 0; i < d.depth; ++i) {
    const int Ci = d.C_in + d.G * i, KS1 = dn::round_up(Ci, 32) / 32;
    const float* a1 = reinterpret_cast<const float*>(blk);
    const float* b1 = a1 + d.CFP;
    const float* c1 = b1 + d.CFP;
    const uint8_t* w1 = reinterpret_cast<const uint8_t*>(c1 + 64);
    const uint8_t* w2 = w1 + static_cast<size_t>(KS1) * MT1 * WFRAG_BYTES;
    {  // bottleneck 1x1: mid = bf16(relu(W1 act(feat) + c1))
      f32x4 acc[4][NTW];
      for (int mt = 0; mt < 4; ++mt) for (int nt = 0; nt < NTW; ++nt) acc[mt][nt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
      for (int ks = 0; ks < KS1; ++ks) {
        bf16x8 b[NTW];
        feat_frags(ks, a1, b1, b);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
          if (mt < MT1) {
            const bf16x8 a = dn::ldg_frag(w1 + (static_cast<size_t>(ks) * MT1 + mt) * WFRAG_BYTES, lane);
#pragma unroll
            for (int nt = 0; nt < NTW; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b[nt], acc[mt][nt], 0, 0, 0);
          }
        }
      }
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        if (mt < MT1) {
          const int m0 = 16 * mt + 4 * q;                      // D: row = 4 * (lane >> 4) + r, column = lane & 15
          const f32x4 bias = *reinterpret_cast<const f32x4*>(c1 + m0);
#pragma unroll
          for (int nt = 0; nt < NTW; ++nt) {
            if (real[nt]) {
              bf16x4 o;
              for (int r = 0; r < 4; ++r) o[r] = static_cast<__bf16>(fmaxf(acc[mt][nt][r] + bias[r], 0.0f));
              *reinterpret_cast<bf16x4*>(mid + cell[nt] * MP + m0) = o;
            }
          }
        }
      }
    }
    __syncthreads();
    {  // k x k over the bottleneck, tap by tap; the G new raw channels go behind the C_i the block read
      f32x4 acc[NTW];
      for (int nt = 0; nt < NTW; ++nt) acc[nt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
      const int steps = KK * KS2;
      bf16x8 a_next = dn::ldg_frag(w2, lane);
      for (int s = 0; s < steps; ++s) {
        const bf16x8 a = a_next;
        if (s + 1 < steps) a_next = dn::ldg_frag(w2 + static_cast<size_t>(s + 1) * WFRAG_BYTES, lane);
        const int tap = s / KS2, ks = s - tap * KS2;
        const int shift = (tap / K - half) * MW + (tap % K - half);
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt) {
          const bf16x8 b = *reinterpret_cast<const bf16x8*>(mid + (cell[nt] + shift) * MP + 32 * ks + 8 * q);
          acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[nt], 0, 0, 0);
        }
      }
#pragma unroll
      for (int nt = 0; nt < NTW; ++nt)
        if (real[nt])
          for (int r = 0; r < 4; ++r)
            if (4 * q + r < d.G) feat[px[nt] * FP + Ci + 4 * q + r] = acc[nt][r];
    }
    __syncthreads();
    blk += dn::block_bytes(bd, i);
  }

  {  // heads' 1x1 over every raw feature: hbuf[m][p] = relu(Wh feat + bh)   (mid is dead: the last block's reads are behind the barrier)
    // SPLIT operands: x = hi + lo and w = hi + lo in bf16 parts, three MFMAs per product (lo * lo, 2^-16 of the product, is left
    // out) - the heads are the fp32 part of the net, and a plain bf16 1x1 here is the largest single error of the tile
    f32x4 acc[4][NTW];
    for (int mt = 0; mt < 4; ++mt) for (int nt = 0; nt < NTW; ++nt) acc[mt][nt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const int KSH = d.CFP / 32;
    const uint8_t* head_lo = w.head_w + static_cast<size_t>(KSH) * 4 * WFRAG_BYTES;
    for (int ks = 0; ks < KSH; ++ks) {
      bf16x8 bh[NTW], bl[NTW];
      const int c0 = 32 * ks + 8 * q;
#pragma unroll
      for (int nt = 0; nt < NTW; ++nt) {
        const float* f = feat + px[nt] * FP + c0;
        const f32x4 x0 = *reinterpret_cast<const f32x4*>(f), x1 = *reinterpret_cast<const f32x4*>(f + 4);
        for (int j = 0; j < 8; ++j) {
          const float x = j < 4 ? x0[j] : x1[j - 4];
          const __bf16 hi = static_cast<__bf16>(x);
          bh[nt][j] = hi;
          bl[nt][j] = static_cast<__bf16>(x - static_cast<float>(hi));
        }
      }
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        const bf16x8 ah = dn::ldg_frag(w.head_w + (static_cast<size_t>(ks) * 4 + mt) * WFRAG_BYTES, lane);
        const bf16x8 al = dn::ldg_frag(head_lo + (static_cast<size_t>(ks) * 4 + mt) * WFRAG_BYTES, lane);
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt) {
          acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh[nt], acc[mt][nt], 0, 0, 0);
          acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl[nt], acc[mt][nt], 0, 0, 0);
          acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh[nt], acc[mt][nt], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      const int m0 = 16 * mt + 4 * q;
      const f32x4 bias = *reinterpret_cast<const f32x4*>(w.head_b + m0);
#pragma unroll
      for (int nt = 0; nt < NTW; ++nt)
        if (real[nt])
          for (int r = 0; r < 4; ++r) hbuf[(m0 + r) * PIX + px[nt]] = fmaxf(acc[mt][nt][r] + bias[r], 0.0f);
    }
  }
  __syncthreads();            // hbuf is whole; feat is dead from here on (logit lies over it)

  const int Hd = d.v_hidden, P1 = d.num_players + 1, M = d.num_moves, pc = d.pc, NG = d.num_global, Hp = d.pi_hidden;
  {  // mean pool of the 64 head rows: four threads per row, pixels part, part + 4, .., then the two butterfly steps
    const int r = tid >> 2, part = tid & 3;
    float s = 0.0f;
    for (int p = part; p < PIX; p += 4) s += hbuf[r * PIX + p];
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    if (part == 0) vec[V_POOL + r] = s / static_cast<float>(PIX);
  }
  if (tid < PIX) {  // pi_conv2 (pi_bn2 folded) of one pixel: logits in the reference's permute(0, 2, 3, 1) order
    float h[HC1];
#pragma unroll
    for (int k = 0; k < HC1; ++k) h[k] = hbuf[(HC1 + k) * PIX + tid];
    for (int c = 0; c < pc; ++c) {
      const float* wr = vec + V_WPI + c * HC1;                // (the same address in every lane: a broadcast read)
      float s = vec[V_BPI + c];
#pragma unroll
      for (int k = 0; k < HC1; ++k) s += wr[k] * h[k];
      logit[tid * pc + c] = s;
    }
  }
  __syncthreads();
  for (int j = tid; j < Hd; j += NTH) {
    const float* wr = w.v_fc1_w + static_cast<size_t>(j) * HC1;
    float s = w.v_fc1_b[j];
    for (int c = 0; c < HC1; ++c) s += wr[c] * vec[V_POOL + c];
    vec[V_VHID + j] = fmaxf(s, 0.0f);
  }
  if (NG > 0) {
    for (int j = tid; j < Hp; j += NTH) {
      const float* wr = w.pg1_w + static_cast<size_t>(j) * HC1;
      float s = w.pg1_b[j];
      for (int c = 0; c < HC1; ++c) s += wr[c] * vec[V_POOL + HC1 + c];
      vec[V_PHID + j] = fmaxf(s, 0.0f);
    }
  }
  __syncthreads();
  {  // the two output layers, eight threads per output: hidden units part, part + 8, .., then three butterfly steps
    const int o = tid >> 3, part = tid & 7;
    float sv = 0.0f, sg = 0.0f;
    if (o < P1) for (int j = part; j < Hd; j += 8) sv += w.v_fc2_w[static_cast<size_t>(o) * Hd + j] * vec[V_VHID + j];
    if (o < NG) for (int j = part; j < Hp; j += 8) sg += w.pg2_w[static_cast<size_t>(o) * Hp + j] * vec[V_PHID + j];
    for (int off = 1; off < 8; off <<= 1) { sv += __shfl_xor(sv, off, 64); sg += __shfl_xor(sg, off, 64); }
    if (part == 0 && o < P1) vec[V_VLOG + o] = sv + w.v_fc2_b[o];
    if (part == 0 && o < NG) vec[V_GLOB + o] = sg + w.pg2_b[o];
  }
  __syncthreads();
  if (tid < NG) {  // LayerNorm over the NG global logits (biased variance around the mean, eps 1e-5)
    float mean = 0.0f;
    for (int e = 0; e < NG; ++e) mean += vec[V_GLOB + e];
    mean /= static_cast<float>(NG);
    float var = 0.0f;
    for (int e = 0; e < NG; ++e) { const float dx = vec[V_GLOB + e] - mean; var += dx * dx; }
    const float inv = 1.0f / sqrtf(var / static_cast<float>(NG) + 1e-5f);
    logit[pc * PIX + tid] = (vec[V_GLOB + tid] - mean) * inv * w.pg_ln_g[tid] + w.pg_ln_b[tid];
  }
  __syncthreads();
  // one softmax over all M logits: thread-strided partials, six butterfly steps, then the four wavefronts' slots in order
  float* red = vec + V_RED;
  float mx = -3.402823466e38f;
  for (int e = tid; e < M; e += NTH) mx = fmaxf(mx, logit[e]);
  for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
  if (lane == 0) red[wave] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  float sum = 0.0f;
  for (int e = tid; e < M; e += NTH) { const float x = expf(logit[e] - mx); logit[e] = x; sum += x; }
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
  if (lane == 0) red[4 + wave] = sum;
  __syncthreads();
  sum = (red[4] + red[5]) + (red[6] + red[7]);
  float* po = pi_out + row * static_cast<size_t>(M);
  for (int e = tid; e < M; e += NTH) po[e] = logit[e] / sum;
  if (tid < P1) {
    const float* x = vec + V_VLOG;
    float vm = x[0];
    for (int e = 1; e < P1; ++e) vm = fmaxf(vm, x[e]);
    float vs = 0.0f;
    for (int e = 0; e < P1; ++e) vs += expf(x[e] - vm);
    v_out[row * P1 + tid] = expf(x[tid] - vm) / vs;
  }
}

}  // namespace dsp
}  // namespace azmi_net_dev
