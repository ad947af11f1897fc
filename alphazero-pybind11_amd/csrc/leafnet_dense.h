// The dense Connect4-family leaf net on the matrix cores: the reference's DenseNet-mode NNArch (neural_net.py:211-230
// DenseBlock, :302-338, :448-510; the TrainConfig default is 4 planes, growth 12, 4 blocks, 5x5) on a 6x7 board with the
// pooled value head and the flat policy head, from the canonical planes to (v, pi) in one kernel.
//
// One wavefront carries one board through the whole net; a workgroup is TBW = 4 such wavefronts, each on its own part of
// the workgroup's LDS (no wavefront reads another's).  Per board in LDS:
//   feat [42 pixels][CFP + 4] f32   every RAW feature, pixel-major: the planes, then G channels per block (CFP = C_in + G*depth
//                                   rounded up to 32; the channels behind the net's own stay 0).  They are re-read by every
//                                   later block and by the heads, each time through another affine, so they stay fp32 and are
//                                   converted to bf16 when an operand is built: a bf16 copy would add a rounding of the raw
//                                   value in front of every block's own BatchNorm scale (up to |a1| * 2^-9 * |x| per use, on top
//                                   of the operand's own rounding), and the 10 - 22 KB per board are there.
//   mid  [10 x 11 cells][72] bf16   the 4G-channel bottleneck relu(bn2(conv1x1(..))) with a zero halo of 2 cells (k = 5; k = 3
//                                   uses the inner ring), 64 channels + 8 of padding per cell.  Channels >= 16 * ceil(4G/16)
//                                   and the halo are zeroed once and never written.
//   hbuf [64][42] f32               the heads' features relu(bn(conv1x1(feat))) (rows 0-31 value, 32-63 policy); reuses mid.
// The matrix instruction is v_mfma_f32_16x16x32_bf16 (A = weights [16 rows][32 k], B = activations [32 k][16 pixels], fp32
// accumulation): the 42 pixels are three 16-column tiles whose last six columns repeat pixel 41 and are dropped on the way
// out (columns of a product do not mix).  Weight fragments are read from global memory (L2) in MFMA lane order, one 16-byte
// load per lane, the next one in flight while the current one is used.
//
// Per block i (C_i = C_in + G*i):
//   1. B = bf16(relu(a1[c] * feat[p][c] + b1[c])), c < roundup32(C_i)           (bn1 of the block; padded a1 = b1 = 0)
//   2. mid[p][m] = bf16(relu(W1 B + c1)), m < 16 * ceil(4G/16)                  (bn2 folded into W1's rows)
//   3. acc[g][p] = sum over taps, k: W2[tap][g][k] * mid[p + tap][k]            (one 16-row tile, rows >= G zero)
//   4. feat[p][C_i + g] = acc[g][p], g < G
// Heads: hbuf = relu(Wh bf16(feat) + bh); v = softmax(fc2(relu(fc1(mean_p hbuf[0:32])))), pi = softmax(fc(hbuf[32:64])): the FC
// parts are plain fp32 (1.4 k + 32*Hd + .. products per board, against 2.4 M in the trunk).
//
// Weight image (alphazero/hip_net.py fold_dense), `frag` = [64 lanes][8 bf16], element j of lane l = W[16*mt + (l & 15)][32*ks + 8*(l >> 4) + j]:
//   block i  a1[CFP] b1[CFP] c1[64] f32 | W1 frag[roundup32(C_i)/32 ks][ceil(4G/16) mt] | W2 frag[K*K taps][ceil(4G/32) ks]
//   heads    bh[64] f32 | Wh frag[CFP/32 ks][4 mt]
//   v_fc1 W[Hd][32] b[Hd] | v_fc2 W[P+1][Hd] b[P+1] | pi_fc1 W[M][32*42] b[M]    (f32, torch layouts)
//
// LAYER instance (trunk_norm = "layer": bn1 / bn2 are nn.GroupNorm(1, C), neural_net.py:166-180; trunk_act relu).  The statistics
// are per board and one wavefront owns one board, so both reductions are wave-local (lane sums, then a 6-step butterfly), in fp32,
// two passes each - the mean, then the variance AROUND it - and need no LDS of their own:
//   bn1 of block i  over the raw fp32 features feat[p][c], p < 42, c < C_i: the channels C_i..roundup32(C_i) of the k-steps and the
//                   row's tail are not read.  step 1 becomes B = bf16(relu(g1[c] * ((x - mean) * inv) + b1[c])): the normalised value
//                   is formed in fp32 before the only rounding (padded g1 = b1 = 0 keep the padded channels 0).
//   bn2             over the 1x1's fp32 accumulators, rows m < 4G (rows 4G.. of the 16-row tiles are left out) x the 42 real pixel
//                   columns (the six repeated columns 42..47 are left out), before anything is rounded; step 2 becomes
//                   mid[p][m] = bf16(relu(g2[m] * ((acc - mean) * inv) + b2[m])) with g2 = b2 = 0 in rows >= 4G.
// inv = 1 / sqrt(var + 1e-5): a constant tensor gives 1 / sqrt(eps) and finite outputs (an idle wavefront runs on zeros).
// Image of a block: g1[CFP] b1[CFP] g2[64] b2[64] f32 | W1 (raw rows) | W2 - 256 bytes more than the batch one; the rest is the same.
// The batch instance is the kernel it was (profiles/leafnet_dense_layer_identity.txt).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "leafnet_c4.h"   // bf16x8 / f32x4, WFRAG_BYTES

namespace azmi_net_dev {
namespace dn {

constexpr int NTH = 256, TBW = 4;          // threads; boards (= wavefronts) per workgroup
constexpr int BH = 6, BW = 7, PIX = BH * BW;
constexpr int HALO = 2, MW = BW + 2 * HALO, MH = BH + 2 * HALO, MCELLS = MW * MH;    // 11 x 10 cells
constexpr int MP = 72;                     // bf16 per cell of mid: 64 channels + 8 (144 B: 16-byte reads stay aligned)
constexpr int MID_BYTES = MCELLS * MP * 2; // 15,840 (>= 64 * 42 * 4 = 10,752 of hbuf)
constexpr int HEADCH = 64, HC1 = 32;
constexpr int VEC_FLOATS = HC1 + 256 + 16 + 4;   // pooled[32] | hidden[<= 256] | logits[<= 16] | value logits[<= 4]
constexpr int MAX_CF = 128, MAX_G = 16;

struct DnDesc {
  int C_in, G, depth, K, CF, CFP;          // CF = C_in + G*depth, CFP = CF rounded up to 32
  int num_moves, num_players, v_hidden;
};
struct DnPtrs {            // device pointers into the folded weight image
  const uint8_t* blocks;
  const float* head_b;     // [64]
  const uint8_t* head_w;   // frag[CFP/32][4]
  const float *v_fc1_w, *v_fc1_b, *v_fc2_w, *v_fc2_b, *pi_fc_w, *pi_fc_b;
};

__host__ __device__ constexpr int round_up(int x, int m) { return (x + m - 1) / m * m; }
__host__ __device__ inline int feat_pitch(int cfp) { return cfp + 4; }                              // floats per pixel
__host__ __device__ inline size_t board_lds(int cfp) { return static_cast<size_t>(PIX) * feat_pitch(cfp) * 4 + MID_BYTES + VEC_FLOATS * 4; }
__host__ __device__ inline size_t block_bytes(const DnDesc& d, int i, bool layer = false) {
  return (2 * static_cast<size_t>(d.CFP) + (layer ? 128 : 64)) * 4 +
         (static_cast<size_t>(round_up(d.C_in + d.G * i, 32) / 32) * round_up(4 * d.G, 16) / 16 +
          static_cast<size_t>(d.K) * d.K * (round_up(4 * d.G, 32) / 32)) * WFRAG_BYTES;
}
inline size_t lds_bytes(const DnDesc& d) { return TBW * board_lds(d.CFP); }

__device__ __forceinline__ bf16x8 ldg_frag(const uint8_t* frag, int lane) {
  return *reinterpret_cast<const bf16x8*>(frag + lane * 16);
}

// rows / row_count (may be NULL): the eval list - board g of the launch is slot rows[g] while g < *row_count, and is not
// evaluated (nothing read, nothing written) from there on; without a list board g is row g while g < batch
template <bool LAYER>
__global__ __launch_bounds__(NTH) void k_leafnet_dense(DnDesc d, DnPtrs w, const float* __restrict__ canon, float* __restrict__ v_out,
                                                       float* __restrict__ pi_out, uint32_t batch, const uint32_t* __restrict__ rows,
                                                       const uint32_t* __restrict__ row_count) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t live = rows ? min(*row_count, batch) : batch;
  if (blockIdx.x * TBW >= live) return;                       // the whole workgroup (uniform)
  const uint32_t g = blockIdx.x * TBW + wave;
  const bool on = g < live;                                   // an idle wavefront runs the net on zeros and stores nothing
  const size_t row = on ? (rows ? rows[g] : g) : 0;
  const int FP = feat_pitch(d.CFP);
  uint8_t* base = lds + wave * board_lds(d.CFP);
  float* feat = reinterpret_cast<float*>(base);
  __bf16* mid = reinterpret_cast<__bf16*>(base + static_cast<size_t>(PIX) * FP * 4);
  float* hbuf = reinterpret_cast<float*>(mid);
  float* vec = reinterpret_cast<float*>(base + static_cast<size_t>(PIX) * FP * 4 + MID_BYTES);

  for (int e = lane; e < PIX * FP; e += 64) feat[e] = 0.0f;
  for (int e = lane; e < MID_BYTES / 4; e += 64) reinterpret_cast<uint32_t*>(mid)[e] = 0u;
  __syncthreads();
  if (on) {
    const float* src = canon + row * static_cast<size_t>(d.C_in) * PIX;
    for (int e = lane; e < d.C_in * PIX; e += 64) feat[(e % PIX) * FP + e / PIX] = src[e];
  }
  __syncthreads();

  const int q = lane >> 4, col = lane & 15;
  int px[3], cell[3];                                         // this lane's pixel in each of the three column tiles
  for (int nt = 0; nt < 3; ++nt) {
    px[nt] = min(nt * 16 + col, PIX - 1);
    cell[nt] = (px[nt] / BW + HALO) * MW + px[nt] % BW + HALO;
  }
  // B fragments of one k-step of a 1x1 convolution over feat: channels 32*ks + 8*q .. + 7 of the lane's pixels, through
  // relu(a * x + b) when a != nullptr
  auto feat_frags = [&](int ks, const float* a, const float* b, bf16x8* out, float mean = 0.0f, float inv = 1.0f) {
    const int c0 = 32 * ks + 8 * q;
    float sa[8], sb[8];
    if (a) {
      const f32x4 a0 = *reinterpret_cast<const f32x4*>(a + c0), a1 = *reinterpret_cast<const f32x4*>(a + c0 + 4);
      const f32x4 b0 = *reinterpret_cast<const f32x4*>(b + c0), b1 = *reinterpret_cast<const f32x4*>(b + c0 + 4);
      for (int j = 0; j < 4; ++j) { sa[j] = a0[j]; sa[4 + j] = a1[j]; sb[j] = b0[j]; sb[4 + j] = b1[j]; }
    }
    for (int nt = 0; nt < 3; ++nt) {
      const float* f = feat + px[nt] * FP + c0;
      const f32x4 x0 = *reinterpret_cast<const f32x4*>(f), x1 = *reinterpret_cast<const f32x4*>(f + 4);
      for (int j = 0; j < 8; ++j) {
        float x = j < 4 ? x0[j] : x1[j - 4];
        if constexpr (LAYER) { if (a) x = fmaxf(sa[j] * ((x - mean) * inv) + sb[j], 0.0f); }
        else if (a) x = fmaxf(sa[j] * x + sb[j], 0.0f);
        out[nt][j] = static_cast<__bf16>(x);
      }
    }
  };

  const int MT1 = round_up(4 * d.G, 16) / 16, KS2 = round_up(4 * d.G, 32) / 32, KK = d.K * d.K, half = d.K / 2;
  const uint8_t* blk = w.blocks;
  for (int i = 0; i < d.depth; ++i) {
    const int Ci = d.C_in + d.G * i, KS1 = round_up(Ci, 32) / 32;
    const float* a1 = reinterpret_cast<const float*>(blk);
    const float* b1 = a1 + d.CFP;
    const float* c1 = b1 + d.CFP;                                // LAYER: g2[64], then b2[64]
    const uint8_t* w1 = reinterpret_cast<const uint8_t*>(c1 + (LAYER ? 128 : 64));
    float mean1 = 0.0f, inv1 = 1.0f;
    if constexpr (LAYER) {  // bn1: the C_i raw features of the 42 pixels, nothing of the padding behind them
      const float cnt = static_cast<float>(PIX * Ci);
      float s = 0.0f;
      for (int p = 0; p < PIX; ++p) for (int c = lane; c < Ci; c += 64) s += feat[p * FP + c];
      for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
      mean1 = s / cnt;
      float qq = 0.0f;
      for (int p = 0; p < PIX; ++p) for (int c = lane; c < Ci; c += 64) { const float dx = feat[p * FP + c] - mean1; qq += dx * dx; }
      for (int off = 32; off > 0; off >>= 1) qq += __shfl_xor(qq, off, 64);
      inv1 = 1.0f / sqrtf(qq / cnt + 1e-5f);
    }
    const uint8_t* w2 = w1 + static_cast<size_t>(KS1) * MT1 * WFRAG_BYTES;
    {  // bottleneck 1x1: mid = bf16(relu(W1 act(feat) + c1))
      f32x4 acc[4][3];
      for (int mt = 0; mt < 4; ++mt) for (int nt = 0; nt < 3; ++nt) acc[mt][nt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
      for (int ks = 0; ks < KS1; ++ks) {
        bf16x8 b[3];
        feat_frags(ks, a1, b1, b, mean1, inv1);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
          if (mt < MT1) {
            const bf16x8 a = ldg_frag(w1 + (static_cast<size_t>(ks) * MT1 + mt) * WFRAG_BYTES, lane);
            for (int nt = 0; nt < 3; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b[nt], acc[mt][nt], 0, 0, 0);
          }
        }
      }
      float mean2 = 0.0f, inv2 = 1.0f;
      if constexpr (LAYER) {  // bn2: the accumulators of rows < 4G and real pixel columns, before the epilogue rounds
        const int M4 = 4 * d.G;
        const float cnt = static_cast<float>(M4 * PIX);
        // 0 / 1 weights in registers, not branches: an element counts where it is a real row (16 mt + 4 q + r < 4G, that is
        // 4 mt + q < G for every r; tiles mt >= MT1 fail it) and a real pixel
        float wt[4][3];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
          for (int nt = 0; nt < 3; ++nt) wt[mt][nt] = (4 * mt + q < d.G && nt * 16 + col < PIX) ? 1.0f : 0.0f;
        float s = 0.0f;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
          for (int nt = 0; nt < 3; ++nt)
            for (int r = 0; r < 4; ++r) s += wt[mt][nt] * acc[mt][nt][r];
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
        mean2 = s / cnt;
        float qq = 0.0f;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
          for (int nt = 0; nt < 3; ++nt)
            for (int r = 0; r < 4; ++r) {
              const float dx = acc[mt][nt][r] - mean2;
              qq += wt[mt][nt] * (dx * dx);
            }
        for (int off = 32; off > 0; off >>= 1) qq += __shfl_xor(qq, off, 64);
        inv2 = 1.0f / sqrtf(qq / cnt + 1e-5f);
      }
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        if (mt < MT1) {
          const int m0 = 16 * mt + 4 * q;                      // D: row = 4 * (lane >> 4) + r, column = lane & 15
          const f32x4 bias = *reinterpret_cast<const f32x4*>(c1 + (LAYER ? 64 : 0) + m0);
          f32x4 gain = f32x4{1.0f, 1.0f, 1.0f, 1.0f};
          if constexpr (LAYER) gain = *reinterpret_cast<const f32x4*>(c1 + m0);
          for (int nt = 0; nt < 3; ++nt) {
            if (nt * 16 + col < PIX) {
              bf16x4 o;
              for (int r = 0; r < 4; ++r) {
                if constexpr (LAYER) o[r] = static_cast<__bf16>(fmaxf(gain[r] * ((acc[mt][nt][r] - mean2) * inv2) + bias[r], 0.0f));
                else o[r] = static_cast<__bf16>(fmaxf(acc[mt][nt][r] + bias[r], 0.0f));
              }
              *reinterpret_cast<bf16x4*>(mid + cell[nt] * MP + m0) = o;
            }
          }
        }
      }
    }
    __syncthreads();
    {  // k x k over the bottleneck, tap by tap; the G new raw channels go behind the C_i the block read
      f32x4 acc[3];
      for (int nt = 0; nt < 3; ++nt) acc[nt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
      const int steps = KK * KS2;
      bf16x8 a_next = ldg_frag(w2, lane);
      for (int s = 0; s < steps; ++s) {
        const bf16x8 a = a_next;
        if (s + 1 < steps) a_next = ldg_frag(w2 + static_cast<size_t>(s + 1) * WFRAG_BYTES, lane);
        const int tap = s / KS2, ks = s - tap * KS2;
        const int shift = (tap / d.K - half) * MW + (tap % d.K - half);
        for (int nt = 0; nt < 3; ++nt) {
          const bf16x8 b = *reinterpret_cast<const bf16x8*>(mid + (cell[nt] + shift) * MP + 32 * ks + 8 * q);
          acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[nt], 0, 0, 0);
        }
      }
      for (int nt = 0; nt < 3; ++nt)
        if (nt * 16 + col < PIX)
          for (int r = 0; r < 4; ++r)
            if (4 * q + r < d.G) feat[px[nt] * FP + Ci + 4 * q + r] = acc[nt][r];
    }
    __syncthreads();
    blk += block_bytes(d, i, LAYER);
  }

  {  // heads' 1x1 over every raw feature: hbuf[m][p] = relu(Wh feat + bh)   (mid is dead: the last block's reads are behind the barrier)
    f32x4 acc[4][3];
    for (int mt = 0; mt < 4; ++mt) for (int nt = 0; nt < 3; ++nt) acc[mt][nt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int ks = 0; ks < d.CFP / 32; ++ks) {
      bf16x8 b[3];
      feat_frags(ks, nullptr, nullptr, b);
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        const bf16x8 a = ldg_frag(w.head_w + (static_cast<size_t>(ks) * 4 + mt) * WFRAG_BYTES, lane);
        for (int nt = 0; nt < 3; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b[nt], acc[mt][nt], 0, 0, 0);
      }
    }
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      const int m0 = 16 * mt + 4 * q;
      const f32x4 bias = *reinterpret_cast<const f32x4*>(w.head_b + m0);
      for (int nt = 0; nt < 3; ++nt)
        if (nt * 16 + col < PIX)
          for (int r = 0; r < 4; ++r) hbuf[(m0 + r) * PIX + px[nt]] = fmaxf(acc[mt][nt][r] + bias[r], 0.0f);
    }
  }
  __syncthreads();

  float* pooled = vec;              // [32]
  float* hidden = vec + HC1;        // [v_hidden]
  float* logit = hidden + 256;      // [num_moves]
  float* vlogit = logit + 16;       // [P + 1]
  const int Hd = d.v_hidden, P1 = d.num_players + 1, M = d.num_moves;
  if (lane < HC1) {
    float s = 0.0f;
    for (int p = 0; p < PIX; ++p) s += hbuf[lane * PIX + p];
    pooled[lane] = s / static_cast<float>(PIX);
  }
  {  // flat policy head: the reference's feature order (c, h, w) is hbuf's own
    const float* h = hbuf + HC1 * PIX;
    for (int m = 0; m < M; ++m) {
      const float* wr = w.pi_fc_w + static_cast<size_t>(m) * HC1 * PIX;
      float s = 0.0f;
      for (int f = lane; f < HC1 * PIX; f += 64) s += wr[f] * h[f];
      for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
      if (lane == 0) logit[m] = s + w.pi_fc_b[m];
    }
  }
  __syncthreads();
  for (int j = lane; j < Hd; j += 64) {
    const float* wr = w.v_fc1_w + static_cast<size_t>(j) * HC1;
    float s = w.v_fc1_b[j];
    for (int c = 0; c < HC1; ++c) s += wr[c] * pooled[c];
    hidden[j] = fmaxf(s, 0.0f);
  }
  __syncthreads();
  if (lane < P1) {
    const float* wr = w.v_fc2_w + static_cast<size_t>(lane) * Hd;
    float s = w.v_fc2_b[lane];
    for (int j = 0; j < Hd; ++j) s += wr[j] * hidden[j];
    vlogit[lane] = s;
  }
  __syncthreads();
  if (!on) return;
  auto softmax_out = [&](const float* x, int n, float* out) {   // lane e < n writes out[e]
    float mx = x[0];
    for (int e = 1; e < n; ++e) mx = fmaxf(mx, x[e]);
    float sum = 0.0f;
    for (int e = 0; e < n; ++e) sum += expf(x[e] - mx);
    if (lane < n) out[lane] = expf(x[lane] - mx) / sum;
  };
  softmax_out(vlogit, P1, v_out + row * P1);
  softmax_out(logit, M, pi_out + row * M);
}

}  // namespace dn
}  // namespace azmi_net_dev
