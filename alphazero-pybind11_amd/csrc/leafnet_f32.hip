// fp32 path of the leaf policy/value network: the inference forward of the reference's NNArch, ResNet and
// DenseNet trunks (/root/reference/src/neural_net.py:211-263, 448-510) in plain fp32, layer by layer.
// This is the precision the north star's 1e-5 tolerance on (v, pi) refers to; the MFMA kernels in
// leafnet.hip are the bf16-operand fast path (what the reference runs under autocast).
// Throughput is not the point here (VALU FMAs, activations round-trip through HBM between layers).
//
// Weight blob (all f32, torch layouts, inference BatchNorms folded on the host in double; K = kernel_size: 3 for a ResNet trunk,
// 1 / 3 / 5 / 7 for a dense one, whose extra head convolutions share it):
//   ResNet trunk (CF = CH = NNArgs.num_channels, any width):
//     stem    W[CH][Cin][K][K] b[CH]
//     block i a1[CH] b1[CH] | W1[CH][CH][K][K] c1[CH] | W2[CH][CH][K][K]
//   DenseNet trunk (G = NNArgs.num_channels = the growth rate, C_i = Cin + G*i, CF = Cin + G*depth; no stem):
//     block i a1[C_i] b1[C_i] | W1[4G][C_i] c1[4G] (bn2 folded) | W2[G][4G][K][K]
//     One feature buffer [rows][CF][HW]: the canonical planes are copied into channels 0..Cin, block i reads channels
//     0..C_i through its own a1 / b1 (+ ReLU) at load time and writes its G raw output channels at offset C_i.
//   value   Wv[HC][CF] bv[HC] | v_head_convs x (W[HC][HC][K][K] b[HC]) | fc1 W[Hd][HC] b[Hd] |
//           (v_fc_layers-1) x (W[Hd][Hd] b[Hd]) | fc2 W[P+1][Hd] b[P+1]
//   policy  Wp[HC][CF] bp[HC] | pi_head_convs x (W[HC][HC][K][K] b[HC]) |
//           flat: Wfc[M][HC*H*W] b[M]      spatial: Wpol[PC][HC] bpol[PC]
//
// The variants of azmi_net_desc2 (azmi_f32::Variant; all three zero: exactly the image above and the launches it always had).
// A = 2 with trunk_act crelu (the convolution behind a CReLU reads cat(relu(x), relu(-x)): input channel ci of the weight meets
// relu(x[ci]), input channel Cin + ci meets relu(-x[ci]); the 2*Cin channels are never materialised), else 1:
//   trunk_norm batch, crelu: the folds above stay, the weights widen -
//     ResNet block i a1[CH] b1[CH] | W1[CH][A*CH][K][K] c1[CH] | W2[CH][A*CH][K][K]
//     dense  block i a1[C_i] b1[C_i] | W1[4G][A*C_i] c1[4G] | W2[G][A*4G][K][K]
//   trunk_norm layer (GroupNorm(1, C): mean and biased variance per sample over (C, H, W), eps 1e-5; data-dependent, so
//   nothing folds; g / b = the norm's weight / bias) -
//     ResNet stem    W[CH][Cin][K][K] | g0[CH] b0[CH]                      (the stem's norm has no activation behind it)
//     ResNet block i g1[CH] b1[CH] | W1[CH][A*CH][K][K] | g2[CH] b2[CH] | W2[CH][A*CH][K][K]
//     dense  block i g1[C_i] b1[C_i] | W1[4G][A*C_i] | g2[4G] b2[4G] | W2[G][A*4G][K][K]
//     k_row_stats (one wavefront per sample, two passes) writes {mean, 1/sqrt(var + eps)} per sample; the convolution behind the
//     norm applies act(g[c] * ((x - mean) * inv) + b[c]) at load time.  A dense block's bn1 spans exactly the C_i channels the
//     block reads (the head of the feature row), its bn2 the 4G raw bottleneck channels; a ResNet block's residual is its input.
//   pi_fc_layers = L > 0 (flat head; Hp = pi_hidden): fc1 W[Hp][HC*H*W] b[Hp] | (L-1) x (W[Hp][Hp] b[Hp]) | out W[M][Hp] b[M]
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "leafnet_f32.h"

namespace {

thread_local std::string g_err;
int fail(const char** err, int code, const char* what, hipError_t e = hipSuccess) {
  char buf[256];
  if (e != hipSuccess) snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
  else snprintf(buf, sizeof buf, "%s", what);
  g_err = buf;
  if (err) *err = g_err.c_str();
  return code;
}

// out[b][co][p] = act_out( bias[co] + sum_{ci,tap} W[co][ci][tap] * act_in(in[b][ci][p + tap]) ) (+ res[b][co][p])
// act_in: relu(a[ci] * x + b[ci]) when pre_a != nullptr (pre-activation BatchNorm + ReLU); zero padding is applied
// AFTER the input activation, as in the reference (the conv pads its already-activated input).
// A row of `in` holds in_ctot channels (the first Cin are read), a row of `out` / `res` out_ctot, and the Cout results go to
// channels out_coff.. of it: the dense trunk appends to its feature buffer in place; everything else passes Cin, Cout, 0.
template <int K>
__global__ void k_conv(const float* __restrict__ in, const float* __restrict__ w, const float* __restrict__ bias,
                       const float* __restrict__ pre_a, const float* __restrict__ pre_b, const float* __restrict__ res,
                       float* __restrict__ out, uint32_t B, int Cin, int Cout, int H, int W, int relu_out,
                       int in_ctot, int out_ctot, int out_coff) {
  const int HW = H * W;
  const size_t idx = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (idx >= static_cast<size_t>(B) * Cout * HW) return;
  const int p = static_cast<int>(idx % HW), co = static_cast<int>((idx / HW) % Cout);
  const size_t b = idx / (static_cast<size_t>(HW) * Cout);
  const int h = p / W, x = p % W;
  float acc = bias ? bias[co] : 0.0f;
  const float* ib = in + b * in_ctot * HW;
  const float* wc = w + static_cast<size_t>(co) * Cin * K * K;
  for (int ci = 0; ci < Cin; ++ci) {
    const float a = pre_a ? pre_a[ci] : 1.0f, sh = pre_a ? pre_b[ci] : 0.0f;
#pragma unroll
    for (int t = 0; t < K * K; ++t) {
      const int hh = h + t / K - K / 2, ww = x + t % K - K / 2;
      if (hh < 0 || hh >= H || ww < 0 || ww >= W) continue;
      float v = ib[ci * HW + hh * W + ww];
      if (pre_a) v = fmaxf(a * v + sh, 0.0f);
      acc += wc[ci * K * K + t] * v;
    }
  }
  if (relu_out) acc = fmaxf(acc, 0.0f);
  const size_t o = (b * out_ctot + out_coff + co) * HW + p;
  if (res) acc += res[o];
  out[o] = acc;
}

// stats[2*b] = mean, stats[2*b + 1] = 1 / sqrt(var + 1e-5) of the `count` floats at in + b * row_floats (GroupNorm(1, C): biased
// variance).  One wavefront per sample; two passes, the variance taken around the mean: one pass over sum and sum of squares
// cancels on a tensor whose mean is large against its spread.  A sample's lanes and order of additions do not depend on the
// batch or on the sample's place in it.
__global__ void k_row_stats(const float* __restrict__ in, float* __restrict__ stats, uint32_t B, uint32_t count, size_t row_floats) {
  const uint32_t row = blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64, lane = threadIdx.x % 64;
  if (row >= B) return;                      // (the whole wavefront)
  const float* x = in + static_cast<size_t>(row) * row_floats;
  float s = 0.0f;
  for (uint32_t e = lane; e < count; e += 64) s += x[e];
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  const float mean = s / static_cast<float>(count);
  float q = 0.0f;
  for (uint32_t e = lane; e < count; e += 64) { const float dx = x[e] - mean; q += dx * dx; }
  for (int off = 32; off > 0; off >>= 1) q += __shfl_xor(q, off, 64);
  if (lane == 0) {
    stats[2 * static_cast<size_t>(row)] = mean;
    stats[2 * static_cast<size_t>(row) + 1] = 1.0f / sqrtf(q / static_cast<float>(count) + 1e-5f);
  }
}

// x[b][c][p] = g[c] * ((x - mean[b]) * inv[b]) + beta[c] in place: the ResNet stem's norm in layer mode, which has no
// activation and no convolution behind it to carry it - its output is the first block's input and residual
__global__ void k_norm_rows(float* __restrict__ x, const float* __restrict__ g, const float* __restrict__ beta, const float* __restrict__ stats,
                            uint32_t B, int C, int HW) {
  const size_t idx = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (idx >= static_cast<size_t>(B) * C * HW) return;
  const int c = static_cast<int>((idx / HW) % C);
  const size_t b = idx / (static_cast<size_t>(HW) * C);
  x[idx] = g[c] * ((x[idx] - stats[2 * b]) * stats[2 * b + 1]) + beta[c];
}

// The trunk convolutions of the variants (file header): k_conv with the input activation
//   y = x, normalised per sample when stats != nullptr: (x - mean[b]) * inv[b], through g[ci] * y + beta[ci] when g != nullptr,
//   then relu(y) on input channel ci of the weight and, CRELU, relu(-y) on input channel Cin + ci (the weight has 2 * Cin).
// Zero padding is applied after the activation, as in k_conv; no output activation (what follows reads raw values).
template <int K, bool CRELU>
__global__ void k_conv_v(const float* __restrict__ in, const float* __restrict__ w, const float* __restrict__ bias,
                         const float* __restrict__ g, const float* __restrict__ beta, const float* __restrict__ stats,
                         const float* __restrict__ res, float* __restrict__ out, uint32_t B, int Cin, int Cout, int H, int W,
                         int in_ctot, int out_ctot, int out_coff) {
  const int HW = H * W;
  const size_t idx = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (idx >= static_cast<size_t>(B) * Cout * HW) return;
  const int p = static_cast<int>(idx % HW), co = static_cast<int>((idx / HW) % Cout);
  const size_t b = idx / (static_cast<size_t>(HW) * Cout);
  const int h = p / W, x = p % W;
  const float mean = stats ? stats[2 * b] : 0.0f, inv = stats ? stats[2 * b + 1] : 1.0f;
  float acc = bias ? bias[co] : 0.0f;
  const float* ib = in + b * in_ctot * HW;
  const float* wc = w + static_cast<size_t>(co) * (CRELU ? 2 : 1) * Cin * K * K;
  for (int ci = 0; ci < Cin; ++ci) {
    const float a = g ? g[ci] : 1.0f, sh = g ? beta[ci] : 0.0f;
#pragma unroll
    for (int t = 0; t < K * K; ++t) {
      const int hh = h + t / K - K / 2, ww = x + t % K - K / 2;
      if (hh < 0 || hh >= H || ww < 0 || ww >= W) continue;
      float v = ib[ci * HW + hh * W + ww];
      if (stats) v = (v - mean) * inv;
      if (g) v = a * v + sh;
      acc += wc[ci * K * K + t] * fmaxf(v, 0.0f);
      if (CRELU) acc += wc[(Cin + ci) * K * K + t] * fmaxf(-v, 0.0f);
    }
  }
  const size_t o = (b * out_ctot + out_coff + co) * HW + p;
  if (res) acc += res[o];
  out[o] = acc;
}

// feat[b][0 .. chw) = canon[b][0 .. chw): the canonical planes into the head of each row of the dense feature buffer
__global__ void k_copy_planes(const float* __restrict__ canon, float* __restrict__ feat, uint32_t B, uint32_t chw, uint32_t row_floats) {
  const size_t idx = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (idx >= static_cast<size_t>(B) * chw) return;
  feat[idx / chw * row_floats + idx % chw] = canon[idx];
}

__global__ void k_avgpool(const float* __restrict__ in, float* __restrict__ out, uint32_t B, int C, int HW) {
  const size_t idx = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (idx >= static_cast<size_t>(B) * C) return;
  float s = 0.0f;
  for (int p = 0; p < HW; ++p) s += in[idx * HW + p];
  out[idx] = s / static_cast<float>(HW);
}

// out[b][n] = act(bias[n] + sum_k W[n][k] * in[b][k])
__global__ void k_fc(const float* __restrict__ in, const float* __restrict__ w, const float* __restrict__ bias,
                     float* __restrict__ out, uint32_t B, int K, int N, int relu) {
  const size_t idx = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (idx >= static_cast<size_t>(B) * N) return;
  const int n = static_cast<int>(idx % N);
  const size_t b = idx / N;
  float acc = bias[n];
  const float* x = in + b * K;
  const float* wr = w + static_cast<size_t>(n) * K;
  for (int k = 0; k < K; ++k) acc += wr[k] * x[k];
  out[idx] = relu ? fmaxf(acc, 0.0f) : acc;
}

// one wavefront per row: out = softmax(row).  `chw` != 0: the row is read as [C][HW] and written as [HW][C]
// (spatial policy head: permute(0, 2, 3, 1) + flatten, neural_net.py:483-487)
// `glob` != nullptr: the row's last G entries are the global-action logits glob[row][G] behind the C*HW spatial ones
// (neural_net.py:486-493), the spatial block of row r then starts at in + r * C * HW
__global__ void k_softmax(const float* __restrict__ in, float* __restrict__ out, uint32_t B, int N, int C, int HW,
                          const float* __restrict__ glob = nullptr, int G = 0) {
  const uint32_t row = blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64, lane = threadIdx.x % 64;
  if (row >= B) return;
  const float* x = in + static_cast<size_t>(row) * (N - G);
  const float* gx = glob ? glob + static_cast<size_t>(row) * G : nullptr;
  auto src = [&](int e) { return e >= N - G ? gx[e - (N - G)] : (C ? x[(e % C) * HW + e / C] : x[e]); };
  float mx = -__builtin_inff();
  for (int e = lane; e < N; e += 64) mx = fmaxf(mx, src(e));
  for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
  float sum = 0.0f;
  for (int e = lane; e < N; e += 64) sum += expf(src(e) - mx);
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
  for (int e = lane; e < N; e += 64) out[static_cast<size_t>(row) * N + e] = expf(src(e) - mx) / sum;
}

// nn.LayerNorm(G) over the last dimension (biased variance, eps 1e-5), one thread per row
__global__ void k_layernorm(const float* __restrict__ in, const float* __restrict__ gamma, const float* __restrict__ beta,
                            float* __restrict__ out, uint32_t B, int G) {
  const uint32_t row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= B) return;
  const float* x = in + static_cast<size_t>(row) * G;
  float mean = 0.0f;
  for (int i = 0; i < G; ++i) mean += x[i];
  mean /= static_cast<float>(G);
  float var = 0.0f;
  for (int i = 0; i < G; ++i) var += (x[i] - mean) * (x[i] - mean);
  var /= static_cast<float>(G);
  const float inv = 1.0f / sqrtf(var + 1e-5f);
  for (int i = 0; i < G; ++i) out[static_cast<size_t>(row) * G + i] = (x[i] - mean) * inv * gamma[i] + beta[i];
}

struct Net {
  azmi_net_desc d{};
  bool dense = false;        // DenseNet trunk: d.channels is the growth rate
  azmi_f32::Variant var{};
  float* stats = nullptr;    // [rows][2] {mean, 1/sqrt(var + eps)} per sample (trunk_norm layer only)
  int device = 0;
  float* blob = nullptr;
  float* buf[3] = {nullptr, nullptr, nullptr};   // [rows][max(CF, 4G, HC, PC)][HW] ping-pong activations
  float* small[2] = {nullptr, nullptr};          // [rows][max(Hd, Hp, M, HC, P+1)] head vectors
  uint32_t rows = 0;
};

// channels the heads read: the trunk width, or every feature of a dense trunk
size_t trunk_out(const azmi_net_desc* d, bool dense) {
  return dense ? static_cast<size_t>(d->in_channels) + static_cast<size_t>(d->channels) * d->depth : static_cast<size_t>(d->channels);
}

size_t count_floats(const azmi_net_desc* d, bool dense, const azmi_f32::Variant& var) {
  const size_t CH = d->channels, KK = static_cast<size_t>(d->kernel_size) * d->kernel_size, CF = trunk_out(d, dense);
  const size_t HW = static_cast<size_t>(d->height) * d->width, HC = d->head_channels, Hd = d->v_hidden, P1 = d->num_players + 1;
  // crelu doubles the input channels of both convolutions of a block; layer: bn2 is g2 b2 instead of the folded c1 (and the
  // stem's norm g0 b0 instead of its folded bias)
  const size_t A = var.trunk_act ? 2 : 1, N2 = var.trunk_norm ? 2 : 1;
  size_t n = 0;
  if (dense) {
    for (size_t i = 0; i < static_cast<size_t>(d->depth); ++i) {
      const size_t Ci = d->in_channels + CH * i;
      n += 2 * Ci + 4 * CH * A * Ci + N2 * 4 * CH + CH * A * 4 * CH * KK;
    }
  } else {
    n = static_cast<size_t>(CH) * d->in_channels * KK + N2 * CH;
    n += static_cast<size_t>(d->depth) * (2 * CH + static_cast<size_t>(CH) * A * CH * KK + N2 * CH + static_cast<size_t>(CH) * A * CH * KK);
  }
  n += HC * CF + HC + static_cast<size_t>(d->v_head_convs) * (HC * HC * KK + HC);
  n += Hd * HC + Hd + static_cast<size_t>(d->v_fc_layers - 1) * (Hd * Hd + Hd) + P1 * Hd + P1;
  n += HC * CF + HC + static_cast<size_t>(d->pi_head_convs) * (HC * HC * KK + HC);
  if (d->policy_channels > 0) {
    n += static_cast<size_t>(d->policy_channels) * HC + d->policy_channels;
    const size_t G = static_cast<size_t>(d->num_moves) - static_cast<size_t>(d->policy_channels) * HW, Hp = d->pi_hidden;
    if (G > 0) n += Hp * HC + Hp + G * Hp + G + 2 * G;     // pi_global: Linear, Linear, LayerNorm (neural_net.py:421-426)
  } else if (var.pi_fc_layers > 0) {
    const size_t Hp = d->pi_hidden, L = var.pi_fc_layers;
    n += Hp * HC * HW + Hp + (L - 1) * (Hp * Hp + Hp) + static_cast<size_t>(d->num_moves) * Hp + d->num_moves;
  } else n += static_cast<size_t>(d->num_moves) * HC * HW + d->num_moves;
  return n;
}

}  // namespace

namespace azmi_f32 {

size_t blob_bytes(const azmi_net_desc* d, bool dense, Variant var) { return count_floats(d, dense, var) * sizeof(float); }

void dims(void* impl, uint32_t* chw, uint32_t* p1, uint32_t* m) {
  const azmi_net_desc& d = static_cast<Net*>(impl)->d;
  *chw = d.in_channels * d.height * d.width; *p1 = d.num_players + 1; *m = d.num_moves;
}

void destroy(void* impl) {
  auto* n = static_cast<Net*>(impl);
  if (!n) return;
  (void)hipSetDevice(n->device);
  if (n->blob) (void)hipFree(n->blob);
  for (float* p : n->buf) if (p) (void)hipFree(p);
  for (float* p : n->small) if (p) (void)hipFree(p);
  if (n->stats) (void)hipFree(n->stats);
  delete n;
}

int reserve(void* impl, uint32_t batch, const char** err) {
  auto* n = static_cast<Net*>(impl);
  if (batch <= n->rows) return AZMI_OK;
  if (hipSetDevice(n->device) != hipSuccess) return fail(err, AZMI_ERR_NO_DEVICE, "hipSetDevice failed");
  (void)hipDeviceSynchronize();
  for (float*& p : n->buf) { if (p) (void)hipFree(p); p = nullptr; }
  for (float*& p : n->small) { if (p) (void)hipFree(p); p = nullptr; }
  if (n->stats) { (void)hipFree(n->stats); n->stats = nullptr; }
  n->rows = 0;
  const size_t HW = static_cast<size_t>(n->d.height) * n->d.width;
  // the widest [rows][c][HW] activation: trunk (a dense one: all features, or the 4G bottleneck), heads, or the spatial
  // policy block [policy_channels][HW] (it may be the widest)
  const size_t trunk = n->dense ? std::max<size_t>(trunk_out(&n->d, true), 4 * static_cast<size_t>(n->d.channels)) : static_cast<size_t>(n->d.channels);
  const size_t CH = std::max<size_t>(std::max<size_t>(trunk, n->d.head_channels), std::max(n->d.policy_channels, 0));
  const size_t wide = std::max<size_t>(std::max<size_t>(std::max<size_t>(std::max<size_t>(n->d.v_hidden, n->d.pi_hidden), n->d.num_moves), n->d.head_channels),
                                       n->d.num_players + 1);
  for (float*& p : n->buf)
    if (hipMalloc(reinterpret_cast<void**>(&p), static_cast<size_t>(batch) * CH * HW * sizeof(float)) != hipSuccess)
      return fail(err, AZMI_ERR_OOM, "hipMalloc(fp32 activations) failed");
  for (float*& p : n->small)
    if (hipMalloc(reinterpret_cast<void**>(&p), static_cast<size_t>(batch) * wide * sizeof(float)) != hipSuccess)
      return fail(err, AZMI_ERR_OOM, "hipMalloc(fp32 head vectors) failed");
  // (crelu's 2 * C channels are never materialised: no wider activation.)  The per-sample statistics, up front with the rest:
  if (n->var.trunk_norm && hipMalloc(reinterpret_cast<void**>(&n->stats), static_cast<size_t>(batch) * 2 * sizeof(float)) != hipSuccess)
    return fail(err, AZMI_ERR_OOM, "hipMalloc(fp32 per-sample statistics) failed");
  n->rows = batch;
  return AZMI_OK;
}

int create(const azmi_net_desc* d, bool dense, const void* blob, size_t bytes, int device, void** impl, const char** err, Variant var) {
  const int K = d->kernel_size;
  if (d->channels < 1 || (!dense && K != 3)) return fail(err, AZMI_ERR_INVALID, "fp32 leaf net: 3x3 convolutions only (a dense trunk: 1, 3, 5 or 7)");
  if (K != 1 && K != 3 && K != 5 && K != 7) return fail(err, AZMI_ERR_INVALID, "fp32 leaf net: a dense trunk takes kernel_size 1, 3, 5 or 7");
  if (dense && d->depth < 1) return fail(err, AZMI_ERR_INVALID, "fp32 leaf net: a dense trunk needs at least one block");
  if (d->in_channels < 1 || d->height < 1 || d->width < 1 || d->depth < 0 || d->v_hidden < 1 || d->num_moves < 1 || d->num_players < 0)
    return fail(err, AZMI_ERR_INVALID, "fp32 leaf net: sizes out of range");
  if (d->head_channels < 1 || d->v_fc_layers < 1 || d->v_head_convs < 0 || d->pi_head_convs < 0)
    return fail(err, AZMI_ERR_INVALID, "fp32 leaf net: head sizes out of range");
  if (d->policy_channels > 0 && d->policy_channels * d->height * d->width > d->num_moves)
    return fail(err, AZMI_ERR_INVALID, "fp32 leaf net: the spatial block exceeds num_moves");
  if (d->policy_channels > 0 && d->policy_channels * d->height * d->width < d->num_moves && d->pi_hidden < 1)
    return fail(err, AZMI_ERR_INVALID, "fp32 leaf net: global actions need pi_hidden");
  if (var.trunk_norm < 0 || var.trunk_norm > 1 || var.trunk_act < 0 || var.trunk_act > 1 || var.pi_fc_layers < 0)
    return fail(err, AZMI_ERR_INVALID, "fp32 leaf net: trunk_norm 0 / 1, trunk_act 0 / 1, pi_fc_layers >= 0");
  if (var.pi_fc_layers > 0 && (d->policy_channels > 0 || d->pi_hidden < 1))
    return fail(err, AZMI_ERR_INVALID, "fp32 leaf net: pi_fc_layers > 0 is the flat policy head's FC stack and needs pi_hidden");
  if (bytes != blob_bytes(d, dense, var)) { char b[128]; snprintf(b, sizeof b, "fp32 weight blob is %zu bytes, expected %zu", bytes, blob_bytes(d, dense, var)); return fail(err, AZMI_ERR_INVALID, b); }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(err, AZMI_ERR_NO_DEVICE, "no HIP device: libazmi has no CPU path");
  if (hipSetDevice(device) != hipSuccess) return fail(err, AZMI_ERR_NO_DEVICE, "hipSetDevice failed");
  auto* n = new Net();
  n->d = *d; n->dense = dense; n->device = device; n->var = var;
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&n->blob), bytes);
  if (e != hipSuccess) { delete n; return fail(err, AZMI_ERR_OOM, "hipMalloc(weights)", e); }
  e = hipMemcpy(n->blob, blob, bytes, hipMemcpyHostToDevice);
  if (e != hipSuccess) { destroy(n); return fail(err, AZMI_ERR_NO_DEVICE, "weight upload", e); }
  const int rc = reserve(n, 4096, err);   // up front: forward() may run under stream capture
  if (rc != AZMI_OK) { destroy(n); return rc; }
  *impl = n;
  return AZMI_OK;
}

}  // namespace azmi_f32

namespace {

// One batch through the net: the launches forward() and trunk_features() share.  trunk() runs the stem and the trunk layer by layer
// and leaves the output of nnet.conv_layers, [B][CF][HW], in `s` (t and u are free again); heads() reads it.
struct Pass {
  Net* n;
  const azmi_net_desc& d;
  const float* canon;
  uint32_t B;
  hipStream_t st;
  const int CH, KK, CF, H, W, HW;
  const float* p;            // the next weight of the blob
  float *s, *t, *u;
  Pass(Net* net, const float* canonical, uint32_t batch, void* stream)
      : n(net), d(net->d), canon(canonical), B(batch), st(static_cast<hipStream_t>(stream)), CH(d.channels), KK(d.kernel_size * d.kernel_size),
        CF(static_cast<int>(trunk_out(&d, net->dense))), H(d.height), W(d.width), HW(d.height * d.width), p(net->blob), s(net->buf[0]),
        t(net->buf[1]), u(net->buf[2]) {}
  const float* take(size_t count) { const float* q = p; p += count; return q; }
  // `at`: {channels per row of in, channels per row of out, first output channel}; the default is a dense [B][c][HW] on both sides
  struct At { int in_ctot, out_ctot, out_coff; };
  void convk(const float* in, const float* w, const float* b, const float* pa, const float* pb, const float* res, float* out, int cin, int cout, int relu,
             At at = At{0, 0, 0}) {
    if (at.in_ctot == 0) at = At{cin, cout, 0};
    const size_t total = static_cast<size_t>(B) * cout * HW;
    const uint32_t grid = static_cast<uint32_t>((total + 255) / 256);
    switch (d.kernel_size) {
      case 1: k_conv<1><<<grid, 256, 0, st>>>(in, w, b, pa, pb, res, out, B, cin, cout, H, W, relu, at.in_ctot, at.out_ctot, at.out_coff); break;
      case 3: k_conv<3><<<grid, 256, 0, st>>>(in, w, b, pa, pb, res, out, B, cin, cout, H, W, relu, at.in_ctot, at.out_ctot, at.out_coff); break;
      case 5: k_conv<5><<<grid, 256, 0, st>>>(in, w, b, pa, pb, res, out, B, cin, cout, H, W, relu, at.in_ctot, at.out_ctot, at.out_coff); break;
      default: k_conv<7><<<grid, 256, 0, st>>>(in, w, b, pa, pb, res, out, B, cin, cout, H, W, relu, at.in_ctot, at.out_ctot, at.out_coff); break;
    }
  }
  void conv1(const float* in, const float* w, const float* b, const float* pa, const float* pb, float* out, int cin, int cout, int relu, int in_ctot) {
    const size_t total = static_cast<size_t>(B) * cout * HW;
    k_conv<1><<<static_cast<uint32_t>((total + 255) / 256), 256, 0, st>>>(in, w, b, pa, pb, nullptr, out, B, cin, cout, H, W, relu, in_ctot, cout, 0);
  }
  void fc(const float* in, const float* w, const float* b, float* out, int K, int N, int relu) {
    const size_t total = static_cast<size_t>(B) * N;
    k_fc<<<static_cast<uint32_t>((total + 255) / 256), 256, 0, st>>>(in, w, b, out, B, K, N, relu);
  }
  // a trunk convolution of a variant: act(norm(in)) through w (+ bias) (+ res); k = 1 or the net's kernel size
  void convv(int k, const float* in, const float* w, const float* b, const float* g, const float* beta, const float* stats, const float* res,
             float* out, int cin, int cout, At at) {
    const bool crelu = n->var.trunk_act != 0;
    const size_t total = static_cast<size_t>(B) * cout * HW;
    const uint32_t grid = static_cast<uint32_t>((total + 255) / 256);
#define AZMI_CONV_V(KS) \
    if (crelu) k_conv_v<KS, true><<<grid, 256, 0, st>>>(in, w, b, g, beta, stats, res, out, B, cin, cout, H, W, at.in_ctot, at.out_ctot, at.out_coff); \
    else k_conv_v<KS, false><<<grid, 256, 0, st>>>(in, w, b, g, beta, stats, res, out, B, cin, cout, H, W, at.in_ctot, at.out_ctot, at.out_coff)
    switch (k) {
      case 1: AZMI_CONV_V(1); break;
      case 3: AZMI_CONV_V(3); break;
      case 5: AZMI_CONV_V(5); break;
      default: AZMI_CONV_V(7); break;
    }
#undef AZMI_CONV_V
  }
  void row_stats(const float* in, int channels, int ctot) {   // over the first `channels` of rows that hold ctot
    k_row_stats<<<(B + 3) / 4, 256, 0, st>>>(in, n->stats, B, static_cast<uint32_t>(channels * HW), static_cast<size_t>(ctot) * HW);
  }
  void trunk();
  void heads(float* v_out, float* pi_out);
};

void Pass::trunk() {
  const bool layer = n->var.trunk_norm != 0, crelu = n->var.trunk_act != 0;
  const int A = crelu ? 2 : 1;
  if (!layer && !crelu) {      // the image and the launches of the first descriptor
    if (n->dense) {  // s = every feature [B][CF][HW]: the planes, then G channels per block
      const uint32_t chw = static_cast<uint32_t>(d.in_channels * HW);
      k_copy_planes<<<static_cast<uint32_t>((static_cast<size_t>(B) * chw + 255) / 256), 256, 0, st>>>(canon, s, B, chw, static_cast<uint32_t>(CF * HW));
      for (int i = 0; i < d.depth; ++i) {  // x = cat(x, conv2(relu(bn2(conv1(relu(bn1(x)))))))
        const int Ci = d.in_channels + CH * i;
        const float* a1 = take(Ci); const float* b1 = take(Ci);
        const float* w1 = take(static_cast<size_t>(4 * CH) * Ci); const float* c1 = take(4 * CH);
        const float* w2 = take(static_cast<size_t>(CH) * 4 * CH * KK);
        conv1(s, w1, c1, a1, b1, t, Ci, 4 * CH, 1, CF);
        convk(t, w2, nullptr, nullptr, nullptr, nullptr, s, 4 * CH, CH, 0, At{4 * CH, CF, Ci});
      }
    } else {
      {  // stem
        const float* w = take(static_cast<size_t>(CH) * d.in_channels * KK); const float* b = take(CH);
        convk(canon, w, b, nullptr, nullptr, nullptr, s, d.in_channels, CH, 0);
      }
      for (int i = 0; i < d.depth; ++i) {  // out = conv2(relu(bn2(conv1(relu(bn1(x)))))) + x
        const float* a1 = take(CH); const float* b1 = take(CH);
        const float* w1 = take(static_cast<size_t>(CH) * CH * KK); const float* c1 = take(CH);
        const float* w2 = take(static_cast<size_t>(CH) * CH * KK);
        convk(s, w1, c1, a1, b1, nullptr, t, CH, CH, 1);
        convk(t, w2, nullptr, nullptr, nullptr, s, u, CH, CH, 0);
        float* x = s; s = u; u = x;
      }
    }
  } else if (n->dense) {       // as above; bn1 over the C_i channels the block reads, bn2 over the 4G raw bottleneck channels
    const uint32_t chw = static_cast<uint32_t>(d.in_channels * HW);
    k_copy_planes<<<static_cast<uint32_t>((static_cast<size_t>(B) * chw + 255) / 256), 256, 0, st>>>(canon, s, B, chw, static_cast<uint32_t>(CF * HW));
    for (int i = 0; i < d.depth; ++i) {
      const int Ci = d.in_channels + CH * i;
      const float* g1 = take(Ci); const float* b1 = take(Ci);
      const float* w1 = take(static_cast<size_t>(4 * CH) * A * Ci);
      const float* c1 = layer ? nullptr : take(4 * CH);                       // batch: bn2 folded into conv1
      const float* g2 = layer ? take(4 * CH) : nullptr; const float* b2 = layer ? take(4 * CH) : nullptr;
      const float* w2 = take(static_cast<size_t>(CH) * A * 4 * CH * KK);
      if (layer) row_stats(s, Ci, CF);
      convv(1, s, w1, c1, g1, b1, layer ? n->stats : nullptr, nullptr, t, Ci, 4 * CH, At{CF, 4 * CH, 0});
      if (layer) row_stats(t, 4 * CH, 4 * CH);
      convv(d.kernel_size, t, w2, nullptr, g2, b2, layer ? n->stats : nullptr, nullptr, s, 4 * CH, CH, At{4 * CH, CF, Ci});
    }
  } else {
    {  // stem: batch folds bn1; layer normalises the raw stem in place (no activation behind this norm)
      const float* w = take(static_cast<size_t>(CH) * d.in_channels * KK);
      const float* b = layer ? nullptr : take(CH);
      convk(canon, w, b, nullptr, nullptr, nullptr, s, d.in_channels, CH, 0);
      if (layer) {
        const float* g0 = take(CH); const float* b0 = take(CH);
        row_stats(s, CH, CH);
        const size_t total = static_cast<size_t>(B) * CH * HW;
        k_norm_rows<<<static_cast<uint32_t>((total + 255) / 256), 256, 0, st>>>(s, g0, b0, n->stats, B, CH, HW);
      }
    }
    for (int i = 0; i < d.depth; ++i) {  // the residual is the block's input s
      const float* g1 = take(CH); const float* b1 = take(CH);
      const float* w1 = take(static_cast<size_t>(CH) * A * CH * KK);
      const float* c1 = layer ? nullptr : take(CH);
      const float* g2 = layer ? take(CH) : nullptr; const float* b2 = layer ? take(CH) : nullptr;
      const float* w2 = take(static_cast<size_t>(CH) * A * CH * KK);
      if (layer) row_stats(s, CH, CH);
      convv(d.kernel_size, s, w1, c1, g1, b1, layer ? n->stats : nullptr, nullptr, t, CH, CH, At{CH, CH, 0});
      if (layer) row_stats(t, CH, CH);
      convv(d.kernel_size, t, w2, nullptr, g2, b2, layer ? n->stats : nullptr, s, u, CH, CH, At{CH, CH, 0});
      float* x = s; s = u; u = x;
    }
  }
}

void Pass::heads(float* v_out, float* pi_out) {
  const int HC = d.head_channels, Hd = d.v_hidden, P1 = d.num_players + 1, M = d.num_moves;
  {  // value head
    const float* wv = take(static_cast<size_t>(HC) * CF); const float* bv = take(HC);
    conv1(s, wv, bv, nullptr, nullptr, t, CF, HC, 1, CF);
    float *a = t, *b2 = u;
    for (int i = 0; i < d.v_head_convs; ++i) {
      const float* w = take(static_cast<size_t>(HC) * HC * KK); const float* b = take(HC);
      convk(a, w, b, nullptr, nullptr, nullptr, b2, HC, HC, 1);
      float* x = a; a = b2; b2 = x;
    }
    k_avgpool<<<static_cast<uint32_t>((static_cast<size_t>(B) * HC + 255) / 256), 256, 0, st>>>(a, n->small[0], B, HC, HW);
    float *x0 = n->small[0], *x1 = n->small[1];
    const float* w = take(static_cast<size_t>(Hd) * HC); const float* b = take(Hd);
    fc(x0, w, b, x1, HC, Hd, 1);
    for (int i = 0; i + 1 < d.v_fc_layers; ++i) {
      const float* we = take(static_cast<size_t>(Hd) * Hd); const float* be = take(Hd);
      fc(x1, we, be, x0, Hd, Hd, 1);
      float* x = x0; x0 = x1; x1 = x;
    }
    const float* w2 = take(static_cast<size_t>(P1) * Hd); const float* bb = take(P1);
    fc(x1, w2, bb, x0, Hd, P1, 0);
    k_softmax<<<(B + 3) / 4, 256, 0, st>>>(x0, v_out, B, P1, 0, 0);
  }
  {  // policy head
    const float* wp = take(static_cast<size_t>(HC) * CF); const float* bp = take(HC);
    conv1(s, wp, bp, nullptr, nullptr, t, CF, HC, 1, CF);
    float *a = t, *b2 = u;
    for (int i = 0; i < d.pi_head_convs; ++i) {
      const float* w = take(static_cast<size_t>(HC) * HC * KK); const float* b = take(HC);
      convk(a, w, b, nullptr, nullptr, nullptr, b2, HC, HC, 1);
      float* x = a; a = b2; b2 = x;
    }
    if (d.policy_channels > 0) {
      const int PC = d.policy_channels;
      const float* w = take(static_cast<size_t>(PC) * HC); const float* b = take(PC);
      conv1(a, w, b, nullptr, nullptr, b2, HC, PC, 0, HC);             // [B][PC][HW]
      const int G = M - PC * HW;
      if (G > 0) {   // pi_global over the average-pooled policy features (head_pool), neural_net.py:413-426, 486-493
        const int Hp = d.pi_hidden;
        k_avgpool<<<static_cast<uint32_t>((static_cast<size_t>(B) * HC + 255) / 256), 256, 0, st>>>(a, n->small[0], B, HC, HW);
        const float* w1 = take(static_cast<size_t>(Hp) * HC); const float* c1 = take(Hp);
        fc(n->small[0], w1, c1, n->small[1], HC, Hp, 1);
        const float* w2 = take(static_cast<size_t>(G) * Hp); const float* c2 = take(G);
        fc(n->small[1], w2, c2, n->small[0], Hp, G, 0);
        const float* lg = take(G); const float* lb = take(G);
        k_layernorm<<<(B + 63) / 64, 64, 0, st>>>(n->small[0], lg, lb, n->small[1], B, G);
        k_softmax<<<(B + 3) / 4, 256, 0, st>>>(b2, pi_out, B, M, PC, HW, n->small[1], G);
      } else
      k_softmax<<<(B + 3) / 4, 256, 0, st>>>(b2, pi_out, B, M, PC, HW);  // permuted to [HW][PC] on the fly
    } else if (n->var.pi_fc_layers > 0) {   // pi_fc1 - ReLU - (pi_fc_extra: Linear - ReLU)* - pi_fc_out
      const int Hp = d.pi_hidden;
      float *x0 = n->small[0], *x1 = n->small[1];
      const float* w = take(static_cast<size_t>(Hp) * HC * HW); const float* b = take(Hp);
      fc(a, w, b, x0, HC * HW, Hp, 1);
      for (int l = 0; l + 1 < n->var.pi_fc_layers; ++l) {
        const float* we = take(static_cast<size_t>(Hp) * Hp); const float* be = take(Hp);
        fc(x0, we, be, x1, Hp, Hp, 1);
        float* x = x0; x0 = x1; x1 = x;
      }
      const float* wo = take(static_cast<size_t>(M) * Hp); const float* bo = take(M);
      fc(x0, wo, bo, x1, Hp, M, 0);
      k_softmax<<<(B + 3) / 4, 256, 0, st>>>(x1, pi_out, B, M, 0, 0);
    } else {
      const float* w = take(static_cast<size_t>(M) * HC * HW); const float* b = take(M);
      fc(a, w, b, n->small[0], HC * HW, M, 0);                         // flatten order (c, h, w) = the buffer's
      k_softmax<<<(B + 3) / 4, 256, 0, st>>>(n->small[0], pi_out, B, M, 0, 0);
    }
  }
}

}  // namespace

namespace azmi_f32 {

int forward(void* impl, const float* canon, float* v_out, float* pi_out, uint32_t B, void* stream, const char** err) {
  auto* n = static_cast<Net*>(impl);
  if (B > n->rows) { const int rc = reserve(n, B, err); if (rc != AZMI_OK) return rc; }
  Pass pass(n, canon, B, stream);
  pass.trunk();
  pass.heads(v_out, pi_out);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(err, AZMI_ERR_NO_DEVICE, "fp32 leaf net launch", e);
  return AZMI_OK;
}

uint32_t trunk_channels(void* impl) {
  auto* n = static_cast<Net*>(impl);
  return static_cast<uint32_t>(trunk_out(&n->d, n->dense));
}

int trunk_features(void* impl, const float* canon, float* feat_out, uint32_t B, void* stream, const char** err) {
  auto* n = static_cast<Net*>(impl);
  if (B > n->rows) { const int rc = reserve(n, B, err); if (rc != AZMI_OK) return rc; }
  Pass pass(n, canon, B, stream);
  pass.trunk();
  // feats.mean(dim=(2, 3)): one thread per (row, channel) adds the HW cells in ascending order (k_avgpool, as the heads pool)
  k_avgpool<<<static_cast<uint32_t>((static_cast<size_t>(B) * pass.CF + 255) / 256), 256, 0, pass.st>>>(pass.s, feat_out, B, pass.CF, pass.HW);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(err, AZMI_ERR_NO_DEVICE, "fp32 leaf net trunk launch", e);
  return AZMI_OK;
}

}  // namespace azmi_f32
