// fp32 reference-precision path of the leaf net (csrc/leafnet_f32.hip): same architecture family as the
// MFMA kernels, plain fp32 arithmetic, for the 1e-5 parity tier.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/azmi.h"

namespace azmi_f32 {
// dense: DenseNet trunk (azmi_net_desc2::dense_net), d->channels = the growth rate.  Bounds: kernel_size 3 (a dense trunk: 1 / 3 / 5 / 7), pooled
// heads, any widths and depth (a dense trunk: depth >= 1); everything else is refused by name.
// Variant: the words of azmi_net_desc2 behind dense_net - trunk_norm (0 batch, 1 layer = GroupNorm(1, C)), trunk_act (0 relu, 1 crelu),
// pi_fc_layers (hidden layers of the flat policy head, d->pi_hidden wide).  All zero: the image and the launches of the first descriptor.
struct Variant { int trunk_norm = 0, trunk_act = 0, pi_fc_layers = 0; };
size_t blob_bytes(const azmi_net_desc* d, bool dense, Variant var = Variant{});
// returns AZMI_OK or a negative status; *err receives a static/thread-local message
int create(const azmi_net_desc* d, bool dense, const void* blob, size_t bytes, int device, void** impl, const char** err, Variant var = Variant{});
int forward(void* impl, const float* canon, float* v, float* pi, uint32_t batch, void* stream, const char** err);
// the trunk read-out: CF = the channels the heads read (a dense trunk: every feature, the input planes first), and
// feat[b][c] = the mean over the H*W cells of the trunk's output - forward()'s stem and trunk launches, none of the heads'
uint32_t trunk_channels(void* impl);
int trunk_features(void* impl, const float* canon, float* feat, uint32_t batch, void* stream, const char** err);
int reserve(void* impl, uint32_t batch, const char** err);
void destroy(void* impl);
void dims(void* impl, uint32_t* chw, uint32_t* p1, uint32_t* m);   // floats per canonical row, P+1, M
}  // namespace azmi_f32
