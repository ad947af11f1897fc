// The Connect4-family leaf net as host code sees it: its description, the device pointers into its folded weights and the view of a
// net object that the engine's fused launch and the pipeline take.  No device code: host-only translation units include this
// instead of leafnet_c4.h.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace azmi_net_dev {

struct NetDesc {
  int C_in, H, W, depth, num_moves, num_players, v_hidden;
};

struct NetPtrs {           // device pointers into the folded weight blob
  const uint8_t* stem_w;   // [2 ks][4 mt] fragments
  const float* stem_b;     // [64]
  const uint8_t* blocks;   // per block: a1[64] b1[64] c1[64] (fp32) | conv1 frags | conv2 frags
  const uint8_t* head_w;   // [2 ks][4 mt] fragments (rows 0-31 value conv, 32-63 policy conv)
  const float* head_b;     // [64]
  const float* v_fc1_w;    // f32 A-fragments [v_hidden / 16][2][64 lanes][4] (hip_net._f32_frags)
  const float* v_fc1_b;    // [v_hidden]
  const float* v_fc2_w;    // [P+1][v_hidden]
  const float* v_fc2_b;    // [P+1]
  const uint8_t* pi_fc_w;  // per pixel position p: bf16 A-fragment of W_p[m][c] = W[m][c*H*W + p] (rows >= M zero), high parts, then low parts
  const float* pi_fc_b;    // [M]
};

}  // namespace azmi_net_dev

// the Connect4-family net behind the C ABI as its launches need it (leafnet_c4_host.hip fills it; engine.hip and the pipeline
// read nd / np / lds_bytes for their fused launches)
struct azmi_net_c4_view {
  azmi_net_dev::NetDesc nd;
  azmi_net_dev::NetPtrs np;
  size_t lds_bytes;
  int x3;                 // the bf16x3 tier (split bf16 operands, Tile<.., SPLIT>): one workgroup per CU; only the pipeline runs it through a view
};
// fills `out` when `net` is a Connect4-family net on the matrix cores (bf16, or bf16x3: out->x3 - the lock-step engine's fused
// launch takes the bf16 tile only and checks the flag); returns 0 otherwise
extern "C" int azmi_net_c4_view_get(const struct azmi_net* net, azmi_net_c4_view* out);
// allocates the per-stream scratch a forward of up to `max_rows` rows on `stream` needs (a forward allocates it on first use,
// which a stream capture does not allow); 0 = ok
extern "C" int azmi_net_reserve_stream(struct azmi_net* net, void* stream, uint32_t max_rows);
