// The x-transformers Encoder stack that CLVP's towers (clvp.hip) and CVVP's CollapsingTransformers (cvvp.hip) share
// (reference: tortoise/models/xtransformers.py:731-1013 as built at clvp.py:54-83 / cvvp.py:23-35): per layer pre-RMSNorm ->
// bias-free q / k / v -> rotary on the first rot_dim dims of q, k AND v -> softmax(q k^T / 8) v -> to_out + residual; pre-RMSNorm ->
// GEGLU feed-forward (value * gelu(gate) formed in the projection's epilogue) -> residual.  Token-major f32 residual stream.
#pragma once
#include "stage_blocks.h"

namespace tt {

struct XencBufs {
  float* x;    // [M][D] f32 residual stream (in / out)
  void* h;     // [M][D] T normalised rows
  void* gg;    // [M][inner] T GEGLU output
  void* attn;  // [M][D] T attention output
  void* q;     // flash layouts
  void* k;
  void* vt;
  int* guard;  // operand-overflow counter of the stage
};

static inline int xenc_layers_run(int dt, const XencBufs& b, const tt_clvp_layer* layers, int depth, const float* inv_freq, int D, int H, int inner,
                                  int rot_dim, int B, int n, hipStream_t s) {
  const int M = B * n;
  HeadsAttnOpts rotary;
  rotary.inv_freq = inv_freq; rotary.rot_dim = rot_dim;
  for (int l = 0; l < depth; ++l) {
    const tt_clvp_layer& w = layers[l];
    TT_TRY(rownorm_launch(dt, rmsnorm_args(b.x, M, D, w.attn_norm_g, 1e-8f, b.h, b.guard), s));
    TT_TRY(heads_attention(dt, b.h, w.w_qkv, nullptr, b.q, b.k, b.vt, b.attn, B, n, D, H, s, rotary));
    TT_TRY(gemm_launch(dt, EPI_STD, gemm_residual_args(b.attn, D, w.w_out, D, M, D, D, w.b_out, b.x, b.x), s));
    TT_TRY(rownorm_launch(dt, rmsnorm_args(b.x, M, D, w.ff_norm_g, 1e-8f, b.h, b.guard), s));
    // GEGLU (xtransformers.py:429-437): value * gelu(gate) formed in the projection's epilogue (value / gate rows interleaved at pack
    // time) - the [M][2 inner] projection (315 MB at 256 candidates x 200 codes of CLVP) is never written or re-read
    GemmArgs g = gemm_args(b.h, D, w.w_ff1, D, M, 2 * inner, D);
    g.bias = w.b_ff1; g.out_t = b.gg; g.ldot = inner;
    TT_TRY(gemm_launch(dt, EPI_GEGLU, g, s));
    TT_TRY(gemm_launch(dt, EPI_STD, gemm_residual_args(b.gg, inner, w.w_ff2, inner, M, D, inner, w.b_ff2, b.x, b.x), s));
  }
  return 0;
}

}  // namespace tt
