// Process-level and operator-level C-ABI entry points (include/tortoise_mi355x.h).
#include "runtime.h"
#include "../../include/tortoise_mi355x.h"
#include "../../include/tortoise_mi355x_test.h"

using namespace tt;
namespace tt { extern bool g_flash32; extern bool g_voc_mfma; extern bool g_gemm_p8; extern bool g_gemm_skinny; extern int g_ar_gemv; extern bool g_nr_select_long; }  // attention.hip, univnet.hip, gemm.hip, gpt2.hip, denoise.hip

extern "C" {

const char* tt_last_error(void) { return tt::last_error(); }
int tt_abi_version(void) { return 6; }  // ABI changes

int tt_init(void) {
  int dev = 0;
  TT_CHECK_HIP(hipGetDevice(&dev));
  hipDeviceProp_t prop;
  TT_CHECK_HIP(hipGetDeviceProperties(&prop, dev));
  TT_REQUIRE(strncmp(prop.gcnArchName, "gfx950", 6) == 0, "tt_init: device is %s; this engine is built for gfx950 (MI355X) only", prop.gcnArchName);
  return gemm_init();
}

// the one argument mapping of the operator-level GEMM entries
static GemmArgs gemm_desc_args(const tt_op_gemm_desc& d) {
  GemmArgs g = gemm_args(d.A, d.lda, d.W, d.ldw, d.M, d.N, d.K);
  g.A2 = d.A2; g.lda2 = d.lda2; g.k_split = d.k_split; g.a2_slot = d.a2_slot; g.a2_slot_stride = d.a2_slot_stride;
  g.taps = d.taps; g.dilation = d.dilation; g.seq_len = d.seq_len > 0 ? d.seq_len : d.M; g.seq_vlen = d.seq_vlen; g.splitk = d.splitk; g.serial_k = d.serial_k;
  g.bias = d.bias; g.act = d.act; g.slope = d.slope; g.res = d.res; g.ldres = d.ldres > 0 ? d.ldres : d.N;
  g.out_f32 = d.out_f32; g.ldo32 = d.ldo32 > 0 ? d.ldo32 : d.N; g.out_t = d.out_t; g.ldot = d.ldot > 0 ? d.ldot : d.N;
  g.act_t = d.act_t; g.slope_t = d.slope_t;
  g.gn_part = d.gn_part; g.gn_seq = d.gn_seq; g.gn_vperiod = d.gn_vperiod;
  for (int i = 0; i < 32; ++i) g.gn_vlen[i] = d.gn_vlen[i];
  g.dmodel = d.dmodel; g.heads = d.heads; g.q = d.q; g.k = d.k; g.v = d.v; g.vt = d.vt; g.seq_pad = d.seq_pad; g.q_scale = d.q_scale != 0.f ? d.q_scale : 1.f;
  g.step = d.step; g.qbuf = d.qbuf; g.kc = d.kc; g.vc = d.vc; g.tmax = d.tmax;
  return g;
}

static tt_op_gemm_desc gemm_desc_std(const void* A, int lda, const void* W, int ldw, int M, int N, int K, int taps, int seq_len, const float* bias, int act,
                                     const float* res, float* out_f32, void* out_t) {
  tt_op_gemm_desc d;
  memset(&d, 0, sizeof(d));
  d.A = A; d.lda = lda; d.W = W; d.ldw = ldw; d.M = M; d.N = N; d.K = K; d.taps = taps; d.seq_len = seq_len; d.splitk = 1; d.q_scale = 1.f;
  d.bias = bias; d.act = act; d.slope = 0.2f; d.res = res; d.out_f32 = out_f32; d.out_t = out_t;
  return d;
}

size_t tt_op_gemm_desc_size(void) { return sizeof(tt_op_gemm_desc); }

int tt_op_gemm_ex(int dtype, int epi, const tt_op_gemm_desc* d, int* ran, void* stream) {
  TT_REQUIRE(d != nullptr, "tt_op_gemm_ex: null descriptor");
  const int rc = gemm_launch(dtype, epi, gemm_desc_args(*d), (hipStream_t)stream);
  if (ran) {
    ran[0] = g_gemm_ran.tile; ran[1] = g_gemm_ran.variant; ran[2] = g_gemm_ran.p8; ran[3] = g_gemm_ran.conv3s;
  }
  return rc;
}

int tt_op_gemm_stat_rows(int dtype, const tt_op_gemm_desc* d) {
  TT_REQUIRE(d != nullptr, "tt_op_gemm_stat_rows: null descriptor");
  return gemm_stat_rows(gemm_desc_args(*d), dtype);
}

int tt_op_gemm(int dtype, const void* A, int lda, const void* W, int ldw, int M, int N, int K, int taps, int seq_len, int splitk,
               const float* bias, int act, const float* res, float* out_f32, void* out_t, void* stream) {
  tt_op_gemm_desc d = gemm_desc_std(A, lda, W, ldw, M, N, K, taps, seq_len, bias, act, res, out_f32, out_t);
  d.splitk = splitk;
  return gemm_launch(dtype, EPI_STD, gemm_desc_args(d), (hipStream_t)stream);
}

int tt_op_gemm_segv(int dtype, const void* A, int lda, const void* W, int ldw, int M, int N, int K, int taps, int dilation, int seq_len,
                    const int* seq_vlen, const float* bias, int act, const float* res, float* out_f32, void* out_t, void* stream) {
  TT_REQUIRE(seq_vlen != nullptr, "tt_op_gemm_segv: seq_vlen is required");
  tt_op_gemm_desc d = gemm_desc_std(A, lda, W, ldw, M, N, K, taps, seq_len, bias, act, res, out_f32, out_t);
  d.dilation = dilation; d.seq_vlen = seq_vlen;
  return gemm_launch(dtype, EPI_STD, gemm_desc_args(d), (hipStream_t)stream);
}

// the one argument mapping of the operator-level row-norm entries
static RowNormArgs rownorm_desc_args(const tt_op_rownorm_desc& d) {
  RowNormArgs a;
  memset(&a, 0, sizeof(a));
  a.x = d.x; a.ldx = d.ldx; a.x_in = d.x_in; a.ldxin = d.ldxin; a.M = d.M; a.D = d.D;
  a.add_bias = d.add_bias; a.add_slabs = d.add_slabs; a.nslab = d.nslab; a.slab_stride = d.slab_stride; a.ldslab = d.ldslab; a.write_x = d.write_x;
  a.mode = d.mode; a.g1 = d.g1; a.b1 = d.b1; a.eps1 = d.eps1; a.g2 = d.g2; a.b2 = d.b2; a.eps2 = d.eps2;
  a.out_t = d.out_t; a.ldot = d.ldot; a.out_f32 = d.out_f32; a.ldo32 = d.ldo32;
  a.f32_slot = d.f32_slot; a.f32_slot_base = d.f32_slot_base; a.f32_slot_stride = d.f32_slot_stride; a.f32_row_slot = d.f32_row_slot;
  a.row_blocks = d.row_blocks; a.guard = d.guard; a.act = d.act;
  return a;
}

size_t tt_op_rownorm_desc_size(void) { return sizeof(tt_op_rownorm_desc); }

int tt_op_rownorm_ex(int dtype, const tt_op_rownorm_desc* d, int* ran, void* stream) {
  TT_REQUIRE(d != nullptr, "tt_op_rownorm_ex: null descriptor");
  const int rc = rownorm_launch(dtype, rownorm_desc_args(*d), (hipStream_t)stream);
  if (ran) {
    ran[0] = g_rownorm_ran.kernel; ran[1] = g_rownorm_ran.nslab; ran[2] = g_rownorm_ran.bias; ran[3] = g_rownorm_ran.rms;
  }
  return rc;
}

static tt_op_rownorm_desc rownorm_desc_std(const float* x, int M, int D, const float* g, const float* b, float eps, void* out_t, float* out_f32) {
  tt_op_rownorm_desc d;
  memset(&d, 0, sizeof(d));
  d.x = (float*)x; d.ldx = D; d.M = M; d.D = D; d.mode = NORM_LAYER; d.g1 = g; d.b1 = b; d.eps1 = eps;
  d.out_t = out_t; d.ldot = D; d.out_f32 = out_f32; d.ldo32 = D;
  return d;
}

int tt_op_layernorm(int dtype, const float* x, int M, int D, const float* g, const float* b, float eps, int rms, void* out_t,
                    float* out_f32, void* stream) {
  tt_op_rownorm_desc d = rownorm_desc_std(x, M, D, g, b, eps, out_t, out_f32);
  d.mode = rms ? NORM_RMS : NORM_LAYER;
  return tt_op_rownorm_ex(dtype, &d, nullptr, stream);
}

// row LayerNorm + activation in one launch (the wav2vec2 feature encoder's LayerNorm + GELU, csrc/align.hip)
int tt_op_layernorm_act(int dtype, const float* x, int M, int D, const float* g, const float* b, float eps, int act, void* out_t, float* out_f32,
                        void* stream) {
  tt_op_rownorm_desc d = rownorm_desc_std(x, M, D, g, b, eps, out_t, out_f32);
  d.act = act;
  return tt_op_rownorm_ex(dtype, &d, nullptr, stream);
}

size_t tt_op_groupnorm_workspace(int B, int S) { return groupnorm_partial_floats(B, S) * sizeof(float); }

// the one argument mapping of the operator-level GroupNorm entries
static GroupNormArgs groupnorm_desc_args(const tt_op_groupnorm_desc& d) {
  GroupNormArgs a;
  memset(&a, 0, sizeof(a));
  a.x = d.x; a.B = d.B; a.S = d.S; a.C = d.C; a.gamma = d.gamma; a.beta = d.beta; a.eps = d.eps;
  a.scale_shift = d.scale_shift; a.ss_batch_stride = d.ss_batch_stride; a.ss_batch_div = d.ss_batch_div; a.act = d.act;
  a.out_t = d.out_t; a.ldot = d.ldot; a.out_f32 = d.out_f32; a.ldo32 = d.ldo32; a.partial = d.partial;
  a.gemm_part = d.gemm_part; a.part_rows = d.part_rows; a.vperiod = d.vperiod;
  for (int i = 0; i < 32; ++i) a.vlen[i] = d.vlen[i];
  a.guard = d.guard;
  return a;
}

static tt_op_groupnorm_desc groupnorm_desc_std(const float* x, int B, int S, int C, const float* g, const float* b, const float* scale_shift, int act,
                                               void* out_t, float* out_f32, float* workspace) {
  tt_op_groupnorm_desc d;
  memset(&d, 0, sizeof(d));
  d.x = x; d.B = B; d.S = S; d.C = C; d.gamma = g; d.beta = b; d.eps = 1e-5f; d.scale_shift = scale_shift;
  d.ss_batch_stride = 2 * (size_t)C; d.act = act; d.out_t = out_t; d.ldot = C; d.out_f32 = out_f32; d.ldo32 = C; d.partial = workspace;
  return d;
}

size_t tt_op_groupnorm_desc_size(void) { return sizeof(tt_op_groupnorm_desc); }

int tt_op_groupnorm_ex(int dtype, const tt_op_groupnorm_desc* d, int* ran, void* stream) {
  TT_REQUIRE(d != nullptr && d->vperiod >= 0 && d->vperiod <= 32, "tt_op_groupnorm_ex: null descriptor or vperiod outside 0 .. 32");
  const int rc = groupnorm_launch(dtype, groupnorm_desc_args(*d), (hipStream_t)stream);
  if (ran) {
    ran[0] = g_groupnorm_ran.stats; ran[1] = g_groupnorm_ran.apply; ran[2] = g_groupnorm_ran.rows; ran[3] = g_groupnorm_ran.fused;
  }
  return rc;
}

int tt_op_groupnorm(int dtype, const float* x, int B, int S, int C, const float* g, const float* b, const float* scale_shift, int act,
                    void* out_t, float* out_f32, float* workspace, void* stream) {
  const tt_op_groupnorm_desc d = groupnorm_desc_std(x, B, S, C, g, b, scale_shift, act, out_t, out_f32, workspace);
  return tt_op_groupnorm_ex(dtype, &d, nullptr, stream);
}

int tt_op_groupnorm_part(int dtype, const float* x, int B, int S, int C, const float* g, const float* b, const float* scale_shift, int act,
                         const float* gemm_part, int part_rows, int vperiod, const int* vlen, void* out_t, float* out_f32, float* workspace,
                         void* stream) {
  TT_REQUIRE(gemm_part != nullptr && vperiod >= 0 && vperiod <= 32 && (vperiod == 0 || vlen != nullptr), "tt_op_groupnorm_part: bad arguments");
  for (int i = 0; i < vperiod; ++i) TT_REQUIRE(vlen[i] > 0 && vlen[i] <= S, "tt_op_groupnorm_part: vlen[%d] = %d outside 1 .. S = %d", i, vlen[i], S);
  tt_op_groupnorm_desc d = groupnorm_desc_std(x, B, S, C, g, b, scale_shift, act, out_t, out_f32, workspace);
  d.gemm_part = gemm_part; d.part_rows = part_rows; d.vperiod = vperiod;
  for (int i = 0; i < vperiod; ++i) d.vlen[i] = vlen[i];
  return tt_op_groupnorm_ex(dtype, &d, nullptr, stream);
}

// Test entry of the fused in_layers launch (gemm_gna.h): out_f32[B*S][N] = Linear(act(GroupNorm32(x)))(W, bias) for x f32 [B][S][1024].
// The statistics partials the kernel finalises are normally left by the producing GEMM's epilogue; here a helper kernel writes them in that
// layout (tiles of 32 rows, slot 1 = the rows of a tile that belong to the next sample, strips of 16 channels).
__global__ void gn_gemm_test_partials_kernel(const float* x, int M, int S, int C, float* part) {
  const int t = blockIdx.x, strip = threadIdx.x;  // one block per 32-row tile, one thread per 16-channel strip
  if (strip >= C / 16) return;
  const int b_first = (t * 32) / S, next_start = (b_first + 1) * S;
  float s0 = 0.f, q0 = 0.f, s1 = 0.f, q1 = 0.f;
  for (int r = t * 32; r < min(t * 32 + 32, M); ++r)
    for (int c = strip * 16; c < strip * 16 + 16; ++c) {
      const float v = x[(size_t)r * C + c];
      if (r < next_start) { s0 += v; q0 += v * v; } else { s1 += v; q1 += v * v; }
    }
  float* p = part + (((size_t)t * 2 + 0) * (C / 16) + strip) * 2;
  p[0] = s0; p[1] = q0;
  p = part + (((size_t)t * 2 + 1) * (C / 16) + strip) * 2;
  p[0] = s1; p[1] = q1;
}
size_t tt_op_gn_gemm_workspace(int B, int S) { return ((size_t)(B * S / 32 + 2) * 2 * 64 * 2 + 64) * 2 * sizeof(float); }

int tt_op_gn_gemm(int dtype, const float* x, int B, int S, const float* gamma, const float* beta, int act, const void* W, const float* bias, int N,
                  float* out_f32, float* workspace, void* stream) {
  TT_REQUIRE(x && gamma && beta && W && bias && out_f32 && workspace && B >= 1 && S >= 1, "tt_op_gn_gemm: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  const int C = 1024, M = B * S;
  float* part_in = workspace;
  float* part_out = workspace + ((size_t)(M / 32 + 2) * 2 * 64 * 2 + 64);
  gn_gemm_test_partials_kernel<<<cdiv(M, 32), 64, 0, s>>>(x, M, S, C, part_in);
  TT_CHECK_HIP(hipGetLastError());
  GemmArgs g = gemm_args(x, C, W, C, M, N, C);
  g.bias = bias; g.out_f32 = out_f32; g.ldo32 = N; g.gn_part = part_out; g.gn_seq = S;
  GemmGnArgs n;
  memset(&n, 0, sizeof(n));
  n.gamma = gamma; n.beta = beta; n.gemm_part = part_in; n.part_rows = 32; n.S = S; n.eps = 1e-5f; n.act = act;
  TT_REQUIRE(gemm_gna_supported(dtype, EPI_STD, g, n), "tt_op_gn_gemm: no fused kernel for B=%d S=%d N=%d act=%d dtype=%d (256 < B*S <= 4096, S >= 32, N %% 256 == 0, SiLU, 16-bit operands)", B, S, N, act, dtype);
  return gemm_gna_launch(dtype, EPI_STD, g, n, s);
}

// Process-wide A/B switches of kernel families (include/tortoise_mi355x_test.h; like tt_graph_replay: set them before an engine captures
// its graphs - a kept graph replays the kernels it was captured with).  Returns the previous value.
int ttx_kernel_variant(int which, int v) {
  if (which == TTX_AR_GEMV) {  // a level, not a switch: 0 MFMA tiles | 1 GEMV launches behind the row-norm launches | 2 the layer norms inside the GEMVs
    TT_REQUIRE(v >= 0 && v <= 2, "ttx_kernel_variant(TTX_AR_GEMV): level %d", v);
    const int prev = tt::g_ar_gemv;
    tt::g_ar_gemv = v;
    return prev;
  }
  bool* sw = which == TTX_FLASH32 ? &tt::g_flash32 : which == TTX_GEMM_P8 ? &tt::g_gemm_p8 : which == TTX_VOC_MFMA ? &tt::g_voc_mfma : which == TTX_GEMM_SKINNY ? &tt::g_gemm_skinny : which == TTX_NR_SELECT_LONG ? &tt::g_nr_select_long : nullptr;
  TT_REQUIRE(sw != nullptr, "ttx_kernel_variant: unknown kernel family %d", which);
  const int prev = *sw ? 1 : 0;
  *sw = v != 0;
  return prev;
}

int tt_op_flash_attention_rows(int dtype, const void* q, const void* k, const void* vt, void* out, int B, int heads, int n, int n_pad,
                               int causal, const float* relpos, const int* nv, int nv_period, int variant, void* stream) {
  TT_REQUIRE(nv_period >= 0 && nv_period <= 32 && (nv_period == 0 || nv != nullptr), "tt_op_flash_attention_rows: nv_period %d (0 .. 32, with nv)", nv_period);
  TT_REQUIRE(variant >= 0 && variant <= 2, "tt_op_flash_attention_rows: variant %d", variant);
  FlashArgs f;
  memset(&f, 0, sizeof(f));
  f.q = q; f.k = k; f.vt = vt; f.out = out; f.ldo = heads * 64; f.BH = B * heads; f.heads = heads; f.n = n; f.n_pad = n_pad;
  f.causal = causal; f.relpos = relpos; f.variant = variant;
  f.nv_period = nv_period;
  for (int i = 0; i < nv_period; ++i) {
    TT_REQUIRE(nv[i] >= 1 && nv[i] <= n, "tt_op_flash_attention_rows: nv[%d] = %d outside 1 .. %d", i, nv[i], n);
    f.nv[i] = nv[i];
  }
  return flash_attention_launch(dtype, f, (hipStream_t)stream);
}
int tt_op_flash_attention(int dtype, const void* q, const void* k, const void* vt, void* out, int B, int heads, int n, int n_pad,
                          int causal, const float* relpos, void* stream) {
  return tt_op_flash_attention_rows(dtype, q, k, vt, out, B, heads, n, n_pad, causal, relpos, nullptr, 0, 0, stream);
}
// what the last flash launch of this thread started (ops.h FlashRan)
int tt_op_flash_ran(int ran[3]) {
  TT_REQUIRE(ran != nullptr, "tt_op_flash_ran: null record");
  ran[0] = g_flash_ran.kernel; ran[1] = g_flash_ran.nq; ran[2] = g_flash_ran.ks;
  return 0;
}

// GEMV-shaped decode GEMM (gemv.hip; handles of <= 4 sequences, wide session handles of <= 16): epi 0 = out_f32 = A W^T + bias, 1 = x (out_f32) += A W^T + bias, 2 = out_t = gelu_tanh(A W^T + bias)
int tt_op_gemv(int dtype, const void* A, const void* W, int M, int N, int K, const float* bias, int epi, float* out_f32, void* out_t, void* stream) {
  TT_REQUIRE(epi >= 0 && epi <= 2, "tt_op_gemv: epi %d (the QKV scatter is tested through the engine)", epi);
  GemvArgs v;
  memset(&v, 0, sizeof(v));
  v.A = A; v.lda = K; v.W = W; v.ldw = K; v.M = M; v.N = N; v.K = K; v.bias = bias; v.epi = epi; v.out_f32 = out_f32; v.ldo32 = N; v.out_t = out_t; v.ldot = N;
  return gemv_launch(dtype, v, (hipStream_t)stream);
}
// out_t[M][N] = gelu_tanh(LayerNorm(x[M][1024]; g, b, eps) W^T + bias): the GEMV with the layer norm inside (the decode step's c_fc at <= 4 sequences)
int tt_op_gemv_ln(int dtype, const float* x, const float* g, const float* b, float eps, const void* W, int M, int N, const float* bias, void* out_t, void* stream) {
  GemvArgs v;
  memset(&v, 0, sizeof(v));
  v.ln_x = x; v.ldx = 1024; v.ln_g = g; v.ln_b = b; v.ln_eps = eps; v.W = W; v.ldw = 1024; v.M = M; v.N = N; v.K = 1024; v.bias = bias; v.epi = GEMV_GELU_T; v.out_t = out_t; v.ldot = N;
  return gemv_launch(dtype, v, (hipStream_t)stream);
}

// The decode step's attention (HF GPT2Attention with a KV cache: one query per (sequence, head) over [shared prefix | own keys]) on
// caller-provided caches.  tgen own keys (slots 0 .. tgen - 1) are valid; the device-side step word the kernels read is made here.
int tt_op_decode_attention(int dtype, const void* q, const void* kp, const void* vp, int P1, const void* kc, const void* vc, int tmax, int tgen,
                           void* out, int B, int heads, int variant, void* stream) {
  TT_REQUIRE(q && kp && vp && kc && vc && out && tgen >= 1 && tgen <= tmax, "tt_op_decode_attention: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  int* step = nullptr;
  TT_CHECK_HIP(hipMalloc((void**)&step, sizeof(int)));
  const int newest = tgen - 1;
  TT_CHECK_HIP(hipMemcpyAsync(step, &newest, sizeof(int), hipMemcpyHostToDevice, s));
  TT_CHECK_HIP(hipStreamSynchronize(s));
  DecodeAttnArgs a;
  memset(&a, 0, sizeof(a));
  a.q = q; a.kp = kp; a.vp = vp; a.P1 = P1; a.kc = kc; a.vc = vc; a.tmax = tmax; a.step = step; a.host_tgen = tgen;
  a.out = out; a.B = B; a.heads = heads; a.variant = variant;
  int rc = decode_attention_launch(dtype, a, s);
  hipError_t e = hipStreamSynchronize(s);
  (void)hipFree(step);
  TT_TRY(rc);
  TT_CHECK_HIP(e);
  return 0;
}

// The decode step's QKV projection + attention in one launch (decode_attention.hip decode_qkv_attn_kernel) on caller-provided caches: own keys
// 0 .. tgen - 2 are in the caches, the launch appends slot tgen - 1 from h W^T + bias and attends [prefix | own keys 0 .. tgen - 1].
int tt_op_decode_qkv_attention(int dtype, const void* h, const void* w_qkv, const float* b_qkv, float q_scale, const void* kp, const void* vp, int P1,
                               void* kc, void* vc, int tmax, int tgen, void* q_out, void* out, int B, int heads, void* stream) {
  TT_REQUIRE(h && w_qkv && kp && vp && kc && vc && out && tgen >= 1 && tgen <= tmax, "tt_op_decode_qkv_attention: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  int* step = nullptr;
  TT_CHECK_HIP(hipMalloc((void**)&step, sizeof(int)));
  const int newest = tgen - 1;
  hipError_t e = hipMemcpyAsync(step, &newest, sizeof(int), hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) (void)hipFree(step);  // (the step word is freed on every path)
  TT_CHECK_HIP(e);
  DecodeQkvAttnArgs g;
  memset(&g, 0, sizeof(g));
  g.d.kp = kp; g.d.vp = vp; g.d.P1 = P1; g.d.kc = kc; g.d.vc = vc; g.d.tmax = tmax; g.d.step = step; g.d.host_tgen = tgen;
  g.d.out = out; g.d.B = B; g.d.heads = heads;
  g.h = h; g.w_qkv = w_qkv; g.b_qkv = b_qkv; g.q_scale = q_scale; g.q_out = q_out;
  int rc = decode_qkv_attention_launch(dtype, g, s);
  e = hipStreamSynchronize(s);
  (void)hipFree(step);
  TT_TRY(rc);
  TT_CHECK_HIP(e);
  return 0;
}

int tt_op_decode_attention_rows(int dtype, const void* q, const void* kp, const void* vp, long long prefix_stride, const int* p1_rows, int p1_cap,
                                const void* kc, const void* vc, int tmax, const int* slot_rows, void* out, int B, int heads, void* stream) {
  TT_REQUIRE(q && kp && vp && p1_rows && kc && vc && slot_rows && out && prefix_stride > 0 && p1_cap >= 1 && B >= 1 && heads >= 1 && tmax >= 1,
             "tt_op_decode_attention_rows: bad arguments");
  TT_REQUIRE(dtype == DT_BF16 || dtype == DT_F16, "tt_op_decode_attention_rows: 16-bit operands only");
  DecodeAttnArgs a;
  memset(&a, 0, sizeof(a));
  a.q = q; a.kp = kp; a.vp = vp; a.P1 = p1_cap; a.kc = kc; a.vc = vc; a.tmax = tmax;
  a.out = out; a.B = B; a.heads = heads;
  a.row_slot = slot_rows; a.row_p1 = p1_rows; a.prefix_group_stride = (size_t)prefix_stride;
  TT_TRY(decode_attention_launch(dtype, a, (hipStream_t)stream));
  TT_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
  return 0;
}

// One sampling step on caller-provided state (seen bitmask, unfinished flags); `step` indexes codes / exp_noise.
int tt_op_sample(const float* logits, int ldl, int B, int V, unsigned* seen, const tt_sampling* sp, int step, int* unfinished,
                 int stop_token, int* codes, int ldcodes, void* stream) {
  TT_REQUIRE(sp, "tt_op_sample: null sampling parameters");
  hipStream_t s = (hipStream_t)stream;
  int* scratch = nullptr;  // state[2] | next_tok[B] | unfinished_count[step+1]
  const size_t n = 2 + (size_t)B + step + 1;
  TT_CHECK_HIP(hipMalloc((void**)&scratch, n * sizeof(int)));
  TT_CHECK_HIP(hipMemsetAsync(scratch, 0, n * sizeof(int), s));
  const int st[2] = {step, step - 1};
  TT_CHECK_HIP(hipMemcpyAsync(scratch, st, sizeof(st), hipMemcpyHostToDevice, s));
  TT_CHECK_HIP(hipStreamSynchronize(s));
  SampleArgs a;
  memset(&a, 0, sizeof(a));
  a.logits = logits; a.ldl = ldl; a.B = B; a.V = V; a.seen = seen;
  a.rep_penalty = sp->repetition_penalty; a.temperature = sp->temperature; a.top_p = sp->top_p; a.top_k = sp->top_k;
  a.exp_noise = sp->exp_noise; a.seed = sp->seed; a.row_offset = sp->row_offset;
  a.state = scratch; a.unfinished = unfinished; a.stop_token = stop_token; a.codes = codes; a.ldcodes = ldcodes;
  a.next_tok = scratch + 2; a.unfinished_count = scratch + 2 + B;
  float* typ = nullptr;
  if (sp->typical_mass != 0.f) {
    if (hipMalloc((void**)&typ, (size_t)B * (ldl ? ldl : V) * sizeof(float)) != hipSuccess) {
      (void)hipFree(scratch);
      set_error("tt_op_sample: hipMalloc failed");
      return -2;
    }
    a.typical_mass = sp->typical_mass; a.typical_out = typ;
  }
  int rc = sample_launch(a, s);
  hipError_t e = hipStreamSynchronize(s);
  (void)hipFree(scratch);
  if (typ) (void)hipFree(typ);
  TT_TRY(rc);
  TT_CHECK_HIP(e);
  return 0;
}

int tt_op_typical_mask(const float* logits, int ldl, int B, int V, const unsigned* seen, float repetition_penalty, float mass, float* out,
                       void* stream) {
  SampleArgs a;
  memset(&a, 0, sizeof(a));
  a.logits = logits; a.ldl = ldl; a.B = B; a.V = V; a.seen = const_cast<unsigned*>(seen);
  a.rep_penalty = repetition_penalty; a.typical_mass = mass; a.typical_out = out;
  return typical_mask_launch(a, (hipStream_t)stream);
}

int tt_op_conv1d(const float* x, const float* w, const float* bias, float* y, int Cin, int Cout, int T, int k, int dilation, int reflect,
                 float in_slope, int out_act, float out_slope, void* stream) {
  Conv1dArgs a;
  memset(&a, 0, sizeof(a));
  a.x = x; a.w = w; a.bias = bias; a.y = y; a.Cin = Cin; a.Cout = Cout; a.T = T; a.k = k; a.dilation = dilation; a.reflect = reflect;
  a.in_slope = in_slope; a.out_act = out_act; a.out_slope = out_slope;
  return conv1d_direct_launch(a, (hipStream_t)stream);
}

int tt_op_convt1d(const float* x, const float* w, const float* bias, float* y, int C, int Tin, int stride, float in_slope, void* stream) {
  ConvT1dArgs a;
  memset(&a, 0, sizeof(a));
  a.x = x; a.w = w; a.bias = bias; a.y = y; a.C = C; a.Tin = Tin; a.stride = stride; a.in_slope = in_slope;
  return convt1d_launch(a, (hipStream_t)stream);
}

int tt_op_lvc(int dtype, const float* x_in, const void* kernels, int ldk, int koff, const float* bias, int ldb, int boff, float* x, int L, int hop,
              void* stream) {
  LvcArgs a;
  memset(&a, 0, sizeof(a));
  a.x_in = x_in; a.kernels = kernels; a.dtype = dtype; a.ldk = ldk; a.koff = koff; a.bias = bias; a.ldb = ldb; a.boff = boff; a.x = x; a.L = L; a.hop = hop;
  a.in_slope = -1.f;
  return lvc_launch(a, (hipStream_t)stream);
}

// the descriptor forms: every caller-set field of Conv1dArgs / ConvT1dArgs / LvcArgs, the ragged batch included
static VocSeqs voc_desc_seqs(int n, int mul, const int* frames) {
  VocSeqs q;
  memset(&q, 0, sizeof(q));
  q.n = n; q.mul = mul;
  for (int i = 0; i < kVocSeqs; ++i) q.frames[i] = frames[i];
  return q;
}
static void voc_ran(int* ran) {
  if (ran) {
    ran[0] = g_voc_ran.kernel; ran[1] = g_voc_ran.a; ran[2] = g_voc_ran.b; ran[3] = g_voc_ran.c;
  }
}

size_t tt_op_conv1d_desc_size(void) { return sizeof(tt_op_conv1d_desc); }
int tt_op_conv1d_ex(const tt_op_conv1d_desc* d, int* ran, void* stream) {
  TT_REQUIRE(d != nullptr, "tt_op_conv1d_ex: null descriptor");
  Conv1dArgs a;
  memset(&a, 0, sizeof(a));
  a.x = d->x; a.w = d->w; a.bias = d->bias; a.y = d->y; a.Cin = d->Cin; a.Cout = d->Cout; a.T = d->T; a.k = d->k; a.dilation = d->dilation;
  a.seq = voc_desc_seqs(d->seq_n, d->seq_mul, d->seq_frames);
  a.reflect = d->reflect; a.in_slope = d->in_slope; a.out_act = d->out_act; a.out_slope = d->out_slope;
  const int rc = conv1d_direct_launch(a, (hipStream_t)stream);
  voc_ran(ran);
  return rc;
}

size_t tt_op_convt1d_desc_size(void) { return sizeof(tt_op_convt1d_desc); }
int tt_op_convt1d_ex(const tt_op_convt1d_desc* d, int* ran, void* stream) {
  TT_REQUIRE(d != nullptr, "tt_op_convt1d_ex: null descriptor");
  ConvT1dArgs a;
  memset(&a, 0, sizeof(a));
  a.x = d->x; a.w = d->w; a.bias = d->bias; a.y = d->y; a.C = d->C; a.Tin = d->Tin; a.stride = d->stride; a.in_slope = d->in_slope;
  a.seq = voc_desc_seqs(d->seq_n, d->seq_mul, d->seq_frames);
  const int rc = convt1d_launch(a, (hipStream_t)stream);
  voc_ran(ran);
  return rc;
}

size_t tt_op_lvc_desc_size(void) { return sizeof(tt_op_lvc_desc); }
int tt_op_lvc_ex(const tt_op_lvc_desc* d, int* ran, void* stream) {
  TT_REQUIRE(d != nullptr, "tt_op_lvc_ex: null descriptor");
  LvcArgs a;
  memset(&a, 0, sizeof(a));
  a.x_in = d->x_in; a.kernels = d->kernels; a.ldk = d->ldk; a.koff = d->koff; a.dtype = d->dtype; a.bias = d->bias; a.ldb = d->ldb; a.boff = d->boff;
  a.x = d->x; a.L = d->L; a.hop = d->hop;
  a.seq = voc_desc_seqs(d->seq_n, d->seq_mul, d->seq_frames);
  a.in_slope = d->in_slope; a.guard = d->guard;
  const int rc = lvc_launch(a, (hipStream_t)stream);
  voc_ran(ran);
  return rc;
}

}  // extern "C"

// sizeof() of every struct that crosses the boundary, so host bindings can verify their mirrors
// without a GPU (tests/test_abi.py).
extern "C" size_t tt_struct_size(int which) {
  switch (which) {
    case 0: return sizeof(tt_gpt_layer);
    case 1: return sizeof(tt_ar_config);
    case 2: return sizeof(tt_ar_weights);
    case 3: return sizeof(tt_sampling);
    case 4: return sizeof(tt_clvp_layer);
    case 5: return sizeof(tt_clvp_tower);
    case 6: return sizeof(tt_clvp_config);
    case 7: return sizeof(tt_attn_block);
    case 8: return sizeof(tt_res_block);
    case 9: return sizeof(tt_diff_config);
    case 10: return sizeof(tt_diff_weights);
    case 11: return sizeof(tt_diff_step);
    case 12: return sizeof(tt_voc_block);
    case 13: return sizeof(tt_voc_config);
    case 14: return sizeof(tt_voc_weights);
    case 15: return sizeof(tt_cond_config);
    case 16: return sizeof(tt_cond_weights);
    case 17: return sizeof(tt_hifi_resblock);
    case 18: return sizeof(tt_hifi_config);
    case 19: return sizeof(tt_hifi_weights);
    case 20: return sizeof(tt_cvvp_tower);
    case 21: return sizeof(tt_cvvp_config);
    case 22: return sizeof(tt_cvvp_weights);
  }
  return 0;
}
