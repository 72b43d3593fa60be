// Stage 3: UnivNetGenerator.inference (reference: tortoise/models/vocoder.py:267-312).
// Mel-rate KernelPredictor convolutions run on MFMA (conv-GEMM); everything at the audio rate is
// f32 matrix-core / VALU work over channels-first rows (univnet.hip).  The predicted location-variable kernels are
// written ONCE, in the operand type, by the KernelPredictor GEMM's epilogue ([L][24576] per LVC block: 43 MB at 9.3 s of
// audio, f32 until round 5) and read once by the four LVC layers of the block, which widen them on the way into LDS.
// A call renders a ragged batch (include/tortoise_mi355x_univnet.h; tt_voc_run is its n = 1 case): sequence b owns a slot of
// L_pad = longest S + 10 frames at the mel rate and L_pad * hop columns at the audio rate, and holds S_b + 10 valid frames at its start.
// The KernelPredictor conv-GEMMs run over all slots in one launch each (M = n * L_pad) with the per-sequence valid-length loader
// (GemmArgs::seq_vlen): a tap that reaches past a sequence's end or before its slot reads zero, exactly the zero padding of a sequence
// rendered alone.  The audio-rate kernels carry the sequence in the grid (ops.h VocSeqs).  k-order per output element does not depend on
// M or on the tile (gemm_impl.h) and nothing here splits K, so every sequence is bit-identical to rendering it alone.
#include "runtime.h"
#include "../../include/tortoise_mi355x.h"
#include "../../include/tortoise_mi355x_univnet.h"

static_assert(tt::kVocSeqs == TT_VOC_MAX_BATCH, "ops.h VocSeqs holds TT_VOC_MAX_BATCH sequences");

using namespace tt;

// guard: workgroups of the location-variable convolutions that met a non-finite predicted kernel value, snapshot at the end of every
// tt_voc_run
struct tt_voc : EngineHandle {
  tt_voc_config cfg;
  tt_voc_weights w;
  std::vector<tt_voc_block> blocks;
  float* c_cf = nullptr;     // [mel][L] padded mel, channels-first
  float* c_tm = nullptr;     // [L][mel] token-major
  void* c_t = nullptr;       // [L][mel_pad] T
  float* kp_h = nullptr;     // [L][64] f32 KernelPredictor hidden state
  void* kp_ht = nullptr;     // [L][64] T
  void* kp_t1 = nullptr;     // [L][64] T
  void* kernels = nullptr;   // [L][24576] T
  float* kbias = nullptr;    // [L][256]
  float* xa = nullptr;       // [32][T] ping
  float* xb = nullptr;       // [32][T] pong
  float* o = nullptr;        // [32][T] conv output (first, the slots of a batch's noise inputs: conv_pre reads them from here)
  int* vlen = nullptr;       // [TT_VOC_MAX_BATCH] valid mel frames per sequence of the running batch (GemmArgs::seq_vlen)
};

namespace {
struct VocSrc { const float* p[TT_VOC_MAX_BATCH]; };  // per-sequence device pointers (kernel argument: no host -> device copy)
struct VocDst { float* p[TT_VOC_MAX_BATCH]; };
}  // namespace

// c[ch][b * Lp + t], channels-first over all slots: sequence b = blockIdx.y's own S frames, then its 10 frames of -11.5129
// (vocoder.py:303-305), then zeros to the end of its slot
__global__ void voc_pad_mel_kernel(const VocSrc mel, float* c, const VocSeqs q, int Lp, int C) {
  const int b = blockIdx.y, L = q.frames[b], S = L - 10;
  const float* m = mel.p[b];
  const size_t ld = (size_t)q.n * Lp;
  const int total = C * Lp;
  for (int f = blockIdx.x * blockDim.x + threadIdx.x; f < total; f += gridDim.x * blockDim.x) {
    const int ch = f / Lp, t = f % Lp;
    c[ch * ld + (size_t)b * Lp + t] = t < S ? m[(size_t)ch * S + t] : t < L ? -11.5129f : 0.f;
  }
}

// zs[b][ch][t] = z_b[ch][t] for t < frames[b]: the noise inputs, one slot of Lp columns per sequence (conv_pre's batch layout)
__global__ void voc_stage_noise_kernel(const VocSrc z, float* zs, const VocSeqs q, int Lp, int C) {
  const int b = blockIdx.y, L = q.frames[b];
  const float* src = z.p[b];
  float* dst = zs + (size_t)b * C * Lp;
  const int total = C * L;
  for (int f = blockIdx.x * blockDim.x + threadIdx.x; f < total; f += gridDim.x * blockDim.x) {
    const int ch = f / L, t = f % L;
    dst[(size_t)ch * Lp + t] = src[f];
  }
}

// audio_b[i] = slots[b * P + i] for i < (frames[b] - 10) * hop: drops each sequence's 10 pad frames
__global__ void voc_gather_audio_kernel(const float* __restrict__ slots, const VocDst audio, const VocSeqs q, size_t P, int hop) {
  const int b = blockIdx.y;
  const int n = (q.frames[b] - 10) * hop;
  float* dst = audio.p[b];
  const float* src = slots + (size_t)b * P;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) dst[i] = src[i];
}

__global__ void voc_vlen_kernel(const VocSeqs q, int* __restrict__ vlen) {
  if ((int)threadIdx.x < q.n) vlen[threadIdx.x] = q.frames[threadIdx.x];
}

extern "C" {

int tt_voc_create(const tt_voc_config* cfg, const tt_voc_weights* w, tt_voc** out) {
  TT_REQUIRE(cfg && w && out, "tt_voc_create: null argument");
  TT_REQUIRE(cfg->mel_pad % 64 == 0 && cfg->mel_pad >= cfg->mel_channels, "tt_voc_create: mel_pad must be a multiple of 64");
  tt_voc* e = new tt_voc();
  e->cfg = *cfg;
  e->w = *w;
  e->blocks.assign(w->blocks_host, w->blocks_host + 3);
  const size_t L = (size_t)cfg->max_frames + 10;
  size_t hop = 1;
  for (int i = 0; i < 3; ++i) hop *= e->blocks[i].stride;
  const size_t T = L * hop;
  // every audio-rate index ([n][32][L_pad * hop] element offsets, int sample positions) and every row offset of the predicted kernels
  // stays within 32 bits: 16 slots of 2186 frames are 34 976 frames -> 32 T = 2.9e8, 24576 L = 8.6e8
  TT_REQUIRE(32 * T < ((size_t)1 << 31) && L * 24576 < ((size_t)1 << 31), "tt_voc_create: max_frames=%d is beyond 32-bit audio-rate indices", cfg->max_frames);
  int rc = e->open("tt_voc_create", true);
  const size_t es = dtype_bytes(cfg->dtype);  // (4: the fp32 verification mode)
  if (!rc) rc = e->arena.alloc_t(&e->c_cf, L * cfg->mel_channels);
  if (!rc) rc = e->arena.alloc_t(&e->c_tm, L * cfg->mel_channels);
  if (!rc) rc = e->arena.alloc(&e->c_t, (L + 8) * cfg->mel_pad * es);
  if (!rc) rc = e->arena.alloc_t(&e->kp_h, (L + 8) * 64);
  if (!rc) rc = e->arena.alloc(&e->kp_ht, (L + 8) * 64 * es);
  if (!rc) rc = e->arena.alloc(&e->kp_t1, (L + 8) * 64 * es);
#if defined(TT_VOC_KERNELS_F32)  // A/B knob (build.py --variant): the round-5 form, predicted kernels materialised in f32
  if (!rc) rc = e->arena.alloc(&e->kernels, L * 24576 * 4 + 64);
#else
  if (!rc) rc = e->arena.alloc(&e->kernels, L * 24576 * es + 64);
#endif
  if (!rc) rc = e->arena.alloc_t(&e->kbias, L * 256);
  if (!rc) rc = e->arena.alloc_t(&e->xa, 32 * T);
  if (!rc) rc = e->arena.alloc_t(&e->xb, 32 * T);
  if (!rc) rc = e->arena.alloc_t(&e->o, 32 * T);
  if (!rc) rc = e->arena.alloc_t(&e->vlen, TT_VOC_MAX_BATCH);
  if (rc) {
    tt_voc_destroy(e);
    return rc;
  }
  *out = e;
  return 0;
}

void tt_voc_destroy(tt_voc* e) {
  if (!e) return;
  e->close();
  delete e;
}

// Operand-overflow guard of this stage (see tt_ar_guard): workgroups that met non-finite predicted kernels (an fp16 KernelPredictor operand
// beyond 65504 upstream - behind the sigmoid * tanh gate and the final tanh the waveform itself would come out finite), as of the end of the
// last tt_voc_run after the caller synchronised its stream.  reset != 0 clears it.
int tt_voc_guard(tt_voc* e, int reset) {
  if (!e) { set_error("tt_voc_guard: null handle"); return -1; }
  return e->read_guard(reset, "tt_voc_guard", "vocoder", e->cfg.dtype, "workgroup(s) met non-finite predicted kernels", "fp16: re-run this stage with bf16 operands");
}

int tt_voc_batch_abi_version(void) { return 1; }  // ABI changes

size_t tt_voc_batch_struct_size(int which) {
  switch (which) {
    case 0: return sizeof(tt_voc_config);
    case 1: return sizeof(tt_voc_weights);
    case 2: return sizeof(tt_voc_block);
  }
  return 0;
}

int tt_voc_batch_capacity(const tt_voc* e) { return e ? e->cfg.max_frames + 10 : 0; }

int tt_voc_run_batch(tt_voc* e, int n, const float* const* mel, const int* S, const float* const* z, float* const* audio, void* stream) {
  TT_REQUIRE(e && mel && S && z && audio, "tt_voc_run_batch: null argument");
  TT_REQUIRE(n >= 1 && n <= TT_VOC_MAX_BATCH, "tt_voc_run_batch: %d sequences (1 .. %d per call)", n, TT_VOC_MAX_BATCH);
  VocSeqs q;       // frames[b] = S_b + 10 valid mel frames of slot b
  VocSrc pm, pz;
  VocDst pa;
  memset(&q, 0, sizeof(q));
  memset(&pm, 0, sizeof(pm));
  memset(&pz, 0, sizeof(pz));
  memset(&pa, 0, sizeof(pa));
  int L = 0;       // frames per slot (L_pad)
  for (int b = 0; b < n; ++b) {
    TT_REQUIRE(mel[b] && z[b] && audio[b], "tt_voc_run_batch: null pointer for sequence %d", b);
    TT_REQUIRE(S[b] >= 1 && S[b] <= e->cfg.max_frames, "tt_voc_run_batch: sequence %d has %d frames (1 .. %d)", b, S[b], e->cfg.max_frames);
    q.frames[b] = S[b] + 10;
    pm.p[b] = mel[b]; pz.p[b] = z[b]; pa.p[b] = audio[b];
    L = std::max(L, S[b] + 10);
  }
  q.n = n;
  TT_REQUIRE((long)n * L <= (long)e->cfg.max_frames + 10, "tt_voc_run_batch: %d slots of %d frames exceed the handle's %d (max_frames %d)", n, L,
             e->cfg.max_frames + 10, e->cfg.max_frames);
  return e->sb.run((hipStream_t)stream, [&](hipStream_t s) -> int {
    const int dt = e->cfg.dtype, MC = e->cfg.mel_channels, MP = e->cfg.mel_pad;
    const int M = n * L;  // mel-rate rows of all slots
    // one sequence: the tap convolutions' own sequence bound is its length; a batch: the per-sequence valid lengths
    const int* vlen = n > 1 ? e->vlen : nullptr;
    voc_pad_mel_kernel<<<dim3(std::min(cdiv(MC * L, 256), 2048), n), 256, 0, s>>>(pm, e->c_cf, q, L, MC);
    if (n > 1) {
      voc_vlen_kernel<<<1, TT_VOC_MAX_BATCH, 0, s>>>(q, e->vlen);
      voc_stage_noise_kernel<<<dim3(std::min(cdiv(64 * L, 256), 2048), n), 256, 0, s>>>(pz, e->o, q, L, 64);
    }
    TT_CHECK_HIP(hipGetLastError());
    TT_TRY(transpose_launch(e->c_cf, e->c_tm, MC, M, s));
    TT_TRY(cast_pad_launch(dt, e->c_tm, MC, e->c_t, MP, M, MC, MP, s));
    // conv_pre: Conv1d(64 -> 32, k7, reflect)   (vocoder.py:255-256, 273)
    Conv1dArgs ca;
    memset(&ca, 0, sizeof(ca));
    ca.x = n > 1 ? e->o : pz.p[0]; ca.w = e->w.w_pre; ca.bias = e->w.b_pre; ca.y = e->xa; ca.Cin = 64; ca.Cout = 32; ca.T = L; ca.k = 7; ca.dilation = 1;
    ca.reflect = 1; ca.in_slope = -1.f; ca.out_act = ACT_NONE; ca.seq = q; ca.seq.mul = 1;
    TT_TRY(conv1d_direct_launch(ca, s));
    float* x = e->xa;
    float* xn = e->xb;
    int hop = 1, T = L;
    static const int dil[4] = {1, 3, 9, 27};
    for (int bi = 0; bi < 3; ++bi) {
      const tt_voc_block& b = e->blocks[bi];
      // convt_pre: LeakyReLU + ConvTranspose1d   (vocoder.py:128-132, 162)
      ConvT1dArgs ta;
      memset(&ta, 0, sizeof(ta));
      ta.x = x; ta.w = b.w_convt; ta.bias = b.b_convt; ta.y = xn; ta.C = 32; ta.Tin = T; ta.stride = b.stride; ta.in_slope = 0.2f;
      ta.seq = q; ta.seq.mul = hop;
      TT_TRY(convt1d_launch(ta, s));
      { float* t = x; x = xn; xn = t; }
      hop *= b.stride;
      T = L * hop;
      // KernelPredictor(c)   (vocoder.py:66-93)
      GemmArgs g = gemm_args(e->c_t, MP, b.w_kp_in, 5 * MP, M, 64, 5 * MP);
      g.taps = 5; g.seq_len = L; g.seq_vlen = vlen; g.bias = b.b_kp_in; g.act = ACT_LRELU; g.slope = 0.2f;
      g.out_f32 = e->kp_h; g.ldo32 = 64; g.out_t = e->kp_ht; g.ldot = 64;
      TT_TRY(gemm_launch(dt, EPI_STD, g, s));
      for (int r = 0; r < 3; ++r) {
        g = gemm_args(e->kp_ht, 64, b.w_kp_res[2 * r], 192, M, 64, 192);
        g.taps = 3; g.seq_len = L; g.seq_vlen = vlen; g.bias = b.b_kp_res[2 * r]; g.act = ACT_LRELU; g.slope = 0.2f; g.out_t = e->kp_t1; g.ldot = 64;
        TT_TRY(gemm_launch(dt, EPI_STD, g, s));
        g = gemm_args(e->kp_t1, 64, b.w_kp_res[2 * r + 1], 192, M, 64, 192);
        g.taps = 3; g.seq_len = L; g.seq_vlen = vlen; g.bias = b.b_kp_res[2 * r + 1]; g.act = ACT_LRELU; g.slope = 0.2f;
        g.res = e->kp_h; g.ldres = 64; g.out_f32 = e->kp_h; g.ldo32 = 64; g.out_t = e->kp_ht; g.ldot = 64;
        TT_TRY(gemm_launch(dt, EPI_STD, g, s));
      }
      g = gemm_args(e->kp_ht, 64, b.w_kp_kernel, 192, M, 24576, 192);
      g.taps = 3; g.seq_len = L; g.seq_vlen = vlen; g.bias = b.b_kp_kernel;
#if defined(TT_VOC_KERNELS_F32)
      g.out_f32 = (float*)e->kernels; g.ldo32 = 24576;
#else
      g.out_t = e->kernels; g.ldot = 24576;
#endif
      TT_TRY(gemm_launch(dt, EPI_STD, g, s));
      g = gemm_args(e->kp_ht, 64, b.w_kp_bias, 192, M, 256, 192);
      g.taps = 3; g.seq_len = L; g.seq_vlen = vlen; g.bias = b.b_kp_bias; g.out_f32 = e->kbias; g.ldo32 = 256;
      TT_TRY(gemm_launch(dt, EPI_STD, g, s));
      for (int j = 0; j < 4; ++j) {
        // conv_blocks[j]: LeakyReLU + dilated Conv1d, then LeakyReLU   (vocoder.py:134-146, 172-173)
        memset(&ca, 0, sizeof(ca));
        ca.x = x; ca.w = b.w_conv[j]; ca.bias = b.b_conv[j]; ca.y = e->o; ca.Cin = 32; ca.Cout = 32; ca.T = T; ca.k = 3;
        ca.dilation = dil[j]; ca.reflect = 0; ca.in_slope = 0.2f; ca.out_act = ACT_LRELU; ca.out_slope = 0.2f; ca.seq = q; ca.seq.mul = hop;
        TT_TRY(conv1d_direct_launch(ca, s));
        LvcArgs la;
        memset(&la, 0, sizeof(la));
        la.x_in = e->o; la.kernels = e->kernels; la.dtype = dt; la.ldk = 24576; la.koff = j * 6144; la.bias = e->kbias; la.ldb = 256; la.boff = j * 64;
#if defined(TT_VOC_KERNELS_F32)
        la.dtype = DT_F32;
#endif
        la.x = x; la.L = L; la.hop = hop; la.in_slope = -1.f; la.guard = e->guard.dev; la.seq = q; la.seq.mul = hop;
        TT_TRY(lvc_launch(la, s));
      }
    }
    // conv_post: LeakyReLU + Conv1d(32 -> 1, k7, reflect) + tanh   (vocoder.py:258-262); drop the 10 pad frames of every sequence
    memset(&ca, 0, sizeof(ca));
    ca.x = x; ca.w = e->w.w_post; ca.bias = e->w.b_post; ca.y = e->o; ca.Cin = 32; ca.Cout = 1; ca.T = T; ca.k = 7; ca.dilation = 1;
    ca.reflect = 1; ca.in_slope = 0.2f; ca.out_act = 5; ca.seq = q; ca.seq.mul = hop;
    TT_TRY(conv1d_direct_launch(ca, s));
    if (n == 1) {
      TT_CHECK_HIP(hipMemcpyAsync(pa.p[0], e->o, (size_t)S[0] * hop * sizeof(float), hipMemcpyDeviceToDevice, s));
    } else {
      voc_gather_audio_kernel<<<dim3(std::min(cdiv((L - 10) * hop, 256), 1024), n), 256, 0, s>>>(e->o, pa, q, (size_t)T, hop);
      TT_CHECK_HIP(hipGetLastError());
    }
    return e->guard.snapshot(s);
  });
}

int tt_voc_run(tt_voc* e, const float* mel, int S, const float* z, float* audio, void* stream) {
  TT_REQUIRE(e && mel && z && audio, "tt_voc_run: null argument");
  TT_REQUIRE(S >= 1 && S <= e->cfg.max_frames, "tt_voc_run: %d frames exceed capacity %d", S, e->cfg.max_frames);
  return tt_voc_run_batch(e, 1, &mel, &S, &z, &audio, stream);
}

}  // extern "C"
