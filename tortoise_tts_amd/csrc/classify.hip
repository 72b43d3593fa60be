// Tortoise detector (reference tortoise/api.py classify_audio_clip, tortoise/models/classifier.py) - include/tortoise_mi355x_classify.h.
// Activations are token-major ([frames][channels]) with an f32 residual stream, as everywhere in the engine.
// New kernels: the 1 -> 32 init conv, the narrow (32 / 64-channel) k5 convolution of the two audio-rate levels - GroupNorm(16) + SiLU
// applied on load for the ResBlock convs, stride 4 for the Downsample - on the matrix cores, the GroupNorm statistics finaliser those
// two feed, the 128-wide-head non-causal attention and the head (Linear(512, 2) on frame 0).  Levels 2 - 4 (C >= 128: 32 groups) and the
// encoder tail are the engine's GroupNorm and GEMM launches: the ResBlock convs are tap GEMMs (taps = 5), the Downsample a GEMM whose A
// rows overlap (lda = 4 C < K = 5 C) over an operand copy that starts 2 zero rows early (padding 2).
#include <limits.h>
#include "stage_blocks.h"
#include "../../include/tortoise_mi355x_classify.h"
#include "../../include/tortoise_mi355x_test.h"

using namespace tt;

namespace tt {

constexpr int kClsGroups = 16;     // arch_util.normalization: 16 groups at 32 and 64 channels
constexpr int kClsInitRows = 256;  // init conv: output rows per workgroup
constexpr int kClsConvRows = 128;  // narrow conv: output rows per workgroup (4 waves x 32)
constexpr int kClsHeadDim = 128, kClsHeads = 4, kClsDim = 512;
constexpr int kClsQPerWave = 4;    // attention: queries per wave
constexpr float kClsEps = 1e-5f;

// Element offsets are formed in size_t; rows are ints.  The largest row index any launch forms from a clip of n samples is the level-0
// Downsample's input row 4 t + 2 for the last row t of its last 128-row tile: t <= ceil(n / 4) + 126, so 4 t + 2 <= n + 509 (the init
// conv's and the stride-1 convs' tiles end below that).  Every int stays in range while n + 4 * 128 + 8 <= INT_MAX.
constexpr int kClsMaxSamples = INT_MAX - (4 * kClsConvRows + 8);

static inline __host__ __device__ int cls_down(int L) { return (L + 3) / 4; }  // Conv1d(k 5, stride 4, pad 2): ceil(L / 4)

// Init conv Conv1d(1, 32, 3, pad 1): out[t][c] = b[c] + sum_j w[c][j] x[t + j - 1].  Thread -> group g = tid & 15 (channels 2g, 2g + 1)
// and rows tid / 16 + 16 i of the workgroup's 256.  part[block][g] = (sum, sum of squares) in double for the first GroupNorm.
__global__ __launch_bounds__(256) void cls_init_kernel(const float* __restrict__ x, int n, const float* __restrict__ w,
                                                       const float* __restrict__ bias, float* __restrict__ out, double* __restrict__ part) {
  __shared__ double red[4][kClsGroups][2];
  const int tid = threadIdx.x, g = tid & 15, lane = tid & 63, wave = tid >> 6;
  float wr[2][3], br[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
#pragma unroll
    for (int k = 0; k < 3; ++k) wr[j][k] = w[(2 * g + j) * 3 + k];
    br[j] = bias[2 * g + j];
  }
  double s = 0.0, q = 0.0;
  const int t0 = blockIdx.x * kClsInitRows;
  for (int i = tid >> 4; i < kClsInitRows; i += 16) {
    const int t = t0 + i;
    if (t >= n) break;
    const float xm = t > 0 ? x[t - 1] : 0.f, x0 = x[t], xp = t + 1 < n ? x[t + 1] : 0.f;
    const float v0 = br[0] + wr[0][0] * xm + wr[0][1] * x0 + wr[0][2] * xp;
    const float v1 = br[1] + wr[1][0] * xm + wr[1][1] * x0 + wr[1][2] * xp;
    *(float2*)(out + (size_t)t * 32 + 2 * g) = make_float2(v0, v1);
    s += (double)v0 + v1;
    q += (double)v0 * v0 + (double)v1 * v1;
  }
  s += __shfl_xor(s, 16); q += __shfl_xor(q, 16);
  s += __shfl_xor(s, 32); q += __shfl_xor(q, 32);
  if (lane < 16) { red[wave][g][0] = s; red[wave][g][1] = q; }
  __syncthreads();
  if (tid < 2 * kClsGroups) {
    const int gg = tid >> 1, k = tid & 1;
    part[((size_t)blockIdx.x * kClsGroups + gg) * 2 + k] = red[0][gg][k] + red[1][gg][k] + red[2][gg][k] + red[3][gg][k];
  }
}

// GroupNorm statistics of 16 groups from `nblocks` workgroup partials: stats[g] = {mean, 1 / sqrt(var + eps)} over count = L * C / 16
// values (biased variance, as torch.group_norm).  One workgroup per group, reduced in double.
__global__ __launch_bounds__(256) void cls_stats_kernel(const double* __restrict__ part, int nblocks, double count, float* __restrict__ stats,
                                                        int* guard) {
  __shared__ double red[2][4];
  const int g = blockIdx.x, tid = threadIdx.x;
  double s = 0.0, q = 0.0;
  for (int b = tid; b < nblocks; b += 256) {
    s += part[((size_t)b * kClsGroups + g) * 2];
    q += part[((size_t)b * kClsGroups + g) * 2 + 1];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    s += __shfl_xor(s, off);
    q += __shfl_xor(q, off);
  }
  if ((tid & 63) == 0) { red[0][tid >> 6] = s; red[1][tid >> 6] = q; }
  __syncthreads();
  if (tid == 0) {
    const double ts = red[0][0] + red[0][1] + red[0][2] + red[0][3], tq = red[1][0] + red[1][1] + red[1][2] + red[1][3];
    const double mean = ts / count;
    const double var = fmax(tq / count - mean * mean, 0.0);
    stats[2 * g] = (float)mean;
    stats[2 * g + 1] = (float)(1.0 / sqrt(var + (double)kClsEps));
    if (guard && !(fabs(mean) < INFINITY && var < INFINITY)) atomicAdd(guard, 1);
  }
}

struct ClsConvArgs {
  const float* x;       // [Lin][CIN] f32
  int Lin, Lout;
  const float* stats;   // stride 1: {mean, rstd} of the 16 groups of x; the conv reads SiLU(GN(x))
  const float* gamma;
  const float* beta;
  const void* w;        // T [COUT][5][CIN]
  const float* bias;
  const float* res;     // optional [Lout][COUT] f32, added after the bias (may alias out)
  float* out;           // [Lout][COUT] f32
  double* part;         // optional (COUT <= 64): [block][16][2] sum / sum of squares of out for the next GroupNorm
};

template <typename T> struct ClsFrag { typedef typename Vec<T>::x8 type; };  // 16-bit operands: 8 k per lane (32x32x16 MFMA)
template <> struct ClsFrag<float> { typedef float type; };                    // f32: 1 k per lane (32x32x2 MFMA, exact)

template <typename T> __device__ __forceinline__ f32x16 cls_mfma(typename ClsFrag<T>::type a, typename ClsFrag<T>::type b, f32x16 c) {
  if constexpr (sizeof(T) == 4) return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
  else return mfma32(a, b, c);
}

// Narrow Conv1d(CIN, COUT, 5, STRIDE, pad 2) on the matrix cores: the GEMM out[t][n] = sum_k A[t][k] W[n][k] with k = tap * CIN + c,
// A[t][k] = in[STRIDE t + tap - 2][c] (zero outside [0, Lin)).  Wave w owns output rows t0 + 32 w .. + 31 and all COUT columns.
// STRIDE 1 (ResBlock convs): the workgroup's 132 input rows pass GroupNorm + SiLU once on their way into LDS, in the operand type.
// STRIDE 4 (Downsample, no norm): A fragments come straight from the f32 rows (each input row is read by at most two output rows).
// Epilogue: + bias (+ res) -> f32 out, and the per-(workgroup, group) statistics of out when part is set.
template <typename T, int CIN, int COUT, int STRIDE>
__global__ __launch_bounds__(256) void cls_conv_kernel(ClsConvArgs a) {
  constexpr int KPL = sizeof(T) == 4 ? 1 : 8;  // k per lane per MFMA
  constexpr int KSTEP = 2 * KPL, K = 5 * CIN, NB = COUT / 32, LROW = CIN + 8;
  constexpr int SROWS = STRIDE == 1 ? kClsConvRows + 4 : 1;
  typedef typename ClsFrag<T>::type Frag;
  __shared__ __attribute__((aligned(16))) T xs[SROWS][LROW];
  __shared__ double red[4][kClsGroups][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int t0 = blockIdx.x * kClsConvRows;
  if constexpr (STRIDE == 1) {
    constexpr int C4 = CIN / 4, CPG = CIN / kClsGroups;
    for (int i = tid; i < SROWS * C4; i += 256) {
      const int r = i / C4, c = (i - r * C4) * 4, t = t0 - 2 + r;
      float v[4] = {0.f, 0.f, 0.f, 0.f};
      if (t >= 0 && t < a.Lin) {
        const float4 u = *(const float4*)(a.x + (size_t)t * CIN + c);
        const float uu[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int g = (c + j) / CPG;
          v[j] = silu((uu[j] - a.stats[2 * g]) * a.stats[2 * g + 1] * a.gamma[c + j] + a.beta[c + j]);
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) xs[r][c + j] = (T)v[j];
    }
    __syncthreads();
  }
  const int i = lane & 31, h = lane >> 5;
  const int trow = t0 + wave * 32 + i;  // output row of this lane's A fragment
  f32x16 acc[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[nb][r] = 0.f;
  const T* W = (const T*)a.w;
#pragma unroll 2
  for (int k0 = 0; k0 < K; k0 += KSTEP) {
    const int k = k0 + h * KPL, tap = k / CIN, c = k - tap * CIN;
    Frag fa;
    if constexpr (STRIDE == 1) {
      fa = *(const Frag*)&xs[wave * 32 + i + tap][c];
    } else {
      const int u = STRIDE * trow + tap - 2;
      const bool ok = u >= 0 && u < a.Lin;
      if constexpr (KPL == 1) {
        fa = ok ? a.x[(size_t)u * CIN + c] : 0.f;
      } else {
        float4 p0 = make_float4(0.f, 0.f, 0.f, 0.f), p1 = p0;
        if (ok) {
          p0 = *(const float4*)(a.x + (size_t)u * CIN + c);
          p1 = *(const float4*)(a.x + (size_t)u * CIN + c + 4);
        }
        fa[0] = (T)p0.x; fa[1] = (T)p0.y; fa[2] = (T)p0.z; fa[3] = (T)p0.w;
        fa[4] = (T)p1.x; fa[5] = (T)p1.y; fa[6] = (T)p1.z; fa[7] = (T)p1.w;
      }
    }
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      const Frag fb = *(const Frag*)(W + (size_t)(nb * 32 + i) * K + k);
      acc[nb] = cls_mfma<T>(fa, fb, acc[nb]);
    }
  }
  // D lane l reg r = D[row = (r & 3) + 8 (r >> 2) + 4 (l >> 5)][col = l & 31]
  constexpr int CPG = COUT / kClsGroups;
  const int rbase = t0 + wave * 32 + 4 * h;
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const int col = nb * 32 + i;
    const float b = a.bias[col];
    double s = 0.0, q = 0.0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = rbase + (r & 3) + 8 * (r >> 2);
      if (row < a.Lout) {
        const size_t o = (size_t)row * COUT + col;
        float v = acc[nb][r] + b;
        if (a.res) v += a.res[o];
        a.out[o] = v;
        s += v;
        q += (double)v * v;
      }
    }
    if constexpr (COUT <= 64) {
      if (a.part) {
        s += __shfl_xor(s, 32); q += __shfl_xor(q, 32);
#pragma unroll
        for (int off = 1; off < CPG; off <<= 1) { s += __shfl_xor(s, off); q += __shfl_xor(q, off); }
        if (h == 0 && (i % CPG) == 0) { red[wave][col / CPG][0] = s; red[wave][col / CPG][1] = q; }
      }
    }
  }
  if constexpr (COUT <= 64) {
    if (a.part) {
      __syncthreads();
      if (tid < 2 * kClsGroups) {
        const int g = tid >> 1, k = tid & 1;
        a.part[((size_t)blockIdx.x * kClsGroups + g) * 2 + k] = red[0][g][k] + red[1][g][k] + red[2][g][k] + red[3][g][k];
      }
    }
  }
}

// Non-causal attention of QKVAttentionLegacy over f32 qkv [n][1536] (head h: q / k / v at columns 384 h + 0 / 128 / 256): out[t][128 h + d]
// for the first nq queries, in the operand type of the proj_out GEMM.  Wave -> 4 queries of one head, lane -> one key of every 64-key
// chunk for the scores (online softmax in f32) and output dims lane, lane + 64 for P V.  q and k are both scaled by 128^-1/4 in the
// reference; here q alone carries 1 / sqrt(128).
template <typename T>
__global__ __launch_bounds__(256) void cls_attention_kernel(const float* __restrict__ qkv, int n, int nq, T* __restrict__ out) {
  constexpr int D = kClsHeadDim, QB = kClsQPerWave, LD = 3 * kClsDim;
  __shared__ __attribute__((aligned(16))) float qs[4][QB][D];
  __shared__ float ps[4][QB][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hh = blockIdx.y;
  const int q0 = blockIdx.x * 4 * QB + wave * QB;
  const float scale = 0.08838834764831845f;  // 1 / sqrt(128)
  for (int e = lane; e < QB * D; e += 64) {
    const int qi = e / D, d = e - qi * D, t = min(q0 + qi, n - 1);
    qs[wave][qi][d] = qkv[(size_t)t * LD + hh * 3 * D + d] * scale;
  }
  __syncthreads();
  float m[QB], l[QB], acc[QB][2];
#pragma unroll
  for (int qi = 0; qi < QB; ++qi) { m[qi] = -INFINITY; l[qi] = 0.f; acc[qi][0] = acc[qi][1] = 0.f; }
  for (int j0 = 0; j0 < n; j0 += 64) {
    const int j = j0 + lane;
    float s[QB];
#pragma unroll
    for (int qi = 0; qi < QB; ++qi) s[qi] = 0.f;
    if (j < n) {
      const float4* kr = (const float4*)(qkv + (size_t)j * LD + hh * 3 * D + D);
#pragma unroll 4
      for (int d4 = 0; d4 < D / 4; ++d4) {
        const float4 kv = kr[d4];
#pragma unroll
        for (int qi = 0; qi < QB; ++qi) {
          const float4 qv = *(const float4*)&qs[wave][qi][4 * d4];
          s[qi] += qv.x * kv.x + qv.y * kv.y + qv.z * kv.z + qv.w * kv.w;
        }
      }
    }
#pragma unroll
    for (int qi = 0; qi < QB; ++qi) {
      const float sv = j < n ? s[qi] : -INFINITY;
      const float mn = fmaxf(m[qi], wave_max(sv));  // finite: lane 0's key j0 < n is valid
      const float p = j < n ? __expf(sv - mn) : 0.f;
      const float corr = __expf(m[qi] - mn);
      l[qi] = l[qi] * corr + wave_sum(p);
      acc[qi][0] *= corr;
      acc[qi][1] *= corr;
      m[qi] = mn;
      ps[wave][qi][lane] = p;
    }
    __syncthreads();
    const int cnt = min(64, n - j0);
    const float* vb = qkv + (size_t)j0 * LD + hh * 3 * D + 2 * D;
    for (int jj = 0; jj < cnt; ++jj) {
      const float v0 = vb[(size_t)jj * LD + lane], v1 = vb[(size_t)jj * LD + lane + 64];
#pragma unroll
      for (int qi = 0; qi < QB; ++qi) {
        const float p = ps[wave][qi][jj];
        acc[qi][0] += p * v0;
        acc[qi][1] += p * v1;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int qi = 0; qi < QB; ++qi) {
    const int t = q0 + qi;
    if (t < nq) {
      const float r = 1.f / l[qi];
      T* o = out + (size_t)t * kClsDim + hh * D;
      o[lane] = (T)(acc[qi][0] * r);
      o[lane + 64] = (T)(acc[qi][1] * r);
    }
  }
}

// Head: logits[j] = b[j] + <W[j], x[0]> for the 2 classes; emb (optional) = x[0][0 .. 512).  One wave, lane -> 8 channels.
__global__ __launch_bounds__(64) void cls_head_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                                                      float* __restrict__ logits, float* __restrict__ emb, int* guard) {
  const int lane = threadIdx.x, c0 = lane * 8;
  float s0 = 0.f, s1 = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float v = x[c0 + j];
    s0 += w[c0 + j] * v;
    s1 += w[kClsDim + c0 + j] * v;
    if (emb) emb[c0 + j] = v;
  }
  s0 = wave_sum(s0) + b[0];
  s1 = wave_sum(s1) + b[1];
  if (lane == 0) {
    logits[0] = s0;
    logits[1] = s1;
    if (guard && !(fabsf(s0) < INFINITY && fabsf(s1) < INFINITY)) atomicAdd(guard, 1);
  }
}

int cls_init_launch(const float* x, int n, const float* w, const float* b, float* out, double* part, hipStream_t s) {
  TT_REQUIRE(n >= 1 && n <= kClsMaxSamples, "cls init: %d samples (1 .. %d)", n, kClsMaxSamples);
  cls_init_kernel<<<cdiv(n, kClsInitRows), 256, 0, s>>>(x, n, w, b, out, part);
  TT_CHECK_HIP(hipGetLastError());
  return 0;
}

int cls_stats_launch(const double* part, int nblocks, int L, int C, float* stats, int* guard, hipStream_t s) {
  TT_REQUIRE(nblocks >= 1 && L >= 1 && C % kClsGroups == 0, "cls stats: bad shape (%d blocks, L=%d, C=%d)", nblocks, L, C);
  cls_stats_kernel<<<kClsGroups, 256, 0, s>>>(part, nblocks, (double)L * (C / kClsGroups), stats, guard);
  TT_CHECK_HIP(hipGetLastError());
  return 0;
}

static inline int cls_conv_blocks(int Lout) { return cdiv(Lout, kClsConvRows); }

// cin 32 / 64; stride 1 (cout == cin, GroupNorm + SiLU on load) or 4 (cout == 2 cin, no norm)
int cls_conv_launch(int dtype, int cin, int cout, int stride, const ClsConvArgs& a, hipStream_t s) {
  TT_REQUIRE((cin == 32 || cin == 64) && ((stride == 1 && cout == cin) || (stride == 4 && cout == 2 * cin)),
             "cls conv: Cin=%d Cout=%d stride=%d (built: Cin 32 / 64, stride 1 with Cout = Cin, stride 4 with Cout = 2 Cin)", cin, cout, stride);
  TT_REQUIRE(a.Lin >= 1 && a.Lin <= kClsMaxSamples && a.Lout == (stride == 1 ? a.Lin : cls_down(a.Lin)), "cls conv: lengths %d -> %d", a.Lin, a.Lout);
  TT_REQUIRE(a.x && a.w && a.bias && a.out && (stride == 4 || (a.stats && a.gamma && a.beta)), "cls conv: null argument");
  TT_REQUIRE(!a.part || cout <= 64, "cls conv: statistics partials are built for the 16-group widths (Cout <= 64)");
  const int blocks = cls_conv_blocks(a.Lout);
#define TT_CLS_CONV(CI, CO, ST) TT_DISPATCH_T(dtype, T, (cls_conv_kernel<T, CI, CO, ST><<<blocks, 256, 0, s>>>(a)))
  if (stride == 1 && cin == 32) TT_CLS_CONV(32, 32, 1);
  else if (stride == 1) TT_CLS_CONV(64, 64, 1);
  else if (cin == 32) TT_CLS_CONV(32, 64, 4);
  else TT_CLS_CONV(64, 128, 4);
#undef TT_CLS_CONV
  TT_CHECK_HIP(hipGetLastError());
  return 0;
}

int cls_attention_launch(int dtype, const float* qkv, int n, int nq, void* out, hipStream_t s) {
  TT_REQUIRE(n >= 1 && nq >= 1 && nq <= n, "cls attention: %d queries over %d frames", nq, n);
  dim3 grid(cdiv(nq, 4 * kClsQPerWave), kClsHeads);
  TT_DISPATCH_T(dtype, T, (cls_attention_kernel<T><<<grid, 256, 0, s>>>(qkv, n, nq, (T*)out)));
  TT_CHECK_HIP(hipGetLastError());
  return 0;
}

int cls_head_launch(const float* x, const float* w, const float* b, float* logits, float* emb, int* guard, hipStream_t s) {
  cls_head_kernel<<<1, 64, 0, s>>>(x, w, b, logits, emb, guard);
  TT_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace tt

struct tt_cls : EngineHandle {  // guard: narrow and wide GroupNorm statistics and the logits; snapshot at the end of every run
  tt_cls_config cfg;
  tt_cls_weights w;
  int es = 2;
  float* xa = nullptr; float* xb = nullptr; float* hf = nullptr;  // f32 [rows][C] residual ping-pong and the ResBlock's inner conv output
  void* ht = nullptr;                                             // T: GroupNorm + SiLU operand of the wide convs / QKV GEMM
  void* xt = nullptr;                                             // T: operand copy of the residual stream, 2 zero rows in front
  float* qkv = nullptr; void* att = nullptr;                      // attention: f32 [frames][1536], T [frames][512]
  double* part = nullptr; float* stats = nullptr; float* gnpart = nullptr;
};

static int cls_gn(tt_cls* e, const float* x, int L, int C, const float* g, const float* b, int act, void* out_t, hipStream_t s) {
  return groupnorm_launch(e->cfg.dtype, groupnorm_args(x, 1, L, C, g, b, kClsEps, act, out_t, nullptr, e->gnpart, e->guard.dev), s);
}

static int cls_forward(tt_cls* e, const float* clip, int n, float* logits, float* emb, hipStream_t s) {
  const int dt = e->cfg.dtype, es = e->es;
  const tt_cls_weights& W = e->w;
  int* guard = e->guard.dev;
  // init conv -> level 0 residual stream (xa) + the first GroupNorm's partials
  TT_TRY(cls_init_launch(clip, n, W.w_init, W.b_init, e->xa, e->part, s));
  int nparts = cdiv(n, kClsInitRows);
  float* x = e->xa;
  float* y = e->xb;
  int L = n, C = 32;
  for (int lv = 0; lv < TT_CLS_DEPTH; ++lv) {
    if (C <= 64) {  // audio-rate levels: the narrow conv kernel, statistics carried between launches
      for (int r = 0; r < TT_CLS_RES_BLOCKS; ++r) {
        const tt_cls_resblock& rb = W.res[lv][r];
        ClsConvArgs a;
        memset(&a, 0, sizeof(a));
        a.Lin = a.Lout = L; a.stats = e->stats;
        TT_TRY(cls_stats_launch(e->part, nparts, L, C, e->stats, guard, s));
        a.x = x; a.gamma = rb.gn1_g; a.beta = rb.gn1_b; a.w = rb.w1; a.bias = rb.b1; a.out = e->hf; a.part = e->part;
        TT_TRY(cls_conv_launch(dt, C, C, 1, a, s));
        nparts = cls_conv_blocks(L);
        TT_TRY(cls_stats_launch(e->part, nparts, L, C, e->stats, guard, s));
        a.x = e->hf; a.gamma = rb.gn2_g; a.beta = rb.gn2_b; a.w = rb.w2; a.bias = rb.b2; a.res = x; a.out = x; a.part = e->part;
        TT_TRY(cls_conv_launch(dt, C, C, 1, a, s));
      }
      ClsConvArgs a;
      memset(&a, 0, sizeof(a));
      a.x = x; a.Lin = L; a.Lout = cls_down(L); a.w = W.w_down[lv]; a.bias = W.b_down[lv]; a.out = y;
      a.part = 2 * C <= 64 ? e->part : nullptr;
      TT_TRY(cls_conv_launch(dt, C, 2 * C, 4, a, s));
      nparts = cls_conv_blocks(a.Lout);
    } else {  // C >= 128: GroupNorm(32) launches and tap GEMMs
      for (int r = 0; r < TT_CLS_RES_BLOCKS; ++r) {
        const tt_cls_resblock& rb = W.res[lv][r];
        TT_TRY(cls_gn(e, x, L, C, rb.gn1_g, rb.gn1_b, ACT_SILU, e->ht, s));
        GemmArgs g = gemm_conv_args(e->ht, C, rb.w1, 5, L, L, C, rb.b1);
        g.out_f32 = e->hf; g.ldo32 = C;
        TT_TRY(gemm_launch(dt, EPI_STD, g, s));
        TT_TRY(cls_gn(e, e->hf, L, C, rb.gn2_g, rb.gn2_b, ACT_SILU, e->ht, s));
        g = gemm_conv_args(e->ht, C, rb.w2, 5, L, L, C, rb.b2);
        g.res = x; g.ldres = C; g.out_f32 = x; g.ldo32 = C;
        if (r == TT_CLS_RES_BLOCKS - 1) { g.out_t = offset_t(e->xt, 2 * (size_t)C, es); g.ldot = C; }
        TT_TRY(gemm_launch(dt, EPI_STD, g, s));
      }
      // the 2 rows in front and the rows past the end that the Downsample windows read are its zero padding (the buffer is shared by the
      // levels and by longer earlier clips, so they are cleared here)
      TT_CHECK_HIP(hipMemsetAsync(e->xt, 0, (size_t)2 * C * es, s));
      TT_CHECK_HIP(hipMemsetAsync(offset_t(e->xt, (size_t)(L + 2) * C, es), 0, (size_t)4 * C * es, s));
      // Downsample: output row t reads operand rows 4 t - 2 .. 4 t + 2 = 5 C contiguous elements 4 t C into the guarded copy
      TT_TRY(gemm_launch(dt, EPI_STD, gemm_f32_args(e->xt, 4 * C, W.w_down[lv], 5 * C, cls_down(L), 2 * C, 5 * C, W.b_down[lv], y), s));
    }
    std::swap(x, y);
    L = cls_down(L);
    C *= 2;
  }
  // final: GroupNorm(1024) -> SiLU -> Conv1d(1024, 512, 1) into y
  TT_TRY(cls_gn(e, x, L, C, W.final_g, W.final_b, ACT_SILU, e->ht, s));
  TT_TRY(gemm_launch(dt, EPI_STD, gemm_f32_args(e->ht, C, W.w_final, C, L, kClsDim, C, W.b_final, y), s));
  x = y;
  for (int b = 0; b < TT_CLS_ATTN_BLOCKS; ++b) {
    const tt_cls_attn& A = W.attn[b];
    const int nq = b == TT_CLS_ATTN_BLOCKS - 1 ? 1 : L;  // only frame 0 of the last block reaches the head
    TT_TRY(cls_gn(e, x, L, kClsDim, A.norm_g, A.norm_b, ACT_NONE, e->ht, s));
    TT_TRY(gemm_launch(dt, EPI_STD, gemm_f32_args(e->ht, kClsDim, A.w_qkv, kClsDim, L, 3 * kClsDim, kClsDim, A.b_qkv, e->qkv), s));
    TT_TRY(cls_attention_launch(dt, e->qkv, L, nq, e->att, s));
    TT_TRY(gemm_launch(dt, EPI_STD, gemm_residual_args(e->att, kClsDim, A.w_proj, kClsDim, nq, kClsDim, kClsDim, A.b_proj, x, x), s));
  }
  return cls_head_launch(x, W.w_head, W.b_head, logits, emb, guard, s);
}

extern "C" {

int tt_cls_abi_version(void) { return 1; }  // ABI changes

size_t tt_cls_struct_size(int which) {
  switch (which) {
    case 0: return sizeof(tt_cls_config);
    case 1: return sizeof(tt_cls_weights);
  }
  return 0;
}

int tt_cls_max_samples(void) { return kClsMaxSamples; }

int tt_cls_create(const tt_cls_config* cfg, const tt_cls_weights* w, tt_cls** out) {
  TT_REQUIRE(cfg && w && out, "tt_cls_create: null argument");
  const tt_cls_config& c = *cfg;
  TT_REQUIRE(c.dtype == DT_BF16 || c.dtype == DT_F16 || c.dtype == DT_F32, "tt_cls_create: unknown dtype %d", c.dtype);
  TT_REQUIRE(c.spec_dim == 1 && c.base_channels == 32 && c.depth == TT_CLS_DEPTH && c.resnet_blocks == TT_CLS_RES_BLOCKS && c.kernel_size == 5 &&
                 c.downsample_factor == 4 && c.embedding_dim == kClsDim && c.attn_blocks == TT_CLS_ATTN_BLOCKS && c.heads == kClsHeads && c.classes == 2,
             "tt_cls_create: only the reference classifier (spec_dim 1, 32 base channels, depth 5, 2 resnet blocks, kernel 5, downsample 4, "
             "embedding 512, 4 attention blocks of 4 heads, 2 classes) is built");
  TT_REQUIRE(c.max_samples >= 1 && c.max_samples <= kClsMaxSamples, "tt_cls_create: max_samples %d (1 .. %d)", c.max_samples, kClsMaxSamples);
  TT_REQUIRE(w->w_init && w->b_init && w->w_final && w->w_head && w->b_head, "tt_cls_create: null weight");
  for (int l = 0; l < TT_CLS_DEPTH; ++l) {
    TT_REQUIRE(w->w_down[l] && w->b_down[l], "tt_cls_create: null Downsample weight at level %d", l);
    for (int r = 0; r < TT_CLS_RES_BLOCKS; ++r) TT_REQUIRE(w->res[l][r].w1 && w->res[l][r].w2, "tt_cls_create: null ResBlock weight");
  }
  for (int b = 0; b < TT_CLS_ATTN_BLOCKS; ++b) TT_REQUIRE(w->attn[b].w_qkv && w->attn[b].w_proj, "tt_cls_create: null attention weight");
  tt_cls* e = new tt_cls();
  e->cfg = c;
  e->w = *w;
  e->es = dtype_bytes(c.dtype);
  const size_t es = e->es;
  // sizes: level l has L_l rows of 32 * 2^l channels; level 0 is the widest f32 tensor, the wide levels (>= 2) the widest T operands
  size_t f32_rows = (size_t)c.max_samples * 32, t_elems = 0, gn_floats = 0;
  int L = c.max_samples;
  for (int l = 0; l <= TT_CLS_DEPTH; ++l) {
    const size_t C = (size_t)32 << l;
    f32_rows = std::max(f32_rows, ((size_t)L + 8) * C);
    if (l >= 2) t_elems = std::max(t_elems, ((size_t)L + 72) * C);
    if (l >= 2) gn_floats = std::max(gn_floats, groupnorm_partial_floats(1, L));
    if (l < TT_CLS_DEPTH) L = cls_down(L);
  }
  const int L5 = L;
  const size_t F = f32_rows + 64 * 32;
  int rc = e->open("tt_cls_create", true);
  if (!rc) rc = e->arena.alloc_t(&e->xa, F);
  if (!rc) rc = e->arena.alloc_t(&e->xb, F);
  if (!rc) rc = e->arena.alloc_t(&e->hf, F);
  if (!rc) rc = e->arena.alloc(&e->ht, t_elems * es);
  if (!rc) rc = e->arena.alloc(&e->xt, t_elems * es);
  if (!rc) rc = e->arena.alloc_t(&e->qkv, ((size_t)L5 + 64) * 3 * kClsDim);
  if (!rc) rc = e->arena.alloc(&e->att, ((size_t)L5 + 64) * kClsDim * es);
  if (!rc) rc = e->arena.alloc_t(&e->part, (size_t)std::max(cdiv(c.max_samples, kClsInitRows), cls_conv_blocks(c.max_samples)) * kClsGroups * 2);
  if (!rc) rc = e->arena.alloc_t(&e->stats, 2 * kClsGroups);
  if (!rc) rc = e->arena.alloc_t(&e->gnpart, gn_floats);
  if (rc) {
    tt_cls_destroy(e);
    return rc;
  }
  *out = e;
  return 0;
}

void tt_cls_destroy(tt_cls* e) {
  if (!e) return;
  e->close();
  delete e;
}

int tt_cls_run(tt_cls* e, const float* clip, int n, float* logits, float* embedding, void* stream) {
  TT_REQUIRE(e && clip && logits, "tt_cls_run: null argument");
  TT_REQUIRE(n >= 1 && n <= e->cfg.max_samples, "tt_cls_run: %d samples (1 .. %d)", n, e->cfg.max_samples);
  return e->sb.run((hipStream_t)stream, [&](hipStream_t s) -> int {
    TT_TRY(cls_forward(e, clip, n, logits, embedding, s));
    return e->guard.snapshot(s);
  });
}

int tt_cls_guard(tt_cls* e, int reset) {
  if (!e) { set_error("tt_cls_guard: null handle"); return -1; }
  return e->read_guard(reset, "tt_cls_guard", "classifier", e->cfg.dtype);
}

// ------------------------------------------------------------------------------ operator-level test entries (tortoise_mi355x_test.h)
size_t tt_op_cls_workspace(int L) { return sizeof(double) * 2 * kClsGroups * (size_t)std::max(cdiv(L > 0 ? L : 1, kClsInitRows), cls_conv_blocks(L > 0 ? L : 1)); }

int tt_op_cls_init(const float* x, int n, const float* w, const float* b, float* out, void* part, void* stream) {
  return cls_init_launch(x, n, w, b, out, (double*)part, (hipStream_t)stream);
}

int tt_op_cls_stats(const void* part, int nblocks, int L, int C, float* stats, void* stream) {
  return cls_stats_launch((const double*)part, nblocks, L, C, stats, nullptr, (hipStream_t)stream);
}

int tt_op_cls_conv(int dtype, int cin, int cout, int stride, const float* x, int Lin, const float* stats, const float* gamma, const float* beta,
                   const void* w, const float* b, const float* res, float* out, void* part, void* stream) {
  ClsConvArgs a;
  memset(&a, 0, sizeof(a));
  a.x = x; a.Lin = Lin; a.Lout = stride == 1 ? Lin : cls_down(Lin); a.stats = stats; a.gamma = gamma; a.beta = beta;
  a.w = w; a.bias = b; a.res = res; a.out = out; a.part = (double*)part;
  return cls_conv_launch(dtype, cin, cout, stride, a, (hipStream_t)stream);
}

int tt_op_cls_attention(int dtype, const float* qkv, int n, int nq, void* out, void* stream) {
  return cls_attention_launch(dtype, qkv, n, nq, out, (hipStream_t)stream);
}

int tt_op_cls_head(const float* x, const float* w, const float* b, float* logits, float* emb, void* stream) {
  return cls_head_launch(x, w, b, logits, emb, nullptr, (hipStream_t)stream);
}

}  // extern "C"
