// CTC forced alignment (include/tortoise_mi355x_ctc.h): the Viterbi path of a known target through per-frame logits.
//
//   ctc_align_kernel<K>  ONE WAVE PER CLIP (blockIdx.x = clip).  The 2L + 1 states are striped over the 64 lanes in contiguous chunks of K
//                        (K = 4 / 8 / 16: up to 255 / 511 / 1023 states), each lane's K path scores in registers.  K is even, so a lane's
//                        first state is a blank: it needs the previous lane's LAST score only (its s - 1; the first token state's s - 2 is
//                        the same value) - one DPP wave shift per frame, no LDS traffic and no barrier inside the recurrence.
//     emissions          the frame's log-probs do not depend on the path scores: the wave stages a chunk of frames (64 at vocab 32) in
//                        its LDS - the next chunk's logits are already in registers while the current one is consumed - and takes the f32
//                        log-softmax there, one lane per frame; a step then reads the blank's value (broadcast) and K / 2 token values.
//     backpointers       2 bits per state, one dword per lane and frame, written to the handle's workspace with coalesced vector stores.
//     backtrace          serial, but not one dependent global load per frame: 64 frames of backpointer words are staged in LDS, the walk
//                        runs on scalars (the word is read once and broadcast), lane f keeps the state of the chunk's frame f, and the
//                        chunk's path goes out in one coalesced store.
//     spans, conf        parallel passes over the finished path (one lane per frame, then one lane per token).
//   The three K forms are three launches over the same grid; a clip is taken by the form its own length selects and by no other, so what
//   a clip computes depends on nothing but the clip.
#include <math.h>
#include "runtime.h"
#include "../../include/tortoise_mi355x_ctc.h"

namespace tt {

constexpr int kCtcChunk = 64;                       // frames per backtrace chunk (= lanes: lane f keeps frame f's state)
constexpr int kCtcPre = 32;                         // logits a lane holds of the next emission chunk
constexpr int kCtcLpFloats = 64 * kCtcPre + 64;     // the chunk in LDS, rows padded to an odd stride
constexpr int kCtcMaxFrames = 1 << 20;

// frames per emission chunk: as many whole rows as 64 * kCtcPre values hold, at most one per lane
__host__ __device__ static inline int ctc_chunk_frames(int vocab) { return std::min(64, 64 * kCtcPre / vocab); }
__host__ __device__ static inline int ctc_k_of(int L) { return L <= 127 ? 4 : L <= 255 ? 8 : 16; }

// lane l gets lane l - 1's v, lane 0 gets -inf (wave_shr:1; bound_ctrl off keeps `old` where there is no source lane)
__device__ __forceinline__ float ctc_prev_lane(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(-INFINITY), __float_as_int(v), 0x138, 0xf, 0xf, false));
}

template <int K>
__global__ __launch_bounds__(64) void ctc_align_kernel(const float* __restrict__ logits, const int* __restrict__ frame_off,
                                                       const int* __restrict__ targets, const int* __restrict__ tok_off, int vocab, int blank,
                                                       int max_frames, int max_tokens, unsigned* __restrict__ bp_ws, float* __restrict__ lse_ws,
                                                       int* __restrict__ path, int* __restrict__ spans, float* __restrict__ conf,
                                                       float* __restrict__ score, int* __restrict__ status) {
  __shared__ float lp_s[kCtcLpFloats];
  __shared__ unsigned bp_s[kCtcChunk * 64];
  const int c = blockIdx.x, lane = threadIdx.x;
  const int f0 = frame_off[c], T = frame_off[c + 1] - f0;
  const int q0 = tok_off[c], L = tok_off[c + 1] - q0;
  // clips that run no recurrence are answered by the K = 4 launch (always made)
  if (f0 < 0 || q0 < 0 || T < 0 || L < 0 || T > max_frames || L > max_tokens) {
    if (K == 4 && lane == 0) status[c] = TT_CTC_REFUSED;
    return;
  }
  if (T == 0 || L == 0) {
    if (K == 4 && lane == 0) status[c] = TT_CTC_EMPTY;
    return;
  }
  if (ctc_k_of(L) != K) return;
  const int* tg = targets + q0;
  int rep = 0, bad = 0;
  for (int i = lane; i < L; i += 64) {
    const int y = tg[i];
    bad |= (y < 0 || y >= vocab || y == blank);
    rep += (i > 0 && y == tg[i - 1]);
  }
  for (int d = 32; d >= 1; d >>= 1) rep += __shfl_xor(rep, d);
  if (__any(bad)) {
    if (lane == 0) status[c] = TT_CTC_REFUSED;
    return;
  }
  if (T < L + rep) {
    if (lane == 0) status[c] = TT_CTC_INFEASIBLE;
    return;
  }
  const int S = 2 * L + 1;
  // this lane's token states: odd j, state lane * K + j, token lane * K / 2 + j / 2.  States beyond 2L never feed a state below them and
  // are never visited by the backtrace: they read the blank and compute freely.
  int lab[K / 2];
  unsigned skip = 0;
#pragma unroll
  for (int h = 0; h < K / 2; ++h) {
    const int tok = lane * (K / 2) + h;
    lab[h] = blank;
    if (tok < L) {
      lab[h] = tg[tok];
      if (tok > 0 && tg[tok] != tg[tok - 1]) skip |= 1u << h;
    }
  }
  // a virtual frame -1 holding 0 in state 0 and -inf elsewhere: the step below then yields the start row (lp + 0 is exact)
  float a[K];
#pragma unroll
  for (int j = 0; j < K; ++j) a[j] = -INFINITY;
  if (lane == 0) a[0] = 0.f;

  const int FC = ctc_chunk_frames(vocab), VP = vocab | 1;
  const float* lg = logits + (size_t)f0 * vocab;
  unsigned* bp_clip = bp_ws + (size_t)c * max_frames * 64;
  float* lse_clip = lse_ws + (size_t)c * max_frames;
  float pre[kCtcPre];
  auto fetch = [&](int t0) {
    const int n = t0 < T ? std::min(FC, T - t0) * vocab : 0;
    const float* src = lg + (size_t)t0 * vocab;
#pragma unroll
    for (int i = 0; i < kCtcPre; ++i) {
      const int e = i * 64 + lane;
      pre[i] = e < n ? src[e] : 0.f;
    }
  };
  fetch(0);
  for (int t0 = 0; t0 < T; t0 += FC) {
    const int nf = std::min(FC, T - t0);
    __syncthreads();  // the previous chunk's reads are done
#pragma unroll
    for (int i = 0; i < kCtcPre; ++i) {
      const int e = i * 64 + lane;
      if (e < nf * vocab) {
        const int f = e / vocab;
        lp_s[f * VP + (e - f * vocab)] = pre[i];
      }
    }
    fetch(t0 + FC);  // in flight while this chunk is consumed
    __syncthreads();
    if (lane < nf) {  // f32 log-softmax of row `lane`, in place
      float* row = lp_s + lane * VP;
      float m = row[0];
      for (int v = 1; v < vocab; ++v) m = fmaxf(m, row[v]);
      float sum = 0.f;
      for (int v = 0; v < vocab; ++v) sum += expf(row[v] - m);
      const float lse = m + logf(sum);
      for (int v = 0; v < vocab; ++v) row[v] -= lse;
      lse_clip[t0 + lane] = lse;
    }
    __syncthreads();
    for (int f = 0; f < nf; ++f) {
      const float* row = lp_s + f * VP;
      const float eb = row[blank];
      float et[K / 2];
#pragma unroll
      for (int h = 0; h < K / 2; ++h) et[h] = row[lab[h]];
      const float up = ctc_prev_lane(a[K - 1]);
      unsigned word = 0;
#pragma unroll
      for (int j = K - 1; j >= 0; --j) {  // descending: a[j - 1], a[j - 2] are still the previous frame's
        const float x1 = j >= 1 ? a[j - 1] : up;
        float v = a[j];
        unsigned b = 0;
        if (x1 > v) { v = x1; b = 1; }
        if (j & 1) {
          const float x2 = j >= 2 ? a[j - 2] : up;
          if (((skip >> (j >> 1)) & 1u) && x2 > v) { v = x2; b = 2; }
          a[j] = et[j >> 1] + v;
        } else {
          a[j] = eb + v;
        }
        word |= b << (2 * j);
      }
      bp_clip[(size_t)(t0 + f) * 64 + lane] = word;
    }
  }
  // end state: 2L unless 2L - 1 is strictly greater
  __syncthreads();
  float* a_s = (float*)bp_s;
#pragma unroll
  for (int j = 0; j < K; ++j) a_s[lane * K + j] = a[j];
  __syncthreads();
  const float a_last = a_s[S - 1], a_tok = a_s[S - 2];
  const float total = a_tok > a_last ? a_tok : a_last;
  int s = __builtin_amdgcn_readfirstlane(a_tok > a_last ? S - 2 : S - 1);
  __syncthreads();
  // backtrace, a chunk of frames at a time from the end
  for (int t0 = (T - 1) / kCtcChunk * kCtcChunk; t0 >= 0; t0 -= kCtcChunk) {
    const int nf = std::min(kCtcChunk, T - t0);
    for (int f = 0; f < nf; ++f) bp_s[f * 64 + lane] = bp_clip[(size_t)(t0 + f) * 64 + lane];  // (each lane reads back its own words)
    __syncthreads();
    int mine = 0;
    for (int f = nf - 1; f >= 0; --f) {
      if (lane == f) mine = s;
      if (t0 + f > 0) {
        const unsigned w = __builtin_amdgcn_readfirstlane(bp_s[f * 64 + s / K]);
        s = std::max(s - (int)((w >> (2 * (s % K))) & 3u), 0);
      }
    }
    if (lane < nf) path[f0 + t0 + lane] = mine;
    __syncthreads();
  }
  // spans: one lane per frame
  for (int t = lane; t < T; t += 64) {
    const int st = path[f0 + t];
    if (st & 1) {
      const int l = q0 + (st >> 1);
      if (t == 0 || path[f0 + t - 1] != st) spans[2 * (size_t)l] = t;
      if (t == T - 1 || path[f0 + t + 1] != st) spans[2 * (size_t)l + 1] = t;
    }
  }
  __syncthreads();
  // confidence: one lane per token
  for (int l = lane; l < L; l += 64) {
    const int first = std::max(spans[2 * (size_t)(q0 + l)], 0), last = std::min(spans[2 * (size_t)(q0 + l) + 1], T - 1);
    const int y = tg[l];
    float sum = 0.f;
    for (int t = first; t <= last; ++t) sum += expf(lg[(size_t)t * vocab + y] - lse_clip[t]);
    conf[q0 + l] = sum / (float)(last - first + 1);
  }
  if (lane == 0) {
    score[c] = total;
    status[c] = TT_CTC_OK;
  }
}

}  // namespace tt

using namespace tt;

struct tt_ctc : EngineHandle {
  int max_frames = 0, max_tokens = 0, max_clips = 0, vocab = 0, blank = 0;
  unsigned* bp = nullptr;  // [max_clips][max_frames][64] backpointer words
  float* lse = nullptr;    // [max_clips][max_frames] log-sum-exp of every frame
};

extern "C" {

int tt_ctc_abi_version(void) { return 1; }  // ABI changes

int tt_ctc_create(int max_frames, int max_tokens, int max_clips, int vocab, int blank, tt_ctc** out) {
  TT_REQUIRE(out, "tt_ctc_create: null argument");
  TT_REQUIRE(max_frames >= 1 && max_frames <= kCtcMaxFrames, "tt_ctc_create: max_frames %d (1 .. %d)", max_frames, kCtcMaxFrames);
  TT_REQUIRE(max_tokens >= 1 && max_tokens <= TT_CTC_MAX_TOKENS, "tt_ctc_create: max_tokens %d (1 .. %d)", max_tokens, TT_CTC_MAX_TOKENS);
  TT_REQUIRE(max_clips >= 1 && max_clips <= TT_CTC_MAX_CLIPS, "tt_ctc_create: max_clips %d (1 .. %d)", max_clips, TT_CTC_MAX_CLIPS);
  TT_REQUIRE(vocab >= 2 && vocab <= TT_CTC_MAX_VOCAB, "tt_ctc_create: vocab %d (2 .. %d)", vocab, TT_CTC_MAX_VOCAB);
  TT_REQUIRE(blank >= 0 && blank < vocab, "tt_ctc_create: blank %d is outside the vocabulary of %d", blank, vocab);
  tt_ctc* e = new tt_ctc();
  e->max_frames = max_frames; e->max_tokens = max_tokens; e->max_clips = max_clips; e->vocab = vocab; e->blank = blank;
  int rc = e->open("tt_ctc_create", false);
  if (!rc) rc = e->arena.alloc_t(&e->bp, (size_t)max_clips * max_frames * 64, false);
  if (!rc) rc = e->arena.alloc_t(&e->lse, (size_t)max_clips * max_frames, false);
  if (rc) {
    tt_ctc_destroy(e);
    return rc;
  }
  *out = e;
  return 0;
}

void tt_ctc_destroy(tt_ctc* e) {
  if (!e) return;
  e->close();
  delete e;
}

int tt_ctc_align(tt_ctc* e, int n, const float* logits, const int* frame_off, const int* targets, const int* tok_off, int* path, int* spans,
                 float* conf, float* score, int* status, void* stream) {
  TT_REQUIRE(e && logits && frame_off && targets && tok_off && path && spans && conf && score && status, "tt_ctc_align: null argument");
  TT_REQUIRE(n >= 1 && n <= e->max_clips, "tt_ctc_align: %d clips (1 .. %d)", n, e->max_clips);
  return e->sb.run((hipStream_t)stream, [&](hipStream_t s) -> int {
    // the offsets live on the device: every K form the handle's longest target can select is launched, and a clip runs in its own only
    ctc_align_kernel<4><<<n, 64, 0, s>>>(logits, frame_off, targets, tok_off, e->vocab, e->blank, e->max_frames, e->max_tokens, e->bp, e->lse, path,
                                         spans, conf, score, status);
    if (e->max_tokens > 127)
      ctc_align_kernel<8><<<n, 64, 0, s>>>(logits, frame_off, targets, tok_off, e->vocab, e->blank, e->max_frames, e->max_tokens, e->bp, e->lse,
                                           path, spans, conf, score, status);
    if (e->max_tokens > 255)
      ctc_align_kernel<16><<<n, 64, 0, s>>>(logits, frame_off, targets, tok_off, e->vocab, e->blank, e->max_frames, e->max_tokens, e->bp, e->lse,
                                            path, spans, conf, score, status);
    TT_CHECK_HIP(hipGetLastError());
    return 0;
  });
}

}  // extern "C"
