// Pauses and silence (include/tortoise_mi355x_sil.h): speech regions of finished clips, edge trimming and pause capping.
//
//   sil_slot_kernel     the work is (clip, tile of kSilTile = 64 slots of 120 samples).  A fixed grid walks the list clip 0's tiles, clip 1's
//                       tiles, ...: every workgroup derives that list from the offsets (at most 64 clips, a uniform loop), so nothing about a
//                       slot depends on where its clip stands in the batch or on which workgroup computes it.  The tile's samples are staged
//                       in LDS with coalesced loads - float4 where the address is 16-byte aligned and the four samples lie inside the clip,
//                       single samples at the ragged ends - by all 256 threads, in rows of 121 words, so the one wave whose lanes then each
//                       walk one slot in ascending order (the header's f64 FMA chain) reads 64 different banks.  q goes to the handle's
//                       workspace.  (The form built first staged 128 slots with 128 threads, 30 dependent load-store rounds per thread:
//                       21.7 us per launch against 9.6 for the plan; profiles/r21_silence.txt has both.)
//   sil_plan_kernel     one workgroup of kSilPlan = 1024 threads per clip, everything in chunks of 1024 frames / regions with a carry:
//                       frame energies and their maximum (shuffles -> LDS; a maximum does not depend on the order), the threshold, prev(f)
//                       by a forward max-scan and next(f) by a backward min-scan, the labels, region bounds by a prefix count of rising
//                       edges, and for the edit the removed lengths and cut counts by two prefix sums over the regions, which give every
//                       segment its place.  Writes R, regions, E, (e_f), K, segments, n_out and the status.
//   sil_render_kernel   (clip, tile of 1024 outputs), the same walk over a tile list made from n_out.  256 threads, four outputs each, 256
//                       apart (coalesced).  An output finds its segment by binary search in the clip's list - a search whose trip count
//                       depends on K alone, so a thread's four searches advance together and their loads overlap - and copies, cross-fades
//                       or fades.
//
// No atomics: the only cross-workgroup value, E, is reduced inside the clip's plan workgroup.
#include <math.h>
#include "runtime.h"
#include "../../include/tortoise_mi355x_sil.h"

namespace tt {

constexpr int kSilS = TT_SIL_SLOT, kSilH = TT_SIL_HOP, kSilX = TT_SIL_FADE;
constexpr int kSilTile = 64;             // slots of a sil_slot_kernel tile: one wave sums them
constexpr int kSilStage = 256;           // threads of sil_slot_kernel: all of them stage the tile
constexpr int kSilRow = kSilS + 1;       // LDS words of a staged slot (odd: conflict-free column walks)
constexpr int kSilPlan = 1024;           // threads of the plan workgroup = frames of a scan chunk
constexpr int kSilOut = 1024;            // outputs of a render tile
constexpr int kSilRender = 256;          // threads of sil_render_kernel: kSilPer outputs each, kSilRender apart
constexpr int kSilPer = kSilOut / kSilRender;
constexpr int kSilGrid = 2048;           // workgroups of the two tiled kernels (they stride over the tile list)
static_assert(TT_SIL_HOP == 2 * TT_SIL_SLOT && TT_SIL_FRAME == 4 * TT_SIL_SLOT && kSilS % 4 == 0, "a frame is four slots, a hop two");
static_assert(kSilTile * kSilRow * sizeof(float) <= 64 * 1024 && kSilPlan >= TT_SIL_MAX_CLIPS && kSilStage >= TT_SIL_MAX_CLIPS && kSilRender >= TT_SIL_MAX_CLIPS && kSilTile <= 64, "LDS plan");

__host__ __device__ static inline int sil_slots(int n) { return (n + kSilS - 1) / kSilS; }
__host__ __device__ static inline int sil_frames(int n) { return (n + kSilH - 1) / kSilH; }
__host__ __device__ static inline int sil_max_regions(int n) { return (sil_frames(n) + 1) / 2; }

struct SilArgs {
  int n_clips, max_samples, trim;  // trim: par has 5 columns and the edit is planned
  const float* audio;
  const int* in_off;
  const double* thr;
  const int* par;
  const int* reg_off;
  const int* seg_off;  // trim
  const int* frm_off;  // with energies
  double* energies;
};

// the status of clip c before its audio is read: 0 (go on), TT_SIL_EMPTY or TT_SIL_REFUSED
__device__ static inline int sil_clip(const SilArgs& a, int c, int* n_p) {
  const int i0 = a.in_off[c], n = a.in_off[c + 1] - i0;
  *n_p = 0;
  if (i0 < 0 || n < 0) return TT_SIL_REFUSED;
  if (n == 0) return TT_SIL_EMPTY;
  if (n > a.max_samples) return TT_SIL_REFUSED;
  const double rel = a.thr[2 * c], floor_e = a.thr[2 * c + 1];
  if (!(rel >= 0.0 && rel <= 1.0) || !(floor_e >= 0.0 && floor_e <= 1.7e308)) return TT_SIL_REFUSED;  // (NaN fails both)
  const int* p = a.par + (a.trim ? 5 : 2) * c;
  if (p[0] < 0 || p[0] > TT_SIL_MAX_FRAMES_PARAM || p[1] < 0 || p[1] > TT_SIL_MAX_FRAMES_PARAM) return TT_SIL_REFUSED;
  const int cap = sil_max_regions(n);
  if (a.reg_off[c] < 0 || a.reg_off[c + 1] - a.reg_off[c] < cap) return TT_SIL_REFUSED;
  if (a.energies && (a.frm_off[c] < 0 || a.frm_off[c + 1] - a.frm_off[c] < sil_frames(n))) return TT_SIL_REFUSED;
  if (a.trim) {
    if (p[2] < -1 || p[2] > TT_SIL_MAX_SAMPLES || p[3] < -1 || p[3] > TT_SIL_MAX_SAMPLES) return TT_SIL_REFUSED;
    if (p[4] != -1 && (p[4] < kSilX || p[4] > TT_SIL_MAX_SAMPLES)) return TT_SIL_REFUSED;
    if (a.seg_off[c] < 0 || a.seg_off[c + 1] - a.seg_off[c] < cap) return TT_SIL_REFUSED;
  }
  *n_p = n;
  return 0;
}

// tile g of the list (clip 0's tiles, clip 1's, ...) -> its clip and its index in the clip; false past the end.  units_s[c]: the clip's
// units (slots or outputs; 0: skipped), per: units of a tile.
__device__ static inline bool sil_tile(const int* units_s, int n_clips, int per, int g, int* c_p, int* tile_p) {
  int first = 0;
  for (int c = 0; c < n_clips; ++c) {
    const int tiles = (units_s[c] + per - 1) / per;
    if (g < first + tiles) {
      *c_p = c;
      *tile_p = g - first;
      return true;
    }
    first += tiles;
  }
  return false;
}

__global__ __launch_bounds__(kSilStage) void sil_slot_kernel(SilArgs a, int slot_cap, double* __restrict__ q_ws) {
  __shared__ float x_s[kSilTile * kSilRow];
  __shared__ int slots_s[TT_SIL_MAX_CLIPS];
  const int t = threadIdx.x;
  if (t < TT_SIL_MAX_CLIPS) {
    int n = 0;
    if (t < a.n_clips) sil_clip(a, t, &n);
    slots_s[t] = sil_slots(n);  // 0: not read
  }
  __syncthreads();
  for (int g = blockIdx.x;; g += gridDim.x) {
    int c, tile;
    if (!sil_tile(slots_s, a.n_clips, kSilTile, g, &c, &tile)) return;  // (uniform over the workgroup)
    const int n = a.in_off[c + 1] - a.in_off[c];
    const int s0 = tile * kSilTile;                                   // the tile's first slot
    const int len = min(n - s0 * kSilS, kSilTile * kSilS);            // its samples, >= 1
    const float* x = a.audio + a.in_off[c] + (size_t)s0 * kSilS;
    const int head = min(len, (int)((4 - (((uintptr_t)x >> 2) & 3)) & 3));  // samples before the first 16-byte boundary
    __syncthreads();  // the previous tile's reads of x_s are done
    if (t < head) x_s[t] = x[t];  // (sample e of the tile sits at x_s[e / S * kSilRow + e % S]; head < 4 <= S)
    for (int e = head + 4 * t; e < len; e += 4 * kSilStage) {
      if (e + 4 <= len) {
        const float4 v = *reinterpret_cast<const float4*>(x + e);
        const float w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) x_s[(e + i) / kSilS * kSilRow + (e + i) % kSilS] = w[i];
      } else {
        for (int i = 0; e + i < len; ++i) x_s[(e + i) / kSilS * kSilRow + (e + i) % kSilS] = x[e + i];
      }
    }
    __syncthreads();
    const int m = t < kSilTile ? min(kSilS, len - t * kSilS) : 0;  // this thread's slot holds m samples (<= 0: none, or past the last slot)
    if (m > 0) {
      const float* row = x_s + t * kSilRow;
      double q = 0.0;
      for (int i = 0; i < m; ++i) {
        const double v = (double)row[i];
        q = fma(v, v, q);
      }
      q_ws[(size_t)c * slot_cap + s0 + t] = q;
    }
  }
}

// Inclusive scan of v over the workgroup's kSilPlan threads with `op` (associative; any order of equal results), *total: the last
// thread's value.  lds: kSilPlan / 64 ints.  Ends with a barrier, so lds can be used again at once.
template <class Op>
__device__ static inline int sil_scan(int v, Op op, int* lds, int* total) {
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(v, d);
    if (lane >= d) v = op(o, v);
  }
  if (lane == 63) lds[w] = v;
  __syncthreads();
  int tot = lds[0];
  int before = 0;
  bool have = false;
#pragma unroll
  for (int i = 1; i < kSilPlan / 64; ++i) {  // (tot: waves 0 .. i - 1)
    if (i == w) {
      before = tot;
      have = true;
    }
    tot = op(tot, lds[i]);
  }
  if (have) v = op(before, v);
  *total = tot;
  __syncthreads();
  return v;
}

struct SilMax { __device__ int operator()(int a, int b) const { return max(a, b); } };
struct SilMin { __device__ int operator()(int a, int b) const { return min(a, b); } };
struct SilAdd { __device__ int operator()(int a, int b) const { return a + b; } };

__device__ static inline double sil_frame_energy(const double* __restrict__ q, int slots, int f) {
  const int s = 2 * f;
  const double q0 = q[s], q1 = s + 1 < slots ? q[s + 1] : 0.0, q2 = s + 2 < slots ? q[s + 2] : 0.0, q3 = s + 3 < slots ? q[s + 3] : 0.0;
  return ((q0 + q1) + q2) + q3;
}

__global__ __launch_bounds__(kSilPlan) void sil_plan_kernel(SilArgs a, int slot_cap, int frame_cap, const double* __restrict__ q_ws,
                                                            int* __restrict__ prev_ws, unsigned char* __restrict__ lab_ws,
                                                            int* __restrict__ n_regions, int* __restrict__ regions, double* __restrict__ peak,
                                                            int* __restrict__ n_out_p, int* __restrict__ n_segments, int* __restrict__ segments,
                                                            int* __restrict__ status) {
  __shared__ int scan_s[kSilPlan / 64];
  __shared__ double max_s[kSilPlan / 64];
  const int c = blockIdx.x, t = threadIdx.x;
  int n;
  const int st = sil_clip(a, c, &n);
  if (st) {  // (uniform)
    if (t == 0) status[c] = st;
    return;
  }
  const int slots = sil_slots(n), F = sil_frames(n);
  const double* q = q_ws + (size_t)c * slot_cap;
  int* prev = prev_ws + (size_t)c * frame_cap;
  unsigned char* lab = lab_ws + (size_t)c * frame_cap;
  int* reg = regions + 2 * (size_t)a.reg_off[c];
  double* en = a.energies ? a.energies + a.frm_off[c] : nullptr;
  const int* par = a.par + (a.trim ? 5 : 2) * c;
  const int min_sil = par[0], pad = par[1];

  // E
  double e_max = 0.0;
  for (int f = t; f < F; f += kSilPlan) {
    const double e = sil_frame_energy(q, slots, f);
    if (en) en[f] = e;
    e_max = fmax(e_max, e);
  }
  for (int s = 32; s >= 1; s >>= 1) e_max = fmax(e_max, __shfl_xor(e_max, s));
  if ((t & 63) == 0) max_s[t >> 6] = e_max;
  __syncthreads();
  e_max = max_s[0];
#pragma unroll
  for (int w = 1; w < kSilPlan / 64; ++w) e_max = fmax(e_max, max_s[w]);
  const double thr = fmax(a.thr[2 * c + 1], a.thr[2 * c] * e_max);

  // prev(f): forward, -1 where none
  int carry = -1, tot;
  for (int f0 = 0; f0 < F; f0 += kSilPlan) {
    const int f = f0 + t;
    const int v = f < F && sil_frame_energy(q, slots, f) > thr ? f : -1;
    const int p = max(carry, sil_scan(v, SilMax(), scan_s, &tot));
    if (f < F) prev[f] = p;
    carry = max(carry, tot);
  }
  const bool silent = carry < 0;  // no active frame
  // next(f): backward, F where none; the label at once
  constexpr int kNone = 0x3fffffff;
  carry = kNone;
  for (int f1 = F; f1 > 0; f1 -= kSilPlan) {
    const int f = f1 - 1 - t;
    const int v = f >= 0 && sil_frame_energy(q, slots, f) > thr ? f : kNone;
    const int nx = min(carry, sil_scan(v, SilMin(), scan_s, &tot));
    if (f >= 0) {
      const int p = prev[f];
      const bool hp = p >= 0, hn = nx != kNone;
      lab[f] = (hp && hn && nx - p - 1 < min_sil) || (hp && f - p <= pad) || (hn && nx - f <= pad);  // (an active frame: p = nx = f)
    }
    carry = min(carry, tot);
  }
  __syncthreads();  // lab is complete
  // regions: a rising edge opens region (count of rising edges so far) - 1, the falling edge of the same run closes it
  int R = 0;
  for (int f0 = 0; f0 < F; f0 += kSilPlan) {
    const int f = f0 + t;
    const bool sp = f < F && lab[f];
    const bool rise = sp && (f == 0 || !lab[f - 1]), fall = sp && (f + 1 == F || !lab[f + 1]);
    const int r = R + sil_scan(rise ? 1 : 0, SilAdd(), scan_s, &tot) - 1;
    if (rise) reg[2 * r] = f * kSilH;
    if (fall) reg[2 * r + 1] = min((f + 1) * kSilH, n);
    R += tot;
  }
  if (t == 0) {
    n_regions[c] = R;
    peak[c] = e_max;
  }
  if (!a.trim) {
    if (t == 0) status[c] = silent ? TT_SIL_SILENT : TT_SIL_OK;
    return;
  }
  int* seg = segments + 3 * (size_t)a.seg_off[c];
  if (R == 0) {  // SILENT: returned as it is
    if (t == 0) {
      seg[0] = 0, seg[1] = 0, seg[2] = n;
      n_segments[c] = 1;
      n_out_p[c] = n;
      status[c] = TT_SIL_SILENT;
    }
    return;
  }
  __syncthreads();  // reg is complete
  const int lead = par[2], trail = par[3], M = par[4];
  const int M2 = (M + kSilX) / 2;
  const int G0 = reg[0], Gt = n - reg[2 * R - 1];
  const int D0 = lead >= 0 && G0 > lead ? G0 - lead : 0, Dt = trail >= 0 && Gt > trail ? Gt - trail : 0;
  int removed = D0, K = 1;  // the carries: samples removed before region r's start, segments begun
  for (int r0 = 0; r0 < R; r0 += kSilPlan) {
    const int r = r0 + t;
    int G = 0;
    bool cut = false;
    if (r >= 1 && r < R) {
      G = reg[2 * r] - reg[2 * r - 1];
      cut = M >= 0 && G >= M + kSilX;
    }
    const int rem = removed + sil_scan(cut ? G - M : 0, SilAdd(), scan_s, &tot);
    removed += tot;
    const int k = K + sil_scan(cut ? 1 : 0, SilAdd(), scan_s, &tot) - 1;
    K += tot;
    if (r == 0) seg[0] = 0, seg[1] = D0;
    if (cut) {
      const int i = reg[2 * r] - M2 + kSilX;
      seg[3 * k] = i - rem;
      seg[3 * k + 1] = i;
    }
  }
  const int n_out = n - removed - Dt;
  __syncthreads();  // every segment's start is written
  for (int k = t; k < K; k += kSilPlan) seg[3 * k + 2] = (k + 1 < K ? seg[3 * (k + 1)] : n_out) - seg[3 * k];
  if (t == 0) {
    n_segments[c] = K;
    n_out_p[c] = n_out;
    status[c] = K > 1 || D0 > 0 || Dt > 0 ? TT_SIL_OK : TT_SIL_UNCHANGED;
  }
}

__global__ __launch_bounds__(kSilRender) void sil_render_kernel(SilArgs a, const int* __restrict__ n_out_p, const int* __restrict__ n_segments,
                                                                const int* __restrict__ segments, const int* __restrict__ status,
                                                                float* __restrict__ out) {
  __shared__ int nout_s[TT_SIL_MAX_CLIPS];
  const int t = threadIdx.x;
  if (t < TT_SIL_MAX_CLIPS) {
    int n_out = 0;
    if (t < a.n_clips && status[t] <= TT_SIL_SILENT) n_out = n_out_p[t];
    nout_s[t] = n_out;  // 0: nothing is written
  }
  __syncthreads();
  for (int g = blockIdx.x;; g += gridDim.x) {
    int c, tile;
    if (!sil_tile(nout_s, a.n_clips, kSilOut, g, &c, &tile)) return;
    const int n_out = nout_s[c], n = a.in_off[c + 1] - a.in_off[c], K = n_segments[c];
    const float* x = a.audio + a.in_off[c];
    float* y = out + a.in_off[c];
    const int* seg = segments + 3 * (size_t)a.seg_off[c];
    const int xe = min(kSilX, n_out);
    const bool lead_cut = seg[1] > 0, trail_cut = seg[3 * (K - 1) + 1] + seg[3 * (K - 1) + 2] < n;
    int m[kSilPer], k[kSilPer];
#pragma unroll
    for (int i = 0; i < kSilPer; ++i) {
      m[i] = min(tile * kSilOut + i * kSilRender + t, n_out - 1);  // (an output past the end searches like the last one and writes nothing)
      k[i] = 0;
    }
    // the last segment whose o_k <= m (o_0 = 0): the trip count depends on K alone, so the kSilPer searches advance together
    for (int len = K; len > 1;) {
      const int half = len >> 1;
#pragma unroll
      for (int i = 0; i < kSilPer; ++i)
        if (seg[3 * (k[i] + half)] <= m[i]) k[i] += half;
      len -= half;
    }
#pragma unroll
    for (int i = 0; i < kSilPer; ++i) {
      if (tile * kSilOut + i * kSilRender + t >= n_out) continue;
      const int mi = m[i], ki = k[i];
      float v = x[seg[3 * ki + 1] + (mi - seg[3 * ki])];
      if (ki + 1 < K) {
        const int j = mi - (seg[3 * (ki + 1)] - kSilX);
        if (j >= 0) {
          const float tail = x[seg[3 * (ki + 1) + 1] - kSilX + j];
          const float w = (float)(2 * j + 1) / (float)(2 * kSilX);
          v = fmaf(w, tail - v, v);
        }
      }
      const int jm = n_out - 1 - mi;
      if (lead_cut && mi < xe) v = v * ((float)(2 * mi + 1) / (float)(2 * kSilX));
      if (trail_cut && jm < xe) v = v * ((float)(2 * jm + 1) / (float)(2 * kSilX));  // (after the fade-in; the two never meet, see the header)
      y[mi] = v;
    }
  }
}

}  // namespace tt

using namespace tt;

struct tt_sil : EngineHandle {
  int max_samples = 0, max_clips = 0, slot_cap = 0, frame_cap = 0;
  double* q = nullptr;           // [max_clips, slot_cap] slot energies
  int* prev = nullptr;           // [max_clips, frame_cap] prev(f)
  unsigned char* lab = nullptr;  // [max_clips, frame_cap] speech labels
};

extern "C" {

int tt_sil_abi_version(void) { return 1; }  // ABI changes

int tt_sil_frames(int n) { return n >= 1 && n <= TT_SIL_MAX_SAMPLES ? sil_frames(n) : 0; }
int tt_sil_max_regions(int n) { return n >= 1 && n <= TT_SIL_MAX_SAMPLES ? sil_max_regions(n) : 0; }

int tt_sil_create(int max_samples, int max_clips, tt_sil** out) {
  TT_REQUIRE(out, "tt_sil_create: null argument");
  TT_REQUIRE(max_samples >= 1 && max_samples <= TT_SIL_MAX_SAMPLES, "tt_sil_create: max_samples %d (1 .. %d)", max_samples, TT_SIL_MAX_SAMPLES);
  TT_REQUIRE(max_clips >= 1 && max_clips <= TT_SIL_MAX_CLIPS, "tt_sil_create: max_clips %d (1 .. %d)", max_clips, TT_SIL_MAX_CLIPS);
  tt_sil* e = new tt_sil();
  e->max_samples = max_samples; e->max_clips = max_clips;
  e->slot_cap = sil_slots(max_samples); e->frame_cap = sil_frames(max_samples);
  int rc = e->open("tt_sil_create", false);
  if (!rc) rc = e->arena.alloc_t(&e->q, (size_t)max_clips * e->slot_cap, false);
  if (!rc) rc = e->arena.alloc_t(&e->prev, (size_t)max_clips * e->frame_cap, false);
  if (!rc) rc = e->arena.alloc_t(&e->lab, (size_t)max_clips * e->frame_cap, false);
  if (rc) {
    tt_sil_destroy(e);
    return rc;
  }
  *out = e;
  return 0;
}

void tt_sil_destroy(tt_sil* e) {
  if (!e) return;
  e->close();
  delete e;
}

static int sil_run(tt_sil* e, const SilArgs& a, float* out, int* n_out, int* n_regions, int* regions, int* n_segments, int* segments,
                   double* peak, int* status, void* stream) {
  return e->sb.run((hipStream_t)stream, [&](hipStream_t s) -> int {
    sil_slot_kernel<<<kSilGrid, kSilStage, 0, s>>>(a, e->slot_cap, e->q);
    TT_CHECK_HIP(hipGetLastError());
    sil_plan_kernel<<<a.n_clips, kSilPlan, 0, s>>>(a, e->slot_cap, e->frame_cap, e->q, e->prev, e->lab, n_regions, regions, peak, n_out,
                                                   n_segments, segments, status);
    TT_CHECK_HIP(hipGetLastError());
    if (a.trim) {
      sil_render_kernel<<<kSilGrid, kSilRender, 0, s>>>(a, n_out, n_segments, segments, status, out);
      TT_CHECK_HIP(hipGetLastError());
    }
    return 0;
  });
}

int tt_sil_find(tt_sil* e, int n_clips, const float* audio, const int* in_off, const double* thr, const int* par, const int* reg_off,
                const int* frm_off, int* n_regions, int* regions, double* peak, double* energies, int* status, void* stream) {
  TT_REQUIRE(e && audio && in_off && thr && par && reg_off && n_regions && regions && peak && status, "tt_sil_find: null argument");
  TT_REQUIRE(!energies == !frm_off, "tt_sil_find: energies and frm_off go together");
  TT_REQUIRE(n_clips >= 1 && n_clips <= e->max_clips, "tt_sil_find: %d clips (1 .. %d)", n_clips, e->max_clips);
  const SilArgs a{n_clips, e->max_samples, 0, audio, in_off, thr, par, reg_off, nullptr, frm_off, energies};
  return sil_run(e, a, nullptr, nullptr, n_regions, regions, nullptr, nullptr, peak, status, stream);
}

int tt_sil_trim(tt_sil* e, int n_clips, const float* audio, const int* in_off, const double* thr, const int* par, const int* reg_off,
                const int* seg_off, float* out, int* n_out, int* n_regions, int* regions, int* n_segments, int* segments, double* peak,
                int* status, void* stream) {
  TT_REQUIRE(e && audio && in_off && thr && par && reg_off && seg_off && out && n_out && n_regions && regions && n_segments && segments &&
                 peak && status, "tt_sil_trim: null argument");
  TT_REQUIRE(out != audio, "tt_sil_trim: out must not overlap audio");
  TT_REQUIRE(n_clips >= 1 && n_clips <= e->max_clips, "tt_sil_trim: %d clips (1 .. %d)", n_clips, e->max_clips);
  const SilArgs a{n_clips, e->max_samples, 1, audio, in_off, thr, par, reg_off, seg_off, nullptr, nullptr};
  return sil_run(e, a, out, n_out, n_regions, regions, n_segments, segments, peak, status, stream);
}

}  // extern "C"
