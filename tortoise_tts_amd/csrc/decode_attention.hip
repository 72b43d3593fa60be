// Decode attention for gfx950, head_dim = 64: one new query per (sequence, head) against [shared prefix | own generated keys].
// HBM-bound on the per-sequence cache: keys are stored in 16-byte dim-chunks that are key-major so the lane-per-key dot product
// issues fully coalesced 1-KiB loads; values are row-major and read 8 whole rows (1 KiB) per wave instruction.
//
// Three kernels, one attention:
//   decode_attn_kernel            one wave per (sequence, head), everything from memory (the prefix does not fit the LDS)
//   decode_attn_lds_kernel<NSEQ>  a workgroup = NSEQ sequences of one head, the head's prefix staged into the LDS once
//   decode_qkv_attn_kernel        the NSEQ = 16 geometry with the step's QKV projection computed in the same launch
// They are built from the wave-level steps below (dec_*), so the arithmetic and the summation order per (sequence, head) are the
// same code in all three: tests/test_gpu_decode_attn_forms.py and tests/test_gpu_qkv_attn.py hold them to equal bits.
#include "ops.h"

namespace tt {

// 8-wide dot product with fp32 accumulation on the packed-pair dot instructions (v_dot2c_f32_bf16 / v_dot2c_f32_f16):
// the query stays packed (32 VGPRs instead of 64 floats) and a key costs 32 VALU ops instead of 64 converts + 64 FMAs.
__device__ __forceinline__ float dot8(Vec<bf16>::x8 a, Vec<bf16>::x8 b, float acc) {
  acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_shufflevector(a, a, 0, 1), __builtin_shufflevector(b, b, 0, 1), acc, false);
  acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_shufflevector(a, a, 2, 3), __builtin_shufflevector(b, b, 2, 3), acc, false);
  acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_shufflevector(a, a, 4, 5), __builtin_shufflevector(b, b, 4, 5), acc, false);
  acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_shufflevector(a, a, 6, 7), __builtin_shufflevector(b, b, 6, 7), acc, false);
  return acc;
}
__device__ __forceinline__ float dot8(Vec<f16>::x8 a, Vec<f16>::x8 b, float acc) {
  acc = __builtin_amdgcn_fdot2(__builtin_shufflevector(a, a, 0, 1), __builtin_shufflevector(b, b, 0, 1), acc, false);
  acc = __builtin_amdgcn_fdot2(__builtin_shufflevector(a, a, 2, 3), __builtin_shufflevector(b, b, 2, 3), acc, false);
  acc = __builtin_amdgcn_fdot2(__builtin_shufflevector(a, a, 4, 5), __builtin_shufflevector(b, b, 4, 5), acc, false);
  acc = __builtin_amdgcn_fdot2(__builtin_shufflevector(a, a, 6, 7), __builtin_shufflevector(b, b, 6, 7), acc, false);
  return acc;
}

constexpr int DEC_VROWS = 4;             // V key rows per lane per register set (two sets in flight)
constexpr int DEC_VKEYS = 8 * DEC_VROWS;  // keys per wave per PV iteration: 8 key sub-rows x DEC_VROWS

// ------------------------------------------------------------------------------- wave-level steps
// Every load below is (wave-uniform base) + (32-bit lane offset) - no 64-bit address pairs held in VGPRs - and unconditional
// (clamped key index), because a branch between two groups of loads makes the compiler drain the first group before it issues
// the second.

// Stage a head's prefix into the LDS, the instructions dealt round-robin to the NW waves of the workgroup.  K instruction (slot s,
// chunk c): lane k <- kp[s*64 + k][c*8 .. c*8+7] (re-laid chunk-major like the per-sequence cache, through the per-lane source
// address); V instruction i: rows 8i .. 8i+7.
template <typename T, int NW>
__device__ __forceinline__ void dec_stage_prefix(const T* kp, const T* vp, unsigned char* Kl, unsigned char* Vl, int P1, int nsp, int wave, int lane) {
  const int nk_ins = nsp * 8, nv_ins = (P1 + 7) >> 3;
  for (int i = wave; i < nk_ins; i += NW) {
    const int sidx = i >> 3, c = i & 7;
    const int key = min(sidx * 64 + lane, P1 - 1);
    __builtin_amdgcn_global_load_lds((gbl_void_a*)((const char*)kp + ((size_t)key * 64 + c * 8) * sizeof(T)), (lds_void_a*)(Kl + (size_t)i * 1024), 16, 0, 0);
  }
  for (int i = wave; i < nv_ins; i += NW) {
    const int row = min(i * 8 + (lane >> 3), P1 - 1);
    __builtin_amdgcn_global_load_lds((gbl_void_a*)((const char*)vp + ((size_t)row * 64 + (lane & 7) * 8) * sizeof(T)), (lds_void_a*)(Vl + (size_t)i * 1024), 16, 0, 0);
  }
}

// Prefix scores from the staged K: lane-per-key, conflict-free ds_read_b128.
template <typename T>
__device__ __forceinline__ void dec_prefix_scores(const typename Vec<T>::x8 (&qk)[8], const unsigned char* Kl, float* sc, int P1, int nsp, int lane, float& mx) {
  typedef typename Vec<T>::x8 x8;
#pragma unroll 1
  for (int sidx = 0; sidx < nsp; ++sidx) {
    float sv = 0.f;
#pragma unroll
    for (int c = 0; c < 8; ++c) sv = dot8(qk[c], *(const x8*)(Kl + ((size_t)(sidx * 8 + c) * 64 + lane) * 16), sv);
    const int k = sidx * 64 + lane;
    if (k < P1) {
      sc[k] = sv;
      mx = fmaxf(mx, sv);
    }
  }
}

// Own keys of a 64-key slot (chunk-major [8][tmax][8]), 8 global_load_dwordx4 per call.  Clamped: an odd slot count repeats the
// last slot, result dropped; `last` is the newest key that may be read from memory.
template <typename T>
__device__ __forceinline__ void dec_load_own(typename Vec<T>::x8 (&kk)[8], const T* kc, int slot, int nso, int last, int tmax, int lane) {
  typedef typename Vec<T>::x8 x8;
  const int k = min(slot, nso - 1) * 64 + lane;
  const unsigned off = (unsigned)min(k, last) * 8u * (unsigned)sizeof(T);
  const unsigned cs = (unsigned)tmax * 8u * (unsigned)sizeof(T);
#pragma unroll
  for (int c = 0; c < 8; ++c) kk[c] = *(const x8*)((const char*)kc + (off + c * cs));
}

// Own value rows of PV iteration `it` (past the end: the last rows again, weighted 0).  A V row is 128 bytes, read as 8 lanes x 16
// bytes, so a wave instruction covers 8 whole key rows (1 KiB, like the K loads; 8-byte loads moved half as much per instruction
// and measured 6 % slower).  Lane -> (key sub-row kk8 = lane >> 3, channel group cg = lane & 7: 8 channels); an iteration covers
// DEC_VKEYS keys.  (Arguments by reference, as a lambda captures them: by value hipcc drops a wait from the fused kernel's code.)
template <typename T>
__device__ __forceinline__ void dec_load_v(typename Vec<T>::x8 (&t)[DEC_VROWS], const char* const& rows, int it, const int& nvo, const int& last, const int& kk8, const int& cg) {
  typedef typename Vec<T>::x8 x8;
  const int k0r = min(it, nvo - 1) * DEC_VKEYS + kk8;
#pragma unroll
  for (int u = 0; u < DEC_VROWS; ++u) {
    const unsigned jc = (unsigned)min(k0r + 8 * u, last);
    t[u] = *(const x8*)(rows + (jc * 64u + (unsigned)cg * 8u) * (unsigned)sizeof(T));  // uniform base + 32-bit byte offset
  }
}

// Own scores, TWO key slots (16 x 16-byte loads) in flight per lane per iteration; the caller has requested slots 0 and 1 into
// k0 / k1.  fix(key, score) may replace a score before it is filed (the fused launch: its new key is not in memory yet).
struct DecKeep { __device__ __forceinline__ void operator()(int, float&) const {} };
template <typename T, typename Fix = DecKeep>
__device__ __forceinline__ void dec_own_scores(const typename Vec<T>::x8 (&qk)[8], typename Vec<T>::x8 (&k0)[8], typename Vec<T>::x8 (&k1)[8], const T* kc, float* sc,
                                               int P1, int tgen, int nso, int last, int tmax, int lane, float& mx, Fix fix = Fix()) {
#pragma unroll 1
  for (int sl0 = 0; sl0 < nso; sl0 += 2) {
    if (sl0 > 0) {
      dec_load_own<T>(k0, kc, sl0, nso, last, tmax, lane);
      dec_load_own<T>(k1, kc, sl0 + 1, nso, last, tmax, lane);
    }
    __builtin_amdgcn_sched_barrier(0);
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int c = 0; c < 8; ++c) s0 = dot8(qk[c], k0[c], s0);
#pragma unroll
    for (int c = 0; c < 8; ++c) s1 = dot8(qk[c], k1[c], s1);
    const int ka = sl0 * 64 + lane, kb = ka + 64;
    fix(ka, s0);
    fix(kb, s1);
    if (ka < tgen) {
      sc[P1 + ka] = s0;
      mx = fmaxf(mx, s0);
    }
    if (kb < tgen && sl0 + 1 < nso) {
      sc[P1 + kb] = s1;
      mx = fmaxf(mx, s1);
    }
  }
}

// Softmax numerators over the wave's score row sc[0, ctx), in place; returns their sum.  The caller makes the row visible to the
// wave before it is read back (a block barrier or a wavefront fence).
__device__ __forceinline__ float dec_softmax(float* sc, int ctx, int lane, float mx) {
  mx = wave_max(mx);
  float sum = 0.f;
  for (int j = lane; j < ctx; j += 64) {
    const float e = __expf(sc[j] - mx);
    sc[j] = e;
    sum += e;
  }
  return wave_sum(sum);
}

// Prefix PV from the staged V rows.
template <typename T>
__device__ __forceinline__ void dec_prefix_pv(float (&o)[8], const unsigned char* Vl, const float* sc, int P1, int nvp, int kk8, int cg) {
  typedef typename Vec<T>::x8 x8;
#pragma unroll 1
  for (int it = 0; it < nvp; ++it) {
    const int k0r = it * DEC_VKEYS + kk8;
#pragma unroll
    for (int u = 0; u < DEC_VROWS; ++u) {
      const int j = k0r + 8 * u;
      const float pj = j < P1 ? sc[j] : 0.f;
      const x8 t = *(const x8*)(Vl + ((size_t)min(j, P1 - 1) * 64 + cg * 8) * sizeof(T));
#pragma unroll
      for (int c = 0; c < 8; ++c) o[c] += pj * (float)t[c];
    }
  }
}

// o += the weighted rows of one register set: rows k0r + 8 u weigh scs[k0r + 8 u] below lim and 0 from there.  NEW (the
// iteration that holds slot t_new, wave-uniform): the lane whose row is slot t_new takes it from vnew (the LDS) instead.
// (The plain form reads t[u] directly: through `row` hipcc waits for the four rows at once instead of one by one.)
template <typename T, bool NEW = false>
__device__ __forceinline__ void dec_consume(float (&o)[8], const typename Vec<T>::x8 (&t)[DEC_VROWS], const float* scs, int k0r, int lim, int t_new = 0, const T* vnew = nullptr) {
  typedef typename Vec<T>::x8 x8;
  x8 vn = {};
  if constexpr (NEW) vn = *(const x8*)vnew;
#pragma unroll
  for (int u = 0; u < DEC_VROWS; ++u) {
    const int j = k0r + 8 * u;
    const float pj = j < lim ? scs[j] : 0.f;
    if constexpr (NEW) {
      const x8 row = j == t_new ? vn : t[u];
#pragma unroll
      for (int c = 0; c < 8; ++c) o[c] += pj * (float)row[c];
    } else {
#pragma unroll
      for (int c = 0; c < 8; ++c) o[c] += pj * (float)t[u][c];
    }
  }
}

// The PV loop over n iterations on two register sets: the next rows are in flight while these are summed.  ta holds iteration 0.
// The fences keep exactly two row sets live (an early third set spills).
template <typename T, typename LoadV, typename Consume>
__device__ __forceinline__ void dec_own_pv(typename Vec<T>::x8 (&ta)[DEC_VROWS], typename Vec<T>::x8 (&tb)[DEC_VROWS], int n, LoadV load_v, Consume consume) {
#pragma unroll 1
  for (int it = 0; it < n; it += 2) {
    load_v(tb, it + 1);
    __builtin_amdgcn_sched_barrier(0);
    consume(ta, it);
    __builtin_amdgcn_sched_barrier(0);
    load_v(ta, it + 2);
    __builtin_amdgcn_sched_barrier(0);
    consume(tb, it + 1);
    __builtin_amdgcn_sched_barrier(0);
  }
}

// Sum the 8 key sub-rows (lanes with equal channel group), normalise, and store the lane's 8 channels of the output row.
template <typename T>
__device__ __forceinline__ void dec_reduce_store(float (&o)[8], float sum, T* out_row, bool live, int kk8, int cg) {
  typedef typename Vec<T>::x8 x8;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    o[c] = add_xor8(o[c]);
    o[c] = add_xor16(o[c]);
    o[c] = add_xor32(o[c]);
  }
  if (live && kk8 == 0) {
    const float inv = 1.0f / sum;
    x8 r;
#pragma unroll
    for (int c = 0; c < 8; ++c) r[c] = (T)(o[c] * inv);
    *(x8*)(out_row + cg * 8) = r;
  }
}

// ------------------------------------------------------------------------------- one wave per (sequence, head)
// 4 waves per block.  Sized to <= 128 VGPRs so that all B*heads = 4096 waves of the full candidate batch are resident at once
// (16 waves per CU): with 3 blocks per CU the 1024 blocks ran as a full round plus a quarter-full tail.  The shared prefix and
// the sequence's own keys are walked as separate, uniform segments of ONE slot list, both from memory.
template <typename T>
__global__ __launch_bounds__(256, 4) void decode_attn_kernel(DecodeAttnArgs a, int ctx_cap) {  // 4 waves per SIMD => <= 128 VGPRs
  typedef typename Vec<T>::x8 x8;
  extern __shared__ __attribute__((aligned(16))) float sc_all[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int pair = min((int)blockIdx.x * 4 + wave, a.B * a.heads - 1);  // surplus waves of the last block repeat its last pair
  const int b = pair / a.heads;
  const int h = pair % a.heads;
  const int tgen = *a.step + 1;       // generated keys 0..*step
  const int P1 = a.P1;
  const int ctx = P1 + tgen;
  float* sc = sc_all + (size_t)wave * ctx_cap;   // scores: [0, P1) prefix keys, [P1, ctx) own keys

  const T* kp = (const T*)a.kp + (size_t)h * P1 * 64;
  const T* vp = (const T*)a.vp + (size_t)h * P1 * 64;
  const size_t bh = (size_t)b * a.heads + h;
  const T* kc = (const T*)a.kc + bh * 8 * a.tmax * 8;
  const T* vc = (const T*)a.vc + bh * a.tmax * 64;

  float mx = -1e30f;
  {
    x8 qk[8];
    const T* qp = (const T*)a.q + (size_t)b * a.heads * 64 + h * 64;
#pragma unroll
    for (int c = 0; c < 8; ++c) qk[c] = *(const x8*)(qp + c * 8);
    // Lane-per-key dot products, TWO key slots (16 x 16-byte loads) in flight per lane per iteration.  Slot list:
    // prefix keys in 64-key slots (row-major rows of 64), then own keys in 64-key slots (chunk-major [8][tmax][8]).
    const int nsp = (P1 + 63) >> 6, nso = (tgen + 63) >> 6;
#pragma unroll 1
    for (int sl0 = 0; sl0 < nsp + nso; sl0 += 2) {
      x8 kk[2][8];
      int key[2];
      bool live[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int slot = min(sl0 + u, nsp + nso - 1);   // an odd slot count repeats the last slot (cached), result dropped
        const bool pre = slot < nsp;                    // wave-uniform
        const int k = (pre ? slot : slot - nsp) * 64 + lane;
        const int lim = pre ? P1 : tgen;
        const int kcl = min(k, lim - 1);
        const char* base = (const char*)(pre ? kp : kc);
        const unsigned off = (pre ? (unsigned)kcl * 64u : (unsigned)kcl * 8u) * (unsigned)sizeof(T);  // byte offsets, 32-bit
        const unsigned cs = (pre ? 8u : (unsigned)a.tmax * 8u) * (unsigned)sizeof(T);
#pragma unroll
        for (int c = 0; c < 8; ++c) kk[u][c] = *(const x8*)(base + (off + c * cs));
        key[u] = (pre ? 0 : P1) + k;
        live[u] = k < lim && sl0 + u < nsp + nso;
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        float sv = 0.f;
#pragma unroll
        for (int c = 0; c < 8; ++c) sv = dot8(qk[c], kk[u][c], sv);
        if (live[u]) {
          sc[key[u]] = sv;
          mx = fmaxf(mx, sv);
        }
      }
    }
  }

  // PV: iteration `it` covers DEC_VKEYS keys of one segment, the prefix's iterations first.
  const int kk8 = lane >> 3, cg = lane & 7;
  const int nvp = (P1 + DEC_VKEYS - 1) / DEC_VKEYS, nvo = (tgen + DEC_VKEYS - 1) / DEC_VKEYS;
  const int nit = nvp + nvo;
  auto load_v = [&](x8 (&t)[DEC_VROWS], int it) {
    const int itc = min(it, nit - 1);  // past the end: repeat the last iteration's rows (cached), weighted 0
    const bool pre = itc < nvp;
    const char* base = (const char*)(pre ? vp : vc);
    const int k0 = (pre ? itc : itc - nvp) * DEC_VKEYS + kk8, lim = pre ? P1 : tgen;
#pragma unroll
    for (int u = 0; u < DEC_VROWS; ++u) {
      const unsigned jc = (unsigned)min(k0 + 8 * u, lim - 1);
      t[u] = *(const x8*)(base + (jc * 64u + (unsigned)cg * 8u) * (unsigned)sizeof(T));  // uniform base + 32-bit byte offset
    }
  };
  // the first V rows do not depend on the scores: request them before the softmax
  x8 ta[DEC_VROWS], tb[DEC_VROWS];
  load_v(ta, 0);
  const float sum = dec_softmax(sc, ctx, lane, mx);
  __syncthreads();  // every lane's sc[] writes are visible to the whole wave (and block)
  float o[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) o[c] = 0.f;
  auto consume = [&](const x8 (&t)[DEC_VROWS], int it) {
    const bool pre = it < nvp;
    dec_consume<T>(o, t, sc + (pre ? 0 : P1), (pre ? it : it - nvp) * DEC_VKEYS + kk8, it < nit ? (pre ? P1 : tgen) : 0);
  };
  dec_own_pv<T>(ta, tb, nit, load_v, consume);
  dec_reduce_store<T>(o, sum, (T*)a.out + (size_t)b * a.heads * 64 + h * 64, (int)blockIdx.x * 4 + wave < a.B * a.heads, kk8, cg);
}

// ------------------------------------------------------------------------------- shared prefix in the LDS
// Every candidate of an utterance attends to the SAME [cond | text | start] prefix keys; the kernel above reads them once per
// (sequence, head) wave - 15 KB per wave, 61 MB of L2 -> CU traffic per launch at 256 candidates, which is on the critical path of
// every wave (per-CU L2 bandwidth is ~50 GB/s) although it never touches HBM.  Here a workgroup is NSEQ waves = NSEQ sequences of
// ONE head: the head's prefix K / V are staged into LDS once per workgroup (dec_stage_prefix), and only the per-sequence cache is
// streamed from HBM.  The first own-key slots are requested before the workgroup waits for the staged prefix (counted vmcnt: the
// direct-to-LDS loads are older in the queue), so the HBM stream starts at once.
// -DTT_ATTN_STAMPS (a variant build, scripts/attn_phases.py): wave 0 of every workgroup keeps the 100 MHz wall clock of its phase
// boundaries in scalar registers (no vector-memory operation: the counted vmcnt waits are untouched) and files them at the end
#ifdef TT_ATTN_STAMPS
__device__ unsigned long long g_attn_stamps[4096][10];
#define TT_ASTAMP(i) do { st[i] = wall_clock64(); } while (0)
#else
#define TT_ASTAMP(i)
#endif
template <typename T, int NSEQ>
__global__ __launch_bounds__(NSEQ * 64, 4) void decode_attn_lds_kernel(DecodeAttnArgs a, int ctx_cap, int kl_bytes, int vl_bytes) {
  typedef typename Vec<T>::x8 x8;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_dec[];
#ifdef TT_ATTN_STAMPS
  unsigned long long st[10];
#endif
  TT_ASTAMP(0);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int h = (int)blockIdx.x;      // grid = (heads, sequence groups)
  const int b_raw = (int)blockIdx.y * NSEQ + wave;
  const int b = min(b_raw, a.B - 1);  // surplus waves of the last group repeat its last sequence (never stored)
  // generated keys 0..*step (read first: a scalar load, nothing in front of it to drain); a session handle's row (NSEQ == 1: one
  // sequence per workgroup) reads its own newest slot, prefix length and prefix cache - a row that does not decode leaves at once
  int tgen, P1 = a.P1;
  size_t goff = 0;
  if (NSEQ == 1 && a.row_slot) {
    const int sl = a.row_slot[b];
    if (sl < 0) return;
    tgen = sl + 1;
    P1 = a.row_p1[b];
    goff = (size_t)b * a.prefix_group_stride;
  } else {
    tgen = *a.step + 1;
  }
  if (a.ngroups > 1) {  // several utterances in one batch: this workgroup's sequences all belong to one of them (group_size % NSEQ == 0)
    const int grp = ((int)blockIdx.y * NSEQ) / a.group_size;
    P1 = a.p1_tab[grp];
    goff = (size_t)grp * a.prefix_group_stride;
  }
  const T* kp = (const T*)a.kp + goff + (size_t)h * P1 * 64;
  const T* vp = (const T*)a.vp + goff + (size_t)h * P1 * 64;
  unsigned char* Kl = smem_dec;                 // [slot][8 chunks][64 keys][8]  (chunk-major like the per-sequence cache)
  unsigned char* Vl = smem_dec + kl_bytes;      // [key][64]
  float* sc = (float*)(smem_dec + kl_bytes + vl_bytes) + (size_t)wave * ctx_cap;
  const int nsp = (P1 + 63) >> 6;

  dec_stage_prefix<T, NSEQ>(kp, vp, Kl, Vl, P1, nsp, wave, lane);
  const int ctx = P1 + tgen;
  const size_t bh = (size_t)b * a.heads + h;
  const T* kc = (const T*)a.kc + bh * 8 * a.tmax * 8;
  const T* vc = (const T*)a.vc + bh * a.tmax * 64;

  float mx = -1e30f;
  // The query is wave-uniform: it lives in 32 SGPRs (two s_load_dwordx16), not in 32 VGPRs per lane, and its load is not on
  // the vector-memory counter, so nothing the compiler places between the staged prefix and the first use of q can force a
  // vmcnt(0) that would also drain the own-key requests below.  (Inline asm: hipcc only emits scalar loads for memory it can
  // prove read-only, and q was written by the previous kernel.)
  typedef int int16v __attribute__((ext_vector_type(16)));
  typedef int int4v __attribute__((ext_vector_type(4)));
  int16v qlo, qhi;
  {
    const T* qp = (const T*)a.q + (size_t)b * a.heads * 64 + h * 64;
    // early-clobber outputs: the second load still reads the address pair after the first one has been issued (and may have landed)
    asm volatile("s_load_dwordx16 %0, %2, 0x0\n\ts_load_dwordx16 %1, %2, 0x40" : "=&s"(qlo), "=&s"(qhi) : "s"(qp) : "memory");
  }
  const int nso = (tgen + 63) >> 6;
  x8 k0[8], k1[8];
  dec_load_own<T>(k0, kc, 0, nso, tgen - 1, a.tmax, lane);
  dec_load_own<T>(k1, kc, 1, nso, tgen - 1, a.tmax, lane);
  TT_ASTAMP(1);
  // the staged prefix must have landed (this wave's direct-to-LDS loads are older than the 16 register loads above)
  asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(qlo), "+s"(qhi)::"memory");  // q has landed (every later use depends on this statement)
  TT_ASTAMP(2);
  x8 qk[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int16v& src = c < 4 ? qlo : qhi;
    int4v w;
    w[0] = src[(c & 3) * 4 + 0]; w[1] = src[(c & 3) * 4 + 1]; w[2] = src[(c & 3) * 4 + 2]; w[3] = src[(c & 3) * 4 + 3];
    qk[c] = __builtin_bit_cast(x8, w);
  }
  dec_prefix_scores<T>(qk, Kl, sc, P1, nsp, lane, mx);
  TT_ASTAMP(3);
  dec_own_scores<T>(qk, k0, k1, kc, sc, P1, tgen, nso, tgen - 1, a.tmax, lane, mx);

  TT_ASTAMP(4);
  const int kk8 = lane >> 3, cg = lane & 7;
  const int nvp = (P1 + DEC_VKEYS - 1) / DEC_VKEYS, nvo = (tgen + DEC_VKEYS - 1) / DEC_VKEYS;
  auto load_v = [&](x8 (&t)[DEC_VROWS], int it) { dec_load_v<T>(t, (const char*)vc, it, nvo, tgen - 1, kk8, cg); };
  x8 ta[DEC_VROWS], tb[DEC_VROWS];
  load_v(ta, 0);  // the first V rows do not depend on the scores: request them before the softmax
  const float sum = dec_softmax(sc, ctx, lane, mx);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // sc[] is private to this wave: LDS operations of a wave execute in order
  TT_ASTAMP(5);
  float o[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) o[c] = 0.f;
  dec_prefix_pv<T>(o, Vl, sc, P1, nvp, kk8, cg);
  TT_ASTAMP(6);
  auto consume = [&](const x8 (&t)[DEC_VROWS], int it) { dec_consume<T>(o, t, sc + P1, it * DEC_VKEYS + kk8, it < nvo ? tgen : 0); };
  dec_own_pv<T>(ta, tb, nvo, load_v, consume);
  TT_ASTAMP(7);
  dec_reduce_store<T>(o, sum, (T*)a.out + (size_t)b * a.heads * 64 + h * 64, b_raw < a.B, kk8, cg);
#ifdef TT_ATTN_STAMPS
  TT_ASTAMP(8);
  if (threadIdx.x == 0) {
    const int wg = (int)blockIdx.y * (int)gridDim.x + (int)blockIdx.x;
    if (wg < 4096) {
      for (int i = 0; i < 9; ++i) g_attn_stamps[wg][i] = st[i];
      unsigned xcc = 0;
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
      g_attn_stamps[wg][9] = xcc;
    }
  }
#endif
}
#ifdef TT_ATTN_STAMPS
}  // namespace tt
extern "C" int ttx_attn_stamps(unsigned long long* out, int nwg) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(tt::g_attn_stamps), (size_t)nwg * 10 * sizeof(unsigned long long));
}
namespace tt {
#endif

// ------------------------------------------------------------------------------- QKV projection + attention, one launch
// A workgroup = one head x 16 sequences (16 waves, the NSEQ = 16 geometry above).  What it needs of the QKV GEMM is a 16 x 192 tile
// over K = 1024 - one MFMA row tile high - and it computes that tile itself instead of reading q and the newest K / V row back from a
// launch before it: waves 0 .. 11 ("projectors") own one 16-column tile of q, k or v each; waves 12 .. 15 request their sequences' keys at
// the top and never wait on the vector-memory counter until the projection is done.  A projector requests its own sequence's keys only
// after its last weight tile (vmcnt retires in order: a weight wait behind an HBM row request would wait for HBM).
// grid = (heads, groups): workgroup id h + 16 group, so under round-robin placement an XCD sees two heads and keeps 2 x 384 KB of the
// weight in its L2 (speed only).
// Bits: per output element the MFMA sequence of gemm_glds_kernel (W fragment as the A operand, k-tiles ascending, the two 32-wide
// k-steps of a tile in order, accumulator from zero), then EpiQkvDecode's bias add, q_scale and rounding; the attention is
// decode_attn_lds_kernel's steps, with two hooks: slot t (written by this launch) is taken from the LDS and never read back from memory.
// LDS: [prefix K | prefix V | R | q 16x64 | new k 16x64 | new v 16x64], R = the 16 activation rows (as 16 swizzled [16][64] k-tiles, the
// GEMM's A image) + the projectors' weight rings during the projection and the 16 score rows after it.
// Where the time goes (profiles/r16_qkv_attn_phase_stamps.txt): a CU's vector-memory path answers in request order, so the
// weight stream is NOT hidden behind the K / V stream as a second, independent stream would be - the projection ends ~14 us after entry
// and the attention of every wave follows it; the launch is still 2.8 us shorter than the two it replaces (one launch ramp, no q / k / v
// round trip through memory, the prefix staged beside the projection).
#ifdef TT_ATTN_STAMPS  // waves 0 and 15 of every workgroup file five wall-clock stamps each (scalar registers until the end)
#define TT_QSTAMP(i) do { qst[i] = wall_clock64(); } while (0)
#else
#define TT_QSTAMP(i)
#endif
template <typename T, int QA_DEPTH>  // QA_DEPTH: k-tiles of a projector wave's weight ring (2 KiB each): 4 where the LDS has room, else 3
__global__ __launch_bounds__(1024, 4) void decode_qkv_attn_kernel(DecodeQkvAttnArgs g, int ctx_cap, int kl_bytes, int vl_bytes, int r_bytes) {
  typedef typename Vec<T>::x8 x8;
  typedef typename Vec<T>::x4 x4;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_qa[];
  const DecodeAttnArgs& a = g.d;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
#ifdef TT_ATTN_STAMPS
  unsigned long long qst[5];
  qst[2] = 0;
#endif
  TT_QSTAMP(0);
  const int h = (int)blockIdx.x;                 // grid = (16 heads, B / 16)
  const int row0 = (int)blockIdx.y * 16;         // first sequence of the group
  const int b = row0 + wave;
  const int t = *a.step;                         // slot of the new key (scalar load, first in the queue); keys 0 .. t-1 are in the cache
  const int tgen = t + 1;
  const int P1 = a.P1;
  const T* kp = (const T*)a.kp + (size_t)h * P1 * 64;
  const T* vp = (const T*)a.vp + (size_t)h * P1 * 64;
  unsigned char* Kl = smem_qa;                   // [slot][8 chunks][64 keys][8]
  unsigned char* Vl = smem_qa + kl_bytes;        // [key][64]
  unsigned char* R = smem_qa + kl_bytes + vl_bytes;
  float* sc = (float*)R + (size_t)wave * ctx_cap;
  T* qs = (T*)(R + r_bytes);                     // [16 sequences][64]
  T* kn = qs + 16 * 64;
  T* vn = kn + 16 * 64;
  const int nsp = (P1 + 63) >> 6;

  {  // stage the prefix (as decode_attn_lds_kernel) and the 16 activation rows: piece i = k-tile i >> 1, rows 8 (i & 1) .. + 7
    dec_stage_prefix<T, 16>(kp, vp, Kl, Vl, P1, nsp, wave, lane);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int i = wave + 16 * u;
      const int row = (i & 1) * 8 + (lane >> 3);
      const int chunk = (lane & 7) ^ ((row >> 1) & 7);
      const T* src = (const T*)g.h + (size_t)(row0 + row) * 1024 + (i >> 1) * 64 + chunk * 8;
      __builtin_amdgcn_global_load_lds((gbl_void_a*)src, (lds_void_a*)(R + (size_t)i * 1024), 16, 0, 0);
    }
  }
  const size_t bh = (size_t)b * 16 + h;
  const T* kc = (const T*)a.kc + bh * 8 * a.tmax * 8;
  const T* vc = (const T*)a.vc + bh * a.tmax * 64;
  // Newest own key that may be read from memory.  At t == 0 there is none: the (clamped, unconditional) requests then have no valid row of the
  // cache to repeat.  The key requests still name slot 0 - whatever they return only feeds a score that is replaced by s_new or never
  // stored - but a value row is MULTIPLIED by its zero weight, and 0 x a stale NaN / Inf of the cache would poison the output row: at
  // t == 0 the value requests read row 0 of the staged head's prefix values instead (P1 >= 1; always written by the prefill, finite)
  const int told = max(t - 1, 0);
  const char* vrows = t > 0 ? (const char*)vc : (const char*)vp;
  const int nso = (tgen + 63) >> 6;
  auto load_own = [&](x8 (&kk)[8], int slot) { dec_load_own<T>(kk, kc, slot, nso, told, a.tmax, lane); };
  const int kk8 = lane >> 3, cg = lane & 7;
  const int nvp = (P1 + DEC_VKEYS - 1) / DEC_VKEYS, nvo = (tgen + DEC_VKEYS - 1) / DEC_VKEYS;
  auto load_v = [&](x8 (&tv)[DEC_VROWS], int it) { dec_load_v<T>(tv, vrows, it, nvo, told, kk8, cg); };
  x8 k0[8], k1[8];
  const bool proj = wave < 12;                   // wave-uniform; projector w owns tile w: part (q, k, v) = w >> 2, columns 16 (w & 3) .. + 15 of the head
  // A projector's weight tile goes global -> LDS directly, whole 128-byte lines (two 1-KiB pieces of 8 rows per k-tile, XOR-swizzled on the
  // source side like the GEMM's W image), into a ring of its OWN: the wave that issued a piece is the only one that reads it, so a counted
  // vmcnt is all the synchronisation the ring needs.  (Fragment loads straight from memory take half a line per row and reached 30 GB/s
  // per CU; profiles/r16_qkv_attn_phase_stamps.txt.)
  constexpr int DEPTH = QA_DEPTH;                // k-tiles per ring: DEPTH - 1 in flight while one is multiplied
  const int fr = lane & 15, fg = lane >> 4;
  const int part = wave >> 2, dcol = (wave & 3) * 16 + fg * 4;
  unsigned char* ring = R + 16 * 1024 * 2 + (size_t)wave * (DEPTH * 2048);
  const T* wsrc[2];
  auto issue_w = [&](int kt) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
      __builtin_amdgcn_global_load_lds((gbl_void_a*)(wsrc[j] + kt * 64), (lds_void_a*)(ring + (kt % DEPTH) * 2048 + j * 1024), 16, 0, 0);
  };
  float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
  if (!proj) {
    load_own(k0, 0);
    load_own(k1, 1);
    // the staged prefix and activation rows have landed: they are older in this wave's queue than the key requests.  Counted on the emitted
    // code: load_own is 8 global_load_dwordx4 per call, so exactly 16 vector loads are younger than this wave's LDS-DMA pieces
    asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
  } else {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int r = j * 8 + (lane >> 3);
      wsrc[j] = (const T*)g.w_qkv + (size_t)(part * 1024 + h * 64 + (wave & 3) * 16 + r) * 1024 + (((lane & 7) ^ ((r >> 1) & 7)) * 8);
    }
    // one global_load_dwordx4, issued AHEAD of the ring (the emitted order is bias, then the pieces), so every counted wait below covers it
    // and none has to count it
    if (g.b_qkv) bv = *(const float4*)(g.b_qkv + part * 1024 + h * 64 + dcol);
    // The first DEPTH - 1 weight tiles (2 pieces each) are requested ahead of the staging barrier; the wait leaves exactly those
    // (DEPTH - 1) * 2 pieces in flight.  (hipcc puts an s_waitcnt vmcnt(0) of its own at the top of this branch - it cannot tell the
    // pending LDS-DMA from the LDS addresses computed here - so in the emitted code the staged rows have in fact landed before the
    // first ring piece goes out; the source order is what a compiler without that wait would give.)
#pragma unroll
    for (int s_ = 0; s_ < DEPTH - 1; ++s_) issue_w(s_);
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"((DEPTH - 1) * 2) : "memory");
  }
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  TT_QSTAMP(1);

  if (proj) {
    const unsigned char* ap = R + fr * 128;
    const int asw = (fr >> 1) & 7;
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kt = 0; kt < 16; ++kt) {
      // tile kt has landed: of the tiles kt + 1 .. kt + DEPTH - 2 requested after it, those that exist may still be in flight (2 pieces
      // per tile and nothing else on the counter: no other vector load or store is issued inside the loop).  hipcc adds a vmcnt(0) of its
      // own in front of the first LDS read at kt = 0, so the ring starts from fully landed
      switch ((kt + DEPTH - 2 < 16 ? DEPTH - 2 : 15 - kt) * 2) {
        case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
        case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
        case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
        default: asm volatile("s_waitcnt vmcnt(%0)" ::"n"((DEPTH - 2) * 2) : "memory"); break;
      }
      if (kt + DEPTH - 1 < 16) issue_w(kt + DEPTH - 1);  // into the slot tile kt - 1 left
      const unsigned char* ws = ring + (kt % DEPTH) * 2048 + fr * 128;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const x8 fw = *(const x8*)(ws + (((ks * 4 + fg) ^ asw) * 16));
        const x8 fa = *(const x8*)(ap + kt * 2048 + (((ks * 4 + fg) ^ asw) * 16));
        acc = mfma16(fw, fa, acc);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    // EpiQkvDecode: lane (fr, fg) holds row fr, columns dcol .. dcol + 3 of the head
    const size_t bhr = (size_t)(row0 + fr) * 16 + h;
    acc[0] += bv.x; acc[1] += bv.y; acc[2] += bv.z; acc[3] += bv.w;
    if (part == 0) {
      const x4 qv = pack4<T>(acc[0] * g.q_scale, acc[1] * g.q_scale, acc[2] * g.q_scale, acc[3] * g.q_scale);
      *(x4*)(qs + fr * 64 + dcol) = qv;
      if (g.q_out) *(x4*)((T*)g.q_out + (size_t)(row0 + fr) * 1024 + h * 64 + dcol) = qv;
    } else if (part == 1) {
      const x4 kv = pack4<T>(acc[0], acc[1], acc[2], acc[3]);
      *(x4*)(kn + fr * 64 + dcol) = kv;
      *(x4*)((T*)a.kc + ((bhr * 8 + (dcol >> 3)) * a.tmax + t) * 8 + (dcol & 7)) = kv;
    } else {
      const x4 vv = pack4<T>(acc[0], acc[1], acc[2], acc[3]);
      *(x4*)(vn + fr * 64 + dcol) = vv;
      *(x4*)((T*)a.vc + (bhr * a.tmax + t) * 64 + dcol) = vv;
    }
    TT_QSTAMP(2);
    load_own(k0, 0);
    load_own(k1, 1);
  }
  // The projectors' q / k / v rows are in the LDS.  Behind the barrier hipcc places an s_waitcnt vmcnt(0) in front of the LDS read of q
  // (pending LDS-DMA and LDS reads it cannot tell apart), which also waits for the 16 key requests: a projector, which asked for its keys
  // just above, pays one HBM round trip there before its prefix scores start.  decode_attn_lds_kernel avoids that wait by taking q through
  // scalar loads; here q only exists in the LDS.  The phase times of DESIGN 5.21 include it.
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#ifdef TT_ATTN_STAMPS
  const unsigned long long qarrive = wall_clock64();  // every wave: its arrival at the second barrier
#endif
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  TT_QSTAMP(3);

  // ---- attention: decode_attn_lds_kernel's steps; the activation image is dead, its place takes the score rows
  const int ctx = P1 + tgen;
  float mx = -1e30f;
  // the query is wave-uniform: 32 SGPRs, not 32 VGPRs per lane (as in decode_attn_lds_kernel; here it comes from the LDS)
  typedef int int4v __attribute__((ext_vector_type(4)));
  x8 qk[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int4v w = *(const int4v*)(qs + wave * 64 + c * 8);
    int4v u;
#pragma unroll
    for (int i = 0; i < 4; ++i) u[i] = __builtin_amdgcn_readfirstlane(w[i]);
    qk[c] = __builtin_bit_cast(x8, u);
  }
  dec_prefix_scores<T>(qk, Kl, sc, P1, nsp, lane, mx);
  float s_new = 0.f;  // the new key's score, from the LDS copy of its row
#pragma unroll
  for (int c = 0; c < 8; ++c) s_new = dot8(qk[c], *(const x8*)(kn + wave * 64 + c * 8), s_new);
  dec_own_scores<T>(qk, k0, k1, kc, sc, P1, tgen, nso, told, a.tmax, lane, mx, [&](int k, float& s) { if (k == t) s = s_new; });
  x8 ta[DEC_VROWS], tb[DEC_VROWS];
  load_v(ta, 0);  // the first V rows do not depend on the scores: request them before the softmax
  const float sum = dec_softmax(sc, ctx, lane, mx);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // sc[] is private to this wave: LDS operations of a wave execute in order
  float o[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) o[c] = 0.f;
  dec_prefix_pv<T>(o, Vl, sc, P1, nvp, kk8, cg);
  const int it_new = t / DEC_VKEYS;  // the PV iteration that holds slot t
  auto consume = [&](const x8 (&tv)[DEC_VROWS], int it) {
    const int k0r = it * DEC_VKEYS + kk8, lim = it < nvo ? tgen : 0;
    const float* scs = sc + P1;
    if (it == it_new) dec_consume<T, true>(o, tv, scs, k0r, lim, t, vn + wave * 64 + cg * 8);  // wave-uniform
    else dec_consume<T>(o, tv, scs, k0r, lim);
  };
#pragma unroll 1
  for (int it = 0; it < nvo; it += 2) {  // dec_own_pv written out: through the template hipcc places this kernel's vmcnt(7..4) waits elsewhere
    load_v(tb, it + 1);
    __builtin_amdgcn_sched_barrier(0);
    consume(ta, it);
    __builtin_amdgcn_sched_barrier(0);
    load_v(ta, it + 2);
    __builtin_amdgcn_sched_barrier(0);
    consume(tb, it + 1);
    __builtin_amdgcn_sched_barrier(0);
  }
  dec_reduce_store<T>(o, sum, (T*)a.out + (size_t)b * 1024 + h * 64, true, kk8, cg);
#ifdef TT_ATTN_STAMPS
  TT_QSTAMP(4);
  if (lane == 0 && (wave == 0 || wave == 15)) {
    const int wg = (int)blockIdx.y * 16 + (int)blockIdx.x;
    if (wg < 4096)
      for (int i = 0; i < 5; ++i) g_attn_stamps[wg][(wave ? 5 : 0) + i] = qst[i];
  }
  if (lane == 0) {  // rows 256 .. 767: every wave's arrival at the second barrier (waves 0 .. 9, then 10 .. 15) of workgroups 0 .. 255
    const int wg = (int)blockIdx.y * 16 + (int)blockIdx.x;
    if (wg < 256) g_attn_stamps[(wave < 10 ? 256 : 512) + wg][wave < 10 ? wave : wave - 10] = qarrive;
  }
#endif
}

// ------------------------------------------------------------------------------- host side
// LDS of the staged-prefix kernels: [prefix K: 64-key slots of 8 KiB | prefix V: 8-row pieces of 1 KiB | `rows` score rows of ctx_cap floats]
struct DecodeLds {
  int kl_bytes, vl_bytes;
  size_t score_bytes;
  DecodeLds(int P1, int rows, int ctx_cap)
      : kl_bytes(((P1 + 63) >> 6) * 8 * 1024), vl_bytes(((P1 + 7) >> 3) * 1024), score_bytes((size_t)rows * ctx_cap * sizeof(float)) {}
  size_t prefix() const { return (size_t)kl_bytes + vl_bytes; }
  size_t total() const { return prefix() + score_bytes; }
};

// Launch a kernel whose dynamic LDS may exceed the 64 KiB default: the attribute is set once per kernel, then every launch is plain.
template <auto Kernel, typename... A>
static int launch_big_lds(const ProfScope& ps, dim3 grid, dim3 block, size_t smem, hipStream_t stream, A&&... args) {
  static bool attr_done = false;
  if (!attr_done) {
    TT_CHECK_HIP(hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)DECODE_LDS_CAP));
    attr_done = true;
  }
  launch_timed(ps, Kernel, grid, block, smem, stream, args...);
  TT_CHECK_HIP(hipGetLastError());
  return 0;
}

static size_t qkv_attention_lds(int P1, int tmax, int depth) {
  const DecodeLds l(P1, 16, P1 + tmax);
  const size_t rows = (l.score_bytes + 15) & ~(size_t)15;
  const size_t image = (size_t)16 * 1024 * 2 + (size_t)12 * depth * 2048;  // the activation rows + the projectors' weight rings
  return l.prefix() + (rows > image ? rows : image) + 3 * 16 * 64 * 2;
}
size_t decode_qkv_attention_lds(int P1, int tmax) { return qkv_attention_lds(P1, tmax, 3); }

template <typename T>
static int launch_qkv_attn(int depth, const ProfScope& ps, dim3 blocks, size_t smem, hipStream_t stream, const DecodeQkvAttnArgs& g, int ctx_cap, const DecodeLds& l, int r_bytes) {
  if (depth == 4) return launch_big_lds<decode_qkv_attn_kernel<T, 4>>(ps, blocks, dim3(1024), smem, stream, g, ctx_cap, l.kl_bytes, l.vl_bytes, r_bytes);
  return launch_big_lds<decode_qkv_attn_kernel<T, 3>>(ps, blocks, dim3(1024), smem, stream, g, ctx_cap, l.kl_bytes, l.vl_bytes, r_bytes);
}

int decode_qkv_attention_launch(int dtype, const DecodeQkvAttnArgs& g, hipStream_t stream) {
  const DecodeAttnArgs& a = g.d;
  TT_REQUIRE(dtype == DT_BF16 || dtype == DT_F16, "decode_qkv_attention: 16-bit operands only");
  TT_REQUIRE(a.B > 0 && a.B % 16 == 0 && a.heads == 16 && a.P1 >= 1 && a.tmax > 0 && a.ngroups <= 1 && !a.row_slot && a.step && g.h && g.w_qkv,
             "decode_qkv_attention: needs 16 heads of 64, a multiple of 16 sequences, one prefix group and no session rows (B=%d heads=%d P1=%d)",
             a.B, a.heads, a.P1);
  const int depth = qkv_attention_lds(a.P1, a.tmax, 4) <= DECODE_LDS_CAP ? 4 : 3;
  const size_t smem = qkv_attention_lds(a.P1, a.tmax, depth);
  TT_REQUIRE(smem <= DECODE_LDS_CAP, "decode_qkv_attention: prefix %d with %d KV slots needs %zu bytes of LDS, %zu available", a.P1, a.tmax, smem, DECODE_LDS_CAP);
  const int ctx_cap = a.P1 + a.tmax;
  const DecodeLds l(a.P1, 16, ctx_cap);
  const int r_bytes = (int)(smem - l.prefix() - 3 * 16 * 64 * 2);
  // projection 2 * B * 3072 * 1024 + attention; K / V rows + prefix + the QKV weight once + activation rows in, attention rows out
  ProfScope ps(PROF_DECODE_QKV_ATTN, stream, 2.0 * a.B * 3072.0 * 1024.0 + 4.0 * a.B * a.heads * 64.0 * (a.P1 + a.host_tgen),
               ((double)a.B * a.host_tgen + a.P1) * a.heads * 64 * 2 * 2.0 + 3072.0 * 1024.0 * 2.0 + 2.0 * a.B * 1024 * 2.0, true);
  const dim3 blocks(16, a.B / 16);
  if (dtype == DT_BF16) return launch_qkv_attn<bf16>(depth, ps, blocks, smem, stream, g, ctx_cap, l, r_bytes);
  return launch_qkv_attn<f16>(depth, ps, blocks, smem, stream, g, ctx_cap, l, r_bytes);
}

size_t decode_attention_session_lds(int p1_cap, int tmax) { return DecodeLds(p1_cap, 1, p1_cap + tmax).total(); }

template <typename T>
static int launch_attn_lds(int nseq, const ProfScope& ps, hipStream_t stream, const DecodeAttnArgs& a, int ctx_cap, const DecodeLds& l) {
  const dim3 blocks(a.heads, cdiv(a.B, nseq));
  if (nseq == 16) return launch_big_lds<decode_attn_lds_kernel<T, 16>>(ps, blocks, dim3(16 * 64), l.total(), stream, a, ctx_cap, l.kl_bytes, l.vl_bytes);
  if (nseq == 1) return launch_big_lds<decode_attn_lds_kernel<T, 1>>(ps, blocks, dim3(64), l.total(), stream, a, ctx_cap, l.kl_bytes, l.vl_bytes);
  return launch_big_lds<decode_attn_lds_kernel<T, 4>>(ps, blocks, dim3(4 * 64), l.total(), stream, a, ctx_cap, l.kl_bytes, l.vl_bytes);
}

int decode_attention_launch(int dtype, const DecodeAttnArgs& a, hipStream_t stream) {
  if (dtype == DT_F32) return decode_attn_f32_launch(a, stream);  // verification mode (attention_f32.hip)
  TT_REQUIRE(a.B > 0 && a.heads > 0 && a.P1 >= 0 && a.tmax > 0, "decode_attention: bad shape");
  const int ctx_cap = a.P1 + a.tmax;
  // algorithmic bytes: every sequence reads its own generated K and V rows once (host_tgen keys) + the shared prefix once
  ProfScope ps(PROF_DECODE_ATTN, stream, 4.0 * a.B * a.heads * 64.0 * (a.P1 + a.host_tgen),
               ((double)a.B * a.host_tgen + a.P1) * a.heads * 64 * 2 * 2.0 + 2.0 * a.B * a.heads * 64 * 2.0, true);
  // shared-prefix kernel with 4 sequences per workgroup (measured 2 % ahead of 16 at 256 candidates and 40 % ahead at 32:
  // more, smaller workgroups); the per-wave kernel only when the staged prefix + score rows do not fit the LDS (very long prompts)
  int nseq = a.variant == 1 ? 0 : a.variant == 2 ? 16 : 4;
  if (a.row_slot) {  // session handle: one row per workgroup, the LDS sized for the prefix capacity a.P1
    TT_REQUIRE(a.row_p1 && a.prefix_group_stride && a.ngroups <= 1 && a.P1 >= 1, "decode_attention: per-row sessions need row_p1, a prefix stride and a prefix capacity");
    nseq = 1;
  }
  if (a.ngroups > 1) {
    TT_REQUIRE(a.ngroups <= 16 && a.group_size > 0 && a.group_size % 4 == 0 && a.B == a.ngroups * a.group_size,
               "decode_attention: %d groups of %d sequences (a multiple of 4) do not make %d sequences", a.ngroups, a.group_size, a.B);
    nseq = 4;
  }
  if (a.P1 < 1) nseq = 0;
  TT_REQUIRE(!a.row_slot || decode_attention_session_lds(a.P1, a.tmax) <= DECODE_LDS_CAP,
             "decode_attention: a session row's prefix capacity %d does not fit the LDS", a.P1);
  if (nseq && DecodeLds(a.P1, nseq, ctx_cap).total() > DECODE_LDS_CAP) nseq = nseq == 16 ? 4 : 0;
  if (nseq && DecodeLds(a.P1, nseq, ctx_cap).total() > DECODE_LDS_CAP) nseq = 0;
  if (nseq) {
    const DecodeLds l(a.P1, nseq, ctx_cap);
    return dtype == DT_BF16 ? launch_attn_lds<bf16>(nseq, ps, stream, a, ctx_cap, l) : launch_attn_lds<f16>(nseq, ps, stream, a, ctx_cap, l);
  }
  TT_REQUIRE(a.ngroups <= 1, "decode_attention: the prefixes of a multi-utterance batch (%d rows) do not fit the LDS", a.P1);
  const size_t smem = (size_t)4 * ctx_cap * sizeof(float);
  TT_REQUIRE(smem <= 64 * 1024, "decode_attention: context %d too long for the score buffer", ctx_cap);
  const int blocks = cdiv(a.B * a.heads, 4);
  if (dtype == DT_BF16) launch_timed(ps, decode_attn_kernel<bf16>, dim3(blocks), dim3(256), smem, stream, a, ctx_cap);
  else launch_timed(ps, decode_attn_kernel<f16>, dim3(blocks), dim3(256), smem, stream, a, ctx_cap);
  TT_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace tt
