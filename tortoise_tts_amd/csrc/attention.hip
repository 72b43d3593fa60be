// Attention kernels for gfx950, head_dim = 64.
//
// flash_attention: a wave owns a block of 16 (or 32) queries and walks the keys 32 at a time with an
// online softmax.  Both products run "swapped" so the softmax axis is lane-local:
//   S^T[key][q] = K[key][:] . Q[q][:]        (MFMA A = K rows, B = Q rows: both 16-B row reads)
//   O^T[d][q]   = V^T[d][key] . P^T[key][q]  (MFMA A = V^T rows, B = P straight from the S^T registers)
// A lane therefore holds one query column (l & 15) in every accumulator: running max / sum and
// the rescale factor are per-lane scalars and the row reductions are two xor-shuffles (16, 32).
// The S^T -> P^T hand-off needs no LDS: the 32 keys of a tile are fed to the second MFMA in the
// order the first one left them in registers, and V^T is read with the same permutation.
//
// Three kernels, one algorithm:
//   flash_kernel<NQ>           n <= 128: K / V^T prefetched into registers, the 4 waves of a block split the keys of ONE 16 * NQ-query block
//   flash_lds_kernel<NQ, KS>   16 * NQ queries per wave, 64-key K / V^T tiles staged once per block through a 3-stage LDS-DMA ring
//   flash32_kernel<KS>         the same ring under 32-query waves on v_mfma_f32_32x32x16
// They are built from the steps below (flash_* : every kernel; q16_* : the two 16-query-wave kernels).  What stays written out per
// kernel is (a) the softmax arithmetic that differs and must keep its rounding: flash_kernel adds a saturated relative-position bucket
// to the eight scores and reduces with fmaxf / max_xor*, the staged kernels fold that bucket into the row maximum and the exponent and
// use v_max3, and flash32_kernel feeds the window bias through the accumulator input of its first product; (b) two short steps that
// hipcc compiles differently once they are functions (profiles/flash_attention_refactor_isa.txt): the two-line ring prologue (as a
// function: flash_lds_kernel<T,1,2> 80 -> 82 VGPRs, one wave per SIMD less) and the 16-query normalise + store (as a function, in eight
// spellings: another ds_read / MFMA order in the loop of flash_lds_kernel<T,1,1>).
//
// The decode-step attention (one new query against [shared prefix | own generated keys]) is in decode_attention.hip.
#include "ops.h"

namespace tt {

constexpr float LOG2E = 1.4426950408889634f;  // exp() is a bare v_exp_f32 (exp2) with log2(e) folded into one FMA

// max without the operand canonicalisation fmaxf() implies (the inputs are MFMA results / finite floats or -inf)
__device__ __forceinline__ float vmax(float a, float b) { float r; asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ float vmax3(float a, float b, float c) { float r; asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }

// ------------------------------------------------------------------------------------------ steps of every kernel
// XCD-aware block order: the dispatcher deals workgroups round-robin over the 8 XCDs (private L2 each), which
// would spread the query blocks of one (batch, head) over all eight L2s and fetch its K / V eight times
// (PMC: FETCH_SIZE 4.4x the algorithmic bytes).  Remap so every XCD owns a contiguous run of (head, query block).
__device__ __forceinline__ void flash_xcd_remap(int& bx, int& bh) {
  const int gx = gridDim.x, total = gx * gridDim.y;
  const int lin = blockIdx.y * gx + blockIdx.x, xcd = lin & 7, slot = lin >> 3;
  const int per = total >> 3, rem = total & 7;
  const int lin2 = xcd * per + min(xcd, rem) + slot;
  bh = lin2 / gx;
  bx = lin2 - bh * gx;
}

// The (batch, head) pair bh of a workgroup: head h, batch row b, its n valid keys / queries (padded batches: FlashArgs::n stays the row
// stride of the operands) and its operand rows.  The pointers are formed where the kernel asks for them, behind its table staging
// (formed up front with the rest, every kernel waits for its kernel arguments at another point).
template <typename T>
struct FlashRows {
  const FlashArgs& a;
  int bh, h, b, n;
  __device__ __forceinline__ FlashRows(const FlashArgs& a_, int bh_) : a(a_), bh(bh_), h(bh_ % a_.heads), b(bh_ / a_.heads) {
    n = a.nv_period > 0 ? a.nv[b % a.nv_period] : a.n;
  }
  __device__ __forceinline__ const T* Q() const { return (const T*)a.q + (size_t)bh * a.n * 64; }
  __device__ __forceinline__ const T* K() const { return (const T*)a.k + (size_t)bh * a.n * 64; }
  __device__ __forceinline__ const T* VT() const { return (const T*)a.vt + (size_t)bh * 64 * a.n_pad; }
};

// two 8-byte V^T reads (keys k .. k+3 and k+16 .. k+19 of a row) as the 8-key MFMA operand
template <typename T>
__device__ __forceinline__ typename Vec<T>::x8 flash_v8(typename Vec<T>::x4 lo, typename Vec<T>::x4 hi) {
  typename Vec<T>::x8 v;
  v[0] = lo[0]; v[1] = lo[1]; v[2] = lo[2]; v[3] = lo[3];
  v[4] = hi[0]; v[5] = hi[1]; v[6] = hi[2]; v[7] = hi[3];
  return v;
}

// ------------------------------------------------------------------------------------------ the LDS ring of the staged kernels
// The four query-group waves (x KS key halves) of a block share every 64-key K / V^T tile, which goes global -> LDS directly
// (global_load_lds_dwordx4, 16 KiB per tile, XOR-swizzled on the source side like the GEMM tiles) through a 3-stage ring with counted
// vmcnt, one raw barrier per tile.  The relative-position table sits behind the ring in the SAME shared object (a second one
// de-pipelines the ring).  Kernels and launcher read the geometry from here.
template <int KS>
struct FlashRing {
  static constexpr int ST = 3, KT = 64;               // ring stages, keys per tile
  static constexpr int STAGE = 2 * KT * 64;           // elements per stage: K tile [64 keys][64] + V^T tile [64 dims][64 keys]
  static constexpr int G = 4 / KS;                    // LDS-DMA instructions per wave per tile: 16 one-KiB pieces over 4 KS waves
  static constexpr int BYTES = ST * STAGE * 2;        // 16-bit elements
  static constexpr int MERGE_FLOATS = BYTES / 4 / 256;  // floats per lane of a query group that flash_merge_halves may park in the ring
};
template <int QB_, int KS, int RP_>
struct FlashStaged : FlashRing<KS> {
  static constexpr int QB = QB_, RP = RP_;            // queries per workgroup; floats reserved for the relative-position table
  static constexpr int THREADS = 256 * KS;            // 4 query groups x KS key halves
  static constexpr int SMEM = FlashRing<KS>::BYTES + RP * 4;
};

// stage fill: 16 one-KiB pieces per tile (8 rows x 128 B each): pieces 0-7 = K rows, 8-15 = V^T rows; 4 / KS per wave.  (Arguments by
// reference, as the lambda this replaces captured them: by value hipcc allocates other registers and reorders the KS = 2 kernels.)
template <typename T, int KS>
__device__ __forceinline__ void flash_ring_fill(T* const& ring, const T* const& K, const T* const& VT, const int& n, const int& n_pad, const int& wave_id,
                                                const int& lr, const int& lc, int t, int stage) {
  typedef FlashRing<KS> R;
  const int key0 = t * R::KT;
  T* base = ring + stage * R::STAGE;
#pragma unroll
  for (int i = 0; i < R::G; ++i) {
    const int piece = wave_id + 4 * KS * i;
    const int row = (piece & 7) * 8 + lr;
    const int chunk = lc ^ ((row >> 1) & 7);
    const T* src;
    if (piece < 8) src = K + (size_t)min(key0 + row, n - 1) * 64 + chunk * 8;                      // key row, 8 dims
    else src = VT + (size_t)row * n_pad + min(key0 + chunk * 8, n_pad - 8);                        // dim row, 8 keys
    __builtin_amdgcn_global_load_lds((gbl_void_a*)src, (lds_void_a*)(base + piece * 512), 16, 0, 0);
  }
}

// tile t: wait for its stage (the oldest request of this wave), one barrier, refill the stage the previous tile freed; returns the staged K tile
template <typename T, int KS>
__device__ __forceinline__ const T* flash_ring_tile(T* const& ring, const T* const& K, const T* const& VT, const int& n, const int& n_pad, const int& wave_id,
                                                    const int& lr, const int& lc, const int& last, int t, int slot) {
  typedef FlashRing<KS> R;
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"((R::ST - 2) * R::G) : "memory");
  __builtin_amdgcn_s_barrier();
  int nslot = slot + R::ST - 1;
  if (nslot >= R::ST) nslot -= R::ST;
  flash_ring_fill<T, KS>(ring, K, VT, n, n_pad, wave_id, lr, lc, min(t + R::ST - 1, last), nslot);
  return ring + slot * R::STAGE;
}

// the 32-key halves of the staged tile this wave works on: both with KS == 1, half kp_own with KS == 2 (wave-uniform: tiles beyond the
// wave's causal horizon kend are skipped)
template <typename T, int KS, typename Process>
__device__ __forceinline__ void flash_ring_halves(const T* kt, int key0, const int& kend, const int& kp_own, Process&& process) {
  const T* vt = kt + FlashRing<KS>::KT * 64;
  if constexpr (KS == 1) {
    if (key0 < kend) process(kt, vt, 0, key0);
    if (key0 + 32 < kend) process(kt, vt, 1, key0 + 32);
  } else {
    if (key0 + kp_own * 32 < kend) process(kt, vt, kp_own, key0 + kp_own * 32);
  }
}

// KS == 2: merge the two key halves' (m, l, acc) of query group `group` through the ring (free now): the upper waves park theirs and
// are done (returns true), the lower ones combine.  NA accumulator floats per lane, held as vectors V.
template <int NA, typename V>
__device__ __forceinline__ bool flash_merge_halves(float* mg, int group, int lane, bool upper, float& m_run, float& l_run, V (&acc)[NA * 4 / sizeof(V)]) {
  constexpr int VN = sizeof(V) / 4;
  float* d = mg + ((size_t)group * (NA + 2)) * 64 + lane;  // [4 query groups][2 + NA][64 lanes]
  __syncthreads();            // every wave is done reading the ring
  if (upper) {
    d[0] = m_run;
    d[64] = l_run;
#pragma unroll
    for (int j = 0; j < NA; ++j) d[(2 + j) * 64] = acc[j / VN][j % VN];
  }
  __syncthreads();
  if (upper) return true;
  const float m1 = d[0], l1 = d[64];
  const float mm = fmaxf(m_run, m1);
  const float a0 = __builtin_amdgcn_exp2f((m_run - mm) * LOG2E), a1 = __builtin_amdgcn_exp2f((m1 - mm) * LOG2E);
  l_run = l_run * a0 + l1 * a1;
#pragma unroll
  for (int j = 0; j < NA; ++j) acc[j / VN][j % VN] = acc[j / VN][j % VN] * a0 + d[(2 + j) * 64] * a1;
  return false;
}

// ------------------------------------------------------------------------------------------ steps of the 16-query-wave kernels
// lane = (query column fr = l & 15, key group fg = l >> 4); score s[kb][r] <-> key key0 + 16 kb + 4 fg + r.

// Q fragment of query row qr (clamped by the caller)
template <typename T>
__device__ __forceinline__ void q16_load(typename Vec<T>::x8 (&qf)[2], const T* Q, int qr, int fg) {
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) qf[ks] = *(const typename Vec<T>::x8*)(Q + (size_t)qr * 64 + ks * 32 + fg * 8);
}

__device__ __forceinline__ void q16_init(float& m_run, float& l_run, f32x4 (&acc)[4]) {
  m_run = -1e30f;
  l_run = 0.f;
#pragma unroll
  for (int blk = 0; blk < 4; ++blk) acc[blk] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// S^T of 32 keys x 16 queries
template <typename T>
__device__ __forceinline__ void q16_scores(float (&s)[2][4], const typename Vec<T>::x8 (&kf)[2][2], const typename Vec<T>::x8 (&qf)[2]) {
#pragma unroll
  for (int kb = 0; kb < 2; ++kb) {
    f32x4 st = f32x4{0.f, 0.f, 0.f, 0.f};
    st = mfma16(kf[kb][0], qf[0], st);
    st = mfma16(kf[kb][1], qf[1], st);
#pragma unroll
    for (int r = 0; r < 4; ++r) s[kb][r] = st[r];
  }
}

// relative-position bias of a tile inside the +-64 window of the query block
__device__ __forceinline__ void q16_window_bias(float (&s)[2][4], const float* rp, int key0, int fg, int qi) {
#pragma unroll
  for (int kb = 0; kb < 2; ++kb)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int d = key0 + kb * 16 + fg * 4 + r - qi;
      d = d < -64 ? -64 : (d > 64 ? 64 : d);
      s[kb][r] += rp[d + 64];
    }
}

// masks only on the last key tile / the causal diagonal (a wave-uniform test; q0 = first query of the block, qi = this lane's)
__device__ __forceinline__ void q16_mask(float (&s)[2][4], int key0, int fg, int q0, int qi, int n, int causal) {
  if (key0 + 32 > n || (causal && key0 + 31 > q0)) {
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = key0 + kb * 16 + fg * 4 + r;
        if (key >= n || (causal && key > qi)) s[kb][r] = -INFINITY;
      }
  }
}

// rescale the running state only if some row maximum of the wave moved (exact when skipped)
__device__ __forceinline__ void q16_rescale(float& m_run, float& l_run, f32x4 (&acc)[4], float m_new) {
  if (__any(m_new > m_run)) {
    const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * LOG2E);
    l_run *= alpha;
#pragma unroll
    for (int blk = 0; blk < 4; ++blk) {
      acc[blk][0] *= alpha; acc[blk][1] *= alpha; acc[blk][2] *= alpha; acc[blk][3] *= alpha;
    }
    m_run = m_new;
  }
}

// O += V^T P^T with P^T the eight numerators in score order
template <typename T>
__device__ __forceinline__ void q16_pv(f32x4 (&acc)[4], const typename Vec<T>::x8 (&vf)[4], const float (&p)[2][4]) {
  typename Vec<T>::x8 pf;
#pragma unroll
  for (int kb = 0; kb < 2; ++kb)
#pragma unroll
    for (int r = 0; r < 4; ++r) pf[kb * 4 + r] = (T)p[kb][r];
#pragma unroll
  for (int blk = 0; blk < 4; ++blk) acc[blk] = mfma16(vf[blk], pf, acc[blk]);
}

// ------------------------------------------------------------------------------- register-prefetch kernel (n <= 128)
// K / V for one (batch, head) is at most a few hundred KB, i.e. L2 resident, so nothing is staged through LDS (the only LDS use is the
// 129-entry relative-position table of DiffusionTts and the final merge).  The 4 waves of a block share ONE block of 16 * NQ queries and
// take every 4th key tile each; partial (max, sum, O) states are merged through LDS: 4x the resident waves for the same work, which is
// what hides the per-tile dependency chain (MFMA -> softmax -> MFMA) when batch*heads is small.  SPLIT stays in the parameter list for
// the kernel's name: the form where every wave owns its own queries is gone.  Only NQ = 1 is built, but the query-block loops stay:
// with the two in the epilogue written as their bodies hipcc takes 135 - 137 instead of 118 VGPRs and rounds all 16 fp16 output
// columns twice (v_pk_mul_f32, then v_cvt_pk_f16_f32) where this form rounds 8 of them once (v_fma_mixlo_f16) - other bits than before
// (profiles/flash_attention_refactor_isa.txt).
template <typename T, int NQ, bool SPLIT>
__global__ __launch_bounds__(256, 2) void flash_kernel(FlashArgs a) {  // 2 waves per SIMD: <= 256 VGPRs (NQ = 4 took 308 => one workgroup per CU)
  static_assert(SPLIT, "flash_kernel: the 4 waves of a workgroup split the keys of one query block");
  typedef typename Vec<T>::x8 x8;
  typedef typename Vec<T>::x4 x4;
  __shared__ float rp[132];
  int bx, bh;
  flash_xcd_remap(bx, bh);
  const FlashRows<T> row(a, bh);
  const int h = row.h, b = row.b;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int fr = lane & 15, fg = lane >> 4;
  const int ns = a.n;                                             // row stride of the operands
  const int n = row.n;
  if (a.relpos) {
    if (threadIdx.x < 129) rp[threadIdx.x] = a.relpos[h * 129 + threadIdx.x];
    __syncthreads();
  }
  const int qbase = bx * 16 * NQ;
  if (qbase >= n) return;
  const T *Q = row.Q(), *K = row.K(), *VT = row.VT();

  x8 qf[NQ][2];
  float m_run[NQ], l_run[NQ];
  f32x4 acc[NQ][4];
#pragma unroll
  for (int iq = 0; iq < NQ; ++iq) {
    q16_load<T>(qf[iq], Q, min(qbase + iq * 16 + fr, n - 1), fg);
    q16_init(m_run[iq], l_run[iq], acc[iq]);
  }
  const int q_last = min(qbase + 16 * NQ, n) - 1;
  const int kend = a.causal ? q_last + 1 : n;

  // K / V^T fragments of tile t+1 are fetched into a second register set while tile t is processed:
  // a wave's loop body is shorter than an L2 round trip, so without this every tile pays the latency.
  auto load_kv = [&](x8 (&kf)[2][2], x8 (&vf)[4], int key0) {
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      const int kr = min(key0 + kb * 16 + fr, n - 1);
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) kf[kb][ks] = *(const x8*)(K + (size_t)kr * 64 + ks * 32 + fg * 8);
    }
#pragma unroll
    for (int blk = 0; blk < 4; ++blk) {
      const T* vrow = VT + (size_t)(blk * 16 + fr) * a.n_pad + key0 + fg * 4;
      vf[blk] = flash_v8<T>(*(const x4*)vrow, *(const x4*)(vrow + 16));
    }
  };
  x8 kfA[2][2], vfA[4], kfB[2][2], vfB[4];

  // The loop body is VALU-bound (PMC: ~24 VALU instructions per MFMA before this diet), so everything that is
  // wave-uniform is decided once per tile: tiles whose keys are all >= 64 positions away from every query of the
  // block take a constant relative-position bias, masks are only evaluated on the last / diagonal tile, the
  // accumulator rescale is skipped when no row maximum moved, the row sums stay lane-partial until the end, and
  // exp() is a bare v_exp_f32 (exp2) with log2(e) folded into one FMA.
  auto process = [&](const x8 (&kf)[2][2], const x8 (&vf)[4], int key0) {
#pragma unroll
    for (int iq = 0; iq < NQ; ++iq) {
      const int q0 = qbase + iq * 16;
      const int qi = q0 + fr;
      float s[2][4];
      q16_scores<T>(s, kf, qf[iq]);
      if (a.relpos) {
        if (key0 - (q0 + 15) >= 64) {          // every key is >= 64 after every query: bucket saturated
          const float bconst = rp[128];
#pragma unroll
          for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int r = 0; r < 4; ++r) s[kb][r] += bconst;
        } else if (q0 - (key0 + 31) >= 64) {   // every key is >= 64 before every query
          const float bconst = rp[0];
#pragma unroll
          for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int r = 0; r < 4; ++r) s[kb][r] += bconst;
        } else {
          q16_window_bias(s, rp, key0, fg, qi);
        }
      }
      q16_mask(s, key0, fg, q0, qi, n, a.causal);
      float mx = fmaxf(fmaxf(fmaxf(s[0][0], s[0][1]), fmaxf(s[0][2], s[0][3])),
                       fmaxf(fmaxf(s[1][0], s[1][1]), fmaxf(s[1][2], s[1][3])));
      mx = max_xor16(mx);
      mx = max_xor32(mx);
      const float m_new = fmaxf(m_run[iq], mx);
      q16_rescale(m_run[iq], l_run[iq], acc[iq], m_new);
      const float mc = m_new * LOG2E;
      float p[2][4];
      float psum = 0.f;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          p[kb][r] = __builtin_amdgcn_exp2f(fmaf(s[kb][r], LOG2E, -mc));
          psum += p[kb][r];
        }
      l_run[iq] += psum;  // lane-partial: reduced over the four key groups once, after the loop
      q16_pv<T>(acc[iq], vf, p);
    }
  };
  // prefetches are unconditional (clamped to the last tile): straight-line body, counted waits
  const int ntile = (kend + 31) / 32;
  constexpr int TSTEP = 4;  // wave w takes tiles w, w + 4, ...
  int t = wave;
  if (t < ntile) {
    load_kv(kfA, vfA, 32 * t);
    while (true) {
      load_kv(kfB, vfB, 32 * min(t + TSTEP, ntile - 1));
      process(kfA, vfA, 32 * t);
      t += TSTEP;
      if (t >= ntile) break;
      load_kv(kfA, vfA, 32 * min(t + TSTEP, ntile - 1));
      process(kfB, vfB, 32 * t);
      t += TSTEP;
      if (t >= ntile) break;
    }
  }
#pragma unroll
  for (int iq = 0; iq < NQ; ++iq) {
    l_run[iq] = add_xor16(l_run[iq]);
    l_run[iq] = add_xor32(l_run[iq]);
  }
  {
    // merge the four waves' partial (max, sum, O) states, one query block at a time, into wave 0
    __shared__ float mbuf[4][16], lbuf[4][16];
    __shared__ float obuf[4][64][17];
#pragma unroll
    for (int iq = 0; iq < NQ; ++iq) {
      if (iq > 0) __syncthreads();  // wave 0 finished reading the previous query block
      if (fg == 0) {
        mbuf[wave][fr] = m_run[iq];
        lbuf[wave][fr] = l_run[iq];
      }
#pragma unroll
      for (int blk = 0; blk < 4; ++blk)
#pragma unroll
        for (int r = 0; r < 4; ++r) obuf[wave][lane][blk * 4 + r] = acc[iq][blk][r];
      __syncthreads();
      if (wave == 0) {
        float mw[4], M = -1e30f;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          mw[w] = mbuf[w][fr];
          M = fmaxf(M, mw[w]);
        }
        float L = 0.f;
        float o[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) o[j] = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          const float f = __expf(mw[w] - M);
          L += f * lbuf[w][fr];
#pragma unroll
          for (int j = 0; j < 16; ++j) o[j] += f * obuf[w][lane][j];
        }
        l_run[iq] = L;
#pragma unroll
        for (int blk = 0; blk < 4; ++blk)
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[iq][blk][r] = o[blk * 4 + r];
      }
    }
    if (wave != 0) return;
  }
#pragma unroll
  for (int iq = 0; iq < NQ; ++iq) {
    const int qi = qbase + iq * 16 + fr;
    if (qi < n) {
      const float inv = 1.0f / l_run[iq];
      T* o = (T*)a.out + ((size_t)b * ns + qi) * a.ldo + h * 64 + fg * 4;
#pragma unroll
      for (int blk = 0; blk < 4; ++blk)
        *(x4*)(o + blk * 16) = pack4<T>(acc[iq][blk][0] * inv, acc[iq][blk][1] * inv, acc[iq][blk][2] * inv, acc[iq][blk][3] * inv);
    }
  }
}

// ------------------------------------------------------------------------------- LDS-staged flash attention
// Same arithmetic as flash_kernel (swapped QK^T / PV MFMAs, online softmax per 32 keys), different data movement: the four
// waves of a block own DIFFERENT queries (16 * NQ each) and SHARE every 64-key K / V^T tile through the ring above.  Against the
// register-prefetch kernel this divides the L2 -> CU traffic by 4 (a K / V byte is fetched once per block, not once per wave), puts
// two more tiles in flight per wave without spending VGPRs on them, and removes the 4-way partial-state merge.
//
// KS = 2 ("key split"): 8 waves per block - wave w works on query group w & 3 like before, but only on half w >> 2 (32 keys) of
// every staged 64-key tile, and the two partial softmax states of a query group are merged through the LDS at the end.  At the
// denoiser's shape (n = 870, 32 (batch, head) pairs) the chip holds 1741 sixteen-query chains for 1024 SIMDs: the launch under-fills
// it, and splitting every key tile over two wave groups doubles the waves per SIMD at no extra K / V traffic (the same staged tile
// serves both halves): -2 % on the sampler iteration (profiles/r03_ab_flash_split.txt).  The kernel itself is bound by VALU issue -
// 15.7 VALU instructions per MFMA, VALU pipe ~76 % busy at four waves per SIMD (profiles/r03_pmc_flash_kbench.txt) - so what
// moves it further is fewer softmax instructions per score, not more parallelism.
template <typename T, int NQ, int KS>
__global__ __launch_bounds__(256 * KS, 2) void flash_lds_kernel(FlashArgs a) {
  typedef typename Vec<T>::x8 x8;
  typedef typename Vec<T>::x4 x4;
  typedef FlashStaged<64 * NQ, KS, 132> R;
  static_assert(KS == 1 || (NQ == 1 && 16 + 2 <= R::MERGE_FLOATS), "the key-split merge parks one 16-query state per wave in the ring");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  T* ring = (T*)smem_raw;                        // [ST][STAGE]
  float* rp = (float*)(ring + R::ST * R::STAGE); // [132] relative-position table
  int bx, bh;
  flash_xcd_remap(bx, bh);
  const FlashRows<T> row(a, bh);
  const int h = row.h, b = row.b;
  const int lane = threadIdx.x & 63, wave_id = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wave = wave_id & 3, kp_own = wave_id >> 2;  // query group of this wave; with KS == 2 the half of every key tile it owns
  const int fr = lane & 15, fg = lane >> 4;
  const int ns = a.n;                                             // row stride of the operands
  const int n = row.n;
  const int qblock = bx * R::QB;                 // first query of the block
  if (qblock >= n) return;                       // a block of padding queries only (block-uniform, before the first barrier)
  if (a.relpos) {
    if (threadIdx.x < 129) rp[threadIdx.x] = a.relpos[h * 129 + threadIdx.x];
    __syncthreads();
  }
  const int qbase = qblock + wave * 16 * NQ;     // first query of this wave (may be >= n: the wave then only helps loading)
  const T *Q = row.Q(), *K = row.K(), *VT = row.VT();

  x8 qf[NQ][2];
  float m_run[NQ], l_run[NQ];
  f32x4 acc[NQ][4];
#pragma unroll
  for (int iq = 0; iq < NQ; ++iq) {
    q16_load<T>(qf[iq], Q, min(qbase + iq * 16 + fr, n - 1), fg);
    q16_init(m_run[iq], l_run[iq], acc[iq]);
  }
  const int q_last_blk = min(qblock + R::QB, n) - 1;
  const int q_last = min(qbase + 16 * NQ, n) - 1;            // < qbase when the wave has no query
  const int kend_blk = a.causal ? q_last_blk + 1 : n;        // block-uniform: every wave walks the same tiles
  const int kend = qbase >= n ? 0 : (a.causal ? q_last + 1 : n);  // keys this wave's queries can see (none: the wave only helps loading)
  const int ntile = (kend_blk + R::KT - 1) / R::KT, last = ntile - 1;
  const int lr = lane >> 3, lc = lane & 7;       // this lane's (row, 16-byte chunk) of a ring piece

  // one 32-key half tile (kp = 0 / 1) of the staged tile against this wave's queries
  auto process = [&](const T* kt, const T* vt, int kp, int key0) {
    x8 kf[2][2], vf[4];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      const int r = kp * 32 + kb * 16 + fr;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) kf[kb][ks] = *(const x8*)(kt + r * 64 + (((ks * 4 + fg) ^ ((r >> 1) & 7)) * 8));
    }
#pragma unroll
    for (int blk = 0; blk < 4; ++blk) {
      const int d = blk * 16 + fr;
      const int sw = (d >> 1) & 7;
      // keys kp*32 + fg*4 .. +3 (lo) and +16 .. +19 (hi): chunk = key / 8, 8-byte half (fg & 1)
      const int c_lo = kp * 4 + (fg >> 1), c_hi = c_lo + 2;
      vf[blk] = flash_v8<T>(*(const x4*)(vt + d * 64 + ((c_lo ^ sw) * 8) + (fg & 1) * 4), *(const x4*)(vt + d * 64 + ((c_hi ^ sw) * 8) + (fg & 1) * 4));
    }
#pragma unroll
    for (int iq = 0; iq < NQ; ++iq) {
      const int q0 = qbase + iq * 16;
      const int qi = q0 + fr;
      float sv[2][4];
      q16_scores<T>(sv, kf, qf[iq]);
      // Relative-position bias.  A tile that lies entirely >= 64 positions after (or before) every query of the group gets ONE
      // saturated bucket value for all its scores: a uniform shift, which is folded into the row maximum and the exponent below
      // instead of being added to the 8 scores (most tiles at n = 870).  Only the tiles inside the +-64 window look the table up.
      float cbias = 0.f;
      if (a.relpos) {
        if (key0 - (q0 + 15) >= 64) cbias = rp[128];         // every key is >= 64 after every query: bucket saturated
        else if (q0 - (key0 + 31) >= 64) cbias = rp[0];      // every key is >= 64 before every query
        else q16_window_bias(sv, rp, key0, fg, qi);
      }
      q16_mask(sv, key0, fg, q0, qi, n, a.causal);
      // row maximum: v_max3 / v_max straight on the MFMA results (fmaxf() would first canonicalise every operand: 8 extra VALU)
      float mx = vmax3(vmax3(vmax3(sv[0][0], sv[0][1], sv[0][2]), sv[0][3], sv[1][0]), sv[1][1], sv[1][2]);
      mx = vmax(mx, sv[1][3]);
      {
        float x0, x1;
        pair_xor16(mx, x0, x1);
        mx = vmax(x0, x1);
        pair_xor32(mx, x0, x1);
        mx = vmax(x0, x1) + cbias;
      }
      const float m_new = vmax(m_run[iq], mx);
      q16_rescale(m_run[iq], l_run[iq], acc[iq], m_new);
      const float mc = (m_new - cbias) * LOG2E;  // exp2(s * log2e - mc) == exp(s + cbias - m_new)
      float pv[2][4];
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int r = 0; r < 4; ++r) pv[kb][r] = __builtin_amdgcn_exp2f(fmaf(sv[kb][r], LOG2E, -mc));
      const float psum = ((pv[0][0] + pv[0][1]) + (pv[0][2] + pv[0][3])) + ((pv[1][0] + pv[1][1]) + (pv[1][2] + pv[1][3]));
      l_run[iq] += psum;  // lane-partial: reduced over the four key groups once, after the loop
      q16_pv<T>(acc[iq], vf, pv);
    }
  };

#pragma unroll
  for (int s_ = 0; s_ < R::ST - 1; ++s_) flash_ring_fill<T, KS>(ring, K, VT, n, a.n_pad, wave_id, lr, lc, min(s_, last), s_);  // prologue
  int slot = 0;
  for (int t = 0; t < ntile; ++t) {
    const T* kt = flash_ring_tile<T, KS>(ring, K, VT, n, a.n_pad, wave_id, lr, lc, last, t, slot);
    flash_ring_halves<T, KS>(kt, t * R::KT, kend, kp_own, process);
    slot = slot + 1 == R::ST ? 0 : slot + 1;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if constexpr (KS == 2) {
    if (flash_merge_halves<16>((float*)ring, wave, lane, kp_own == 1, m_run[0], l_run[0], acc[0])) return;
  }
#pragma unroll
  for (int iq = 0; iq < NQ; ++iq) {
    l_run[iq] = add_xor16(l_run[iq]);
    l_run[iq] = add_xor32(l_run[iq]);
    const int qi = qbase + iq * 16 + fr;
    if (qi < n) {
      const float inv = 1.0f / l_run[iq];
      T* o = (T*)a.out + ((size_t)b * ns + qi) * a.ldo + h * 64 + fg * 4;
#pragma unroll
      for (int blk = 0; blk < 4; ++blk)
        *(x4*)(o + blk * 16) = pack4<T>(acc[iq][blk][0] * inv, acc[iq][blk][1] * inv, acc[iq][blk][2] * inv, acc[iq][blk][3] * inv);
    }
  }
}

// ---------------------------------------------------------------------------------------------- 32-query waves (round 5)
// The same algorithm on v_mfma_f32_32x32x16: a wave owns 32 queries, a workgroup 128 (4 query groups x KS key halves), K / V^T tiles
// of 64 keys staged once per workgroup through the same 3-stage LDS-DMA ring.  Why: flash_lds_kernel issues 15.7 VALU instructions per
// 16x16x32 MFMA (profiles/r03_pmc_flash_kbench.txt) - per 16 queries x 32 keys a lane holds 8 scores, and everything that is per ROW
// (cross-lane maximum, running-state update, the relative-position window test, the LDS fragment addresses) is paid per 8 scores.  Here
// a lane holds ONE query (l & 31) and 16 scores of it per 32-key block; its row maximum is 15 in-lane v_max + one permlane32 swap, the
// fragment reads serve twice the flops (a K fragment feeds a 32 x 32 x 16 product), and the P^T operand of the second product is again
// the score registers in the order the first product left them: lane half h = l >> 5 holds keys 4 h + 8 i + j of the block (reg 4 i + j),
// so k-slot e of PV step kk is score register 8 kk + e, and V^T is read with that permutation (two 8-byte reads per fragment).
// (A 4-way key split - 16 waves, tiles of 128 keys - measured equal to KS = 2 at the denoiser's shape and is not built:
// profiles/r05_ab_flash_ks4_and_epilogue_prefetch.txt.)
template <typename T, int KS>
__global__ __launch_bounds__(256 * KS, 2 * KS) void flash32_kernel(FlashArgs a) {
  typedef typename Vec<T>::x8 x8;
  typedef typename Vec<T>::x4 x4;
  typedef FlashStaged<128, KS, 260> R;
  static_assert(KS == 1 || 32 + 2 <= R::MERGE_FLOATS, "the key-split merge parks one 32-query state per wave in the ring");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  T* ring = (T*)smem_raw;
  float* rp = (float*)(ring + R::ST * R::STAGE);
  int bx, bh;
  flash_xcd_remap(bx, bh);
  const FlashRows<T> row(a, bh);
  const int h = row.h, b = row.b;
  const int lane = threadIdx.x & 63, wave_id = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wave = wave_id & 3, kp_own = wave_id >> 2;
  const int ql = lane & 31, hh = lane >> 5;
  const int ns = a.n;
  const int n = row.n;
  const int qblock = bx * R::QB;
  if (qblock >= n) return;
  // relative-position table with the saturated buckets extended by 64 entries on both sides: rp[i] = bias(clamp(i - 128, -64, 64)), so a
  // tile that straddles the +-64 window reads rp[key - query + 128] without clamping (|key - query| <= 125 there)
  if (a.relpos) {
    for (int i = threadIdx.x; i < 257; i += R::THREADS) rp[i] = a.relpos[h * 129 + min(max(i - 64, 0), 128)];
    __syncthreads();
  }
  const int qbase = qblock + wave * 32;
  const T *Q = row.Q(), *K = row.K(), *VT = row.VT();

  x8 qf[4];
  {
    const int qr = min(qbase + ql, n - 1);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) qf[ks] = *(const x8*)(Q + (size_t)qr * 64 + ks * 16 + hh * 8);
  }
  float m_run = -1e30f, l_run = 0.f;
  f32x16 acc[2];
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[db][v] = 0.f;
  const int q_last_blk = min(qblock + R::QB, n) - 1;
  const int q_last = min(qbase + 32, n) - 1;
  const int kend_blk = a.causal ? q_last_blk + 1 : n;
  const int kend = qbase >= n ? 0 : (a.causal ? q_last + 1 : n);
  const int ntile = (kend_blk + R::KT - 1) / R::KT, last = ntile - 1;
  const int lr = lane >> 3, lc = lane & 7;

  const int qi = qbase + ql;
  // one 32-key block (kp = 0 / 1 of the staged tile; key0 = its first key) against this wave's 32 queries
  auto process = [&](const T* kt, const T* vt, int kp, int key0) {
    x8 kf[4], vf[2][2];
    {
      const int r = kp * 32 + ql;
      const int sw = (r >> 1) & 7;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) kf[ks] = *(const x8*)(kt + r * 64 + (((ks * 2 + hh) ^ sw) * 8));
    }
#pragma unroll
    for (int db = 0; db < 2; ++db) {
      const int d = db * 32 + ql;
      const int sw = (d >> 1) & 7;
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        const int c = kp * 4 + 2 * kk;  // 8-key chunk of keys 16 kk .. +7 of the block; this lane half takes keys 4 hh .. +3 of it and of the next
        vf[db][kk] = flash_v8<T>(*(const x4*)(vt + d * 64 + ((c ^ sw) * 8) + hh * 4), *(const x4*)(vt + d * 64 + (((c + 1) ^ sw) * 8) + hh * 4));
      }
    }
    // score register v <-> key key0 + 8 (v >> 2) + 4 hh + (v & 3).  Relative-position bias: a block entirely >= 64 positions after (or
    // before) every query of the group gets ONE saturated bucket value for all its scores - folded into the row maximum and the exponent
    // below; a block that straddles the window takes its 16 bias values as the ACCUMULATOR INPUT of the first product (S^T = K Q^T + C), so
    // no score register is touched after the MFMA chain on either path (a post-MFMA add made hipcc copy all 16 registers out and back on
    // the common, saturated path).
    float cbias = 0.f;
    f32x16 st;
    const bool window = a.relpos != nullptr && key0 - (qbase + 31) < 64 && qbase - (key0 + 31) < 64;  // wave-uniform
    if (window) {
      const float* rb = rp + (key0 - qi + 4 * hh + 128);  // one address per lane, 16 reads at constant offsets
#pragma unroll
      for (int v = 0; v < 16; ++v) st[v] = rb[8 * (v >> 2) + (v & 3)];
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) st = mfma32(kf[ks], qf[ks], st);
    } else {
      if (a.relpos) cbias = key0 - (qbase + 31) >= 64 ? rp[256] : rp[0];
#pragma unroll
      for (int v = 0; v < 16; ++v) st[v] = 0.f;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) st = mfma32(kf[ks], qf[ks], st);
    }
    float sv[16];
#pragma unroll
    for (int v = 0; v < 16; ++v) sv[v] = st[v];
    if (key0 + 32 > n || (a.causal && key0 + 31 > qbase)) {
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int key = key0 + 8 * (v >> 2) + 4 * hh + (v & 3);
        if (key >= n || (a.causal && key > qi)) sv[v] = -INFINITY;
      }
    }
    float mx = vmax3(sv[0], sv[1], sv[2]);
    mx = vmax3(mx, sv[3], sv[4]);
    mx = vmax3(mx, sv[5], sv[6]);
    mx = vmax3(mx, sv[7], sv[8]);
    mx = vmax3(mx, sv[9], sv[10]);
    mx = vmax3(mx, sv[11], sv[12]);
    mx = vmax3(mx, sv[13], sv[14]);
    mx = vmax(mx, sv[15]);
    {
      float x0, x1;
      pair_xor32(mx, x0, x1);
      mx = vmax(x0, x1) + cbias;
    }
    const float m_new = vmax(m_run, mx);
    if (__any(m_new > m_run)) {
      const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * LOG2E);
      l_run *= alpha;
#pragma unroll
      for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[db][v] *= alpha;
      m_run = m_new;
    }
    const float mc = (m_new - cbias) * LOG2E;
    float pv[16];
#pragma unroll
    for (int v = 0; v < 16; ++v) pv[v] = __builtin_amdgcn_exp2f(fmaf(sv[v], LOG2E, -mc));
    x8 pf[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int e = 0; e < 8; ++e) pf[kk][e] = (T)pv[kk * 8 + e];
    l_run += (((pv[0] + pv[1]) + (pv[2] + pv[3])) + ((pv[4] + pv[5]) + (pv[6] + pv[7]))) +
             (((pv[8] + pv[9]) + (pv[10] + pv[11])) + ((pv[12] + pv[13]) + (pv[14] + pv[15])));
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int db = 0; db < 2; ++db) acc[db] = mfma32(vf[db][kk], pf[kk], acc[db]);
  };

#pragma unroll
  for (int s_ = 0; s_ < R::ST - 1; ++s_) flash_ring_fill<T, KS>(ring, K, VT, n, a.n_pad, wave_id, lr, lc, min(s_, last), s_);  // prologue
  int slot = 0;
  for (int t = 0; t < ntile; ++t) {
    const T* kt = flash_ring_tile<T, KS>(ring, K, VT, n, a.n_pad, wave_id, lr, lc, last, t, slot);
    flash_ring_halves<T, KS>(kt, t * R::KT, kend, kp_own, process);
    slot = slot + 1 == R::ST ? 0 : slot + 1;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if constexpr (KS == 2) {
    if (flash_merge_halves<32>((float*)ring, wave, lane, kp_own == 1, m_run, l_run, acc)) return;
  }
  l_run = add_xor32(l_run);
  if (qi < n) {
    const float inv = 1.0f / l_run;
    T* o = (T*)a.out + ((size_t)b * ns + qi) * a.ldo + h * 64 + hh * 4;
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        *(x4*)(o + db * 32 + i * 8) = pack4<T>(acc[db][4 * i] * inv, acc[db][4 * i + 1] * inv, acc[db][4 * i + 2] * inv, acc[db][4 * i + 3] * inv);
  }
}

// ------------------------------------------------------------------------------------------ launch
// the two staged kernels: the shared-memory attribute once per kernel; grid, block and bytes from the kernel's geometry
template <typename R, void (*KERNEL)(FlashArgs)>
static int launch_flash_staged(const ProfScope& ps, const FlashArgs& a, hipStream_t stream) {
  static bool attr_set = false;
  if (!attr_set) {
    TT_CHECK_HIP(hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, R::SMEM));
    attr_set = true;
  }
  launch_timed(ps, KERNEL, dim3(cdiv(a.n, R::QB), a.BH), dim3(R::THREADS), R::SMEM, stream, a);
  TT_CHECK_HIP(hipGetLastError());
  return 0;
}
// the bf16 / f16 pick: f(T()) with the launch's operand type T
template <typename F>
static int flash_with_type(int dtype, F&& f) { return dtype == DT_BF16 ? f(bf16()) : f(f16()); }
template <int NQ, int KS>
static int launch_flash_lds(int dtype, const ProfScope& ps, const FlashArgs& a, hipStream_t stream) {
  typedef FlashStaged<64 * NQ, KS, 132> R;
  g_flash_ran = FlashRan{FLASH_RAN_LDS, NQ, KS};
  return flash_with_type(dtype, [&](auto t) { return launch_flash_staged<R, flash_lds_kernel<decltype(t), NQ, KS>>(ps, a, stream); });
}
template <int KS>
static int launch_flash32(int dtype, const ProfScope& ps, const FlashArgs& a, hipStream_t stream) {
  typedef FlashStaged<128, KS, 260> R;
  g_flash_ran = FlashRan{FLASH_RAN_32, 2, KS};
  return flash_with_type(dtype, [&](auto t) { return launch_flash_staged<R, flash32_kernel<decltype(t), KS>>(ps, a, stream); });
}

thread_local FlashRan g_flash_ran = {-1, 0, 0};
bool g_flash32 = true;  // tt_flash_variant: 0 = the 16-query-wave kernels everywhere (A/B runs)

int flash_attention_launch(int dtype, const FlashArgs& a, hipStream_t stream) {
  if (dtype == DT_F32) return flash_f32_launch(a, stream);  // verification mode (attention_f32.hip)
  TT_REQUIRE(a.BH > 0 && a.n > 0 && a.heads > 0 && a.BH % a.heads == 0, "flash: bad shape BH=%d n=%d heads=%d", a.BH, a.n, a.heads);
  TT_REQUIRE(a.n_pad % 32 == 0 && a.n_pad >= ((a.n + 31) / 32) * 32, "flash: n_pad=%d must be a multiple of 32 covering n=%d", a.n_pad, a.n);
  TT_REQUIRE(a.ldo % 4 == 0, "flash: ldo must be a multiple of 4");
  // 32 queries per wave once there is enough work to fill the chip; 16 otherwise.
  // QK^T + PV: 4 * n * n * 64 flops per (batch, head) (halved when causal); Q, K, V read + O written once
  ProfScope ps(PROF_FLASH, stream, 4.0 * a.BH * (double)a.n * a.n * 64 * (a.causal ? 0.5 : 1.0), 4.0 * a.BH * (double)a.n * 64 * 2.0, true);
  if (a.n > 128 && !a.causal && a.variant != 2 && g_flash32) {
    // 32-query waves on v_mfma_f32_32x32x16 (flash32_kernel), 128 queries per workgroup; launches of fewer than ~2 workgroups per CU
    // split every key tile over two wave groups (the denoiser: 7 x 32 workgroups)
    const long blocks128 = (long)cdiv(a.n, 128) * a.BH;
    if (blocks128 < 512 && a.variant != 1) return launch_flash32<2>(dtype, ps, a, stream);
    return launch_flash32<1>(dtype, ps, a, stream);
  }
  if (a.n > 128) {
    // LDS-staged kernel: 64 queries per block while that keeps >= 2 blocks per CU busy, 128 otherwise (half the K / V traffic per
    // flop; measured on the kbench shapes: 32 queries per wave only pays from ~2048 blocks of 64 queries on)
    const long blocks64 = (long)cdiv(a.n, 64) * a.BH;
    if (blocks64 >= 2048) return launch_flash_lds<2, 1>(dtype, ps, a, stream);
    // fewer than ~4 blocks per CU: the launch is paid for the per-wave dependency chain - split every key tile over two wave groups
    // (in-situ A/B, profiles/r03_ab_flash_split.txt: denoiser iteration 1.555 -> 1.520 ms; the softmax VALU diet of this round -4 % per launch)
    if (blocks64 < 1024 && a.variant != 1) return launch_flash_lds<1, 2>(dtype, ps, a, stream);
    return launch_flash_lds<1, 1>(dtype, ps, a, stream);
  }
  // short sequences (prefill of a few dozen rows, reduced test configurations): the register-prefetch kernel, the 4 waves of a
  // block share one 16-query block and split the keys
  dim3 grid(cdiv(a.n, 16), a.BH);
  g_flash_ran = FlashRan{FLASH_RAN_REG, 1, 0};
  return flash_with_type(dtype, [&](auto t) {
    launch_timed(ps, flash_kernel<decltype(t), 1, true>, grid, dim3(256), 0, stream, a);
    TT_CHECK_HIP(hipGetLastError());
    return 0;
  });
}

}  // namespace tt
