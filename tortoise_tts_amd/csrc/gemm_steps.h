// The steps that the MFMA GEMM kernels share (gemm_glds_kernel, gemm_conv3s_kernel in gemm_impl.h; gemm_gna.h; gemm_p8.h; the split-K range
// also in gemm_f32.hip): tile origin, LDS swizzle, the wave-tile MFMA step of one k-tile, accumulator zeroing, ring slot arithmetic, split-K
// range.  Included by gemm_impl.h behind the device argument block.  Each kernel keeps its own schedule - which step runs when, and the
// counted waits - and takes the steps from here.
#pragma once

namespace tt {

// XCD-aware tile order.  Hardware deals workgroup i to XCD i % 8, each with a private 4 MiB L2, and everything that is
// not in the LOCAL L2 arrives over the fabric at HBM-like bandwidth (~6.5 TB/s for the whole chip, Infinity-Cache hits
// included: scripts/kbench.py bw).  So the tile grid is cut into row bands and every XCD owns a contiguous run of
// (band, column, row-in-band)-ordered tiles, i.e. a rectangle of about (gx / bands) x (8 gy / ...) tiles: it pulls
// A / bands + W * bands / 8 over the fabric instead of all of A (one band, the decode shapes where A is tiny) or all
// of W (8 bands).  gemm_launch picks the band count to minimise that sum.  The grid is one-dimensional
// (gx * gy workgroups, z = split-K slab) and every division is a multiply-high by a host-computed reciprocal.
__device__ __forceinline__ void tile_origin(const GemmCore& c, unsigned id, unsigned& bx, unsigned& by) {
  const unsigned xcd = id & 7, loc = id >> 3;
  const unsigned nid = xcd * c.xq + min(xcd, c.xr) + loc;
  unsigned rem, rr;
  const unsigned band = fdiv(nid, c.band, rem);
  const bool lastb = band == c.last_band;
  FastDiv hd;
  hd.d = lastb ? c.hlast.d : c.hfull.d;
  hd.m = lastb ? c.hlast.m : c.hfull.m;
  by = fdiv(rem, hd, rr);
  bx = band * c.hb + rr;
}

// LDS tiles are unpadded rows of 64 elements (128 B = eight 16-byte chunks).  Bank conflicts are removed by an XOR swizzle: LDS chunk c of
// row r holds global chunk c ^ ((r >> 1) & 7).  The involution is applied on the SOURCE side by whoever fills a tile (the LDS-DMA lane
// geometry, gemm_gna's register-staged stores) and again by every fragment read; both go through this one function: the element offset
// inside row `row` at which global chunk `chunk` lives (equally: the global element offset that LDS chunk `chunk` is filled from).
__device__ __forceinline__ constexpr int swz(int row, int chunk) { return (chunk ^ ((row >> 1) & 7)) * 8; }

template <int FN, int FM>
__device__ __forceinline__ void zero_acc(f32x4 (&acc)[FN][FM]) {
#pragma unroll
  for (int i = 0; i < FN; ++i)
#pragma unroll
    for (int j = 0; j < FM; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// Wave-tile MFMA step of one 64-wide k-tile: for each of the two 32-wide k-steps read the FM activation fragments (rows a_row + 16 j of the
// A tile `as`) and the FN weight fragments (rows w_row + 16 i of the W tile `ws`), then FN x FM MFMAs, issued "swapped" (gemm_impl.h).
// a_row / w_row are the LANE's first rows (wave offset + lane & 15); fg = lane >> 4 is its 8-element k-group.
template <typename T, int FM, int FN>
__device__ __forceinline__ void wave_tile_mfma(f32x4 (&acc)[FN][FM], const T* as, const T* ws, int a_row, int w_row, int fg) {
  typedef typename Vec<T>::x8 x8;
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    x8 fa[FM], fw[FN];
#pragma unroll
    for (int j = 0; j < FM; ++j) {
      const int r = a_row + j * 16;
      fa[j] = *(const x8*)(as + r * 64 + swz(r, ks * 4 + fg));
    }
#pragma unroll
    for (int i = 0; i < FN; ++i) {
      const int r = w_row + i * 16;
      fw[i] = *(const x8*)(ws + r * 64 + swz(r, ks * 4 + fg));
    }
#pragma unroll
    for (int i = 0; i < FN; ++i)
#pragma unroll
      for (int j = 0; j < FM; ++j) acc[i][j] = mfma16(fw[i], fa[j], acc[i][j]);
  }
}

// ST-stage ring with ST - 1 tiles in flight: while `slot` is consumed, the slot consumed last iteration is refilled
template <int ST> __device__ __forceinline__ int ring_fill_slot(int slot) {
  int nslot = slot + ST - 1;
  if (nslot >= ST) nslot -= ST;
  return nslot;
}
template <int ST> __device__ __forceinline__ int ring_next_slot(int slot) { return slot + 1 == ST ? 0 : slot + 1; }

// split-K slab z covers k-tiles [begin, end): nk_total / splitk each, the first nk_total % splitk slabs one more.
struct KRange { int begin, end; };
__device__ __forceinline__ KRange splitk_range(const GemmCore& c, int z) {
  KRange r;
  r.begin = z * c.sk_quot + min(z, c.sk_rem);
  r.end = r.begin + c.sk_quot + (z < c.sk_rem ? 1 : 0);
  return r;
}

}  // namespace tt
