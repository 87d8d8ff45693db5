// Device blocks shared by the implicit-GEMM kernels: igemm_bf16_kernel, igemm_kpair_kernel and splitk_reduce_kernel (gemm.hip), g8p_kernel
// (gemm8p.hip).  A block is defined here once and the kernels call it in place of their own text; the loop structures stay in the kernels.
//
// A block is accepted on the device code (tools/isa_equal.sh, tools/isa_kernels.py): every caller keeps its assembly, or differs from it only
// behind its main loop, with the same register / scratch / LDS figures and a timing against the text it replaces (profiles/igemm_blocks_ab.txt).
// hipcc optimises a __forceinline__ function on its own BEFORE it inlines it, so the function form is not neutral and every block has to be tried.
// What was observed for the blocks below (necessary here, not a recipe: profiles/igemm_blocks_isa.txt lists blocks in the same shapes that failed):
//   * NrGemmParams as a POINTER.  As a reference (`dereferenceable`) the stand-alone pass widened the scalar load of out_scale in front of its
//     splat to a 16-byte vector load of the struct; inlined, that load kept a slice of the kernel's pinned copy of the params in memory until a
//     late pass and the register allocation of every caller changed.
//   * scalars and single vectors in by value, results returned or written through references to scalars; a block that took the accumulator or
//     fragment ARRAYS by reference moved the schedule of nearly every caller.
#pragma once
#include "device_prims.h"

namespace {

// Tile (bm, bn) of logical workgroup id `bid` among ntm x ntn tiles.  Inside an XCD's range the operand that is re-used by neighbouring tiles
// should be the BIG one.  m_fast == 1: neighbours share a weight panel (weight-heavy 4x4 / 8x8 levels); 0: an activation panel.
// Grouped order (m_fast = G >= 2): bands of G m-tiles, inside a band the m index runs fastest, then n.  The tiles that are in flight together on
// an XCD (2 per CU) then form a G x (64 / G) block: both operand panels of the block fit its 4 MiB L2, where a plain n-fastest walk streams the
// whole weight matrix past the L2 once per m-tile row (W > L2: GEGLU / q|k|v at 16x16, 8x8)
__device__ __forceinline__ void igemm_tile_order(int bid, int m_fast, int ntm, int ntn, int& bm, int& bn) {
  if (m_fast >= 2) {
    const int G = m_fast;
    const int band = nr_fdiv_small(bid, G * ntn);
    const int first = band * G;
    const int gsz = min(G, ntm - first);
    const int r = bid - band * G * ntn;
    bn = nr_fdiv_small(r, gsz);
    bm = first + r - bn * gsz;
  } else if (m_fast) { bn = nr_fdiv_small(bid, ntm); bm = bid - bn * ntm; } else { bm = nr_fdiv_small(bid, ntn); bn = bid - bm * ntn; }
}

// Phase form (NrGemmParams::ups == 2): the output row (pixel index) of row r = source pixel (image, y, x) of phase (py, px) = (phase >> 1, phase & 1):
// pixel (2 y + py, 2 x + px) of the upsampled image
__device__ __forceinline__ size_t igemm_phase_out_row(const NrGemmParams* p, int phase, int r) {
  const int hw = p->H * p->W;
  const int n = nr_fdiv_small(r, hw);
  const int q = r - n * hw;
  const int y = nr_fdiv_small(q, p->W), x = q - y * p->W;
  return (size_t)((n * p->OH + 2 * y + (phase >> 1)) * p->OW + 2 * x + (phase & 1));
}

// Pixel decode: row m of nimg images of hw = H * W pixels -> (img, y, x).  The tiled and K-pair kernels' per-lane A rows (output pixels of a 3x3 conv,
// source pixels of the phase form)
__device__ __forceinline__ void igemm_pixel_decode(int m, int hw, int W, int& img, int& y, int& x) {
  const int n = nr_fdiv_small(m, hw);
  const int r = m - n * hw;
  img = n; y = nr_fdiv_small(r, W); x = r - y * W;
}

// Tap-inner K order: byte offset of tap st_tap = 3 ky + kx from the centre pixel, (ky - 1) rows and (kx - 1) pixels of stride ld elements (wave-uniform)
__device__ __forceinline__ long long igemm_tap_delta(int st_tap, int W, int ld) {
  const int ky = st_tap / 3, kx = st_tap - ky * 3;
  return ((long long)(ky - 1) * W + (kx - 1)) * ld * (long long)sizeof(bf16);
}

// Tap-inner K order: byte offset of pixel (img, y, x) of an H x W image with pixel stride ld elements (a row's centre pixel; the tap offset is added per k-tile)
__device__ __forceinline__ long long igemm_pixel_byte(int img, int y, int x, int H, int W, int ld) {
  return (((long long)img * H + y) * W + x) * ld * (long long)sizeof(bf16);
}

// Tap-inner K order, one k-tile on: the next tap of the same 64 channels, after the ninth the next 64 channels
__device__ __forceinline__ void igemm_k_next_tap_inner(int& st_tap, int& st_c) {
  st_tap += 1;
  if (st_tap == 9) { st_tap = 0; st_c += 64; }
}

// One MFMA fragment of row `row`, 16-byte chunk `chunk` (k-step * 4 + lane >> 4) of an LDS tile of 64-element rows: the chunk index is
// XOR-swizzled with row & 7, the involution of the staging side, so the ds_read_b128 of a wave is conflict-free
__device__ __forceinline__ bf16x8 igemm_frag(const bf16* tile, int row, int chunk) { return *(const bf16x8*)(tile + row * 64 + ((chunk ^ (row & 7)) << 3)); }

// Direct finish of the 4 consecutive columns n .. n + 3 of row m that a lane's accumulator v holds: + bias, + row vector (rv: the row's
// p->rowvec + nr_rowvec_row, or null), * scale, quick-GELU, + residual, -> bf16 for one 8-byte store
__device__ __forceinline__ bf16x4 igemm_finish4(const NrGemmParams* p, f32x4 v, const float* rv, int m, int n) {
  if (p->bias) { const f32x4 b = *(const f32x4*)(p->bias + n); v += b; }
  if (rv) { const f32x4 t = *(const f32x4*)(rv + n); v += t; }
  v *= p->out_scale;
  if (p->act == 1) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = quick_gelu_f(v[e]);
  }
  if (p->res) {
    const bf16x4 r = *(const bf16x4*)(p->res + (size_t)m * p->ldr + n);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] += (float)r[e];
  }
  bf16x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = (bf16)v[e];
  return o;
}

// Staged finish: columns 8 c8 .. 8 c8 + 7 of row `row` of the fp32 C tile in LDS (sC: rows of BN floats, 16-byte chunks XOR-swizzled with
// row & 7) = output (m, n).  The arithmetic of igemm_finish4 on 8 columns, so that bias / row vector / residual loads and the bf16 store are
// 16 / 32-byte accesses; a GEGLU tile was finished when it was parked
template <int BN>
__device__ __forceinline__ bf16x8 igemm_finish8(const float* sC, int row, int c8, const NrGemmParams* p, int m, int n) {
  f32x4 va = *(const f32x4*)(sC + row * BN + (((2 * c8) ^ (row & 7)) << 2));
  f32x4 vb = *(const f32x4*)(sC + row * BN + (((2 * c8 + 1) ^ (row & 7)) << 2));
  if (!p->geglu) {
    if (p->bias) { va += *(const f32x4*)(p->bias + n); vb += *(const f32x4*)(p->bias + n + 4); }
    if (p->rowvec) {
      const float* rv = p->rowvec + nr_rowvec_row(*p, m) + n;
      va += *(const f32x4*)rv; vb += *(const f32x4*)(rv + 4);
    }
    va *= p->out_scale; vb *= p->out_scale;
    if (p->act == 1) {
#pragma unroll
      for (int e = 0; e < 4; ++e) { va[e] = quick_gelu_f(va[e]); vb[e] = quick_gelu_f(vb[e]); }
    }
    if (p->res) {
      const bf16x8 r = *(const bf16x8*)(p->res + (size_t)m * p->ldr + n);
#pragma unroll
      for (int e = 0; e < 4; ++e) { va[e] += (float)r[e]; vb[e] += (float)r[4 + e]; }
    }
  }
  bf16x8 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) { o[e] = (bf16)va[e]; o[4 + e] = (bf16)vb[e]; }
  return o;
}

}  // namespace
