// Implicit-GEMM convolution / Linear kernel on bf16 MFMA (v_mfma_f32_16x16x32_bf16), gfx950.
//
// One kernel serves every GEMM-shaped op on the denoiser path:
//   * 3x3 convs, stride 1/2, optional nearest-2x upsample gather, optional channel-concat of two
//     sources (reference: InflatedConv3d animatediff/models/resnet.py:10-18, Upsample3D :32-80,
//     Downsample3D :83-106, skip concat unet_blocks.py:634,740)
//   * 1x1 convs / nn.Linear (proj_in/out, to_q/k/v/out, GEGLU FF, conv_shortcut, ControlNet zero-convs)
// with fused epilogues: +bias, +time-embedding row vector (resnet.py:193-194), *scale, +residual,
// GEGLU gate (motion_module_new.py:516-518).
//
// Structure (per 256-thread workgroup = 2x2 waves, BMxBN output tile, BK = 64):
//   * global -> LDS by LDS-DMA (global_load_lds_dwordx4: 1 KiB = 8 tile rows per wave-instruction, no
//     VGPR staging).  The im2col gather, the zero padding and the M/N tails are all expressed through the
//     per-lane SOURCE address (invalid lanes read a 16-byte zero word), the LDS image stays lane-linear.
//   * LDS image [rows][64] bf16 (128-B rows); the 16-B chunk index is XOR-swizzled with (row & 7) on the
//     source side and on the ds_read_b128 side (same involution) -> conflict-free fragment reads.
//   * two LDS buffers, ONE barrier per k-tile: tile k+1 streams in while tile k is multiplied.
//   * the MFMA is issued "transposed" (weights = A operand, activations = B operand) so a lane's 4
//     accumulator registers are 4 consecutive output channels of one pixel -> 8/16-byte epilogue accesses.
//   * split-K for small-M / huge-K layers (the 4x4 and 8x8 levels: M = 512..2048, K up to 23 040):
//     each slice writes an fp32 slab, a second kernel sums the slabs in fixed order (deterministic, no
//     atomics) and applies the epilogue.
#include "launchers.h"
#include "igemm_blocks.h"
#include <cstdio>
#include <cstdlib>
#include <utility>

namespace {

// the BUILTIN form of nr_glds16 (device_prims.h says what the compiler does with it): see ADMA below
__device__ __forceinline__ void glds16_builtin(const void* src, void* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)lds_wave_base, 16, 0, 0);
}

// Diagnostic build only (make stamp -> libneurons_amd_stamp.so, tools/igemm_timeline.py): shader-clock stamps of wave 0 of the first
// 512 workgroups; _RT: the chip-wide 100 MHz counter
NR_STAMP_BUF(nr_stamp_buf, 512, 48);
#define NR_STAMP_AT(slot) NR_STAMP_PUT(nr_stamp_buf, slot)
#define NR_STAMP_RT(slot) NR_STAMP_PUT_RT(nr_stamp_buf, slot)

// WGM x WGN = wave grid over the (M, N) tile; 64*WGM*WGN threads
// ADMA: LDS-DMA issued from inline asm (tiles really stay in flight across the barrier; pays for long K) instead of the builtin
// (the compiler then drains the DMA in front of the next fragment read: DMA and MFMA of a k-tile do not overlap, but its M0
// handling is cheaper: measured faster for the short-K Linears of this workload).
// LIN: the launch is a plain Linear (1x1, one source): the im2col / tap / two-source paths are compiled out.  Same arithmetic; what it buys is
// code size: a launch starts with a cold instruction cache (tools/icache_probe.py: +0.4-1.4 us per launch when instantiations alternate, as
// they do in the engine's graphs), and two thirds of the launches of a denoising step are Linears.  LayerNorm-folded launches are always Linears.
// PH: the PHASE form of a nearest-2x upsample conv (NrGemmParams::ups == 2): the 3x3 conv on the replicated image is four 2x2 convs on the source,
// one per output parity (py, px), with the taps that read the same source pixel summed in the weights beforehand (w = [phase][N][tap][Cin], K = 4 Cin:
// 4/9 of the multiply-adds).  Rows are phase-major: 4 x ceil(Mp / BM) row tiles, Mp = nimg H W source pixels, a tile belongs to ONE phase (= one weight
// matrix); row (phase, r) is source pixel r on the A side and output pixel (2 y + py, 2 x + px) wherever a row index becomes an output address.
// A template parameter, not a run-time branch: every other instantiation is compiled from the text it had.
template <int BM, int BN, int NS, int WGM, int WGN, bool LNF = false, bool ADMA = false, bool LIN = LNF, bool PH = false>
__global__ __launch_bounds__(64 * WGM * WGN, (LNF && WGM * WGN == 8) ? 4 : 1) void igemm_bf16_kernel(NrGemmParams p_arg, int splitk, float* partial, int m_fast) {
  NrGemmParams p = nr_pin_params(p_arg);
  if constexpr (LIN) { p.ksize = 1; p.stride = 1; p.ups = 0; p.a1 = nullptr; p.c1 = 0; p.tap_inner = 0; p.pad_tl0 = 0; }
  static_assert(!PH || (!LIN && !LNF), "the phase form is a conv");
  if constexpr (PH) { p.ksize = 3; p.stride = 1; p.ups = 2; p.a1 = nullptr; p.c1 = 0; p.tap_inner = 0; p.pad_tl0 = 0; p.geglu = 0; p.rowvec = nullptr; p.res = nullptr; }
  splitk = nr_pin(splitk); partial = nr_pin(partial); m_fast = nr_pin(m_fast);
  constexpr int BK = 64;
  constexpr int NW = WGM * WGN;
  constexpr int WM = BM / WGM, WN = BN / WGN;
  constexpr int MT = WM / 16, NT = WN / 16;
  constexpr int GA = BM / (8 * NW), GB = BN / (8 * NW);   // 8-row groups per wave for the A / B tile
  static_assert(BM % (8 * NW) == 0 && BN % (8 * NW) == 0, "tile rows must split evenly over the waves");
  constexpr int TILE = (BM + BN) * BK;               // elements per LDS buffer
  extern __shared__ __attribute__((aligned(16))) bf16 smem[];   // NS * TILE elements (ring of NS k-tiles)

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  NR_STAMP_AT(0);
  NR_STAMP_RT(44);
  const int wm = wave / WGN, wn = wave % WGN;
  const int ntn = (p.N + BN - 1) / BN;
  const int Mrows = PH ? p.M >> 2 : p.M;          // rows a row-tile index runs over (PH: the source pixels of one phase)
  const int ntmp = (Mrows + BM - 1) / BM;
  const int ntm = PH ? 4 * ntmp : ntmp;
  int bid = nr_xcd_bid();                         // the n-tiles that share one A row-panel share an L2
  const int slice = splitk > 1 ? nr_fdiv_small(bid, ntn * ntm) : 0;
  bid -= slice * ntn * ntm;
  int bm, bn;
  igemm_tile_order(bid, m_fast, ntm, ntn, bm, bn);
  // PH: row tiles [phase * ntmp, (phase + 1) * ntmp) are one phase's, so in every tile order the tiles that share a weight matrix stay neighbours
  const int phase = PH ? nr_fdiv_small(bm, ntmp) : 0;
  if constexpr (PH) bm -= phase * ntmp;
  const int ph_py = phase >> 1, ph_px = phase & 1;
  const int m0 = bm * BM, n0 = bn * BN;
  NR_STAMP_AT(40);
  const int lr = lane >> 3;                 // row within the 8-row group
  const int lp = lane & 7;                  // physical 16-B chunk
  const int lchunk = (lp ^ lr) << 3;        // logical chunk (elements) this lane must fetch

  const int Cin = p.c0 + p.c1;

  // ---- per-lane A rows: group g = wave*GA + j, tile row = 8*g + lr ----
  int a_pix[GA], a_oy[GA], a_ox[GA];
  bool a_ok[GA];
#pragma unroll
  for (int j = 0; j < GA; ++j) {
    const int m = m0 + 8 * (wave * GA + j) + lr;
    a_ok[j] = m < Mrows;
    const int mm = a_ok[j] ? m : 0;
    if constexpr (PH) {      // (image, y, x) of the SOURCE pixel
      const int hw = p.H * p.W;
      igemm_pixel_decode(mm, hw, p.W, a_pix[j], a_oy[j], a_ox[j]);
    } else if (p.ksize == 1) {
      a_pix[j] = mm; a_oy[j] = 0; a_ox[j] = 0;
    } else {
      const int ohw = p.OH * p.OW;
      igemm_pixel_decode(mm, ohw, p.OW, a_pix[j], a_oy[j], a_ox[j]);
    }
  }
  const bf16* zsrc = (const bf16*)nr_zero16;
  // tap-inner K order (p.tap_inner): per row the byte offset of the centre pixel and a 9-bit mask of the taps that stay inside the image
  // (compiled out of the LayerNorm-fused instantiations, which only ever run 1x1: their 8-wave tiles must stay within 128 VGPRs to keep
  // two workgroups per CU)
  const bool tap_inner = !LNF && p.tap_inner != 0;
  long long a_cbyte[GA];
  unsigned a_tapmask[GA];
  if (tap_inner) {
#pragma unroll
    for (int j = 0; j < GA; ++j) {
      a_cbyte[j] = igemm_pixel_byte(a_pix[j], a_oy[j], a_ox[j], p.H, p.W, p.lda0);
      unsigned msk = 0;
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int iy = a_oy[j] + t / 3 - 1, ix = a_ox[j] + t % 3 - 1;
        if (a_ok[j] && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W) msk |= 1u << t;
      }
      a_tapmask[j] = msk;
    }
  }

  NR_STAMP_AT(41);
  const int nk_total = p.K / BK;
  int kt_begin = 0, kt_end = nk_total;
  if (splitk > 1) { kt_begin = nr_fdiv_small(nk_total * slice, splitk); kt_end = nr_fdiv_small(nk_total * (slice + 1), splitk); }

  // ---- running source pointers of the NEXT k-tile to stage.  The k index walks (tap, channel) with the
  // channel fastest, so between two k-tiles every pointer simply advances by 64 elements; the im2col
  // address arithmetic (border test, pixel index, 64-bit multiply) is redone only when the tap or the concat
  // source changes (once per Cin/64 tiles).  Rows that are padding / out of range sit on a 16-byte zero word
  // with increment 0.  This keeps the main loop at ~2 VALU per LDS-DMA instead of ~15. ----
  const bf16* ap[GA];
  int ainc[GA];
  const bf16* wp[GB];
  int winc[GB];
  int st_tap, st_c;
  {
    const int kbase = kt_begin * BK;
    if (tap_inner) { const int q9 = nr_fdiv_small(kt_begin, 9); st_tap = kt_begin - 9 * q9; st_c = q9 * BK; }
    else { st_tap = p.ksize == 3 ? nr_fdiv_small(kbase, Cin) : 0; st_c = kbase - st_tap * Cin; }
#pragma unroll
    for (int j = 0; j < GB; ++j) {
      const int n = n0 + 8 * (wave * GB + j) + lr;
      const bool ok = n < p.N;
      wp[j] = ok ? p.w + ((size_t)phase * p.N + n) * p.K + kbase + lchunk : zsrc;
      winc[j] = ok ? BK : 0;
    }
  }
  // tap-inner: every k-tile is another tap of the same 64 channels: pointer = centre + (wave-uniform) tap offset, or the zero word
  auto setup_rows_tap_inner = [&]() {
    const long long delta = igemm_tap_delta(st_tap, p.W, p.lda0);
    const char* base = reinterpret_cast<const char*>(p.a0 + st_c + lchunk) + delta;
#pragma unroll
    for (int j = 0; j < GA; ++j) {
      const bool ok = (a_tapmask[j] >> st_tap) & 1u;
      ap[j] = ok ? reinterpret_cast<const bf16*>(base + a_cbyte[j]) : zsrc;
    }
  };
  auto setup_rows = [&]() {
    if (tap_inner) { setup_rows_tap_inner(); return; }
    const bf16* src; int ld;
    if (st_c < p.c0) { src = p.a0 + st_c; ld = p.lda0; } else { src = p.a1 + (st_c - p.c0); ld = p.lda1; }
    src += lchunk;
    if constexpr (PH) {      // tap (a, b) of phase (py, px) reads source pixel (y + a + py - 1, x + b + px - 1), zero outside the source
      const int dy = (st_tap >> 1) + ph_py - 1, dx = (st_tap & 1) + ph_px - 1;
#pragma unroll
      for (int j = 0; j < GA; ++j) {
        const int iy = a_oy[j] + dy, ix = a_ox[j] + dx;
        const bool ok = a_ok[j] && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
        const size_t pix = ((size_t)a_pix[j] * p.H + iy) * p.W + ix;
        ap[j] = ok ? src + pix * ld : zsrc;
        ainc[j] = ok ? BK : 0;
      }
    } else if (p.ksize == 1) {
#pragma unroll
      for (int j = 0; j < GA; ++j) {
        ap[j] = a_ok[j] ? src + (size_t)a_pix[j] * ld : zsrc;
        ainc[j] = a_ok[j] ? BK : 0;
      }
    } else {
      const int ky = st_tap / 3, kx = st_tap - ky * 3;
      const int VH = p.ups ? p.H * 2 : p.H, VW = p.ups ? p.W * 2 : p.W;
#pragma unroll
      for (int j = 0; j < GA; ++j) {
        int iy = a_oy[j] * p.stride + ky - (p.pad_tl0 ? 0 : 1);
        int ix = a_ox[j] * p.stride + kx - (p.pad_tl0 ? 0 : 1);
        const bool ok = a_ok[j] && iy >= 0 && iy < VH && ix >= 0 && ix < VW;
        if (p.ups) { iy >>= 1; ix >>= 1; }
        const size_t pix = ((size_t)a_pix[j] * p.H + iy) * p.W + ix;
        ap[j] = ok ? src + pix * ld : zsrc;
        ainc[j] = ok ? BK : 0;
      }
    }
  };
  NR_STAMP_AT(42);
  setup_rows();
  NR_STAMP_AT(43);

  auto stage = [&](int buf) {
    bf16* sA = smem + buf * TILE;
    bf16* sB = sA + BM * BK;
    if constexpr (ADMA) {
      const unsigned la = nr_lds_addr(sA + wave * GA * 8 * BK), lb = nr_lds_addr(sB + wave * GB * 8 * BK);
#pragma unroll
      for (int j = 0; j < GA; ++j) nr_glds16(ap[j], la + (unsigned)(j * 8 * BK * (int)sizeof(bf16)));
#pragma unroll
      for (int j = 0; j < GB; ++j) nr_glds16(wp[j], lb + (unsigned)(j * 8 * BK * (int)sizeof(bf16)));
    } else {
#pragma unroll
      for (int j = 0; j < GA; ++j) glds16_builtin(ap[j], sA + (wave * GA + j) * 8 * BK);
#pragma unroll
      for (int j = 0; j < GB; ++j) glds16_builtin(wp[j], sB + (wave * GB + j) * 8 * BK);
    }
    // advance to the next k-tile
#pragma unroll
    for (int j = 0; j < GB; ++j) wp[j] += winc[j];
    if (tap_inner) {
      igemm_k_next_tap_inner(st_tap, st_c);
      setup_rows_tap_inner();
      return;
    }
    st_c += BK;
    bool resetup = false;
    if (st_c == Cin) { st_c = 0; st_tap += 1; resetup = true; }
    else if (p.c1 > 0 && st_c == p.c0) resetup = true;
    if (resetup) {
      if (st_tap < (PH ? 4 : p.ksize * p.ksize)) setup_rows();
    } else {
#pragma unroll
      for (int j = 0; j < GA; ++j) ap[j] += ainc[j];
    }
  };

  f32x4 acc[NT][MT];
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int j = 0; j < MT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int fr = lane & 15, fg = lane >> 4;
  // LayerNorm fusion: row sums / sums of squares of the raw activation fragments.  The WGN waves that share an A slab
  // split the k-steps between them (v_dot2c_f32_bf16: 8 VALU ops per fragment), combined through LDS after the loop.
  float ln_s1[MT], ln_s2[MT];
#pragma unroll
  for (int j = 0; j < MT; ++j) { ln_s1[j] = 0.f; ln_s2[j] = 0.f; }
  float* ln_stat = reinterpret_cast<float*>(smem + NS * TILE);   // LNF only: 2 * WGN * BM floats behind the operand ring

  // ---- main loop: ring of NS LDS buffers, tiles kt+1 .. kt+NS-2 stay in flight across the barrier ----
  constexpr int G = GA + GB;                 // LDS-DMA instructions per wave per k-tile (wave-uniform)
#pragma unroll
  for (int s0 = 0; s0 < NS - 1; ++s0)
    if (kt_begin + s0 < kt_end) stage(s0);
  int cur = 0;
  NR_STAMP_AT(1);
  for (int kt = kt_begin; kt < kt_end; ++kt) {
    // tile kt must have landed; the younger (NS-2) tiles may stay outstanding (vmcnt counts in issue order)
    if (kt + (NS - 2) < kt_end) nr_wait_vmcnt<(NS - 2) * G>(); else nr_wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();            // everyone's pieces of tile kt landed; everyone left tile kt-1
    NR_STAMP_AT(4 + (kt - kt_begin));
    const bf16* sA = smem + cur * TILE;
    const bf16* sB = sA + BM * BK;
    // fragment reads of k-step 0 go out FIRST, so their LDS latency is covered by the staging code below
    // (pointer bumps + LDS-DMA issue for tile kt+NS-1) instead of sitting exposed in front of the MFMAs
    bf16x8 wf[2][NT], xf[2][MT];
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      const int row = wn * WN + i * 16 + fr;
      wf[0][i] = igemm_frag(sB, row, fg);
    }
#pragma unroll
    for (int j = 0; j < MT; ++j) {
      const int row = wm * WM + j * 16 + fr;
      xf[0][j] = igemm_frag(sA, row, fg);
    }
    __builtin_amdgcn_sched_barrier(0);
    {
      const int nxt = kt + NS - 1;           // refill the buffer tile kt-1 occupied
      int nb = cur + NS - 1; if (nb >= NS) nb -= NS;
      if (nxt < kt_end) stage(nb);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      const int row = wn * WN + i * 16 + fr;
      wf[1][i] = igemm_frag(sB, row, 4 + fg);
    }
#pragma unroll
    for (int j = 0; j < MT; ++j) {
      const int row = wm * WM + j * 16 + fr;
      xf[1][j] = igemm_frag(sA, row, 4 + fg);
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int j = 0; j < MT; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[ks][i], xf[ks][j], acc[i][j], 0, 0, 0);
    if constexpr (LNF) {
      const bf16x2 one2 = {(bf16)1.0f, (bf16)1.0f};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        if (((2 * kt + ks) & (WGN - 1)) != wn) continue;      // this k-step belongs to a sibling wave
#pragma unroll
        for (int j = 0; j < MT; ++j)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const bf16x2 pr = {xf[ks][j][2 * e], xf[ks][j][2 * e + 1]};
            ln_s2[j] = __builtin_amdgcn_fdot2_f32_bf16(pr, pr, ln_s2[j], false);
            ln_s1[j] = __builtin_amdgcn_fdot2_f32_bf16(pr, one2, ln_s1[j], false);
          }
      }
    }
    cur = cur + 1 == NS ? 0 : cur + 1;
  }
  NR_STAMP_AT(2);
  // per-row mean / rstd of this wave's MT row tiles (lane: row fr of each tile)
  float ln_mu[MT], ln_rs[MT];
  if constexpr (LNF) {
#pragma unroll
    for (int j = 0; j < MT; ++j) {
      float a = ln_s1[j], b = ln_s2[j];
      a += __shfl_xor(a, 16, 64); b += __shfl_xor(b, 16, 64);
      a += __shfl_xor(a, 32, 64); b += __shfl_xor(b, 32, 64);
      if (fg == 0) {
        const int row = wm * WM + j * 16 + fr;
        ln_stat[(0 * WGN + wn) * BM + row] = a;
        ln_stat[(1 * WGN + wn) * BM + row] = b;
      }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < MT; ++j) {
      const int row = wm * WM + j * 16 + fr;
      float a = 0.f, b = 0.f;
#pragma unroll
      for (int w = 0; w < WGN; ++w) { a += ln_stat[(0 * WGN + w) * BM + row]; b += ln_stat[(1 * WGN + w) * BM + row]; }
      const float inv = 1.0f / (float)p.K;
      const float mu = a * inv;
      ln_mu[j] = mu;
      ln_rs[j] = rsqrtf(fmaxf(b * inv - mu * mu, 0.f) + p.ln_eps);
    }
    // acc <- rstd_m * (acc - mean_m * sum_k W'[n][k]); the (beta . W + bias) term is p.bias, added by the epilogues below
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      const int n = n0 + wn * WN + i * 16 + 4 * fg;
      const f32x4 cn = n < p.N ? *(const f32x4*)(p.ln_c + n) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < MT; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[i][j][r] = ln_rs[j] * (acc[i][j][r] - ln_mu[j] * cn[r]);
    }
  }

  // ---- epilogue: lane holds out[m = ..+fr][n = ..+4*fg + r], r = 0..3 ----
  if (partial) {
    float* slab = partial + (size_t)slice * p.M * p.N;
#pragma unroll
    for (int j = 0; j < MT; ++j) {
      const int m = m0 + wm * WM + j * 16 + fr;
      if (m >= Mrows) continue;
      const int ms = PH ? phase * Mrows + m : m;      // the slabs stay dense: [slice][phase * Mp + r][N]
#pragma unroll
      for (int i = 0; i < NT; ++i) {
        const int n = n0 + wn * WN + i * 16 + 4 * fg;
        if (n >= p.N) continue;
        nr_store16f(slab + (size_t)ms * p.N + n, acc[i][j]);
      }
    }
    return;
  }
  // Staged epilogue (whenever the fp32 C tile fits in the LDS ring): accumulators -> LDS (16-byte chunks
  // XOR-swizzled with row&7: conflict-free both ways) -> each thread handles 8 consecutive output channels of one
  // row, so bias / time-embedding / residual loads and the bf16 store are 16/32-byte accesses that cover whole
  // 128..256-byte row segments (the direct path below writes 8 bytes per lane in 32-byte segments).
  constexpr bool STAGED = (size_t)BM * BN * sizeof(float) <= (size_t)NS * TILE * sizeof(bf16);
  if constexpr (STAGED) {
    constexpr int NTH = 64 * NW;
    float* sC = reinterpret_cast<float*>(smem);
    __syncthreads();                       // every wave is done with the operand tiles
    const int bno = p.geglu ? BN / 2 : BN; // output columns of this tile
#pragma unroll
    for (int j = 0; j < MT; ++j) {
      const int row = wm * WM + j * 16 + fr;
      if (!p.geglu) {
#pragma unroll
        for (int i = 0; i < NT; ++i) {
          const int c4 = ((wn * WN + i * 16) >> 2) + fg;
          *(f32x4*)(sC + row * BN + ((c4 ^ (row & 7)) << 2)) = acc[i][j];
        }
      } else {
        if constexpr (NT % 2 == 0) {
#pragma unroll
          for (int i = 0; i < NT; i += 2) {
            const int nv = n0 + wn * WN + i * 16 + 4 * fg;
            f32x4 v = acc[i][j], g = acc[i + 1][j];
            if (p.bias && nv < p.N) { v += *(const f32x4*)(p.bias + nv); g += *(const f32x4*)(p.bias + nv + 16); }
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = v[e] * gelu_erf_fast(g[e]);
            const int c4 = (((wn * WN + i * 16) >> 1) >> 2) + fg;
            *(f32x4*)(sC + row * BN + ((c4 ^ (row & 7)) << 2)) = o;
          }
        }
      }
    }
    __syncthreads();
    const int c8n = bno >> 3;
    const int nout = p.geglu ? p.N / 2 : p.N;
    const int nb0 = p.geglu ? n0 / 2 : n0;
    for (int idx = tid; idx < BM * c8n; idx += NTH) {
      const int row = idx / c8n, c8 = idx - row * c8n;
      const int m = m0 + row, n = nb0 + c8 * 8;
      if (m >= Mrows || n >= nout) continue;
      const bf16x8 o = igemm_finish8<BN>(sC, row, c8, &p, m, n);
      nr_store16(p.out + (size_t)(PH ? igemm_phase_out_row(&p, phase, m) : m) * p.ldo + n, o);
    }
#ifdef NR_STAMP
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
    NR_STAMP_AT(3);
    NR_STAMP_RT(45);
    return;
  }
#pragma unroll
  for (int j = 0; j < MT; ++j) {
    const int m = m0 + wm * WM + j * 16 + fr;
    if (m >= Mrows) continue;
    const size_t mo = PH ? igemm_phase_out_row(&p, phase, m) : m;
    const float* rv = p.rowvec ? p.rowvec + nr_rowvec_row(p, m) : nullptr;
    if (!p.geglu) {
#pragma unroll
      for (int i = 0; i < NT; ++i) {
        const int n = n0 + wn * WN + i * 16 + 4 * fg;
        if (n >= p.N) continue;
        const bf16x4 o = igemm_finish4(&p, acc[i][j], rv, m, n);
        nr_store8(p.out + mo * p.ldo + n, o);
      }
    } else {
      if constexpr (NT % 2 == 0) {
#pragma unroll
        for (int i = 0; i < NT; i += 2) {
          const int nv = n0 + wn * WN + i * 16 + 4 * fg;  // value columns (permuted W row index)
          if (nv >= p.N) continue;
          const int ng = nv + 16;                          // matching gate columns
          f32x4 v = acc[i][j], g = acc[i + 1][j];
          if (p.bias) {
            v += *(const f32x4*)(p.bias + nv);
            g += *(const f32x4*)(p.bias + ng);
          }
          const int oc = ((n0 + wn * WN + i * 16) >> 1) + 4 * fg;
          bf16x4 o;
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = (bf16)(v[e] * gelu_erf_fast(g[e]));
          nr_store8(p.out + mo * p.ldo + oc, o);
        }
      }
    }
  }
}

// K-PAIR form of the 128 x 160 tile (TiledPlan::waves == 82): the two K slices (2 j, 2 j + 1) of an S-slice plan in ONE 512-thread workgroup.  Waves
// 0-3 and 4-7 are two K groups; each is the 2 x 2 wave grid of igemm_bf16_kernel<128, 160, 2, 2, 2, false, true> on the same output tile, with its own
// two-stage ring (2 x 2 x 36 KiB = the LDS two free workgroups of that kernel hold on a CU), its own running pointers and its own 20 accumulator tiles, and
// group g covers exactly the k-tiles slice 2 j + g has there.  After the loop group 1 hands its accumulators to group 0 through the (dead) ring, group 0
// adds them -- slice 2 j first, the order of splitk_reduce_kernel -- and runs the direct epilogue (nslab == 1: no slab, no reduce launch) or writes
// slab j of nslab = S / 2.  Same partial sums in the same order as the S-slice plan when nslab == 1.
// Loop: waves w and w + 4 share a SIMD, and s_barrier is workgroup-wide: with both groups in igemm_bf16_kernel's one-barrier loop they wait together and
// issue their MFMAs together (measured 10-35 % slower than two free workgroups, profiles/kpair_ab.txt).  So the loop takes two barriers per k-tile and
// group 1 runs half an iteration late: after barrier 2 t group 0 reads the fragments of its tile t and issues the DMA of tile t + 1 while group 1 multiplies
// its tile t - 1; after barrier 2 t + 1 the roles swap -- a matrix segment beside a memory segment on every SIMD (gemm8p.hip's stagger with the groups
// splitting K instead of M).  Each group's "my tile has landed" wait sits in front of the barrier that opens its own load segment; a group that runs out
// of k-tiles (the slices differ by one when 2 nslab does not divide the k-tiles) keeps arriving at the barriers.
// LIN: as igemm_bf16_kernel.  TAPI: the tap-inner K order of a one-source stride-1 conv; a template parameter because the rows' state of the two K orders
// together (centre byte offsets and tap masks | pixel coordinates) does not fit beside 80 accumulator and 72 fragment registers in the 256 a wave has.
template <bool LIN, bool TAPI>
__global__ __launch_bounds__(512, 1) void igemm_kpair_kernel(NrGemmParams p_arg, int nslab, float* partial, int m_fast) {
  NrGemmParams p = nr_pin_params(p_arg);
  static_assert(!(LIN && TAPI), "the tap-inner order is a conv's");
  p.ups = 0;
  if constexpr (LIN) { p.ksize = 1; p.stride = 1; p.a1 = nullptr; p.c1 = 0; p.pad_tl0 = 0; }
  if constexpr (TAPI) { p.ksize = 3; p.stride = 1; p.a1 = nullptr; p.c1 = 0; p.pad_tl0 = 0; }
  nslab = nr_pin(nslab); partial = nr_pin(partial); m_fast = nr_pin(m_fast);
  constexpr int BM = 128, BN = 160, BK = 64, WGN = 2, NW = 4;      // per K group
  constexpr int WM = 64, WN = 80, MT = WM / 16, NT = WN / 16;
  constexpr int GA = BM / (8 * NW), GB = BN / (8 * NW);
  constexpr int TILE = (BM + BN) * BK;               // elements per LDS buffer
  extern __shared__ __attribute__((aligned(16))) bf16 smem[];   // 2 groups x 2 stages x TILE elements

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int grp = __builtin_amdgcn_readfirstlane(tid >> 8);            // K group
  const int wave = __builtin_amdgcn_readfirstlane((tid >> 6) & 3);      // wave within the group
  NR_STAMP_AT(0);
  NR_STAMP_RT(44);
  const int wm = wave / WGN, wn = wave % WGN;
  const int ntn = (p.N + BN - 1) / BN;
  const int ntm = (p.M + BM - 1) / BM;
  int bid = nr_xcd_bid();
  const int pair = nslab > 1 ? nr_fdiv_small(bid, ntn * ntm) : 0;
  bid -= pair * ntn * ntm;
  int bm, bn;
  igemm_tile_order(bid, m_fast, ntm, ntn, bm, bn);
  const int m0 = bm * BM, n0 = bn * BN;
  const int lr = lane >> 3;                 // row within the 8-row group
  const int lp = lane & 7;                  // physical 16-B chunk
  const int lchunk = (lp ^ lr) << 3;        // logical chunk (elements) this lane must fetch
  const int Cin = p.c0 + p.c1;

  // ---- per-lane A rows: group g = wave*GA + j, tile row = 8*g + lr ----
  int a_pix[GA], a_oy[GA], a_ox[GA];
  bool a_ok[GA];
#pragma unroll
  for (int j = 0; j < GA; ++j) {
    const int m = m0 + 8 * (wave * GA + j) + lr;
    a_ok[j] = m < p.M;
    const int mm = a_ok[j] ? m : 0;
    if (p.ksize == 1) {
      a_pix[j] = mm; a_oy[j] = 0; a_ox[j] = 0;
    } else {
      const int ohw = p.OH * p.OW;
      igemm_pixel_decode(mm, ohw, p.OW, a_pix[j], a_oy[j], a_ox[j]);
    }
  }
  const bf16* zsrc = (const bf16*)nr_zero16;
  constexpr bool tap_inner = TAPI;
  long long a_cbyte[GA];
  unsigned a_tapmask[GA];
  if constexpr (tap_inner) {
#pragma unroll
    for (int j = 0; j < GA; ++j) {
      a_cbyte[j] = igemm_pixel_byte(a_pix[j], a_oy[j], a_ox[j], p.H, p.W, p.lda0);
      unsigned msk = 0;
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int iy = a_oy[j] + t / 3 - 1, ix = a_ox[j] + t % 3 - 1;
        if (a_ok[j] && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W) msk |= 1u << t;
      }
      a_tapmask[j] = msk;
    }
  }

  // the k-tiles of slice 2 pair + grp of the 2 nslab slices, and how many the sibling group has (the groups take the same number of barriers)
  const int nk_total = p.K / BK;
  const int S = 2 * nslab, slice = 2 * pair + grp;
  const int kt_begin = nr_fdiv_small(nk_total * slice, S), kt_end = nr_fdiv_small(nk_total * (slice + 1), S);
  const int nmine = kt_end - kt_begin;
  const int nsib = nr_fdiv_small(nk_total * ((slice ^ 1) + 1), S) - nr_fdiv_small(nk_total * (slice ^ 1), S);
  const int nmax = max(nmine, nsib);

  // ---- running source pointers of the NEXT k-tile to stage (igemm_bf16_kernel) ----
  const bf16* ap[GA];
  const bf16* wp[GB];
  int st_tap, st_c;
  {
    const int kbase = kt_begin * BK;
    if constexpr (tap_inner) { const int q9 = nr_fdiv_small(kt_begin, 9); st_tap = kt_begin - 9 * q9; st_c = q9 * BK; }
    else { st_tap = p.ksize == 3 ? nr_fdiv_small(kbase, Cin) : 0; st_c = kbase - st_tap * Cin; }
#pragma unroll
    for (int j = 0; j < GB; ++j) {
      // a W row past N feeds only columns that are never stored: it reads the last row instead of the zero word, so every row advances alike
      const int n = min(n0 + 8 * (wave * GB + j) + lr, p.N - 1);
      wp[j] = p.w + (size_t)n * p.K + kbase + lchunk;
    }
  }
  auto setup_rows_tap_inner = [&]() {
    const long long delta = igemm_tap_delta(st_tap, p.W, p.lda0);
    const char* base = reinterpret_cast<const char*>(p.a0 + st_c + lchunk) + delta;
#pragma unroll
    for (int j = 0; j < GA; ++j) {
      const bool ok = (a_tapmask[j] >> st_tap) & 1u;
      ap[j] = ok ? reinterpret_cast<const bf16*>(base + a_cbyte[j]) : zsrc;
    }
  };
  auto setup_rows = [&]() {
    if constexpr (tap_inner) { setup_rows_tap_inner(); return; }
    const bf16* src; int ld;
    if (st_c < p.c0) { src = p.a0 + st_c; ld = p.lda0; } else { src = p.a1 + (st_c - p.c0); ld = p.lda1; }
    src += lchunk;
    if (p.ksize == 1) {
#pragma unroll
      for (int j = 0; j < GA; ++j) {
        ap[j] = a_ok[j] ? src + (size_t)a_pix[j] * ld : zsrc;
      }
    } else {
      const int ky = st_tap / 3, kx = st_tap - ky * 3;
#pragma unroll
      for (int j = 0; j < GA; ++j) {
        const int iy = a_oy[j] * p.stride + ky - (p.pad_tl0 ? 0 : 1);
        const int ix = a_ox[j] * p.stride + kx - (p.pad_tl0 ? 0 : 1);
        const bool ok = a_ok[j] && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
        const size_t pix = ((size_t)a_pix[j] * p.H + iy) * p.W + ix;
        ap[j] = ok ? src + pix * ld : zsrc;
      }
    }
  };
  setup_rows();

  bf16* ring = smem + grp * 2 * TILE;      // this group's two buffers
  auto stage = [&](int buf) {
    bf16* sA = ring + buf * TILE;
    bf16* sB = sA + BM * BK;
    const unsigned la = nr_lds_addr(sA + wave * GA * 8 * BK), lb = nr_lds_addr(sB + wave * GB * 8 * BK);
#pragma unroll
    for (int j = 0; j < GA; ++j) nr_glds16(ap[j], la + (unsigned)(j * 8 * BK * (int)sizeof(bf16)));
#pragma unroll
    for (int j = 0; j < GB; ++j) nr_glds16(wp[j], lb + (unsigned)(j * 8 * BK * (int)sizeof(bf16)));
    // advance to the next k-tile
#pragma unroll
    for (int j = 0; j < GB; ++j) wp[j] += BK;
    if constexpr (tap_inner) {
      igemm_k_next_tap_inner(st_tap, st_c);
      setup_rows_tap_inner();
      return;
    }
    st_c += BK;
    bool resetup = false;
    if (st_c == Cin) { st_c = 0; st_tap += 1; resetup = true; }
    else if (p.c1 > 0 && st_c == p.c0) resetup = true;
    if (resetup) {
      if (st_tap < p.ksize * p.ksize) setup_rows();
    } else {
#pragma unroll
      for (int j = 0; j < GA; ++j) ap[j] += ap[j] != zsrc ? BK : 0;      // a row on the zero word (padding, M tail) stays there
    }
  };

  f32x4 acc[NT][MT];
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int j = 0; j < MT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int fr = lane & 15, fg = lane >> 4;
  bf16x8 wf[2][NT], xf[2][MT];
  // the fragments of k-step ks of the tile in buffer `buf`
  auto read_frags = [&](int buf, int ks) {
    const bf16* sA = ring + buf * TILE;
    const bf16* sB = sA + BM * BK;
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      const int row = wn * WN + i * 16 + fr;
      wf[ks][i] = igemm_frag(sB, row, 4 * ks + fg);
    }
#pragma unroll
    for (int j = 0; j < MT; ++j) {
      const int row = wm * WM + j * 16 + fr;
      xf[ks][j] = igemm_frag(sA, row, 4 * ks + fg);
    }
  };
  auto multiply = [&]() {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int j = 0; j < MT; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[ks][i], xf[ks][j], acc[i][j], 0, 0, 0);
  };
  // a workgroup-wide barrier no MFMA, LDS access or DMA issue moves across
  auto barrier = [&]() {
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
  };

  // the load segment of tile t: its fragments into registers, the DMA of tile t + 1 into the buffer whose fragments (tile t - 1) every wave of the group
  // consumed in the multiply segment one barrier earlier
  auto load_tile = [&](int t) {
    if (t < nmine) {
      read_frags(t & 1, 0);
      __builtin_amdgcn_sched_barrier(0);
      if (t + 1 < nmine) stage((t & 1) ^ 1);
      __builtin_amdgcn_sched_barrier(0);
      read_frags(t & 1, 1);
    }
  };
  if (nmine > 0) stage(0);
  NR_STAMP_AT(1);
  if (grp == 0) {
    for (int t = 0; t < nmax; ++t) {
      if (t < nmine) nr_wait_vmcnt<0>();      // tile t of this group has landed
      barrier();
      if (t < 18) NR_STAMP_AT(4 + 2 * t);
      load_tile(t);                           // ... beside group 1's MFMAs of its tile t - 1
      barrier();
      if (t < 18) NR_STAMP_AT(5 + 2 * t);
      if (t < nmine) multiply();              // ... beside group 1's load segment of its tile t
    }
  } else {
    for (int t = 0; t < nmax; ++t) {
      barrier();
      if (t > 0 && t - 1 < nmine) multiply();
      if (t < nmine) nr_wait_vmcnt<0>();
      barrier();
      load_tile(t);
    }
    if (nmax - 1 < nmine) multiply();
  }
  NR_STAMP_AT(2);

  // ---- acc(slice 2 pair) + acc(slice 2 pair + 1): group 1 -> LDS in lane order (20 x 256 x 16 B = 80 KiB of the 144 KiB ring) -> group 0 ----
  f32x4* xch = reinterpret_cast<f32x4*>(smem);
  const int t256 = tid & 255;
  barrier();                                   // both groups are done with their rings
  if (grp == 1) {
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
      for (int j = 0; j < MT; ++j) xch[(i * MT + j) * 256 + t256] = acc[i][j];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // s_barrier waits for no counter: the stores have reached the LDS before group 0 is let through
  }
  barrier();
  if (grp == 1) return;
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int j = 0; j < MT; ++j) acc[i][j] = acc[i][j] + xch[(i * MT + j) * 256 + t256];

  // ---- epilogue of group 0: lane holds out[m = ..+fr][n = ..+4*fg + r], r = 0..3 (the slab / direct paths of igemm_bf16_kernel) ----
  if (partial) {
    float* slab = partial + (size_t)pair * p.M * p.N;
#pragma unroll
    for (int j = 0; j < MT; ++j) {
      const int m = m0 + wm * WM + j * 16 + fr;
      if (m >= p.M) continue;
#pragma unroll
      for (int i = 0; i < NT; ++i) {
        const int n = n0 + wn * WN + i * 16 + 4 * fg;
        if (n >= p.N) continue;
        nr_store16f(slab + (size_t)m * p.N + n, acc[i][j]);
      }
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < MT; ++j) {
    const int m = m0 + wm * WM + j * 16 + fr;
    if (m >= p.M) continue;
    const float* rv = p.rowvec ? p.rowvec + nr_rowvec_row(p, m) : nullptr;
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      const int n = n0 + wn * WN + i * 16 + 4 * fg;
      if (n >= p.N) continue;
      const bf16x4 o = igemm_finish4(&p, acc[i][j], rv, m, n);
      nr_store8(p.out + (size_t)m * p.ldo + n, o);
    }
  }
#ifdef NR_STAMP
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
  NR_STAMP_AT(3);
  NR_STAMP_RT(45);
}

// out[m][n] = epilogue( sum_s partial[s][m][n] ), 4 consecutive n per thread.  PH: slab row m = phase * Mp + r of a phase-form launch goes to the
// output pixel of (phase, r) (igemm_bf16_kernel); such a launch has neither rowvec nor res
template <bool PH>
__global__ __launch_bounds__(256) void splitk_reduce_kernel(NrGemmParams p_arg, int splitk, const float* __restrict__ partial) {
  const NrGemmParams p = nr_pin_params(p_arg);
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const int n4 = p.N >> 2;
  if (idx >= (long long)p.M * n4) return;
  const int m = (int)(idx / n4);
  const int n = (int)(idx - (long long)m * n4) << 2;
  const size_t slab = (size_t)p.M * p.N;
  const float* src = partial + (size_t)m * p.N + n;
  f32x4 v = *(const f32x4*)src;
  for (int s = 1; s < splitk; ++s) v += *(const f32x4*)(src + s * slab);
  const bf16x4 o = igemm_finish4(&p, v, p.rowvec ? p.rowvec + nr_rowvec_row(p, m) : nullptr, m, n);
  size_t mo = (size_t)m;
  if constexpr (PH) {
    const int Mp = p.M >> 2, phase = m / Mp;
    mo = igemm_phase_out_row(&p, phase, m - phase * Mp);
  }
  nr_store8(p.out + mo * p.ldo + n, o);
}

typedef TiledPlan Plan;       // gemm_route.h

// THE instantiations of igemm_bf16_kernel: one row per (tile, wave grid) with the ring depths NS compiled for the conv / Linear forms (per depth: builtin
// DMA and ADMA, and up to LIN_MAX_RING deep the LIN form of both), for the LayerNorm-folded form (one kernel per depth) and whether the phase form
// exists (ADMA or not, always PHASE_RING deep).  The route's legalisation (legalise) and the launcher's dispatch (launch_exact) are both generated from
// this table and nothing else names a tile or a depth: a plan is routable exactly when it is launchable.  160 kernels.
constexpr unsigned rings(std::initializer_list<int> ns) { unsigned m = 0; for (int n : ns) m |= 1u << n; return m; }
constexpr bool has_ring(unsigned set, int ns) { return ns >= 0 && ns < 32 && (set >> ns & 1); }
struct TileRow {
  int bm, bn, wgm, wgn;
  unsigned ns, ns_ln;      // ring depths of the conv / Linear forms | of the LayerNorm-folded form (bit NS)
  bool phase;
  constexpr int waves() const { return wgn == 1 ? 41 : wgm * wgn; }      // TiledPlan::waves (41 = 4 x 1 row waves)
  // dynamic LDS: the ring, and behind it the row-statistics exchange of the LayerNorm-folded form
  constexpr size_t lds_bytes(int NS, bool ln) const { return (size_t)NS * (bm + bn) * 64 * sizeof(bf16) + (ln ? (size_t)2 * wgn * bm * sizeof(float) : 0); }
};
constexpr int RING_MIN = 2, RING_MAX = 8, LIN_MAX_RING = 4, PHASE_RING = 2;
constexpr TileRow TILES[] = {
    {256, 160, 2, 2, rings({2, 3}), 0, false},
    {256, 128, 2, 2, rings({2, 3}), 0, false},
    {256, 128, 4, 2, rings({2, 3}), 0, true},
    {128, 160, 4, 1, rings({3, 4}), rings({3, 4}), false},      // row-wave tile of the wide GEGLU projections: 108 / 144 KiB, one workgroup per CU
    {128, 160, 2, 2, rings({2, 3, 4}), 0, true},
    {128, 128, 2, 4, rings({2, 3, 4}), rings({2}), true},
    {128, 128, 2, 2, rings({2, 3, 4}), rings({2}), false},
    {128, 64, 4, 2, rings({2, 3, 4}), rings({2, 4}), false},
    {128, 64, 2, 2, rings({2, 3, 4}), rings({2, 4}), true},
    {64, 160, 2, 2, rings({2, 3, 4}), rings({2, 3}), false},    // one-round tile of the N = 1280 Linears at M = 1024 / 2048
    {64, 64, 2, 2, rings({2, 3, 4, 6, 8}), rings({2, 4}), true},      // depths 6 / 8: tools/shortk_sweep.py
    {64, 32, 2, 2, rings({2, 3, 4, 6, 8}), rings({2, 4}), false},
};
constexpr int NTILES = sizeof(TILES) / sizeof(TILES[0]), NRINGS = RING_MAX - RING_MIN + 1;
constexpr bool table_fits_lds() {
  for (const TileRow& t : TILES)
    for (int ns = 0; ns < 32; ++ns)
      if ((has_ring(t.ns, ns) && (ns < RING_MIN || ns > RING_MAX || t.lds_bytes(ns, false) > 160 * 1024)) ||
          (has_ring(t.ns_ln, ns) && (!has_ring(t.ns, ns) || t.lds_bytes(ns, true) > 160 * 1024)) || (t.phase && !has_ring(t.ns, PHASE_RING))) return false;
  return true;
}
static_assert(table_fits_lds(), "every ring is RING_MIN .. RING_MAX deep and fits the 160 KiB of a CU's LDS; a LayerNorm-folded depth and the phase depth are depths of the tile");
// the row of a tile with this wave count (0: any), among the rows with the phase form when `phase`
constexpr const TileRow* find_row(int bm, int bn, int waves, bool phase = false) {
  for (const TileRow& t : TILES)
    if (t.bm == bm && t.bn == bn && (waves == 0 || t.waves() == waves) && (!phase || t.phase)) return &t;
  return nullptr;
}

// Tile / wave-grid / split-K choice.  Rules distilled from tools/gemm_sweep.py on MI355X (profiles/): two LDS
// stages (2 workgroups per CU) beat a deeper ring; 8 waves help the 128x128 tile; long-K layers with few
// tiles gain 1.3-1.7x from split-K; 128x160 only pays for N = 320.
// row tiles of a launch: the phase form tiles each of its four phases (M / 4 source pixels) on its own
inline long long row_tiles(const NrGemmParams& p, int bm) { return p.ups == 2 ? 4ll * ((p.M / 4 + bm - 1) / bm) : (p.M + bm - 1) / bm; }
// tiles of a launch on bm x bn tiles
inline long long tile_count(const NrGemmParams& p, int bm, int bn) { return row_tiles(p, bm) * ((p.N + bn - 1) / bn); }

// Phase-form upsample convs: four GEMMs of M / 4 rows and K = 4 Cin that share one launch, so the rules of choose_plan keyed on nk >= 128 (K = 9 Cin)
// do not fire.  Per shape by NR_IGEMM_FORCE sweeps of the op (HBM-cold weights, profiles/ups_phase_ab.txt; us per launch, the 3x3 form beside it):
//   M = 2048  N = 1280 K = 5120  (3x3: 72-82)    128x160 split-K 4: 50.5   split-K 2: 55   one slice: 87   128x128: 62-77   128x64: 61-72   64x64: 67-79
//   M = 8192  N = 1280 K = 5120  (3x3: 322)      128x160 one slice (512 tiles, one round): 108   two slices: 132   128x128: 140-163   128x64: 148   256x128: 201
//   M = 32768 N = 640  K = 2560  (3x3: 231-240)  128x160: 109   128x128: 115   128x64: 135   256x128: 139
//   N = 512 / 256 (the VAE: no 160-column tiling)  128x128 8 waves: 140 / 551 / 640 against 256x128: 156 / 610 / 774 (3x3: 292 / 1153 / 1241)
// The split-K rule for under-filled grids below is choose_plan's reasoning, not a measurement of this form.
Plan choose_plan_phase(const NrGemmParams& p) {
  const int nk = p.K / 64;
  Plan pl{};
  pl.splitk = 1; pl.stages = 2; pl.waves = 4;
  // N a multiple of 160: the 128 x 160 tile on every measured shape; four K slices where the four phases of <= 2048 rows leave 128 tiles of a long K
  if (p.N % 160 == 0) {
    pl.bm = 128; pl.bn = 160;
    if (p.M <= 2048 && nk >= 64) { pl.splitk = 4; return pl; }
  } else {
    const bool n128 = p.N % 128 == 0 || p.N >= 960;
    if (n128 && tile_count(p, 128, 128) >= 400) { pl.bm = 128; pl.bn = 128; pl.waves = 8; }
    else if (tile_count(p, 128, 64) >= 256) { pl.bm = 128; pl.bn = 64; }
    else { pl.bm = 64; pl.bn = 64; }
  }
  // under-filled grids with a K worth cutting: deterministic split-K as in choose_plan (every slice keeps >= 16 k-tiles, <= 4 slabs)
  const long long tiles = tile_count(p, pl.bm, pl.bn);
  if (tiles < 512 && nk >= 64) {
    int s_ = (int)((1024 + tiles - 1) / tiles);
    if (s_ > nk / 16) s_ = nk / 16;
    if (s_ > 4) s_ = 4;
    pl.splitk = s_ < 1 ? 1 : s_;
  }
  return pl;
}
Plan choose_plan_slices(const NrGemmParams& p) {
  const int nk = p.K / 64;
  Plan pl{};
  pl.splitk = 1; pl.stages = 2; pl.waves = 4;
  if (p.ups == 2) return choose_plan_phase(p);
  // 4x4-level convs (M <= 1024, K >= 8192): L2-bandwidth-bound with small tiles (every n-tile re-reads A, every m-tile
  // re-reads W), so take the biggest tile and get the parallelism from a deep deterministic split-K instead
  if (!p.geglu && p.M <= 1024 && nk >= 128 && p.N % 160 == 0) {
    pl.bm = 128; pl.bn = 160; pl.splitk = nk >= 300 ? 16 : 8;
    return pl;
  }
  // same reasoning one level up (8x8 convs, M = 2048, K >= 8192): +1.5 % on the DDIM step over 128x64 tiles with split-K 4
  if (!p.geglu && p.ksize == 3 && p.M <= 2048 && nk >= 128 && p.N % 160 == 0) {
    pl.bm = 128; pl.bn = 160; pl.splitk = 4;
    return pl;
  }
  // 16x16-level convs (M = 8192, N = 640, K >= 5760): 128x160 with two K slices instead of 128x64 (per-shape in-situ A/B,
  // tools/igemm_ab_shapes.py: -0.06 / -0.09 ms per DDIM step)
  if (!p.geglu && p.ksize == 3 && p.M <= 8192 && p.N % 160 == 0 && p.N < 960 && nk >= 64 && tile_count(p, 128, 160) >= 128 && tile_count(p, 128, 160) < 512) {
    pl.bm = 128; pl.bn = 160; pl.splitk = 2;
    return pl;
  }
  // folded FeedForward.net.2 + proj_out GEMMs (K = 5C = 6400) at the 8x8 level: same as the long-K convs above (tools/sweep_ff.sh:
  // 46.6 vs 55.2 us)
  if (!p.geglu && p.ksize == 1 && p.M <= 2048 && p.M > 512 && nk >= 96 && p.N % 160 == 0) {
    pl.bm = 128; pl.bn = 160; pl.splitk = 4;
    return pl;
  }
  // Linears whose 64 x 160 tiling is ONE round of the chip (128-256 tiles: N = 1280 at the 8x8 level, M = 1024 / 2048) with K = 1024..3072: one
  // workgroup per CU with a 3-deep ring instead of 320-640 smaller tiles two per CU: 16.2 vs 19.2 us at M = 2048, N = K = 1280, 26.5 vs 36.3 at
  // K = 2560, 17.1 vs 20.1 LayerNorm-folded (2-deep ring there) (profiles/r05_sweep_64x160.txt, HBM-cold weights)
  static const bool t64x160_rule = env_not_0("NR_IGEMM_T64X160");   // A/B switch
  if (t64x160_rule && p.ksize == 1 && !p.geglu && p.N % 160 == 0 && p.M > 512 && nk >= 16 && nk <= 48 && tile_count(p, 64, 160) >= 128 && tile_count(p, 64, 160) <= 256) {
    pl.bm = 64; pl.bn = 160; pl.stages = 3;
    return pl;
  }
  const bool n128 = p.N % 128 == 0 || p.N >= 960;          // <= 6 % padded columns otherwise
  if (!p.geglu && p.N % 160 == 0 && p.N < 960 && p.N % 128 != 0 && nk >= 20 && tile_count(p, 128, 160) >= 256) { pl.bm = 128; pl.bn = 160; }
  else if (n128 && tile_count(p, 128, 128) >= 400) { pl.bm = 128; pl.bn = 128; pl.waves = 8; }
  else if (tile_count(p, 128, 64) >= 512 || (tile_count(p, 128, 64) >= 256 && nk > 32)) { pl.bm = 128; pl.bn = 64; pl.waves = nk <= 32 ? 8 : 4; }
  else if (tile_count(p, 64, 64) >= 256 && nk <= 96) { pl.bm = 64; pl.bn = 64; }
  else if (p.M >= 1024 && tile_count(p, 128, 64) >= 64) { pl.bm = 128; pl.bn = 64; }
  else { pl.bm = 64; pl.bn = 64; }
  // 4x4-level / sgm 16x16-level Linears (M <= 512): fewer blocks than CUs, every k-step waits for cold weights from HBM.
  // A 4-deep ring (3 tiles in flight) and, where the epilogue allows, 64x32 tiles (twice the blocks) measured -10 % on the
  // sgm keyframe step (tools/igemm_ab_sgm.sh); deeper rings (6, 8) and split-K + reduce were slower.
  static const bool smallm_rule = env_not_0("NR_IGEMM_SMALLM");   // A/B switch
  static const bool wide_rule = env_not_0("NR_IGEMM_WIDE");         // A/B switch
  static const bool rowwave_rule = env_not_0("NR_IGEMM_ROWWAVE");   // A/B switch
  if (smallm_rule && p.ksize == 1 && p.M <= 512 && nk >= 8) {
    pl.bm = 64; pl.bn = p.geglu ? 64 : 32; pl.waves = 4; pl.stages = 4;
    // wide GEGLU projections (N = 10240): enough 128x128 tiles for the chip, 22.4 vs 29.9 us; K = 6400 (folded net.2 + proj_out):
    // 64x64 tiles with four K slices, 23.1 vs 29.6 us (tools/sweep_ff.sh)
    if (p.geglu && p.N >= 8192 && p.M >= 256) { pl.bm = 128; pl.bn = 128; pl.waves = 8; pl.stages = 2; }
    // ... and exactly 256 tiles of 128 x 160 at M = 512 (one round, one workgroup per CU, ring 3-4 deep: the 320 tiles of 128 x 128 wait for
    // HBM-cold k-tiles with one in flight): 4 x 1 waves of 32 x 160 so that a wave holds whole (value, gate) pairs; 23.1 vs 28.9 us plain,
    // 27.0 vs 31.7 us LayerNorm-folded (profiles/r05_sweep_rowwave.txt)
    if (rowwave_rule && p.geglu && p.N >= 8192 && p.N % 160 == 0 && p.M > 256 && tile_count(p, 128, 160) <= 256) {
      pl.bm = 128; pl.bn = 160; pl.waves = 41; pl.stages = p.ln_c ? 3 : 4;
    }
    else if (!p.geglu && nk >= 96 && !p.ln_c) { pl.bm = 64; pl.bn = 64; pl.stages = 2; pl.splitk = 4; return pl; }
    // wide projections (q|k|v, N = 3840): 960 tiles of 64 x 32 re-read A 120 times; 240 tiles of 128 x 64 with the same 4-deep ring:
    // 13.3 vs 19.8 us plain, 15.2 vs 17.5 us LayerNorm-folded (profiles/r05_sweep_ln_ns4.txt, HBM-cold weights)
    else if (wide_rule && !p.geglu && tile_count(p, 64, 32) > 640 && tile_count(p, 128, 64) >= 192) { pl.bm = 128; pl.bn = 64; pl.waves = 8; pl.stages = 4; }
  }
  if (!p.geglu) {
    const long long tiles = tile_count(p, pl.bm, pl.bn);
    const int cap_m = p.M >= 8192 ? 2 : (p.M >= 2048 ? 4 : 8);      // bounds the fp32 slab traffic (8*M*N*split bytes)
    const int min_tiles = p.M <= 1024 ? 8 : 16;                      // k-tiles each slice keeps
    if (tiles < 512 && nk >= 4 * min_tiles) {
      int s_ = (int)((1280 + tiles - 1) / tiles);
      if (s_ > nk / min_tiles) s_ = nk / min_tiles;
      if (s_ > cap_m) s_ = cap_m;
      if (s_ < 1) s_ = 1;
      pl.splitk = s_;
    }
  }
  return pl;
}

constexpr int KPAIR_WAVES = 82;      // TiledPlan::waves of a K-pair plan: 8 waves as 2 K groups; its splitk counts the slabs written (1: none)
// THE test of a K-pair plan, asked by the rule, the override, the legalisation and the launcher: a form igemm_kpair_kernel is built for -- a plain conv or
// Linear (no LayerNorm fold, GEGLU, upsample gather of either form or raw fp32 result) -- on the 128 x 160 tile, at least one k-tile per K group
inline bool kpair_ok(const NrGemmParams& p, const Plan& pl) {
  return pl.waves == KPAIR_WAVES && !p.ln_c && !p.geglu && !p.ups && !p.out_f32 && pl.bm == 128 && pl.bn == 160 && pl.splitk >= 1 && 2 * pl.splitk <= p.K / 64;
}
// a K-pair plan as the plan on free workgroups that computes the same sums: one slice per K group
inline void kpair_undo(Plan& pl) { if (pl.waves == KPAIR_WAVES) { pl.waves = 4; pl.splitk *= 2; } }

// choose_plan_slices, and where that is the two-stage 128 x 160 tile with an even number of K slices on a form the K-pair kernel has: the slices in
// pairs, one 8-wave workgroup per pair and half the slabs (none, and no reduce launch, for two slices).  Same LDS, waves per SIMD and bytes in flight
// per CU.  Admitted by measurement (us per launch, HBM-cold weights, slices on free workgroups -> K pairs; profiles/kpair_ab.txt):
//   M = 8192 N = 640   3x3 K = 5760 tap-inner 80 -> 77    K = 11520 two-source 134 -> 129    K = 17280 two-source 182 -> 182
//   M = 2048 N = 1280  3x3 K = 11520 tap-inner 75 -> 69   stride 2 77 -> 69   K = 23040 two-source 129 -> 126   Linear K = 6400 48.8 -> 45.1
//   M = 512  N = 1280  3x3 K = 23040 (16 slices -> 8 pairs) 52 -> 44
// Kept out: M = 512, K = 11520 (8 slices -> 4 pairs: 128 workgroups leave half the CUs idle, 35.7 -> 39.3), hence the full-round condition; the
// replicated upsample gather (ups == 1), whose routes tests/test_ups_phase_host.py records.
// The one-slice M = 8192, N = 640, K = 3200 Linears (one 4-wave workgroup per CU on 128 x 64 tiles, no second wave on a SIMD) run as one pair per 128 x 160
// tile, one round of the chip: 44.3 -> 40.2 us (two free slices + reduce: 47.0).  No other one-slice shape was measured, so none is admitted.
Plan choose_plan(const NrGemmParams& p) {
  const Plan pl = choose_plan_slices(p);
  static const bool kpair_rule = env_not_0("NR_IGEMM_KPAIR");      // A/B switch
  if (!kpair_rule) return pl;
  const long long tiles = tile_count(p, 128, 160);      // (a K-pair plan is never a phase form's: kpair_ok)
  Plan kp = pl;
  kp.waves = KPAIR_WAVES;
  if (pl.bm == 128 && pl.bn == 160 && pl.waves == 4 && pl.stages == 2 && pl.splitk >= 2 && pl.splitk % 2 == 0) {
    kp.splitk = pl.splitk / 2;
    if (tiles * kp.splitk >= 256 && kpair_ok(p, kp)) return kp;
  } else if (p.ksize == 1 && pl.bm == 128 && pl.bn == 64 && pl.waves == 4 && pl.stages == 2 && pl.splitk == 1 && p.N == 640 && p.K == 3200 && tiles == 256) {
    kp.bm = 128; kp.bn = 160;      // the one measured shape (M in 8065 .. 8192) on the plan it was measured against, no other
    if (kpair_ok(p, kp)) return kp;
  }
  return pl;
}

// the shape the plan is chosen for: plan_m rows when the caller asks for batch-independent arithmetic (common.h), else the real M
inline NrGemmParams plan_view(const NrGemmParams& p) {
  NrGemmParams q = p;
  q.M = nr_plan_rows(p);
  return q;
}

typedef void (*igemm_kern_t)(NrGemmParams, int, float*, int);

// The instantiation (row I of TILES, ring depth NS) of the form the request and the plan name.  Returns 0; 9 when the table has none (nothing is launched);
// 2 when the runtime refuses the LDS opt-in
template <int I, int NS>
int launch_inst(const NrGemmParams& p, unsigned grid, const Plan& pl, float* partial, int m_fast, hipStream_t stream) {
  constexpr TileRow T = TILES[I];
  constexpr int BM = T.bm, BN = T.bn, WGM = T.wgm, WGN = T.wgn;
  const bool ln = p.ln_c != nullptr, plain = !ln && p.ups != 2;
  igemm_kern_t k = nullptr;
  int ki = 0;                   // LayerNorm-folded | 1 + 2 lin + adma | 5 + adma phase form
  // LayerNorm-folded: its row-statistics exchange buffer lives in the DYNAMIC allocation behind the ring (TileRow::lds_bytes): a static __shared__ array
  // next to > 64 KiB of dynamic LDS made the first launch (and any hipGraph node captured from it) run with a short allocation.
  if constexpr (has_ring(T.ns_ln, NS))
    if (ln) k = igemm_bf16_kernel<BM, BN, NS, WGM, WGN, true>;
  if constexpr (T.phase && NS == PHASE_RING)
    if (p.ups == 2 && !ln) { k = !pl.adma ? igemm_bf16_kernel<BM, BN, NS, WGM, WGN, false, false, false, true> : igemm_bf16_kernel<BM, BN, NS, WGM, WGN, false, true, false, true>; ki = 5 + pl.adma; }
  if constexpr (has_ring(T.ns, NS))
    if (plain && !pl.lin) { k = !pl.adma ? igemm_bf16_kernel<BM, BN, NS, WGM, WGN, false, false> : igemm_bf16_kernel<BM, BN, NS, WGM, WGN, false, true>; ki = 1 + pl.adma; }
  if constexpr (has_ring(T.ns, NS) && NS <= LIN_MAX_RING)      // plain Linears (1x1, one source) on the instantiation without the conv paths
    if (plain && pl.lin) { k = !pl.adma ? igemm_bf16_kernel<BM, BN, NS, WGM, WGN, false, false, true> : igemm_bf16_kernel<BM, BN, NS, WGM, WGN, false, true, true>; ki = 3 + pl.adma; }
  if (!k) return 9;
  const size_t shm = T.lds_bytes(NS, ln);
  static unsigned long long attr_done[7] = {};          // per instantiation
  if (const int rc = nr_lds_opt_in(attr_done[ki], {(const void*)k}, shm)) return rc;
  hipLaunchKernelGGL(k, dim3(grid), dim3(64 * WGM * WGN), shm, stream, p, pl.splitk, partial, m_fast);
  return 0;
}
// the exact lookup of (bm, bn, waves, stages) in TILES x [RING_MIN, RING_MAX]; J = row * NRINGS + depth - RING_MIN.  Never a neighbour: 9 when nothing matches
template <size_t... J>
int launch_exact(std::index_sequence<J...>, const NrGemmParams& p, unsigned grid, const Plan& pl, float* partial, int m_fast, hipStream_t stream) {
  int rc = 9;
  const auto is = [&](const TileRow& t, int ns) { return pl.bm == t.bm && pl.bn == t.bn && pl.waves == t.waves() && pl.stages == ns; };
  (void)((is(TILES[J / NRINGS], RING_MIN + (int)(J % NRINGS)) &&
          ((rc = launch_inst<(int)(J / NRINGS), RING_MIN + (int)(J % NRINGS)>(p, grid, pl, partial, m_fast, stream)), true)) || ...);
  return rc;
}

// igemm_kpair_kernel: the K pairs of a 128 x 160 plan (waves == 82), pl.splitk slabs.  Returns 0; 2 when the runtime refuses the LDS opt-in
int launch_kpair(const NrGemmParams& p, unsigned grid, const Plan& pl, float* partial, int m_fast, hipStream_t stream) {
  const igemm_kern_t k = pl.lin ? igemm_kpair_kernel<true, false> : (p.tap_inner ? igemm_kpair_kernel<false, true> : igemm_kpair_kernel<false, false>);
  constexpr size_t shm = 2 * find_row(128, 160, 4)->lds_bytes(2, false);      // two K groups, each the two-stage ring of the tile's 2 x 2 row
  static unsigned long long attr_done[3] = {};          // per instantiation
  if (const int rc = nr_lds_opt_in(attr_done[pl.lin ? 0 : (p.tap_inner ? 1 : 2)], {(const void*)k}, shm)) return rc;
  hipLaunchKernelGGL(k, dim3(grid), dim3(512), shm, stream, p, pl.splitk, partial, m_fast);
  return 0;
}

// smallest depth of the set not below the request, else the deepest
constexpr int pick_ring(unsigned set, int want) {
  int deepest = 0;
  for (int ns = RING_MIN; ns <= RING_MAX; ++ns)
    if (has_ring(set, ns)) { if (ns >= want) return ns; deepest = ns; }
  return deepest;
}
// The one step from the plan the heuristics and NR_IGEMM_FORCE ask for to a row and ring of TILES that exist for the request's form (plain, LayerNorm-folded,
// phase): afterwards (bm, bn, waves, stages) is what runs.  Returns 9 for a tile the table does not have
int legalise(const NrGemmParams& p, Plan& pl) {
  const bool ln = p.ln_c != nullptr, phase = p.ups == 2;
  const bool row_wave = pl.waves == 41;          // as planned, whatever tile NR_IGEMM_FORCE then named
  if (pl.waves == KPAIR_WAVES) {                 // the K-pair kernel: one tile, one ring (the rule and the override only ever name it where kpair_ok holds)
    pl.stages = 2;
    return kpair_ok(p, pl) ? 0 : 9;
  }
  if (ln && pl.bn == 32) pl.bn = 64;             // every n-tile recomputes the row statistics: keep the n-tiles wide
  if (!find_row(pl.bm, pl.bn, 0)) return 9;
  const TileRow* t = phase ? find_row(pl.bm, pl.bn, 0, true) : find_row(pl.bm, pl.bn, pl.waves);      // phase form: the tile's phase row, whatever its wave grid
  if (!t && !phase) t = find_row(pl.bm, pl.bn, 4);             // a wave grid the tile is not built with: its 2 x 2 one (every tile has it)
  if (!t || (ln && !t->ns_ln)) t = find_row(128, 128, 8);      // a tile the form is not built for: 128 x 128 on 8 waves
  pl.bm = t->bm; pl.bn = t->bn; pl.waves = t->waves();
  if (phase) pl.stages = PHASE_RING;
  // LayerNorm-folded: a depth the form is not built with falls back to the two-stage ring (two workgroups per CU), NOT to the next deeper one; a row-wave
  // plan (one workgroup per CU, no two-stage ring) follows the rule of the plain forms
  else if (ln) pl.stages = row_wave || has_ring(t->ns_ln, pl.stages) ? pick_ring(t->ns_ln, pl.stages) : 2;
  else pl.stages = pick_ring(t->ns, pl.stages);
  return 0;
}

// test/tuning override: NR_IGEMM_FORCE="bm,bn,splitk,stages,order,waves" (a field < 0 or left out keeps the heuristic's choice): a tile of TILES (both
// fields or neither), K slices, ring depth 2 .. 8, tile order (0 n-fast, 1 m-fast, 8 grouped), waves 4 / 8 / 41 / 82 (41: the row-wave grid of 128 x 160;
// 82: its K-pair kernel, the K-slices field then counts slabs).  What
// it names goes through legalise like any plan, so the route records and the launcher runs the nearest instantiation of the request's form
void apply_override(const NrGemmParams& p, Plan& pl, int& m_fast) {
  const char* e = getenv("NR_IGEMM_FORCE");
  if (!e) return;
  // optional filters so an in-situ A/B (bench.py under hipGraph, no per-launch host overhead) can target one shape class:
  // NR_IGEMM_FORCE_MAXM / _MINM bound p.M, NR_IGEMM_FORCE_KS selects 1x1 or 3x3 launches
  if (const char* f = getenv("NR_IGEMM_FORCE_MAXM")) if (p.M > atoi(f)) return;
  if (const char* f = getenv("NR_IGEMM_FORCE_MINM")) if (p.M < atoi(f)) return;
  if (const char* f = getenv("NR_IGEMM_FORCE_KS")) if (p.ksize != atoi(f)) return;
  if (const char* f = getenv("NR_IGEMM_FORCE_N")) if (p.N != atoi(f)) return;
  if (const char* f = getenv("NR_IGEMM_FORCE_K")) if (p.K != atoi(f)) return;
  int bm = -1, bn = -1, sk = -1, st = -1, ord = -1, wv = -1;
  sscanf(e, "%d,%d,%d,%d,%d,%d", &bm, &bn, &sk, &st, &ord, &wv);
  kpair_undo(pl);      // a K-pair plan only where the sixth field names it: every other field means what it meant
  if (bm > 0 && bn > 0) {
    if (find_row(bm, bn, 0) && !(p.geglu && ((bn == 160 && !(bm == 128 && wv == 41)) || bn == 32))) { pl.bm = bm; pl.bn = bn; }
  }
  if (wv == 4 || wv == 8) pl.waves = wv;
  if (pl.bm == 256 && pl.bn == 128 && wv != 4) pl.waves = 8;
  if (pl.bn == 160 || pl.bm == 64) pl.waves = 4;
  if (wv == 41 && pl.bm == 128 && pl.bn == 160) pl.waves = 41;      // 4 x 1 waves (32 x 160 each): the row-wave tile
  if (sk > 0 && !p.geglu) { const int nk = p.K / 64; pl.splitk = sk > nk ? nk : sk; }
  // 82: the K-pair kernel on the 128 x 160 tile; the third field is then the number of slabs (1: none), each the sum of two K slices
  if (wv == KPAIR_WAVES) {
    Plan kp = pl;
    kp.waves = KPAIR_WAVES;
    if (sk <= 0) kp.splitk = pl.splitk >= 2 ? pl.splitk / 2 : 1;      // no slab count named: the planned slices in pairs
    if (2 * kp.splitk > p.K / 64) kp.splitk = p.K / 128;
    if (kpair_ok(p, kp)) pl = kp;
  }
  if (st >= 2 && st <= 8) pl.stages = st;
  if (ord >= 0) m_fast = ord;
}

// tile order: the bigger operand is the one neighbouring tiles share (1: m-fast, the weights); with enough tiles both ways 8 x 8 blocks of tiles
// (tools/gemm_sweep.py SWEEP_SET=order: never slower than either plain order, up to 12 % faster where the weights exceed one L2, and fewer L2 misses)
int tile_order(double w_elems, double a_elems, int ntm, int ntn) {
  static const bool grouped = env_not_0("NR_IGEMM_GROUPED");
  static const double grouped_minw = getenv("NR_IGEMM_GROUPED_MINW") ? atof(getenv("NR_IGEMM_GROUPED_MINW")) : 3.0e6;   // weight elements (in situ: 1e6 / 3e6 / 0 = 15.85 / 15.89 / 15.80 frames/s, off 15.93; HBM 49.3 -> 44.4 GB per step at 1e6)
  if (grouped && ntm >= 8 && ntn >= 4 && w_elems >= grouped_minw) return 8;
  return w_elems > a_elems ? 1 : 0;
}

// the one place the kernel classes are ordered.  packed_ok: the caller can hand the kernel a packed copy of W
int route(const NrGemmParams& p, NrGemmRoute* r, bool packed_ok) {
  std::memset(r, 0, sizeof(*r));
  r->weight_layout = p.tap_inner ? NR_W_TAP_INNER : NR_W_ROWMAJOR;
  const int Cin = p.c0 + p.c1;
  // the phase form of an upsample conv (ups == 2, w = [4 phases][N][4 taps][Cin], K = 4 Cin): the tiled kernel only, and only the plain conv --
  // 10: a field the form has no path for (second source, stride, tap_inner, pad_tl0, geglu, ln_c, out_f32; res / rowvec: their rows are not
  // mapped to output pixels); 11: the geometry is not a 2x upsample of H x W
  const bool phase = p.ups == 2;
  if (phase) {
    r->cls = NR_GEMM_TILED;
    if (p.ksize != 3 || p.stride != 1 || p.a1 || p.c1 || p.tap_inner || p.pad_tl0 || p.geglu || p.ln_c || p.out_f32 || p.res || p.rowvec) return 10;
    if (p.H < 1 || p.W < 1 || p.OH != 2 * p.H || p.OW != 2 * p.W || p.M < 4 || p.M % (p.OH * p.OW) != 0) return 11;
  } else if (p.ups != 0 && p.ups != 1) return 11;
  // M <= 512 Linears with K a multiple of 640: the panel-resident kernel on fragment-major weights (smallm.hip)
  // (the e4m3 request p.w8 names the weight layout of THIS class and nothing else: smallm_plan does not see it, the classes below ignore it)
  if (!phase && packed_ok && smallm_plan(p, &r->smallm)) { r->cls = NR_GEMM_SMALLM; r->weight_layout = p.w8 ? NR_W_FRAGMAJOR_E4M3 : NR_W_FRAGMAJOR; return 0; }
  // short-K Linears (K = 640 / 1280) on >= 2048 rows: the stage-stream kernel and its register-panel form (lin160.hip)
  if (!phase && packed_ok && lin160_plan(p, &r->lin160)) { r->cls = NR_GEMM_LIN160; r->weight_layout = r->lin160.form == 4 ? NR_W_LIN128Q : NR_W_LIN160; return 0; }
  // K = 320 Linears on >= 4096 rows: the register-resident row-panel kernel (rowpanel.hip)
  if (!phase && p.K == p.ksize * p.ksize * Cin && rowpanel_plan(p, &r->rowpanel)) { r->cls = NR_GEMM_ROWPANEL; return 0; }
  const double w_elems = (double)p.N * p.K;
  if (!phase && g8p_plan(p, &r->g8p)) {
    r->cls = NR_GEMM_G8P;
    r->m_fast = tile_order(w_elems, (double)p.M * Cin, (p.M + 255) / 256, (p.N + 64 * r->g8p.nt - 1) / (64 * r->g8p.nt));
    return 0;
  }
  r->cls = NR_GEMM_TILED;
  if (p.K % 64 != 0 || Cin % 64 != 0 || p.N % 32 != 0) return 1;
  if (p.a1 && (p.c0 % 64 != 0)) return 2;
  if (p.K != (phase ? 4 : p.ksize * p.ksize) * Cin) return 3;
  if (p.ksize != 1 && p.ksize != 3) return 4;
  if (p.tap_inner && (p.ksize != 3 || p.stride != 1 || p.ups || p.pad_tl0 || p.a1)) return 5;
  Plan& pl = r->tiled;
  pl = choose_plan(plan_view(p));
  const double a_elems = (double)p.M * Cin * (p.ksize == 3 ? (p.stride == 2 ? 4.0 : (p.ups ? 0.25 : 1.0)) : 1.0);
  // (phase form: w_elems is ONE phase's matrix and the order is chosen on one phase's row tiles; bands of 8 row tiles must not straddle two phases)
  const int ntm1 = (int)(phase ? row_tiles(p, pl.bm) / 4 : row_tiles(p, pl.bm));
  r->m_fast = tile_order(w_elems, a_elems, ntm1, (p.N + pl.bn - 1) / pl.bn);
  apply_override(p, pl, r->m_fast);
  if (p.ln_c) {      // LayerNorm-fused: every block must see the whole row (K = C) -> no split-K
    if (p.ksize != 1 || p.a1 || p.out_f32) return 8;
    pl.splitk = 1;
  }
  if (legalise(p, pl)) return 9;
  if (phase && r->m_fast >= 2 && (row_tiles(p, pl.bm) / 4) % r->m_fast != 0) r->m_fast = w_elems > a_elems ? 1 : 0;
  if (p.out_f32) {   // raw fp32 result: the kernel's slab path with a single K slice, no reduce pass
    if (p.geglu) return 7;
    pl.splitk = 1;
  }
  static const int adma_min = getenv("NR_IGEMM_ADMA_MINK") ? atoi(getenv("NR_IGEMM_ADMA_MINK")) : 24;   // k-tiles per slice; A/B switch
  static const bool lin_on = env_not_0("NR_IGEMM_LIN");                                                  // A/B switch
  pl.adma = pl.waves == KPAIR_WAVES || (p.K / 64) / (pl.splitk > 1 ? pl.splitk : 1) >= adma_min;      // the K-pair kernel: asm DMA only
  pl.lin = lin_on && p.ksize == 1 && !p.a1 && p.c1 == 0;
  if (pl.stages > LIN_MAX_RING) pl.lin = 0;       // the Linear-only instantiation exists for the rings Linears are planned with
  if (p.ln_c) { pl.adma = 0; pl.lin = 1; }        // the LayerNorm-folded form is one instantiation per ring: builtin DMA, a Linear by construction
  r->ws_bytes = pl.splitk > 1 ? (size_t)pl.splitk * p.M * p.N * sizeof(float) : 0;
  return 0;
}

// the tiled kernel as planned, then its split-K reduce
int launch_tiled(const NrGemmParams& p, const Plan& pl, int m_fast, float* workspace, hipStream_t stream) {
  if (pl.splitk < 1 || pl.splitk > p.K / 64 || ((p.ln_c || p.out_f32) && pl.splitk != 1)) return 9;
  const bool kpair = pl.waves == KPAIR_WAVES;
  if (kpair && !(kpair_ok(p, pl) && pl.stages == 2)) return 9;
  if (pl.splitk > 1 && !workspace) return 6;
  float* partial = p.out_f32 ? p.out_f32 : (pl.splitk > 1 ? workspace : nullptr);
  const unsigned grid = (unsigned)(tile_count(p, pl.bm, pl.bn) * pl.splitk);
  // no such instantiation (9) or no LDS opt-in (2): fail loudly, never launch a neighbour on a grid computed for this tile
  if (const int rc = kpair ? launch_kpair(p, grid, pl, partial, m_fast, stream)
                           : launch_exact(std::make_index_sequence<NTILES * NRINGS>{}, p, grid, pl, partial, m_fast, stream)) return rc;
  if (pl.splitk > 1) {
    const long long total = (long long)p.M * (p.N / 4);
    hipLaunchKernelGGL(p.ups == 2 ? splitk_reduce_kernel<true> : splitk_reduce_kernel<false>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, p,
                       pl.splitk, (const float*)partial);
  }
  return 0;
}

}  // namespace

extern "C" int nr_gemm_route(const NrGemmParams* pp, NrGemmRoute* r) { return route(*pp, r, true); }
extern "C" int nr_gemm_route_rowmajor(const NrGemmParams* pp, NrGemmRoute* r) { return route(*pp, r, false); }

// Launches what the route says; reads no environment, no mode and no eligibility rule.  Returns 0 on success, nonzero when the route does not fit
// the launch (6: split-K planned and no workspace given)
extern "C" int nr_launch_gemm(const NrGemmParams* pp, const NrGemmRoute* r, const bf16* packed_w, float* ws, hipStream_t stream) {
  switch (r->cls) {
    case NR_GEMM_SMALLM: return nr_launch_smallm(pp, &r->smallm, packed_w, r->weight_layout, stream);
    case NR_GEMM_LIN160: return nr_launch_lin160(pp, &r->lin160, packed_w, stream);
    case NR_GEMM_ROWPANEL: return nr_launch_rowpanel(pp, &r->rowpanel, stream);
    case NR_GEMM_G8P: return nr_launch_g8p(pp, &r->g8p, r->m_fast, stream);
    case NR_GEMM_TILED: return launch_tiled(*pp, r->tiled, r->m_fast, ws, stream);
  }
  return 9;
}

// the packed copies of a row-major [N][K] weight matrix: bytes (0: the shape has none) and the pack launch
extern "C" size_t nr_gemm_packed_bytes(int layout, int N, int K) {
  switch (layout) {
    case NR_W_FRAGMAJOR: return (N % 16 == 0 && K % 32 == 0) ? (size_t)N * K * sizeof(bf16) : 0;
    case NR_W_FRAGMAJOR_E4M3: return (N > 0 && K > 0 && N % 16 == 0 && K % 64 == 0) ? (size_t)N * K + (size_t)N * sizeof(float) : 0;   // codes + row scales
    case NR_W_LIN160: return nr_lin160_stream_bytes(N, K);
    case NR_W_LIN128Q: return nr_lin128q_stream_bytes(N, K);
  }
  return 0;
}
extern "C" int nr_launch_gemm_w_pack(int layout, const bf16* w, int N, int K, bf16* dst, hipStream_t stream) {
  switch (layout) {
    case NR_W_FRAGMAJOR: return nr_launch_smallm_w_pack(w, dst, N, K, stream);
    case NR_W_FRAGMAJOR_E4M3: return nr_launch_smallm_w8_pack(w, dst, N, K, stream);
    case NR_W_LIN160: return nr_launch_lin160_w_pack(w, N, K, dst, stream);
    case NR_W_LIN128Q: return nr_launch_lin128q_w_pack(w, N, K, dst, stream);
  }
  return 1;
}

#ifdef NR_STAMP
extern "C" int nr_stamp_read(void* dst, size_t bytes, int clear) { return nr_stamp_read_buf(nr_stamp_buf, dst, bytes, clear); }
#endif
