// Host side of the GEMM family: the ROUTE of one NrGemmParams -- which of the five kernel classes serves it, with which tile, split-K depth, tile
// order, weight layout and scratch -- decided ONCE by nr_gemm_route (gemm.hip) when a launch description is built, and launched as decided by
// nr_launch_gemm.  Each kernel file keeps the knowledge of its own kernel in one X_plan function that only the route calls; the launchers
// take the plan and read neither the environment nor a mode variable, so a replay can never disagree with the scratch and the packed weights its
// plan was given.  Host only; also the home of the small host helpers every kernel file uses.
#pragma once
#include "common.h"
#include <cstdlib>
#include <initializer_list>

// environment switch that is on unless set to 0
inline bool env_not_0(const char* name) {
  const char* v = getenv(name);
  return !(v && v[0] == '0');
}

// the rows every choice that can change a row's arithmetic is made for (NrGemmParams::plan_m): one clip's rows under deterministic batching, else M
inline int nr_plan_rows(const NrGemmParams& p) { return (p.plan_m > 0 && p.plan_m < p.M) ? p.plan_m : p.M; }

// > 64 KiB of dynamic LDS needs the opt-in attribute (gfx950 has 160 KiB per CU), once per device for the kernels in `fns`: `mask` holds one bit per
// device ordinal.  Returns 0, or 2 when the runtime refuses (the bit then stays clear)
inline int nr_lds_opt_in(unsigned long long& mask, std::initializer_list<const void*> fns, size_t bytes) {
  int dev = 0;
  (void)hipGetDevice(&dev);
  const unsigned long long bit = 1ull << (dev & 63);
  if (mask & bit) return 0;
  for (const void* fn : fns)
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) return 2;
  mask |= bit;
  return 0;
}

// in the order nr_gemm_route asks them
enum NrGemmClass { NR_GEMM_SMALLM, NR_GEMM_LIN160, NR_GEMM_ROWPANEL, NR_GEMM_G8P, NR_GEMM_TILED, NR_GEMM_NCLASS };
inline const char* const nr_gemm_class_name[NR_GEMM_NCLASS] = {"smallm", "lin160", "rowpanel", "gemm8p", "tiled"};
// what the chosen kernel reads as W: the matrix as the caller holds it ([N][K], for a tap-inner 3x3 conv [N][Cin/64][9][64]) or a packed copy.
// NR_W_FRAGMAJOR_E4M3 (smallm.hip, on request NrGemmParams::w8 only): OCP e4m3 codes [N/16][K/64][64 lanes][16 bytes] -- lane (fr, fg) of block
// (T, kp) holds, for the k-steps 2 kp + j (j = 0, 1), the eight codes of W[16 T + fr][32 (2 kp + j) + 8 fg .. + 7] -- then float scale[N] = 2^e[n]
enum NrWeightLayout { NR_W_ROWMAJOR, NR_W_TAP_INNER, NR_W_FRAGMAJOR, NR_W_LIN160, NR_W_LIN128Q, NR_W_FRAGMAJOR_E4M3 };

// gemm.hip: tile, ring depth, wave grid (41 = 4 x 1 row waves; 82 = the K-pair kernel of the 128 x 160 tile: 8 waves as two K groups) and split-K depth
// after the LayerNorm / out_f32 adjustments; adma / lin: the A-operand LDS-DMA and the Linear-only instantiation.  waves == 82: splitk is the number of
// fp32 slabs written (1: none, no reduce launch), each the sum of TWO K slices, and ws_bytes follows from it
struct TiledPlan { int bm, bn, splitk, stages, waves, adma, lin; };
// smallm.hip: nt n-tiles per slab, G column groups x J slabs each, C chunks of 640 along K
struct SmallmPlan { int nt, G, J, C; };
// lin160.hip: form 1 plain (big: 128-row tiles), 2 LayerNorm-folded GEGLU, 4 register panel (J column blocks per workgroup, workgroups by column group)
struct Lin160Plan { int form, big, J, cgmajor; };
struct RowPanelPlan { int nsplit; };     // rowpanel.hip: workgroups per 256-row panel
struct G8pPlan { int nt, phases; };      // gemm8p.hip: 64 nt columns per tile, 2 or 4 phases per k-tile

struct NrGemmRoute {
  int cls;             // NrGemmClass
  int weight_layout;   // NrWeightLayout: the `packed_w` nr_launch_gemm wants
  int m_fast;          // tile order of the tiled and ping-pong kernels: 0 n-fast, 1 m-fast, 8 grouped
  size_t ws_bytes;     // fp32 split-K scratch nr_launch_gemm wants (0: none)
  TiledPlan tiled;
  SmallmPlan smallm;
  Lin160Plan lin160;
  RowPanelPlan rowpanel;
  G8pPlan g8p;
};
