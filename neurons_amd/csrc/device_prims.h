// Device primitives shared by the kernel files (*.hip except engine.hip): a primitive used by two kernel files lives here, once.
// Everything is __device__ __forceinline__ or sits in the anonymous namespace, so every translation unit keeps its own copy and the
// device code of a kernel does not depend on which other kernels are linked beside it.
#pragma once
#include "common.h"

namespace {

typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

// what an invalid lane of an LDS-DMA gather reads instead of its tile element (padding, M / N tails)
__device__ __attribute__((aligned(16))) const unsigned int nr_zero16[4] = {0u, 0u, 0u, 0u};

// ----------------------------------------------------------------------------------------------
// LDS-DMA and its waits
// ----------------------------------------------------------------------------------------------

// the wave-uniform LDS byte address of p, as M0 wants it
__device__ __forceinline__ unsigned nr_lds_addr(const void* p) {
  return __builtin_amdgcn_readfirstlane((unsigned)(unsigned long long)(lptr_t)p);
}

// LDS-DMA (global_load_lds_dwordx4: 16 bytes per lane, 1 KiB per wave-instruction to lds_wave_base + 16 lane) as inline asm: the compiler
// must NOT see it.  A BUILTIN global_load_lds is a pending LDS write to hipcc, which then puts s_waitcnt vmcnt(0) in front of the next
// ds_read that may alias it, i.e. behind every barrier of a main loop: a ring deeper than two stages never has more than one tile in
// flight, and the drain takes the previous iteration's output stores with it (rowpanel.hip measured 4.2 us per chunk instead of ~1.3).
// Hidden in asm, only the counted wait (nr_wait_vmcnt) + barrier of the caller's loop order the DMA against the fragment reads
// (cdna_hip_programming.md 5.7).  M0 (the LDS destination) is written in the same statement that reads it and declared clobbered, so
// nothing is saved or restored per transfer.  hipcc keeps no value in M0 across the statement; all the clobber draws is -Winline-asm
// ("clobber list contains reserved registers"), once per instantiation = several hundred per build, which is why that one diagnostic
// is switched off around this one definition and nowhere else.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
__device__ __forceinline__ void nr_glds16(const void* src, unsigned lds_wave_base) {
  asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" : : "v"(src), "s"(lds_wave_base) : "memory", "m0");
}
#pragma clang diagnostic pop

// The same transfer with M0 saved and restored inside the statement (two more SALU instructions, no clobber): the form rowpanel.hip was
// measured and shipped with; whether it may take the clobbering form is a question for a measured change.
__device__ __forceinline__ void nr_glds16_keep_m0(const void* src, unsigned lds_wave_base) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(src), "s"(lds_wave_base) : "memory");
}

// s_waitcnt vmcnt(N): at most N vector-memory operations of this wave still in flight.  The counter is six bits wide on gfx950, so a
// ring that asks for N > 63 gets the only wait that is still correct, vmcnt(0).
template <int N> __device__ __forceinline__ void nr_wait_vmcnt() {
  static_assert(N >= 0, "a count of operations");
  if constexpr (N <= 63) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
  else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// ----------------------------------------------------------------------------------------------
// Lane-row reductions
// ----------------------------------------------------------------------------------------------

// Own and partner value across the 16-lane rows of a wave on the VALU: v_permlane16_swap exchanges the odd rows of its first operand
// with the even rows of its second, v_permlane32_swap the upper half of the first with the lower half of the second; with both
// operands = v every lane gets {own, partner} in the two results (lane ^ 16 / lane ^ 32), where __shfl_xor is a ds_bpermute round
// trip through the LDS -- four to eight of them per row tile sat on the latency chain of the attention phases.  max / + are
// commutative: bit-identical to the shuffle form.
__device__ __forceinline__ float nr_xmax16(float v) {
  auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
}
__device__ __forceinline__ float nr_xmax32(float v) {
  auto a = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
}
__device__ __forceinline__ float nr_xsum16(float v) {
  auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(a[0]) + __uint_as_float(a[1]);
}
__device__ __forceinline__ float nr_xsum32(float v) {
  auto a = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(a[0]) + __uint_as_float(a[1]);
}
// max / sum over the four 16-lane rows of a wave (lanes l, l^16, l^32, l^48)
__device__ __forceinline__ float nr_rows_max(float v) { return nr_xmax32(nr_xmax16(v)); }
__device__ __forceinline__ float nr_rows_sum(float v) { return nr_xsum32(nr_xsum16(v)); }

// ----------------------------------------------------------------------------------------------
// MFMA operands and asm MFMAs
// ----------------------------------------------------------------------------------------------

// four fp32 accumulators -> the bf16x4 operand of v_mfma_f32_16x16x16_bf16
__device__ __forceinline__ s16x4 nr_pack4(const f32x4& v) {
  bf16x4 b;
#pragma unroll
  for (int e = 0; e < 4; ++e) b[e] = (bf16)v[e];
  return __builtin_bit_cast(s16x4, b);
}

// eight values (float[8] or a bf16x8 fragment: whatever converts to float) -> eight OCP e4m3 codes (v_cvt_pk_fp8_f32: e4m3fn on gfx950,
// round to nearest even, saturating), element e in byte e: the 64-bit operand of the fp8 MFMAs, or two dwords of a packed weight
template <class V> __device__ __forceinline__ unsigned long long nr_e4m3x8(const V& v) {
  int lo = 0, hi = 0;
  lo = __builtin_amdgcn_cvt_pk_fp8_f32((float)v[0], (float)v[1], lo, false);
  lo = __builtin_amdgcn_cvt_pk_fp8_f32((float)v[2], (float)v[3], lo, true);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32((float)v[4], (float)v[5], hi, false);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32((float)v[6], (float)v[7], hi, true);
  return ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo;
}

// acc += A B (16 x 16 x 32 bf16) with the accumulator PINNED in the AGPR half of the register file ("+a": vDst = SrcC = an AGPR quad):
// the out tiles of xattn.hip and tattn.hip.  Left to hipcc the 160 accumulator registers of the out tile live in VGPRs between the heads
// and every group of MFMAs is bracketed by v_accvgpr copies (xattn: 478 copies for 200 MFMAs, the o stage at 37 instead of 16 cycles per
// MFMA, tools/xattn_timeline.py; tattn: 584 copies per head iteration for 272 MFMAs).  Both files are compiled with
// -amdgpu-mfma-vgpr-form so their short-lived accumulators stay in VGPRs.  An asm MFMA is invisible to the compiler's hazard bookkeeping;
// each call site says why no VALU-written operand sits directly in front of it and where the wait states behind the last one are.
__device__ __forceinline__ void nr_mfma_acc_agpr(f32x4& acc, const bf16x8& a, const bf16x8& b) {
  asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(acc) : "v"(a), "v"(b));
}

// acc += A B (16 x 16 x 16 bf16) with the accumulator TIED (vDst = SrcC), as attention.hip's mfma_bf16_tied.  Left to hipcc 7.2 the
// accumulation chains of xattnw.hip and of tattnw.hip's 32-frame epilogue are allocated as v[28:31] <- v[30:33] style chains (destination
// PARTIALLY overlapping the SrcC the previous MFMA wrote) with no wait states between the dependent MFMAs: wrong sums on gfx950
// (tools/check_mfma_overlap.py scans the shipped ISA for that pattern).  The asm carries its own hazard cover: the leading s_nop 1 is
// for a VALU-written operand (packed q / P tiles, a zeroed accumulator) directly in front of it; nr_mfma_results, or the caller's own
// s_nop run, puts the wait states of MFMA result -> VALU read behind the chain.
// Two forms, and they are not interchangeable: xattnw.hip was written with a plain asm (ordered by its operands alone), tattnw.hip with a
// volatile one (it keeps its place among the kernel's other volatile statements; an empty-asm pin between the steps of the interleaved
// K Q^T chains did not cure the overlap there).  Giving either kernel the other's form changes its schedule and register allocation
// (tools/isa_equal.sh), so each keeps the one it was measured with.
__device__ __forceinline__ void nr_mfma16_tied(f32x4& acc, const s16x4& a, const s16x4& b) {
  asm("s_nop 1\n\tv_mfma_f32_16x16x16_bf16 %0, %1, %2, %0" : "+v"(acc) : "v"(a), "v"(b));
}
__device__ __forceinline__ void nr_mfma16_tied_ordered(f32x4& acc, const s16x4& a, const s16x4& b) {
  asm volatile("s_nop 1\n\tv_mfma_f32_16x16x16_bf16 %0, %1, %2, %0" : "+v"(acc) : "v"(a), "v"(b));
}
__device__ __forceinline__ void nr_mfma_results(f32x4& acc) { asm volatile("s_nop 7\n\ts_nop 7" : "+v"(acc)); }

// ----------------------------------------------------------------------------------------------
// Epilogue and index helpers
// ----------------------------------------------------------------------------------------------

// XCD-aware remap of blockIdx.x over gridDim.x (bijective): workgroups are dealt round-robin over the 8 XCDs, so give each XCD a
// CONTIGUOUS range of logical ids: the workgroups that share an operand (the n-tiles of one A row-panel, the query blocks of one head)
// then hit the same L2 instead of re-fetching it from HBM once per XCD.  Placement only affects speed.  Each caller says what its
// neighbouring ids share.
__device__ __forceinline__ int nr_xcd_bid() {
  const int nwg = gridDim.x, orig = blockIdx.x;
  const int q = nwg >> 3, r = nwg & 7, xcd = orig & 7, local = orig >> 3;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + local;
}

// a / d for d > 0 through the float reciprocal with one correction step: exact for 0 <= a < 2^24 and a quotient < 2^22.  The tile-index
// and im2col-row arithmetic of the igemm prologue used ~10 integer (two of them 64-bit) divisions = 2,300-3,100 of the 4,400-4,900
// cycles between kernel entry and the first LDS-DMA (in-kernel stamps, profiles/r03_igemm_timeline_smallm.txt): per WORKGROUP, i.e.
// once per tile.
__device__ __forceinline__ int nr_fdiv_small(int a, int d) {
  int q = (int)((float)a * __builtin_amdgcn_rcpf((float)d));
  const int r = a - q * d;
  q += (r >= d ? 1 : 0) - (r < 0 ? 1 : 0);
  return q;
}

// element offset of row m's fp32 row-vector term (NrGemmParams::rowvec)
__device__ __forceinline__ size_t nr_rowvec_row(const NrGemmParams& p, int m) {
  int r = m / p.rowvec_div;
  if (p.rowvec_mod) r %= p.rowvec_mod;
  return (size_t)r * p.rowvec_ld;
}

// GEGLU: value * gelu(gate), the gate through gelu_erf_fast of common.h (the epilogues are VALU-bound)
__device__ __forceinline__ float nr_geglu(float v, float g) { return v * gelu_erf_fast(g); }

}  // namespace

// ----------------------------------------------------------------------------------------------
// Stamps: the diagnostic build only (make stamp -> libneurons_amd_stamp.so, read by tools/*_timeline.py).  Shader-clock stamps go to a
// buffer of the kernel file's own; no output value depends on them.  A kernel file declares its buffer with NR_STAMP_BUF(name, rows, slots)
// and defines its put-macros in terms of the three below; in the product build all of them are empty.
//   NR_STAMP_PUT(buf, slot)      thread 0 of workgroup b < rows: buf[b][slot] = s_memtime (slots >= the buffer's are dropped)
//   NR_STAMP_PUT_RT(buf, slot)   the same with s_memrealtime, the chip-wide 100 MHz counter (s_memtime counters are not synchronised
//                                across the chip): entry spread / kernel span over all workgroups
//   NR_STAMP_PUT_AT(cond, buf, row, slot)   the general form: who stamps and into which row is the caller's
// ----------------------------------------------------------------------------------------------
#ifdef NR_STAMP
#define NR_STAMP_BUF(name, rows, slots) __device__ unsigned long long name[rows][slots]
#define NR_STAMP_ROWS(buf) ((int)(sizeof(buf) / sizeof(buf[0])))
#define NR_STAMP_SLOTS(buf) ((int)(sizeof(buf[0]) / sizeof(buf[0][0])))
#define NR_STAMP_PUT_AT(cond, buf, row, slot) do { if (cond) buf[(row)][(slot)] = __builtin_amdgcn_s_memtime(); } while (0)
#define NR_STAMP_PUT(buf, slot) NR_STAMP_PUT_AT(threadIdx.x == 0 && blockIdx.x < NR_STAMP_ROWS(buf) && (slot) < NR_STAMP_SLOTS(buf), buf, blockIdx.x, slot)
#define NR_STAMP_PUT_RT(buf, slot) do { if (threadIdx.x == 0 && blockIdx.x < NR_STAMP_ROWS(buf)) buf[blockIdx.x][(slot)] = __builtin_amdgcn_s_memrealtime(); } while (0)

// host side of every nr_*_stamp_read: copy up to `bytes` of the buffer to dst (if non-null), then zero the buffer if `clear`
template <class Buf> static int nr_stamp_read_buf(const Buf& buf, void* dst, size_t bytes, int clear) {
  const size_t n = bytes < sizeof(Buf) ? bytes : sizeof(Buf);
  int rc = 0;
  if (dst) rc = (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(buf), n, 0, hipMemcpyDeviceToHost);
  if (clear) { void* d = nullptr; (void)hipGetSymbolAddress(&d, HIP_SYMBOL(buf)); (void)hipMemset(d, 0, sizeof(Buf)); }
  return rc;
}
#else
#define NR_STAMP_BUF(name, rows, slots) static_assert(true, "")
#define NR_STAMP_PUT_AT(cond, buf, row, slot) do { } while (0)
#define NR_STAMP_PUT(buf, slot) do { } while (0)
#define NR_STAMP_PUT_RT(buf, slot) do { } while (0)
#endif
