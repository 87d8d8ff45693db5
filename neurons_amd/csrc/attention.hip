// Flash-style softmax(scale * Q K^T) V on bf16 MFMA for every attention on the denoiser path:
//   spatial self-attention  (L = h*w tokens per frame-image, heads 8, d = C/8 in {40,80,160})
//   text cross-attention    (Lk = 77 keys shared by all frames of a clip)
//   temporal self-attention (L = F frames per pixel; the "(b f) d c -> (b d) f c" regroup of
//                            animatediff/models/motion_module.py:274-278,327 is done purely by the
//                            q/k/v/out strides below - nothing is transposed in memory)
// and for the wide heads (d = 256 / 512) of the VAE's mid-block AttnBlock.
// Reference arithmetic: diffusers-0.11.1 CrossAttention._attention, vendored at
// animatediff/models/motion_module_new.py:258-287 (baddbmm(alpha=scale) -> softmax -> bmm) with the
// head split of :181-193.  The score matrix is never materialised; softmax statistics are fp32.
//
// Common to every kernel: a wave owns 16 queries of one (batch, head).  The scores are computed TRANSPOSED,
// S^T = K Q^T (keys on MFMA rows, queries on lanes), so a lane's accumulator registers are the
// probabilities of ITS query for 8 keys - exactly the B-operand fragment the second product
// O^T = V^T P^T needs (k-slot permutation applied identically to both operands), i.e. P never leaves
// registers.  V tiles are staged row-major in LDS and read transposed (read_vt).
//
// The file: the list of instantiated widths, the LDS layouts (read by the kernels and by nr_attn_route), the per-wave kernel
// (attn_fwd_kernel: wave-private V tiles, causal mask), the block-shared kernel template (attn_fwd_shared_kernel over a traits type:
// the narrow heads d <= 160 with their fp8 / ones-column / K48 forms, and the wide heads), the launcher, the route and the entry point.
// The base offsets, the Q-fragment load and the output epilogue are spelled out in both kernels: moved into shared functions they
// change the register allocation of the shipped kernels (tools/isa_equal.sh), so they stay statements.
#include "launchers.h"
#include "device_prims.h"

namespace {

// every (DK, DT) = (ceil(d / 32) k-steps of K Q^T, ceil(d / 16) row tiles of O^T) the narrow kernels are instantiated for, and the wide
// heads: the route refuses and the launcher dispatches by this one list.  On the product path: d = 40, 64, 80, 160 and 512; the rest
// serve reduced-width tests.
#define NR_ATTN_NARROW(X) X(1, 1) X(1, 2) X(2, 3) X(2, 4) X(3, 5) X(3, 6) X(4, 8) X(5, 10)
#define NR_ATTN_WIDE_HEADS(X) X(8, 16) X(16, 32)
#define NR_ATTN_IS(DK, DT) if (dk == DK && dt == DT) return true;
constexpr bool attn_narrow_instantiated(int dk, int dt) { NR_ATTN_NARROW(NR_ATTN_IS) return false; }
constexpr bool attn_wide_instantiated(int dk, int dt) { NR_ATTN_WIDE_HEADS(NR_ATTN_IS) return false; }
#undef NR_ATTN_IS

// ------------------------------------------------------------------------------------------------
// LDS layouts (elements of bf16), one per kernel class
// ------------------------------------------------------------------------------------------------
constexpr size_t CU_LDS_BYTES = 160 * 1024;

// V rows of a tile [keys][16 DT]: a stride = 16 (mod 32) elements, so the 8 rows a half-wave touches in one ds_read_b64_tr_b16 start 8 banks
// apart (conflict-free transpose reads)
__host__ __device__ constexpr int v_row_stride(int DT) { return (DT * 16) % 32 == 16 ? DT * 16 : DT * 16 + 16; }

// per-wave kernel: four wave-private V tiles of 32 keys
struct WaveLds {
  static constexpr int KT = 32;          // keys per iteration
  int vs;
  size_t lds_bytes;
  __host__ __device__ constexpr WaveLds(int DT) : vs(v_row_stride(DT)), lds_bytes((size_t)4 * KT * vs * sizeof(bf16)) {}
};

// block-shared kernel: two buffers, each the K image then the V image of one tile of kt keys.  K (d <= 64): [kt][64], 128-byte rows with the
// 16-byte chunk index XOR-swizzled by (key & 7): the b128 fragment reads (lane = key 16t + c, chunk 4ks + g) are conflict-free, the layout
// gemm.hip uses for its operand tiles; larger heads keep padded rows of 32 DK + 8 elements (an odd number of 16-byte units).
struct BlockLds {
  int kt;
  bool kswz;
  int ksk, ksv, tilek, tile2;            // row strides, elements of the K image and of one buffer
  size_t lds_bytes;
  __host__ __device__ constexpr BlockLds(int kt_, int DK, int DT)
      : kt(kt_), kswz(DK <= 2), ksk(kswz ? 64 : DK * 32 + 8), ksv(v_row_stride(DT)), tilek(kt * ksk), tile2(kt * (ksk + ksv)),
        lds_bytes((size_t)2 * tile2 * sizeof(bf16)) {}
};
constexpr int KT_NARROW = 64, KT_WIDE = 32;      // keys per tile of the two families of the block-shared kernel

// ------------------------------------------------------------------------------------------------
// Shared steps
// ------------------------------------------------------------------------------------------------

// The A fragment of O^T += V^T P^T from a row-major V tile: two ds_read_b64_tr_b16, each handing the lane V[4 keys][its dv column], for the
// keys at a0 and 16 rows further on (k-slot j of the MFMA -> key j < 4 ? 4g + j : 16 + 4g + j - 4, as the P fragment has them).
// a0 = tile + (4 g + tq) * stride + 16 i + 4 tp with tq = c >> 2, tp = c & 3: the transpose-read role inside the 16-lane group.
// EXEC must be all ones at these reads: every lane runs them (queries >= Lq are clamped and not stored; keys >= Lk are clamped or zero rows
// whose probability is 0), none sits under a per-lane condition.
__device__ __forceinline__ bf16x8 read_vt(const bf16* a0, int stride) {
  const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)a0);
  const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)(a0 + 16 * stride));
  bf16x8 vf;
#pragma unroll
  for (int e = 0; e < 4; ++e) { vf[e] = lo[e]; vf[4 + e] = hi[e]; }
  return vf;
}

// OCP e4m3 operands of the fp8 form: 8 values (a bf16x8 fragment or 8 fp32) -> one 64-bit MFMA operand
template <class V> __device__ __forceinline__ long to_fp8x8(const V& v) { return (long)nr_e4m3x8(v); }

// acc += A B with the accumulator TIED (vDst = SrcC).  In the ONES instantiation hipcc 7.2 otherwise allocates the third accumulator as a
// v[2:5] -> v[0:3] -> v[2:5] chain (destination partially overlapping the SrcC the previous MFMA wrote) with no wait states between the
// dependent MFMAs, and the kernel returns wrong sums on gfx950 (tools/check_mfma_overlap.py scans the shipped ISA for that pattern).
// The compiler keeps no hazard bookkeeping for an MFMA it cannot see, so the asm carries its own:
//  * VALU write -> MFMA read of that register needs wait states (measured: a v_cvt_pk_bf16_f32 of the P operand directly in front of the
//    MFMA, with only an already-satisfied s_waitcnt between them, gave NaN; one wait state cures it): the leading s_nop 1 gives two,
//    the figure LLVM uses for its own MFMAs;
//  * MFMA result -> VALU / LDS read: the accumulators are next touched by the rescale (after the next tile's barrier and its eight K Q^T
//    MFMAs) or after the loop's final barrier -- far beyond the 18 wait states of an 8-pass MFMA.
__device__ __forceinline__ void mfma_bf16_tied(f32x4& acc, const bf16x8& a, const bf16x8& b) {
  asm("s_nop 1\n\tv_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(acc) : "v"(a), "v"(b));
}

// ------------------------------------------------------------------------------------------------
// Per-wave kernel (short, strided or causal sequences): one wave = 16 queries with its own V tile of 32 keys in LDS; K fragments come
// straight from global memory.  Row max / row sum are two xor-shuffles across the 4 lane groups.
// DK = ceil(d/32) k-steps for QK^T;  DT = ceil(d/16) row tiles of O^T
// ------------------------------------------------------------------------------------------------
template <int DK, int DT>
__global__ __launch_bounds__(256) void attn_fwd_kernel(NrAttnParams p) {
  extern __shared__ __attribute__((aligned(16))) bf16 vt_all[];
  constexpr WaveLds L(DT);
  static_assert(L.lds_bytes <= CU_LDS_BYTES, "the four tiles fit a CU's LDS");
  constexpr int KT = WaveLds::KT, VS = L.vs;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  bf16* vt = vt_all + (size_t)wave * KT * VS;             // this wave's private V tile, row-major [key][dim]
  const int c = lane & 15, g = lane >> 4;
  const int tq = c >> 2, tp = c & 3;                      // read_vt

  const int qtiles = (p.Lq + 15) >> 4;
  const long long total = (long long)p.nbatch * p.heads * qtiles;
  long long wid = (long long)blockIdx.x * 4 + wave;
  const bool active = wid < total;
  if (!active) wid = total - 1;   // keep the wave in step with the block barriers; results discarded
  const int qt = (int)(wid % qtiles);
  const int h = (int)((wid / qtiles) % p.heads);
  const int nb = (int)(wid / ((long long)qtiles * p.heads));
  const int nbkv = nb / p.kv_div;

  const long long qbase = (long long)(nb / p.inner) * p.q_outer + (long long)(nb % p.inner) * p.q_inner_stride + (long long)h * p.d;
  const long long obase = (long long)(nb / p.inner) * p.o_outer + (long long)(nb % p.inner) * p.o_inner_stride + (long long)h * p.d;
  const long long kbase = (long long)(nbkv / p.kv_inner) * p.kv_outer + (long long)(nbkv % p.kv_inner) * p.kv_inner_stride + (long long)h * p.d;

  const bf16x8 zero8 = bf16x8_zero();
  const int qrow = qt * 16 + c;
  const int qrow_c = min(qrow, p.Lq - 1);
  const int klim = p.causal ? min(p.Lk, qrow + 1) : p.Lk;   // keys visible to this lane's query

  // Q fragments (B operand of S^T = K Q^T): lane holds Q[query c][dim 32*ks + 8*g .. +7]
  bf16x8 qf[DK];
#pragma unroll
  for (int ks = 0; ks < DK; ++ks) {
    const int dim0 = ks * 32 + g * 8;
    qf[ks] = dim0 < p.d ? *(const bf16x8*)(p.q + qbase + (long long)qrow_c * p.q_seq + dim0) : zero8;
  }

  f32x4 acc[DT];
#pragma unroll
  for (int i = 0; i < DT; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_i = -1e30f, l_i = 0.f;

  const int chunks_per_key = p.d >> 3;
  const int vchunks = KT * chunks_per_key;
  // the tile is wave-private and a wave's LDS operations execute in order, so no workgroup barrier is needed around it; the pad
  // columns [d, 16 DT) are cleared once (they only feed output rows that are never stored, but must be finite)
  for (int id = lane; id < KT * (VS >> 3); id += 64) *(bf16x8*)(vt + id * 8) = zero8;

  for (int k0 = 0; k0 < p.Lk; k0 += KT) {
    // ---- stage the V tile row-major with 16-byte stores: vt[key - k0][dim]; the MFMA A operand (V^T) is read transposed ----
    __builtin_amdgcn_wave_barrier();
    for (int id = lane; id < vchunks; id += 64) {
      const int kk = id / chunks_per_key;
      const int x0 = (id - kk * chunks_per_key) << 3;
      const int key = k0 + kk;
      bf16x8 vv = zero8;
      if (key < p.Lk) vv = *(const bf16x8*)(p.v + kbase + (long long)key * p.kv_seq + x0);
      *(bf16x8*)(vt + kk * VS + x0) = vv;
    }

    // ---- S^T = K Q^T for two 16-key tiles ----
    f32x4 s[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      s[t] = f32x4{0.f, 0.f, 0.f, 0.f};
      const int key = k0 + 16 * t + c;
      const int keyc = min(key, p.Lk - 1);
      const bf16* kp = p.k + kbase + (long long)keyc * p.kv_seq;
#pragma unroll
      for (int ks = 0; ks < DK; ++ks) {
        const int dim0 = ks * 32 + g * 8;
        const bf16x8 kf = dim0 < p.d ? *(const bf16x8*)(kp + dim0) : zero8;
        s[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[ks], s[t], 0, 0, 0);
      }
    }
    // s[t][r]: key = k0 + 16t + 4g + r, query = c
    float mx = -1e30f;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = k0 + 16 * t + 4 * g + r;
        const float v = key < klim ? s[t][r] * p.scale : -1e30f;
        s[t][r] = v;
        mx = fmaxf(mx, v);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(m_i, mx);
    const float alpha = __expf(m_i - m_new);
    float rs = 0.f;
    bf16x8 pf;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = k0 + 16 * t + 4 * g + r;
        const float e = key < klim ? __expf(s[t][r] - m_new) : 0.f;
        rs += e;
        pf[t * 4 + r] = (bf16)e;
      }
    rs += __shfl_xor(rs, 16, 64);
    rs += __shfl_xor(rs, 32, 64);
    l_i = l_i * alpha + rs;
    m_i = m_new;
#pragma unroll
    for (int i = 0; i < DT; ++i) acc[i] *= alpha;

    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();   // the wave's own stores are ordered before its transposed reads
    // ---- O^T += V^T P^T : A = V^T rows dv = 16*i + c ----
#pragma unroll
    for (int i = 0; i < DT; ++i)
      acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(read_vt(vt + (4 * g + tq) * VS + 16 * i + 4 * tp, VS), pf, acc[i], 0, 0, 0);
  }

  // ---- epilogue: acc[i][r] = O[query c][dv = 16i + 4g + r] ----
  if (active && qrow < p.Lq) {
    const float inv = 1.0f / l_i;
    bf16* op = p.out + obase + (long long)qrow * p.o_seq;
#pragma unroll
    for (int i = 0; i < DT; ++i) {
      const int dv0 = i * 16 + 4 * g;
      if (dv0 < p.d) {
        bf16x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (bf16)(acc[i][e] * inv);
        nr_store8(op + dv0, o);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Block-shared kernel: a 256-thread workgroup = 4 waves = 64 queries of one (batch, head); K and V tiles are staged ONCE per workgroup
// into LDS (row-major, 16-byte loads -> ds_write_b128, register-prefetched one tile ahead, two LDS buffers, one barrier per tile).  K rows
// are the A operand of S^T = K Q^T (ds_read_b128, conflict-free by BlockLds); V is consumed through read_vt.  Softmax in the log2 domain
// with a lazy running maximum.  One template over a traits type, two families:
//
// NarrowHead<DK, DT, FP8, ONES>: long sequences of the heads d <= 160 (spatial self-attention, text cross-attention), 64-key tiles, the
// head dim padded to 32 DK / 16 DT: every pad column of the K / V images is zero in both buffers (whole images cleared once, the staging
// only writes the d data columns), so the fragment reads need no head-dim predicate (a predicated 16-byte LDS read costs an exec-mask
// branch each); Q loads and output stores keep theirs.
//   FP8: both products on v_mfma_f32_16x16x32_fp8_fp8 with OCP e4m3 operands converted in registers (Q, K, V from their bf16 tiles; P
//     straight from its fp32 exponentials, scaled by 256 so the probabilities use the e4m3 normal range, and the sum divided back in fp32;
//     the exact running maximum, LAZY = 0, keeps P <= 1); softmax statistics and accumulators stay fp32.  The non-scaled fp8 MFMA issues
//     at the bf16 rate (MI355X_MICROARCH.md), so this form is about the numerics of config 5, not about speed.
//   K48 (d = 40 / 48 in bf16): the second k-step of K Q^T covers dims 32..47 only, so it runs on v_mfma_f32_16x16x16_bf16 (K = 16: half the
//     matrix-pipe cycles of the 32-deep form, whose upper 16 dims would multiply zeros): lane group g supplies dims 32 + 4g .. 32 + 4g + 3.
//   ONES (d = 40 in its 48-wide V image only): pad column d of the V image holds 1.0 for every key, so row d of O^T = V^T P^T IS the
//     softmax denominator: the sum of the probabilities exactly as the matrix pipe sees them (bf16 / e4m3, fp32 accumulation), rescaled
//     with the accumulator for free.  It replaces 17 dependent v_add_f32 per key tile in a loop whose bound is the vector issue port
//     (DESIGN 3e).
//
// WideHead<D>, D = 256 / 512: the VAE's mid-block AttnBlock (one head of d = C = 512, sgm/modules/diffusionmodules/model.py:161-201) and any
// self- / cross-attention with heads * d = C at those widths; not served: causal, fp8, inner != 1 (nr_attn_route).  32-key tiles:
// 2 x 32 x (D + 8 + D + 16) x 2 B = 131 KiB at D = 512 -> one workgroup per CU, one wave per SIMD, so the O tile of a wave (D / 16
// accumulator quads = 128 registers at D = 512) and the Q fragments (64) fit the 512-entry register file.  The head dim is EXACT: no pad
// columns, nothing to clear, no head-dim predicates, inner == 1 addressing, the chunks of a tile dealt evenly to the 256 threads.  The
// denominator is summed in fp32 from the ROUNDED bf16 probabilities: what the second product multiplies.
//
// FORM names what is the same computation written two ways: each family keeps the statements it was measured and shipped with, because
// the other family's spelling changes its schedule or register allocation (tools/isa_equal.sh).  The narrow family names the next tile
// by its first key, multiplies row offsets by the 64-bit kv_seq, computes the log2 scale inside the key loop, starts its score accumulators
// from a register-held zero and addresses the output by dv0; the wide family names the tile by its index, multiplies by a 32-bit kv_seq,
// hoists the scale, zeroes in place and adds the two output offsets in turn.
// ------------------------------------------------------------------------------------------------
enum AttnForm { FORM_NARROW, FORM_WIDE };

template <int DK_, int DT_, bool FP8_ = false, bool ONES_ = false>
struct NarrowHead {
  static_assert(!ONES_ || (DK_ == 2 && DT_ == 3), "the ones column lives in the pad of the 48-wide image of d = 40");
  static constexpr int DK = DK_, DT = DT_, KT = KT_NARROW;
  static constexpr bool EXACT = false, FP8 = FP8_, ONES = ONES_, K48 = !FP8_ && DK_ == 2 && DT_ == 3;
  static constexpr bool SUM_ROUNDED = false;      // the denominator (without ONES) sums the fp32 exponentials
  static constexpr int LAZY = FP8_ ? 0 : 8;
  static constexpr AttnForm FORM = FORM_NARROW;
};
template <int D>
struct WideHead {
  static_assert(D % 64 == 0, "whole 32-wide k-steps, 16-byte chunks dealt evenly to 256 threads");
  static constexpr int DK = D / 32, DT = D / 16, KT = KT_WIDE;
  static constexpr bool EXACT = true, FP8 = false, ONES = false, K48 = false;
  static constexpr bool SUM_ROUNDED = true;
  static constexpr int LAZY = 8;
  static constexpr AttnForm FORM = FORM_WIDE;
};

template <class T>
__global__ __launch_bounds__(256) void attn_fwd_shared_kernel(NrAttnParams p) {
  constexpr int DK = T::DK, DT = T::DT, KT = T::KT;
  constexpr int NT = KT / 16, NU = KT / 32;   // 16-key score quads and 32-key steps of P V per tile
  constexpr bool FP8 = T::FP8, ONES = T::ONES, K48 = T::K48, EXACT = T::EXACT, WIDE_FORM = T::FORM == FORM_WIDE;
  static_assert(!FP8 || NU == 2, "the e4m3 P operands are packed for two 32-key steps");
  constexpr BlockLds L(KT, DK, DT);
  static_assert(L.lds_bytes <= CU_LDS_BYTES, "the two buffers fit a CU's LDS");
  constexpr bool KSWZ = L.kswz;
  constexpr int KSK = L.ksk, KSV = L.ksv, TILEK = L.tilek, TILE2 = L.tile2;
  constexpr int CH = (KT * DT + 127) / 128;   // 16-B chunks per thread per matrix per tile
  extern __shared__ __attribute__((aligned(16))) bf16 lds[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int d = EXACT ? 16 * DT : p.d;
  const int qblocks = (p.Lq + 63) >> 6;
  // (image, head, query-block) ids: the 16 query blocks of a head, and the heads that share its 128-byte lines of the fused q|k|v rows,
  // read their K / V through one L2
  const int bid = nr_xcd_bid();
  const int qb = bid % qblocks;
  const int h = (bid / qblocks) % p.heads;
  const int nb = bid / (qblocks * p.heads);
  const int nbkv = nb / p.kv_div;
  long long qbase, obase;
  if constexpr (EXACT) {                       // inner == 1 (nr_attn_route)
    qbase = (long long)nb * p.q_outer + (long long)h * d;
    obase = (long long)nb * p.o_outer + (long long)h * d;
  } else {
    qbase = (long long)(nb / p.inner) * p.q_outer + (long long)(nb % p.inner) * p.q_inner_stride + (long long)h * d;
    obase = (long long)(nb / p.inner) * p.o_outer + (long long)(nb % p.inner) * p.o_inner_stride + (long long)h * d;
  }
  const long long kbase = (long long)(nbkv / p.kv_inner) * p.kv_outer + (long long)(nbkv % p.kv_inner) * p.kv_inner_stride + (long long)h * d;

  const int qrow = qb * 64 + wave * 16 + c;
  const int qrow_c = min(qrow, p.Lq - 1);
  // Q fragments (B operand of S^T = K Q^T): lane holds Q[query c][dim 32 ks + 8 g .. + 7]
  bf16x8 qf[DK];
#pragma unroll
  for (int ks = 0; ks < DK; ++ks) {
    if constexpr (EXACT) qf[ks] = *(const bf16x8*)(p.q + qbase + (long long)qrow_c * p.q_seq + ks * 32 + g * 8);
    else {
      const int dim0 = ks * 32 + g * 8;
      qf[ks] = dim0 < d ? *(const bf16x8*)(p.q + qbase + (long long)qrow_c * p.q_seq + dim0) : bf16x8_zero();
    }
  }
  s16x4 qf4 = {0, 0, 0, 0};
  if constexpr (K48) {
    const int dim0 = 32 + 4 * g;
    if (dim0 < d) qf4 = *(const s16x4*)(p.q + qbase + (long long)qrow_c * p.q_seq + dim0);
  }
  long qf8[DK];
  if constexpr (FP8) {
#pragma unroll
    for (int ks = 0; ks < DK; ++ks) qf8[ks] = to_fp8x8(qf[ks]);
  }

  // ---- K / V staging: each thread owns CH fixed (key-in-tile, 16-byte chunk) slots, so its K / V source pointers just advance by one
  // tile per iteration: workgroup-uniform bases (scalar registers) + 32-bit lane offsets, two VGPRs per slot instead of two 64-bit
  // pointers.  Only the last, partial tile clamps the key; the clamped rows are finite data that the softmax masks out (probability
  // exactly 0), so they are harmless.  EXACT: no slot clamp and no store predicate ----
  const int cpk = d >> 3;                     // chunks per key row
  const int nchunk = KT * cpk;
  bf16x8 rk[CH], rv[CH];
  int s_kk[CH];
  int s_off[CH];                              // element offset of the slot inside one (batch, head) K / V sequence (fits 32 bits)
  int s_lok[CH], s_lov[CH];                   // LDS element offsets of the slot in the K / V image
#pragma unroll
  for (int i = 0; i < CH; ++i) {
    const int id = EXACT ? tid + 256 * i : min(tid + 256 * i, nchunk - 1);
    const int kk = id / cpk, x0 = (id - kk * cpk) << 3;
    s_kk[i] = kk;
    s_lok[i] = KSWZ ? kk * KSK + ((((x0 >> 3) ^ (kk & 7))) << 3) : kk * KSK + x0;
    s_lov[i] = kk * KSV + x0;
    if constexpr (WIDE_FORM) s_off[i] = kk * (int)p.kv_seq + x0;
    else s_off[i] = kk * p.kv_seq + x0;
  }
  const bf16* kb = p.k + kbase;
  const bf16* vb = p.v + kbase;
  const long long tile_step = (long long)KT * p.kv_seq;
  auto load_regs = [&](int a) {                // a tile into the registers.  a: FORM_NARROW its first key, FORM_WIDE its index
    const bf16* kt = kb + (long long)(WIDE_FORM ? a : a / KT) * tile_step;
    const bf16* vtp = vb + (long long)(WIDE_FORM ? a : a / KT) * tile_step;
    const int k0 = WIDE_FORM ? a * KT : a;
    if (k0 + KT <= p.Lk) {
#pragma unroll
      for (int i = 0; i < CH; ++i) {
        rk[i] = *(const bf16x8*)(kt + s_off[i]);
        rv[i] = *(const bf16x8*)(vtp + s_off[i]);
      }
    } else {
#pragma unroll
      for (int i = 0; i < CH; ++i) {
        const int back = WIDE_FORM ? max(k0 + s_kk[i] - (p.Lk - 1), 0) * (int)p.kv_seq : max(k0 + s_kk[i] - (p.Lk - 1), 0) * p.kv_seq;
        rk[i] = *(const bf16x8*)(kt + (s_off[i] - back));
        rv[i] = *(const bf16x8*)(vtp + (s_off[i] - back));
      }
    }
  };
  auto write_lds = [&](int buf) {
    bf16* sk = lds + buf * TILE2;
    bf16* sv = sk + TILEK;
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      if constexpr (EXACT) {
        *(bf16x8*)(sk + s_lok[i]) = rk[i];
        *(bf16x8*)(sv + s_lov[i]) = rv[i];
      } else if (tid + 256 * i < nchunk) {
        *(bf16x8*)(sk + s_lok[i]) = rk[i];
        *(bf16x8*)(sv + s_lov[i]) = rv[i];
      }
    }
  };

  f32x4 acc[DT];
#pragma unroll
  for (int i = 0; i < DT; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_i = -1e30f, l_i = 0.f;

  if constexpr (!EXACT) {                      // the pad columns (see NarrowHead)
    for (int id = tid; id < 2 * TILE2 / 8; id += 256) *(bf16x8*)(lds + id * 8) = bf16x8_zero();
    __syncthreads();
  }
  if constexpr (ONES) {                        // column d of both V images (the staging never touches pad columns)
    if (tid < 2 * KT) lds[(tid / KT) * TILE2 + TILEK + (tid % KT) * KSV + d] = (bf16)1.0f;
  }
  const int ntile = (p.Lk + KT - 1) / KT;
  load_regs(0);
  write_lds(0);
  __syncthreads();
  // FORM_NARROW: a zero accumulator the compiler cannot rematerialise: it stays in 4 registers instead of 16 v_mov per key tile
  f32x4 zacc = f32x4{0.f, 0.f, 0.f, 0.f};
  if constexpr (!WIDE_FORM) asm volatile("" : "+v"(zacc));
  const int tq = c >> 2, tp = c & 3;          // read_vt
  // softmax in the log2 domain: exp(scale*s - m) = exp2(fma(s, scale*log2(e), -m2)): one fma + one v_exp per score
  const float sl2_hoisted = p.scale * 1.4426950408889634f;
  for (int it = 0; it < ntile; ++it) {
    const int k0 = it * KT;
    if (it + 1 < ntile) load_regs(WIDE_FORM ? it + 1 : k0 + KT);
    const bf16* sk = lds + (it & 1) * TILE2;
    const bf16* sv = sk + TILEK;
    // ---- S^T = K Q^T for NT 16-key tiles: s[t][r] = score of key k0 + 16 t + 4 g + r and query c ----
    f32x4 s[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      s[t] = zacc;
#pragma unroll
      for (int ks = 0; ks < DK; ++ks) {
        if constexpr (K48) {
          if (ks == 1) {       // dims 32 + 4g ..: 8 bytes of chunk 4 + (g >> 1) of the swizzled K row (pad dims >= d are zero in the image)
            const s16x4 kf4 = *(const s16x4*)(sk + (16 * t + c) * KSK + ((((4 + (g >> 1)) ^ (c & 7)) << 3) + ((g & 1) << 2)));
            s[t] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(kf4, qf4, s[t], 0, 0, 0);
            continue;
          }
        }
        const bf16x8 kf = KSWZ ? *(const bf16x8*)(sk + (16 * t + c) * KSK + (((ks * 4 + g) ^ (c & 7)) << 3))
                               : *(const bf16x8*)(sk + (16 * t + c) * KSK + ks * 32 + g * 8);
        if constexpr (FP8) s[t] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(to_fp8x8(kf), qf8[ks], s[t], 0, 0, 0);
        else s[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[ks], s[t], 0, 0, 0);
      }
    }
    const float sl2 = WIDE_FORM ? sl2_hoisted : p.scale * 1.4426950408889634f;
    // ---- the maximum of this lane's 4 NT raw scores.  Full tiles (every key valid) skip the key-mask selects (2 NT v_max3_f32);
    // otherwise keys >= Lk score -1e30 from here on ----
    const bool full = k0 + KT <= p.Lk;
    float mx = -1e30f;
    if (full) {
#pragma unroll
      for (int t = 0; t < NT; ++t) mx = fmaxf(fmaxf(fmaxf(fmaxf(mx, s[t][0]), s[t][1]), s[t][2]), s[t][3]);
    } else {
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = k0 + 16 * t + 4 * g + r;
          const float v = key < p.Lk ? s[t][r] : -1e30f;
          s[t][r] = v;
          mx = fmaxf(mx, v);
        }
    }
    // ---- Lazy running maximum: the reference maximum of a query only moves when the tile's maximum exceeds it by more than 2^LAZY, so
    // with LAZY = 8 the probabilities stay <= 256 (exact in the fp32 sums, in range for bf16) and the accumulator rescale, which costs a
    // register round trip of the whole O tile, runs on the first tile and then almost never (wave-uniform skip).
    // The cross-lane maximum (two permlane swaps + selects: ~16 issue slots of a loop bound by its issue port) is only needed when the
    // reference moves.  If NO lane's own scores exceed its query's reference by the margin, no query's tile maximum does (it is the
    // maximum over that query's four lanes), so m_new = m_i for every lane exactly as the full computation would find: skip it ----
    constexpr float LAZY = (float)T::LAZY;
    mx *= sl2;                                 // sl2 > 0: the max of this lane's scaled scores
    float m_new = m_i;
    if (__builtin_amdgcn_ballot_w64(mx > m_i + LAZY) != 0ull) {
      mx = nr_rows_max(mx);
      m_new = mx > m_i + LAZY ? mx : m_i;
      // l_i stays a per-lane partial sum (this lane's keys of every tile); the four rows are added once after the loop
      const float alpha = __builtin_amdgcn_exp2f(m_i - m_new);      // 1 for the queries whose reference stays
      if constexpr (!ONES) l_i *= alpha;
#pragma unroll
      for (int i = 0; i < DT; ++i) acc[i] *= alpha;
      m_i = m_new;
    }
    float rs = 0.f;
    bf16x8 pf[NU];
    float pe[NU][8];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float e = __builtin_amdgcn_exp2f(__builtin_fmaf(s[t][r], sl2, -m_new));   // masked keys: exp2(-huge) = 0
        if constexpr (T::SUM_ROUNDED) {
          const bf16 pb = (bf16)e;
          rs += (float)pb;
          pf[t >> 1][(t & 1) * 4 + r] = pb;
        } else {
          if constexpr (!ONES) rs += e;
          if constexpr (FP8) pe[t >> 1][(t & 1) * 4 + r] = e * 256.0f;
          else pf[t >> 1][(t & 1) * 4 + r] = (bf16)e;
        }
      }
    long pf8[2];
    if constexpr (FP8) { pf8[0] = to_fp8x8(pe[0]); pf8[1] = to_fp8x8(pe[1]); }
    if constexpr (!ONES) l_i += rs;
    // ---- O^T += V^T P^T : A = V^T rows dv = 16 i + c, step u = keys 32 u .. 32 u + 31 of the tile ----
#pragma unroll
    for (int i = 0; i < DT; ++i) {
#pragma unroll
      for (int u = 0; u < NU; ++u) {
        const bf16x8 vf = read_vt(sv + (32 * u + 4 * g + tq) * KSV + 16 * i + 4 * tp, KSV);
        if constexpr (FP8) acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(to_fp8x8(vf), pf8[u], acc[i], 0, 0, 0);
        else if constexpr (ONES) mfma_bf16_tied(acc[i], vf, pf[u]);
        else acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[u], acc[i], 0, 0, 0);
      }
    }
    if (it + 1 < ntile) write_lds((it + 1) & 1);
    __syncthreads();
  }

  // all lanes active here; acc[i][r] = O[query c][dv = 16 i + 4 g + r].  ONES: dv = 40 = 16 * 2 + 4 * 2 + 0 is element 0 of acc[2] in
  // lane group g = 2 of the query's column c
  float l_all;
  // ONES: the last P.V MFMAs are inline asm (mfma_bf16_tied), so hipcc does not know acc[] is an in-flight MFMA result and inserts no wait
  // states in front of its first reader (the ds_bpermute of the shuffle below).  An 8-pass XDL write needs ~11 issue slots on gfx950; the
  // compiled stream happened to leave ~13 (two branches, a wait, a barrier, four VALU ops): state the distance instead of relying on it.
  if constexpr (ONES) asm volatile("s_nop 7\n\ts_nop 7" ::: "memory");
  if constexpr (ONES) l_all = __shfl(acc[2][0], 32 + c, 64);
  else l_all = nr_rows_sum(l_i);
  if (qrow < p.Lq) {
    const float inv = (FP8 && !ONES ? 1.0f / 256.0f : 1.0f) / l_all;      // ONES + FP8: the 256 of the scaled probabilities is in l_all too
    bf16* op = p.out + obase + (long long)qrow * p.o_seq;
#pragma unroll
    for (int i = 0; i < DT; ++i) {
      const int dv0 = i * 16 + 4 * g;
      if (EXACT || dv0 < d) {
        bf16x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (bf16)(acc[i][e] * inv);
        nr_store8(WIDE_FORM ? op + i * 16 + 4 * g : op + dv0, o);
      }
    }
  }
}

// One launch: the kernel of the routed class and width, opted in (once per device) to its layout's LDS size
template <int DK, int DT>
int launch_attn(const NrAttnParams& p, const NrAttnRoute& r, hipStream_t stream) {
  typedef void (*kern_t)(NrAttnParams);
  static unsigned long long opted[3] = {0, 0, 0};      // per-wave or wide | block-shared | its ones-column form: a bit per device
  kern_t bf, f8;                                       // the class's bf16 and e4m3 kernels
  size_t bytes;
  int m = 0;
  if constexpr (attn_wide_instantiated(DK, DT)) {
    if (r.cls != NR_ATTN_WIDE) return 3;
    bf = f8 = attn_fwd_shared_kernel<WideHead<16 * DT>>;
    bytes = BlockLds(KT_WIDE, DK, DT).lds_bytes;
  } else if (r.cls == NR_ATTN_WAVE) {
    bf = f8 = attn_fwd_kernel<DK, DT>;
    bytes = WaveLds(DT).lds_bytes;
  } else if (r.cls == NR_ATTN_SHARED) {
    bf = attn_fwd_shared_kernel<NarrowHead<DK, DT, false>>, f8 = attn_fwd_shared_kernel<NarrowHead<DK, DT, true>>, m = 1;
    if constexpr (DK == 2 && DT == 3) {
      if (r.ones) bf = attn_fwd_shared_kernel<NarrowHead<DK, DT, false, true>>, f8 = attn_fwd_shared_kernel<NarrowHead<DK, DT, true, true>>, m = 2;
    }
    bytes = BlockLds(KT_NARROW, DK, DT).lds_bytes;
  } else return 3;
  if (r.lds_bytes != bytes) return 3;
  if (const int rc = nr_lds_opt_in(opted[m], {(const void*)bf, (const void*)f8}, bytes)) return rc;
  hipLaunchKernelGGL(r.fp8 ? f8 : bf, dim3(r.grid), dim3(256), r.lds_bytes, stream, p);
  return 0;
}

}  // namespace

extern "C" int nr_attn_route(const NrAttnParams* pp, NrAttnRoute* r) {
  const NrAttnParams& p = *pp;
  const bool wide = p.d % 32 == 0 && attn_wide_instantiated(p.d / 32, p.d / 16);
  if (p.d % 8 != 0 || (p.d > 160 && !wide) || p.d <= 0) return 1;
  if (p.Lq <= 0 || p.Lk <= 0 || p.nbatch <= 0) return 2;
  if (wide) {
    if (p.causal || p.fp8 || p.inner != 1) return 4;      // the wide heads: bf16, unmasked, one sequence per batch entry
    *r = NrAttnRoute{};
    r->cls = NR_ATTN_WIDE; r->dk = p.d / 32; r->dt = p.d / 16;
    r->lds_bytes = BlockLds(KT_WIDE, r->dk, r->dt).lds_bytes;
    r->grid = (unsigned)((long long)p.nbatch * p.heads * ((p.Lq + 63) / 64));
    return 0;
  }
  const int DK = (p.d + 31) / 32, DT = (p.d + 15) / 16;
  if (!attn_narrow_instantiated(DK, DT)) return 3;  // d = 104 .. 112, 136 .. 144
  *r = NrAttnRoute{};
  r->dk = DK; r->dt = DT; r->cls = NR_ATTN_WAVE;
  if (p.Lq >= 48 && p.inner == 1 && !p.causal) {   // long sequences: block-shared K/V tiles; causal masking lives in the per-wave kernel only
    r->cls = NR_ATTN_SHARED; r->fp8 = p.fp8;
    // d = 40: the denominator rides on the pad column of V (NR_ATTN_ROWSUM=adds keeps the VALU sums: A/B only)
    static const bool ones = !(getenv("NR_ATTN_ROWSUM") && getenv("NR_ATTN_ROWSUM")[0] == 'a');
    r->ones = ones && p.d == 40;
    r->lds_bytes = BlockLds(KT_NARROW, DK, DT).lds_bytes;
    r->grid = (unsigned)((long long)p.nbatch * p.heads * ((p.Lq + 63) / 64));
    return 0;
  }
  r->lds_bytes = WaveLds(DT).lds_bytes;
  r->grid = (unsigned)(((long long)p.nbatch * p.heads * ((p.Lq + 15) / 16) + 3) / 4);
  return 0;
}

extern "C" int nr_launch_attention(const NrAttnParams* pp, const NrAttnRoute* r, hipStream_t stream) {
  if (r->dt != (pp->d + 15) / 16) return 3;        // a route nr_attn_route does not make, here and below
#define NR_ATTN_CASE(DK, DT) case DT: return r->dk == DK ? launch_attn<DK, DT>(*pp, *r, stream) : 3;
  switch (r->dt) { NR_ATTN_NARROW(NR_ATTN_CASE) NR_ATTN_WIDE_HEADS(NR_ATTN_CASE) }
#undef NR_ATTN_CASE
  return 3;
}
