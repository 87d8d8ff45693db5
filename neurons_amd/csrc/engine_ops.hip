// Single-op entry points of the C ABI (nr_op_*): test and tool hooks that launch ONE kernel class the way the engine's planner would, on
// tensors in the engine's converted formats.  Host code only.
#include "engine.h"
#include <tuple>

using namespace nre;

// grow-only device scratch of the op hooks (process lifetime).  Growing waits for the device first (the old buffer may still be read) and
// returns true
struct OpScratch { void* ptr = nullptr; size_t cap = 0; };
static bool op_scratch(OpScratch& b, size_t need) {
  if (need <= b.cap) return false;
  if (b.ptr) { HIP_OK(hipDeviceSynchronize()); (void)hipFree(b.ptr); }
  b.ptr = nullptr; b.cap = 0;
  HIP_OK(hipMalloc(&b.ptr, need));
  b.cap = need;
  return true;
}

// One GEMM / conv launch the way the engine's planner would make it: route, pack, launch.  A route that names a packed weight layout (fragment-major
// for smallm.hip, the stage streams of lin160.hip) gets that copy packed on the launch stream into a scratch buffer of its layout on EVERY call
// (tests: always consistent with the tensor passed in); NR_OP_FM_CACHE=1 keeps one copy per (weight pointer, layout, shape) instead (timing tools
// that replay graphs over a pool of weights; nr_op_fm_cache_clear when the pool is freed).  NR_W8=1, read per call like NR_SMALLM, sets the e4m3 weight
// request (NrGemmParams::w8) of every GEMM hook
static std::map<std::tuple<const void*, int, int, int>, bf16*> g_op_fm_cache;
extern "C" void nr_op_fm_cache_clear() {
  (void)hipDeviceSynchronize();
  for (auto& kv : g_op_fm_cache) (void)hipFree(kv.second);
  g_op_fm_cache.clear();
}
static const bf16* op_pack(const NrGemmParams& p, const NrGemmRoute& r, hipStream_t s) {
  if (r.weight_layout == NR_W_ROWMAJOR || r.weight_layout == NR_W_TAP_INNER) return p.w;      // the kernel reads the matrix as the caller holds it
  const size_t need = nr_gemm_packed_bytes(r.weight_layout, p.N, p.K);
  if (!need) throw NrError(NR_ERR_STATE, "op_pack: shape has no packed form");
  if (env_is_1("NR_OP_FM_CACHE")) {
    auto it = g_op_fm_cache.find({p.w, r.weight_layout, p.N, p.K});
    if (it == g_op_fm_cache.end()) {
      bf16* d = nullptr;
      HIP_OK(hipMalloc((void**)&d, need));
      LAUNCH_OK(nr_launch_gemm_w_pack(r.weight_layout, p.w, p.N, p.K, d, s));
      it = g_op_fm_cache.emplace(std::make_tuple(p.w, r.weight_layout, p.N, p.K), d).first;
    }
    return it->second;
  }
  static OpScratch scratch[2];                   // fragment-major copies | stage streams
  OpScratch& b = scratch[(r.weight_layout == NR_W_FRAGMAJOR || r.weight_layout == NR_W_FRAGMAJOR_E4M3) ? 0 : 1];
  op_scratch(b, need);
  LAUNCH_OK(nr_launch_gemm_w_pack(r.weight_layout, p.w, p.N, p.K, (bf16*)b.ptr, s));
  return (const bf16*)b.ptr;
}
static void op_gemm(const NrGemmParams& p_arg, hipStream_t s) {
  NrGemmParams p = p_arg;
  p.w8 = env_is_1("NR_W8") ? 1 : 0;
  NrGemmRoute r;
  LAUNCH_OK(nr_gemm_route(&p, &r));
  const bf16* wk = op_pack(p, r, s);
  static OpScratch ws;
  op_scratch(ws, r.ws_bytes);
  LAUNCH_OK(nr_launch_gemm(&p, &r, wk, r.ws_bytes ? (float*)ws.ptr : nullptr, s));
}

extern "C" nr_status nr_op_gemm(nr_stream stream, const void* a, int32_t lda, const void* w, const float* bias,
                                const void* res, int32_t ldr, void* out, int32_t ldo, int32_t M, int32_t N, int32_t K,
                                int32_t geglu) {
  NR_TRY
  NrGemmParams p = nr_gemm_params((const bf16*)a, K, lda, nullptr, 0, 0, M, 1, 1, 1, 1, 0, (const bf16*)w, N, bias, (const bf16*)res, ldr, (bf16*)out, ldo);
  p.geglu = geglu;
  op_gemm(p, (hipStream_t)stream);
  NR_CATCH
}

// the e4m3 form of a bf16 [N][K] matrix as smallm.hip reads it (NR_W_FRAGMAJOR_E4M3: N K code bytes, then N float row scales) into out_dev
extern "C" nr_status nr_op_w8_pack(nr_stream stream, const void* w_dev, int32_t N, int32_t K, void* out_dev, int64_t capacity) {
  NR_TRY
  if (!w_dev || !out_dev) throw NrError(NR_ERR_ARG, "null argument");
  const size_t need = nr_gemm_packed_bytes(NR_W_FRAGMAJOR_E4M3, N, K);
  if (!need) throw NrError(NR_ERR_ARG, "e4m3 weights: N must be a multiple of 16 and K of 64");
  if (capacity < (int64_t)need) throw NrError(NR_ERR_ARG, "output buffer too small");
  LAUNCH_OK(nr_launch_gemm_w_pack(NR_W_FRAGMAJOR_E4M3, (const bf16*)w_dev, N, K, (bf16*)out_dev, (hipStream_t)stream));
  NR_CATCH
}

// two-source operand [a0 | a1] (the skip concat of unet_blocks.py:634,740 as a 1x1 GEMM; the [t | g] operand of the folded FeedForward)
extern "C" nr_status nr_op_gemm2(nr_stream stream, const void* a0, int32_t c0, int32_t lda0, const void* a1, int32_t c1, int32_t lda1,
                                 const void* w, const float* bias, const void* res, int32_t ldr, void* out, int32_t ldo, int32_t M, int32_t N) {
  NR_TRY
  NrGemmParams p = nr_gemm_params((const bf16*)a0, c0, lda0, (const bf16*)a1, c1, lda1, M, 1, 1, 1, 1, 0, (const bf16*)w, N, bias, (const bf16*)res, ldr,
                                  (bf16*)out, ldo);
  op_gemm(p, (hipStream_t)stream);
  NR_CATCH
}

extern "C" nr_status nr_op_ln_gemm(nr_stream stream, const void* a, int32_t lda, const void* w_scaled, const float* ln_c,
                                   const float* bias_folded, float eps, const void* res, int32_t ldr, void* out, int32_t ldo,
                                   int32_t M, int32_t N, int32_t K, int32_t geglu, int32_t act) {
  NR_TRY
  if (!ln_c) throw NrError(NR_ERR_ARG, "ln_c is required");
  NrGemmParams p = nr_gemm_params((const bf16*)a, K, lda, nullptr, 0, 0, M, 1, 1, 1, 1, 0, (const bf16*)w_scaled, N, bias_folded, (const bf16*)res, ldr,
                                  (bf16*)out, ldo);
  p.geglu = geglu; p.ln_c = ln_c; p.ln_eps = eps; p.act = act;
  op_gemm(p, (hipStream_t)stream);
  NR_CATCH
}

extern "C" nr_status nr_op_gemm_ex(nr_stream stream, const void* a, int32_t lda, const void* w, const float* bias, const float* ln_c,
                                   float ln_eps, const float* rowvec, int32_t rowvec_div, int32_t rowvec_mod, int32_t rowvec_ld,
                                   const void* res, int32_t ldr, void* out, int32_t ldo, int32_t M, int32_t N, int32_t K, int32_t geglu,
                                   int32_t act, float out_scale) {
  NR_TRY
  NrGemmParams p = nr_gemm_params((const bf16*)a, K, lda, nullptr, 0, 0, M, 1, 1, 1, 1, 0, (const bf16*)w, N, bias, (const bf16*)res, ldr, (bf16*)out, ldo);
  p.out_scale = out_scale; p.geglu = geglu; p.act = act;
  p.rowvec = rowvec; p.rowvec_div = rowvec_div > 0 ? rowvec_div : 1; p.rowvec_mod = rowvec_mod; p.rowvec_ld = rowvec_ld;
  p.ln_c = ln_c; p.ln_eps = ln_eps;
  op_gemm(p, (hipStream_t)stream);
  NR_CATCH
}

extern "C" nr_status nr_op_conv3x3(nr_stream stream, const void* x0, int32_t c0, const void* x1, int32_t c1, int32_t nimg,
                                   int32_t H, int32_t W, int32_t stride, int32_t ups, const void* w, const float* bias,
                                   const float* rowvec, int32_t rowvec_div, const void* res, void* out, int32_t Cout) {
  NR_TRY
  NrGemmParams p = nr_gemm_params((const bf16*)x0, c0, c0, (const bf16*)x1, c1, c1, nimg, H, W, 3, stride, ups, (const bf16*)w, Cout, bias, (const bf16*)res,
                                  Cout, (bf16*)out, Cout);
  p.rowvec = rowvec; p.rowvec_div = rowvec_div > 0 ? rowvec_div : 1; p.rowvec_ld = Cout;
  op_gemm(p, (hipStream_t)stream);
  NR_CATCH
}

// the upsample conv in phase form (NrGemmParams::ups == 2) on phase weights; nr_op_conv3x3 with ups = 1 stays the 3x3 route on raw taps
extern "C" nr_status nr_op_conv3x3_ups_phase(nr_stream stream, const void* x, int32_t Cin, int32_t nimg, int32_t H, int32_t W, const void* wp,
                                             const float* bias, void* out, int32_t Cout) {
  NR_TRY
  if (!x || !wp || !out) throw NrError(NR_ERR_ARG, "null argument");
  NrGemmParams p = nr_gemm_params((const bf16*)x, Cin, Cin, nullptr, 0, 0, nimg, H, W, 3, 1, 2, (const bf16*)wp, Cout, bias, nullptr, 0, (bf16*)out, Cout);
  op_gemm(p, (hipStream_t)stream);
  NR_CATCH
}
extern "C" nr_status nr_ups_phase_weights(const float* w_tap, int32_t Cout, int32_t Cin, void* out) {
  NR_TRY
  if (!w_tap || !out || Cout < 1 || Cin < 1) throw NrError(NR_ERR_ARG, "bad argument");
  nr_ups_phase_pack(w_tap, (size_t)9 * Cin, 1, (size_t)Cin, Cout, Cin, (uint16_t*)out);
  NR_CATCH
}

extern "C" nr_status nr_op_condembed_in(nr_stream stream, const float* cond, const float* mask, int32_t c0, int32_t nsrc, int32_t F, int32_t H,
                                        int32_t W, const int32_t* fmap, int32_t nframes, const float* w, const float* bias, int32_t Cout,
                                        void* out) {
  NR_TRY
  if (!fmap) throw NrError(NR_ERR_ARG, "fmap is null");
  LAUNCH_OK(nr_launch_condembed_in(cond, mask, c0, nsrc, F, H, W, fmap, nframes, w, bias, Cout, (bf16*)out, (hipStream_t)stream));
  NR_CATCH
}

extern "C" nr_status nr_op_condembed_conv(nr_stream stream, const void* x, int32_t nimg, int32_t H, int32_t W, int32_t Cin, int32_t stride,
                                          const void* wfm, const float* bias, int32_t Cout, int32_t silu, void* out) {
  NR_TRY
  LAUNCH_OK(nr_launch_condembed_conv((const bf16*)x, nimg, H, W, Cin, stride, (const bf16*)wfm, bias, Cout, silu, (bf16*)out,
                                     (hipStream_t)stream));
  NR_CATCH
}

// as nr_op_conv3x3 (stride 1, no upsample, single source) with the weight in the tap-inner layout [Cout][Cin/64][3][3][64]
extern "C" nr_status nr_op_conv3x3_tap_inner(nr_stream stream, const void* x0, int32_t c0, int32_t nimg, int32_t H, int32_t W, const void* w,
                                             const float* bias, const float* rowvec, int32_t rowvec_div, const void* res, void* out,
                                             int32_t Cout) {
  NR_TRY
  NrGemmParams p = nr_gemm_params((const bf16*)x0, c0, c0, nullptr, 0, 0, nimg, H, W, 3, 1, 0, (const bf16*)w, Cout, bias, (const bf16*)res, Cout, (bf16*)out,
                                  Cout);
  p.tap_inner = 1;
  p.rowvec = rowvec; p.rowvec_div = rowvec_div > 0 ? rowvec_div : 1; p.rowvec_ld = Cout;
  op_gemm(p, (hipStream_t)stream);
  NR_CATCH
}

extern "C" nr_status nr_op_groupnorm(nr_stream stream, const void* x0, int32_t c0, const void* x1, int32_t c1, int32_t nimg,
                                     int32_t hw, int32_t groups, const float* gamma, const float* beta, float eps,
                                     int32_t silu, float* partial_ws, void* out) {
  NR_TRY
  NrGnParams p = nr_gn_params((const bf16*)x0, c0, c0, (const bf16*)x1, c1, c1, nimg, hw, groups, gamma, beta, eps, silu, partial_ws, (bf16*)out,
                              c0 + (x1 ? c1 : 0));
  NrGnRoute r;      // routed per call
  if (const int rc = nr_gn_route(&p, &r)) throw NrError(NR_ERR_UNSUPPORTED, "nr_gn_route -> " + std::to_string(rc) + ": no kernel serves this shape, nr_launch_groupnorm not called");
  LAUNCH_OK(nr_launch_groupnorm(&p, &r, (hipStream_t)stream));
  NR_CATCH
}

extern "C" nr_status nr_op_layernorm(nr_stream stream, const void* x, void* out, int32_t M, int32_t C, const float* gamma,
                                     const float* beta, float eps, const float* pe, int32_t pe_hw, int32_t pe_F) {
  NR_TRY
  LAUNCH_OK(nr_launch_layernorm((const bf16*)x, C, (bf16*)out, C, M, C, gamma, beta, eps, pe, pe_hw > 0 ? pe_hw : 1,
                                pe_F > 0 ? pe_F : 1, (hipStream_t)stream));
  NR_CATCH
}

extern "C" nr_status nr_op_attention(nr_stream stream, int32_t mode, const void* qp, const void* kvp, void* outp,
                                     int32_t nimg, int32_t L, int32_t Lk, int32_t C, int32_t heads, int32_t frames,
                                     int32_t kv_div) {
  NR_TRY
  const int fp8_flag = (mode & 8) ? 1 : 0;      // mode | 8: e4m3 MFMA operands (spatial / cross kernels)
  const int causal_flag = (mode & 16) ? 1 : 0;  // mode | 16: causal mask (mode 0 only; the CLIP text encoder's form)
  mode &= 7;
  if (causal_flag && (mode != 0 || fp8_flag)) throw NrError(NR_ERR_ARG, "causal attention: mode 0 only");
  if (mode > 2) throw NrError(NR_ERR_ARG, "bad attention mode");
  // the hook's tensors are dense: q|k|v rows of 3C (modes 0 / 2), q rows of C and k|v rows of 2C (mode 1), output rows of C
  const NrAttnParams p = nr_attn_params(mode, (const bf16*)qp, (const bf16*)kvp, (bf16*)outp, mode == 1 ? C : 3 * C, 2 * C, C, nimg, L, Lk, C, heads, frames, kv_div,
                                        causal_flag, fp8_flag);
  NrAttnRoute r;      // routed per call
  if (const int rc = nr_attn_route(&p, &r)) throw NrError(NR_ERR_UNSUPPORTED, "nr_attn_route -> " + std::to_string(rc) + ": no kernel serves this shape, nr_launch_attention not called");
  LAUNCH_OK(nr_launch_attention(&p, &r, (hipStream_t)stream));
  NR_CATCH
}

// ---- the five fused transformer kernels (tensors and formats: include/neurons_amd.h).  Each hook packs its streams / tables into process-lifetime scratch, fills the
// kernel's launch description as the engine's emitter does and calls the same launcher.  A NULL weight matrix = reuse what the previous call packed (timing loops) ----
template <class T> static T* op_packed(OpScratch& b, size_t bytes) { op_scratch(b, bytes); return (T*)b.ptr; }

extern "C" nr_status nr_op_ff_fused(nr_stream stream, const void* t_dev, const void* x_dev, void* out_dev, int32_t M, int32_t C, const void* w1_geglu_dev,
                                    const float* gamma_dev, const float* beta_dev, const float* b1_geglu_dev, const void* wc_dev, const float* bc_dev, float ln_eps) {
  NR_TRY
  if (!nr_ff_fused_supported(C, C, C, C)) throw NrError(NR_ERR_UNSUPPORTED, "the fused FeedForward kernel is built for C = 320");
  static OpScratch buf;
  bf16* ws = op_packed<bf16>(buf, nr_ff_stream_bytes(C));
  if (w1_geglu_dev) LAUNCH_OK(nr_launch_ff_stream_pack((const bf16*)w1_geglu_dev, (const bf16*)wc_dev, ws, (hipStream_t)stream));
  const NrFfFusedParams p{.t = (const bf16*)t_dev, .ldt = C, .x = (const bf16*)x_dev, .ldx = C, .out = (bf16*)out_dev, .ldo = C, .M = M, .stream = ws, .gamma = gamma_dev,
                          .beta = beta_dev, .b1 = b1_geglu_dev, .bc = bc_dev, .ln_eps = ln_eps, .norot = env_is_1("NR_DETERMINISTIC_BATCH"), .waves = nr_ff_waves()};
  LAUNCH_OK(nr_launch_ff_fused(&p, (hipStream_t)stream));
  NR_CATCH
}
extern "C" nr_status nr_op_tattn_fused_frames(nr_stream stream, void* t_dev, int32_t nbatch, int32_t frames, int32_t hw, const void* wq_dev, const void* wk_dev,
                                              const void* wv_dev, const void* wo_dev, const float* gamma_dev, const float* gb_dev, const float* bo_dev, float ln_eps) {
  NR_TRY
  if (!nr_tattn_fused_supported(320, 8, frames, hw))
    throw NrError(NR_ERR_UNSUPPORTED, "fused temporal attention: C = 320, 8 heads, 16 or 32 frames, hw % (128 / frames) == 0");
  static OpScratch buf;
  bf16* ws = op_packed<bf16>(buf, nr_tattn_stream_bytes());
  if (wq_dev) LAUNCH_OK(nr_launch_tattn_stream_pack((const bf16*)wq_dev, (const bf16*)wk_dev, (const bf16*)wv_dev, (const bf16*)wo_dev, ws, (hipStream_t)stream));
  const NrTattnFusedParams p{.t = (bf16*)t_dev, .nbatch = nbatch, .frames = frames, .hw = hw, .stream = ws, .gamma = gamma_dev, .gb = gb_dev, .bo = bo_dev, .ln_eps = ln_eps,
                             .norot = env_is_1("NR_DETERMINISTIC_BATCH")};
  LAUNCH_OK(nr_launch_tattn_fused(&p, (hipStream_t)stream));
  NR_CATCH
}
extern "C" nr_status nr_op_xattn_fused(nr_stream stream, void* t_dev, int32_t nimg, int32_t hw, int32_t img_per_ctx, const void* wq_dev, const void* wo_dev,
                                       const void* kv_dev, int32_t ldkv, int32_t Lk, int32_t nctx, const float* gamma_dev, const float* beta_dev, const float* bo_dev,
                                       float ln_eps) {
  NR_TRY
  if (!t_dev || !kv_dev || !gamma_dev || !beta_dev || !bo_dev) throw NrError(NR_ERR_ARG, "null argument");
  if (!nr_xattn_fused_supported(320, 8, Lk, hw) || nimg <= 0 || img_per_ctx <= 0 || nctx <= 0 || (nimg + img_per_ctx - 1) / img_per_ctx > nctx)
    throw NrError(NR_ERR_UNSUPPORTED, "fused cross attention: C = 320, 8 heads, Lk <= 80, hw % 128 == 0, one context per img_per_ctx images");
  static OpScratch wbuf, kvbuf;
  bf16* ws = op_packed<bf16>(wbuf, nr_xattn_wstream_bytes());
  bf16* kvs = op_packed<bf16>(kvbuf, nr_xattn_kvstream_bytes(nctx));
  if (wq_dev) {
    LAUNCH_OK(nr_launch_xattn_w_pack((const bf16*)wq_dev, (const bf16*)wo_dev, ws, (hipStream_t)stream));
    LAUNCH_OK(nr_launch_xattn_kv_pack((const bf16*)kv_dev, ldkv, Lk, nctx, kvs, (hipStream_t)stream));
  }
  const NrXattnFusedParams p{.t = (bf16*)t_dev, .nimg = nimg, .hw = hw, .img_per_ctx = img_per_ctx, .nctx = nctx, .Lk = Lk, .wstream = ws, .kvstream = kvs, .gamma = gamma_dev,
                             .beta = beta_dev, .bo = bo_dev, .ln_eps = ln_eps, .norot = env_is_1("NR_DETERMINISTIC_BATCH")};
  LAUNCH_OK(nr_launch_xattn_fused(&p, (hipStream_t)stream));
  NR_CATCH
}
extern "C" nr_status nr_op_xattn_head(nr_stream stream, const void* t_dev, void* a_dev, int32_t nimg, int32_t hw, int32_t img_per_ctx, int32_t C,
                                      const void* wq_folded_dev, const float* lnc_dev, const float* bias_dev, const void* kv_dev, int32_t ldkv, int32_t Lk,
                                      int32_t nctx, float ln_eps) {
  NR_TRY
  if (!t_dev || !a_dev || !kv_dev) throw NrError(NR_ERR_ARG, "null argument");
  if (!nr_xattnw_supported(C, 8, Lk, hw) || nimg <= 0 || nctx <= 0 || img_per_ctx <= 0 || (nimg + img_per_ctx - 1) / img_per_ctx > nctx)
    throw NrError(NR_ERR_UNSUPPORTED, "cross-attention head kernel: C = 640 or 1280, 8 heads, Lk <= 80, hw % 64 == 0, one context per img_per_ctx images");
  static std::map<int, OpScratch> wbuf, tbuf;
  static OpScratch kvbuf;
  bf16* ws = op_packed<bf16>(wbuf[C], nr_xattnw_wstream_bytes(C));
  float* tbl = op_packed<float>(tbuf[C], nr_xattnw_table_bytes(C));
  const size_t need = nr_xattnw_kvstream_bytes(C, nctx);
  if (op_scratch(kvbuf, need)) HIP_OK(hipMemset(kvbuf.ptr, 0, need));
  bf16* kvs = (bf16*)kvbuf.ptr;
  if (wq_folded_dev) {
    if (!lnc_dev || !bias_dev) throw NrError(NR_ERR_ARG, "null argument");
    LAUNCH_OK(nr_launch_xattnw_w_pack((const bf16*)wq_folded_dev, C, ws, (hipStream_t)stream));
    LAUNCH_OK(nr_launch_xattnw_table_pack(lnc_dev, bias_dev, C, tbl, (hipStream_t)stream));
    LAUNCH_OK(nr_launch_xattnw_kv_pack((const bf16*)kv_dev, ldkv, Lk, nctx, C, kvs, (hipStream_t)stream));
  }
  const NrXattnHeadParams p{.t = (const bf16*)t_dev, .out = (bf16*)a_dev, .nimg = nimg, .hw = hw, .img_per_ctx = img_per_ctx, .nctx = nctx, .Lk = Lk, .C = C, .wstream = ws,
                            .kvstream = kvs, .table = tbl, .ln_eps = ln_eps};
  LAUNCH_OK(nr_launch_xattnw(&p, (hipStream_t)stream));
  NR_CATCH
}
// the table is packed for one frame count, so w_folded == NULL reuses the packing of the same frame count only
extern "C" nr_status nr_op_tattn_head_frames(nr_stream stream, const void* t_dev, void* a_dev, int32_t nbatch, int32_t frames, int32_t hw, int32_t C,
                                             const void* w_folded_dev, const float* lnc_dev, const float* bias_dev, const float* rowvec_dev, float ln_eps) {
  NR_TRY
  if (!t_dev || !a_dev || !lnc_dev || !bias_dev || !rowvec_dev) throw NrError(NR_ERR_ARG, "null argument");
  if (!nr_tattnw_supported(C, 8, frames, hw) || nbatch <= 0)
    throw NrError(NR_ERR_UNSUPPORTED, "temporal attention head kernel: C = 640 (hw % 8 == 0) or 1280 (hw % 4 == 0), 8 heads, 16 or 32 frames");
  static std::map<int, OpScratch> wbuf;
  static std::map<std::pair<int, int>, OpScratch> tbuf;
  static std::map<int, int> wbuf_frames;      // the frame count of the last packing call at this C
  bf16* w = op_packed<bf16>(wbuf[C], nr_tattnw_stream_bytes(C));
  float* tb = op_packed<float>(tbuf[{C, frames}], nr_tattnw_table_bytes(C, frames));
  if (w_folded_dev) {
    LAUNCH_OK(nr_launch_tattnw_stream_pack((const bf16*)w_folded_dev, C, w, (hipStream_t)stream));
    LAUNCH_OK(nr_launch_tattnw_table_pack(lnc_dev, bias_dev, rowvec_dev, C, frames, tb, (hipStream_t)stream));
    wbuf_frames[C] = frames;
  } else if (wbuf_frames[C] != frames) {
    throw NrError(NR_ERR_ARG, "temporal attention head kernel: w_folded == NULL needs a previous call at this C and frame count");
  }
  const NrTattnHeadParams p{.t = (const bf16*)t_dev, .out = (bf16*)a_dev, .nbatch = nbatch, .frames = frames, .hw = hw, .C = C, .stream = w, .table = tb, .ln_eps = ln_eps};
  LAUNCH_OK(nr_launch_tattnw(&p, (hipStream_t)stream));
  NR_CATCH
}
extern "C" nr_status nr_op_tattn_head(nr_stream stream, const void* t_dev, void* a_dev, int32_t nbatch, int32_t hw, int32_t C, const void* w_folded_dev,
                                      const float* lnc_dev, const float* bias_dev, const float* rowvec_dev, float ln_eps) {
  return nr_op_tattn_head_frames(stream, t_dev, a_dev, nbatch, 16, hw, C, w_folded_dev, lnc_dev, bias_dev, rowvec_dev, ln_eps);
}
extern "C" nr_status nr_op_tattn_fused(nr_stream stream, void* t_dev, int32_t nbatch, int32_t hw, const void* wq_dev, const void* wk_dev, const void* wv_dev,
                                       const void* wo_dev, const float* gamma_dev, const float* gb_dev, const float* bo_dev, float ln_eps) {
  return nr_op_tattn_fused_frames(stream, t_dev, nbatch, 16, hw, wq_dev, wk_dev, wv_dev, wo_dev, gamma_dev, gb_dev, bo_dev, ln_eps);
}
