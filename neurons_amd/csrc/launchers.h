// The one declaration of every launcher, eligibility rule and size function that crosses a translation unit of this library.  Included by the file that defines a
// function and by every file that calls it, so the compiler checks each definition against the prototype its callers see (the names are extern "C": a mismatch would
// otherwise link cleanly).  A long launch description is a struct of common.h, filled by field name (GEMM, GroupNorm, attention, the five fused transformer kernels).
#pragma once
#include "common.h"
#include "gemm_route.h"

// norm.hip, attention.hip: as nr_gemm_route, nr_gn_route / nr_attn_route decide once, are the only readers of their kernels' switches and return nonzero for a shape
// no kernel serves.  The route of one GroupNorm: the register-resident slab kernel (gs groups per workgroup, nv 16-byte chunks per thread), the fused small-image
// kernel (<= maxp channel pairs per thread) or the chunked stats [+ finalize] + apply passes; its kernel count and the floats `partial` must hold
enum NrGnKind { NR_GN_SLAB, NR_GN_SMALL, NR_GN_CHUNKED };
struct NrGnRoute { int kind, gs, nv, threads, maxp, pix_per_blk, nchunk, finalized, lds_stats, lds_apply, launches, ws_floats; };
// attention.hip: K/V tiles per wave (short, strided or causal sequences) or shared by the block (there only: e4m3 operands, the ones column of V at d = 40);
// NR_ATTN_WIDE: the wide heads d = 256 / 512 (bf16, not causal, inner == 1), 64 queries per workgroup on 32-key tiles
enum NrAttnClass { NR_ATTN_WAVE, NR_ATTN_SHARED, NR_ATTN_WIDE };
struct NrAttnRoute { int cls, dk, dt, fp8, ones; unsigned grid; size_t lds_bytes; };      // dk / dt: 32- / 16-wide tiles of the head dim
extern "C" {
// gemm.hip: the route of a GEMM / conv launch (gemm_route.h) and the tiled implicit GEMM (1x1 / 3x3) with its split-K scratch.
// nr_gemm_route orders the kernel classes (smallm, lin160, row-panel, gemm8p, tiled) and is the only reader of their switches; it returns nonzero
// for a shape no kernel serves.  nr_gemm_route_rowmajor: for a W that is no converted weight matrix (an activation as the W operand) or an epilogue
// set at launch -- only the classes that read `w` as the caller holds it.  nr_launch_gemm launches what the route says: `packed_w` in
// route->weight_layout (p.w itself for the unpacked layouts), `ws` of route->ws_bytes bytes
int nr_gemm_route(const NrGemmParams* pp, NrGemmRoute* route);
int nr_gemm_route_rowmajor(const NrGemmParams* pp, NrGemmRoute* route);
int nr_launch_gemm(const NrGemmParams* pp, const NrGemmRoute* route, const bf16* packed_w, float* ws, hipStream_t stream);
size_t nr_gemm_packed_bytes(int layout, int N, int K);      // 0: the shape has no such packed form
int nr_launch_gemm_w_pack(int layout, const bf16* w, int N, int K, bf16* dst, hipStream_t stream);
// rowpanel.hip: K = 320 row-panel GEMM
bool rowpanel_plan(const NrGemmParams& p, RowPanelPlan* pl);
int nr_launch_rowpanel(const NrGemmParams* pp, const RowPanelPlan* pl, hipStream_t stream);
// gemm8p.hip: 256-row ping-pong kernel for the big launches (SparseCtrl groups, several clips per call, 32-frame clips, the VAE)
bool g8p_plan(const NrGemmParams& p, G8pPlan* pl);
int nr_launch_g8p(const NrGemmParams* pp, const G8pPlan* pl, int m_fast, hipStream_t stream);
// lin160.hip: short-K Linears (K = 640 / 1280, N % 160 == 0, >= 2048 rows) on fragment-major weights
size_t nr_lin160_stream_bytes(int N, int K);
bool lin160_plan(const NrGemmParams& p, Lin160Plan* pl);
int nr_lin160_panel_rule(int Mp, int N, int K);
size_t nr_lin128q_stream_bytes(int N, int K);
int nr_launch_lin128q_w_pack(const bf16* w, int N, int K, bf16* stream, hipStream_t s);
int nr_launch_lin160_w_pack(const bf16* w, int N, int K, bf16* stream, hipStream_t s);
int nr_launch_lin160(const NrGemmParams* pp, const Lin160Plan* pl, const bf16* stream, hipStream_t s);
int nr_gn_route(const NrGnParams* pp, NrGnRoute* route);
int nr_launch_groupnorm(const NrGnParams* pp, const NrGnRoute* route, hipStream_t stream);
int nr_attn_route(const NrAttnParams* pp, NrAttnRoute* route);
int nr_launch_attention(const NrAttnParams* pp, const NrAttnRoute* route, hipStream_t stream);
int nr_launch_layernorm(const bf16* x, int ldx, bf16* out, int ldo, int M, int C, const float* gamma, const float* beta,
                        float eps, const float* pe, int pe_hw, int pe_F, hipStream_t stream);
int nr_launch_conv_in_small(const float* s0, const float* s1, int c0, int c1, int src_batch, int nimg, int F, int H, int W,
                            const float* wT, const float* bias, const float* addend, int Cout, bf16* out, float in_scale,
                            float in_shift, hipStream_t stream);
int nr_launch_clip_embed(const int* ids, const float* tok, const float* pos, bf16* out, int M, int L, int C, int vocab,
                         hipStream_t stream);
int nr_launch_bf16_to_f32(const bf16* a, float* out, long long n, hipStream_t stream);
int nr_launch_gaussian_sample(const float* moments, const float* noise, float* out, int n, int zc, int hw, float scale,
                              hipStream_t stream);
int nr_launch_post_quant(const float* z, float scale, const float* Q, const float* qb, float* out, int nimg, int C, int hw,
                         hipStream_t stream);
int nr_launch_softmax_rows(const float* S, bf16* P, int rows, int L, float scale, hipStream_t stream);
int nr_launch_conv_out_small(const bf16* x, int Cin, int nimg, int F, int H, int W, const bf16* w, const float* bias,
                             int Cout, float* out, float out_mul, float out_add, int clamp01, hipStream_t stream);
int nr_launch_timestep_sincos(const float* t, int M, int dim, float* out, hipStream_t stream);
int nr_launch_linear_small(const float* x, int M, int K, const bf16* W, const float* b, int N, int in_act, int out_act,
                           float* y, const float* addend, hipStream_t stream);
int nr_launch_add_bf16(const bf16* a, const bf16* b, bf16* out, long long n, hipStream_t stream);
int nr_launch_f32_to_bf16(const float* a, bf16* out, long long n, hipStream_t stream);
int nr_launch_add_bf16_multi(const NrAddMulti* p, hipStream_t stream);
int nr_launch_frame_gather(const bf16* src, bf16* dst, int B, int Fs, int Fd, long long frame_elems, const int* map, hipStream_t stream);
int nr_launch_ncfhw_to_nhwc(const float* src, bf16* dst, int B, int C, int F, int HW, hipStream_t stream);
int nr_launch_nhwc_to_ncfhw(const bf16* src, float* dst, int B, int C, int F, int HW, hipStream_t stream);
int nr_launch_fold_linear_pair(const float* w2, const float* w1, const float* b2, const float* b1, int C, int J, bf16* wc, float* bc,
                               hipStream_t stream);
// smallm.hip: panel-resident kernel of the M <= 512 Linears (fragment-major weights)
bool smallm_plan(const NrGemmParams& p, SmallmPlan* pl);
int nr_launch_smallm(const NrGemmParams* pp, const SmallmPlan* pl, const bf16* w_fm, int layout, hipStream_t stream);
int nr_launch_smallm_w_pack(const void* w, void* out, int N, int K, hipStream_t stream);
int nr_launch_smallm_w8_pack(const void* w, void* out, int N, int K, hipStream_t stream);      // NR_W_FRAGMAJOR_E4M3: codes, then the row scales
// The five fused transformer kernels: the engine's emitter (engine_layers.hip X_block) and the nr_op_* hook both fill the kernel's struct and nr_launch_X launches it,
// nonzero for a shape the kernel does not serve.  X_supported = the kernel's hard shape constraints (for its launcher and its hook); X_eligible adds its A/B switch
// and its row floor (for the engine's planner; rows: the launch's, one clip's under deterministic batching)
// xattn.hip / tattn.hip: one kernel per cross- / temporal-attention block of the C = 320 level
size_t nr_xattn_wstream_bytes(void);
size_t nr_xattn_kvstream_bytes(int nctx);
int nr_xattn_fused_supported(int C, int heads, int Lk, int hw);
int nr_xattn_fused_eligible(int C, int heads, int Lk, int hw, long long rows);
int nr_launch_xattn_w_pack(const bf16* wq, const bf16* wo, bf16* stream, hipStream_t s);
int nr_launch_xattn_kv_pack(const bf16* kv, int ldkv, int Lk, int nctx, bf16* stream, hipStream_t s);
int nr_launch_xattn_fused(const NrXattnFusedParams* pp, hipStream_t s);
size_t nr_tattn_stream_bytes(void);
int nr_tattn_fused_supported(int C, int heads, int frames, int hw);
int nr_tattn_fused_eligible(int C, int heads, int frames, int hw, long long rows);
int nr_launch_tattn_stream_pack(const bf16* wq, const bf16* wk, const bf16* wv, const bf16* wo, bf16* stream, hipStream_t s);
int nr_launch_tattn_fused(const NrTattnFusedParams* pp, hipStream_t s);
// xattnw.hip: q projection + context attention per (64 rows, 160 columns) above the C = 320 level (C = 640 / 1280, <= 80 text tokens)
size_t nr_xattnw_wstream_bytes(int C);
size_t nr_xattnw_kvstream_bytes(int C, int nctx);
size_t nr_xattnw_table_bytes(int C);
int nr_xattnw_supported(int C, int heads, int Lk, int hw);
int nr_xattnw_eligible(int C, int heads, int Lk, int hw, long long rows);
int nr_launch_xattnw_w_pack(const bf16* w_folded, int C, bf16* stream, hipStream_t s);
int nr_launch_xattnw_table_pack(const float* lnc, const float* bias, int C, float* table, hipStream_t s);
int nr_launch_xattnw_kv_pack(const bf16* kv, int ldkv, int Lk, int nctx, int C, bf16* kvs, hipStream_t s);
int nr_launch_xattnw(const NrXattnHeadParams* pp, hipStream_t s);
// tattnw.hip: q|k|v projection of one head + F x F attention per (pixel group, head) above the C = 320 level (C = 640 / 1280, F = 16 / 32)
size_t nr_tattnw_stream_bytes(int C);
int nr_tattnw_supported(int C, int heads, int frames, int hw);
int nr_tattnw_eligible(int C, int heads, int frames, int hw, long long rows);
int nr_launch_tattnw_stream_pack(const bf16* w_folded, int C, bf16* stream, hipStream_t s);
size_t nr_tattnw_table_bytes(int C, int frames);
int nr_launch_tattnw_table_pack(const float* lnc, const float* bias, const float* rowvec, int C, int frames, float* table, hipStream_t s);
int nr_launch_tattnw(const NrTattnHeadParams* pp, hipStream_t s);
// ffpanel.hip: fused FeedForward(GEGLU) + proj_out of the C = 320 level
size_t nr_ff_stream_bytes(int C);
int nr_ff_fused_supported(int C, int ldt, int ldx, int ldo);
int nr_ff_fused_eligible(int C, long long M);
int nr_ff_waves(void);      // waves per workgroup (8 or 4) of a launch described now: nr_ff_set_waves, else NR_FF_WAVES, else 8
int nr_launch_ff_stream_pack(const bf16* w1, const bf16* wc, bf16* stream, hipStream_t s);
int nr_launch_ff_fused(const NrFfFusedParams* pp, hipStream_t s);
// elementwise.hip condembed_*: SparseCtrl image-condition embedding (first conv from the fp32 planes, small-channel MFMA convs, batch / frame broadcast)
int nr_condembed_in_supported(int cin, int Cout);
int nr_launch_condembed_in(const float* cond, const float* mask, int c0, int nsrc, int F, int H, int W, const int* fmap, int Fe,
                           const float* wT, const float* bias, int Cout, bf16* out, hipStream_t s);
int nr_condembed_conv_supported(int Cin, int stride, int Cout);
long long nr_condembed_wfm_elems(int Cin, int Cout);
int nr_launch_condembed_conv(const bf16* x, int nimg, int H, int W, int Cin, int stride, const bf16* wfm, const float* bias, int Cout,
                             int silu, bf16* out, hipStream_t s);
int nr_launch_condembed_bcast(const bf16* emb, int cb, int Fe, const int* emap, int B, int F, long long img_elems, const bf16* add,
                              bf16* out, hipStream_t s);
}
