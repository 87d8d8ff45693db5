// Plan emitters of the engine (engine.h): the arena and plan helpers, one emitter per kernel class (conv / linear, GroupNorm, LayerNorm, attention, each
// fused transformer kernel) and the builders of the reference modules on top of them, through temporal_module.  The plan follows the reference module graph:
//   ResnetBlock3D                       animatediff/models/resnet.py:182-212
//   Transformer3DModel / BasicTransformerBlock   animatediff/models/attention.py:95-142,256-300
//   TemporalTransformer3DModel / Block / VersatileAttention   animatediff/models/motion_module.py:134-158,210-222,270-329
// Host code only.
#include "engine.h"

using namespace nre;

size_t Arena::alloc(size_t bytes) {
  bytes = align(bytes);
  for (size_t i = 0; i < free_.size(); ++i) {
    if (free_[i].size >= bytes) {
      const size_t off = free_[i].off;
      if (free_[i].size == bytes) free_.erase(free_.begin() + i);
      else { free_[i].off += bytes; free_[i].size -= bytes; }
      return off;
    }
  }
  const size_t off = top;
  top += bytes;
  if (top > high) high = top;
  return off;
}
void Arena::release(size_t off, size_t bytes) {
  bytes = align(bytes);
  size_t i = 0;
  while (i < free_.size() && free_[i].off < off) ++i;
  free_.insert(free_.begin() + i, Blk{off, bytes});
  if (i + 1 < free_.size() && free_[i].off + free_[i].size == free_[i + 1].off) {
    free_[i].size += free_[i + 1].size;
    free_.erase(free_.begin() + i + 1);
  }
  if (i > 0 && free_[i - 1].off + free_[i - 1].size == free_[i].off) {
    free_[i - 1].size += free_[i].size;
    free_.erase(free_.begin() + i);
  }
  if (!free_.empty() && free_.back().off + free_.back().size == top) {
    top = free_.back().off;
    free_.pop_back();
  }
}

// ------------------------------------------------------------------ plan helpers
Act nr_net::act_in(Arena& ar, size_t base, bool keep, int nimg, int h, int w, int C) {
  Act a;
  const size_t bytes = (size_t)nimg * h * w * C * sizeof(bf16);
  auto b = std::make_shared<Buf>();
  b->arena = &ar; b->bytes = bytes; b->off = ar.alloc(bytes); b->keep = keep;
  a.buf = b; a.ptr = at<bf16>(base + b->off); a.nimg = nimg; a.H = h; a.W = w; a.C = C; a.ld = C;
  return a;
}
std::shared_ptr<Buf> nr_net::new_tmp(size_t bytes) {
  auto b = std::make_shared<Buf>();
  b->arena = &arena; b->bytes = bytes; b->off = arena.alloc(bytes); b->keep = keep_all;
  return b;
}
nr_net::SplitK nr_net::splitk_scratch(size_t bytes) {
  SplitK k;
  if (bytes) { k.buf = new_tmp(bytes); k.ws = at<float>(k.buf->off); }
  return k;
}
void nr_net::emit(std::function<void(hipStream_t)> fn, int kind, double flops, double bytes, const std::string& desc) {
  if (dry) return;
  if (building_ctx) { ctx_ops.push_back(std::move(fn)); return; }
  ops.push_back(std::move(fn));
  op_meta.push_back(OpMeta{kind, flops, bytes, desc});
}
// named by plan position and kernel class
void nr_net::op_tap(const char* kind, const Act& a) {
  static const bool on = getenv("NR_OP_TAPS") != nullptr;
  if (on && !dry && keep_all && !building_ctx) taps.push_back(Tap{"op" + std::to_string(ops.size()) + "." + kind, a.ptr, a.rows(), a.C, a.ld});
}
void nr_net::begin_plan() {
  ctx_persist.clear(); ops.clear(); ctx_ops.clear(); op_meta.clear(); taps.clear(); arena.reset(); parena.reset();
  ctx_dirty = true;
  { const char* e = getenv("NR_UPS_PHASE"); ups_phase_mode = (e && e[0]) ? (e[0] != '0' ? 1 : 0) : -1; }      // per plan, never per process: two handles may differ
  temb_slots.clear(); temb_total = 0; temb_all = nullptr;
  n_res = 0; res_shapes.clear();
  t_dev = new_scratch<float>(NR_MAX_BATCH);
}
Act nr_net::stage_context() {
  Act ctx_bf = new_act_persistent(1, 1, B2 * ctx_len, cfg.cross_attention_dim);
  bf16* cp = ctx_bf.ptr; const long long n = (long long)B2 * ctx_len * cfg.cross_attention_dim;
  building_ctx = true;
  emit([this, cp, n](hipStream_t s) { LAUNCH_OK(nr_launch_f32_to_bf16(io.ctx, cp, n, s)); });
  building_ctx = false;
  ctx_persist.push_back(ctx_bf);
  return ctx_bf;
}
Act nr_net::context_kv(const Act& ctx_bf, const std::string& b, int C, size_t stream_bytes, const std::function<void(const bf16*, int, bf16*, hipStream_t)>& pack) {
  building_ctx = true;
  Act kv = new_act_persistent(ctx_bf.nimg, ctx_bf.H, ctx_bf.W, 2 * C);
  GemmOpt ok; ok.out = &kv;
  linear(ctx_bf, wts.w_linear_cat({b + ".attn2.to_k.weight", b + ".attn2.to_v.weight"}, C, cfg.cross_attention_dim), 2 * C, ok);
  Act stream;
  if (pack) {
    stream = new_act_persistent(1, 1, 1, (int)(stream_bytes / sizeof(bf16)));
    const bf16* kvp = kv.ptr; bf16* sp = stream.ptr; const int ldkv = kv.ld;
    emit([=](hipStream_t s) { pack(kvp, ldkv, sp, s); });
  }
  building_ctx = false;
  ctx_persist.push_back(kv);
  if (pack) ctx_persist.push_back(stream);
  return pack ? stream : kv;
}

// ------------------------------------------------------------------ emitters
// generic conv / linear.  x1: optional channel-concat second source.
Act nr_net::conv(const Act& x0, const Act* x1, const bf16* w, int Cout, int ksize, int stride, int ups, const GemmOpt& o) {
  int OH, OW;
  nr_conv_out_hw(x0.H, x0.W, ksize, stride, ups, &OH, &OW);
  const int outC = o.geglu ? Cout / 2 : Cout;
  Act out = o.out ? *o.out : new_act(x0.nimg, OH, OW, outC);
  if (out.C != outC || out.rows() != (int64_t)x0.nimg * OH * OW) throw NrError(NR_ERR_STATE, "conv: output shape mismatch");
  if (o.res && (o.res->C != outC || o.res->rows() != out.rows())) throw NrError(NR_ERR_STATE, "conv: residual shape mismatch");
  NrGemmParams p = nr_gemm_params(x0.ptr, x0.C, x0.ld, x1 ? x1->ptr : nullptr, x1 ? x1->C : 0, x1 ? x1->ld : 0, x0.nimg, x0.H, x0.W, ksize, stride, ups,
                                  w, Cout, o.bias, o.res ? o.res->ptr : nullptr, o.res ? o.res->ld : 0, out.ptr, out.ld);
  p.rowvec = o.rowvec; p.rowvec_div = o.rowvec_div; p.rowvec_ld = o.rowvec_ld; p.rowvec_mod = o.rowvec_mod;
  p.out_scale = o.scale; p.geglu = o.geglu; p.pad_tl0 = o.pad_tl0; p.act = o.act; p.ln_c = o.ln_c; p.ln_eps = 1e-5f;
  p.tap_inner = o.tap_inner;
  p.plan_m = det_batch ? (int)det_rows(p.M) : 0;
  p.w8 = (w8 && ksize == 1 && !o.derived_w) ? 1 : 0;      // a request: only a launch smallm.hip takes reads e4m3 weights
  NrGemmRoute r;
  LAUNCH_OK(nr_gemm_route(&p, &r));
  // the weights as the chosen kernel reads them: fragment-major (bf16, or e4m3 codes + row scales on request) for the M <= 512 Linears (smallm.hip), a
  // stage stream for the short-K Linears on >= 2048 rows (lin160.hip)
  const bf16* wk = dry ? reinterpret_cast<const bf16*>(uintptr_t(16)) : wts.w_layout(w, Cout, p.K, r.weight_layout);
  const double in_elems = (double)x0.rows() * (p.c0 + p.c1);   // every input element is needed at least once
  const double w_elems = (double)p.N * p.K * (ups == 2 ? 4 : 1);   // phase form: one [N][K] matrix per phase
  const double bytes = 2.0 * (in_elems + w_elems + (double)p.M * outC + (o.res ? (double)p.M * outC : 0.0));
  const bool l160 = r.cls == NR_GEMM_LIN160;
  const std::string d = l160 ? descf("%s M=%d N=%d K=%d res=%d geglu=%d ln=%d", r.lin160.form == 4 ? "lin160 panel" : "lin160", p.M, p.N, p.K, o.res ? 1 : 0, p.geglu, p.ln_c ? 1 : 0)
                             : descf("igemm ks=%d s=%d ups=%d M=%d N=%d K=%d geglu=%d res=%d%s", ksize, stride, ups, p.M, p.N, p.K, p.geglu, o.res ? 1 : 0,
                                     r.weight_layout == NR_W_FRAGMAJOR_E4M3 ? " w=e4m3" : "");
  const SplitK sk = splitk_scratch(r.ws_bytes);
  float* ws = sk.ws;
  emit([p, r, wk, ws](hipStream_t s) { LAUNCH_OK(nr_launch_gemm(&p, &r, wk, ws, s)); }, NR_PROF_IGEMM, 2.0 * p.M * (double)p.N * p.K, bytes, d);
  if (ws) last_op_launches(2);           // split-K: the igemm + its reduce kernel
  op_tap(l160 ? "lin160" : (ksize == 3 ? "conv3" : (p.ln_c ? "lngemm" : "gemm")), out);
  return out;
}

// Which upsample convs take the phase form when NR_UPS_PHASE is unset: M output pixels, N = Cout, Cin.  Only shapes whose line gained in every one of three
// interleaved same-box pairs (profiles/ups_phase_ab.txt; per launch in the engine, 3x3 -> phase form):
//   headline (+2.2-2.3 % frames/s)   M = 2048  N = Cin = 1280   75 -> 55 us      M = 8192 N = Cin = 1280   335 -> 112 us      M = 32768 N = Cin = 640   244 -> 118 us
//   VAE round trip (+7.2-7.8 %)      M = 65536 / 262144 N = Cin = 512   0.29 -> 0.14 / 1.15 -> 0.55 ms       M = 1048576 N = Cin = 256   1.24 -> 0.64 ms
// Not admitted: the keyframe model's 32 x 32 level (M = 8192, N = Cin = 640: 70 -> 48 us alone, but its line moved -0.05 / +0.44 / +0.11 %, inside the
// spread) and everything unmeasured (fewer rows than the shapes above)
static bool nr_ups_phase_rule(long long M, int N, int Cin) {
  (void)N;
  return Cin >= 1280 ? M >= 2048 : M >= 32768;
}
Act nr_net::upsample_conv(const Act& x, const std::string& wkey, int Cout, const GemmOpt& o) {
  const int Cin = x.C;
  const long long M = det_rows((long long)x.nimg * x.H * x.W * 4);      // NR_DETERMINISTIC_BATCH: decided on one clip's rows
  // what nr_gemm_route takes as ups = 2: the plain conv (bias only), whole 64-channel k-tiles
  const bool eligible = Cin % 64 == 0 && Cout % 32 == 0 && !o.res && !o.rowvec && !o.geglu && !o.ln_c && !o.tap_inner && !o.pad_tl0;
  const bool phase = eligible && ups_phase_mode != 0 && (ups_phase_mode == 1 || nr_ups_phase_rule(M, Cout, Cin));
  if (phase) return conv(x, nullptr, wts.w_conv3_ups_phase(wkey, Cout, Cin), Cout, 3, 1, 2, o);
  return conv(x, nullptr, wts.w_conv3(wkey, Cout, Cin), Cout, 3, 1, 1, o);
}

// nn.Linear / 1x1 conv `key` (<key>.weight [N][x.C], <key>.bias) on x, + res, into *out
Act nr_net::linear_wb(const Act& x, const std::string& key, int N, const Act* res, Act* out) {
  GemmOpt o; o.bias = wts.w_f32(key + ".bias", N); o.res = res; o.out = out;
  return linear(x, wts.w_linear(key + ".weight", N, x.C), N, o);
}

// plain GEMM on raw pointers (the VAE's attention): out = A[M][K] . W[N][K]^T (+bias) -> bf16 [M][ldo], or raw fp32 [M][N] when out32
void nr_net::gemm_raw(const bf16* a, int lda, const bf16* w, int M, int N, int K, const float* bias, bf16* out, int ldo, float* out32,
                      const char* what) {
  NrGemmParams p = nr_gemm_params(a, K, lda, nullptr, 0, 0, M, 1, 1, 1, 1, 0, w, N, bias, nullptr, 0, out, ldo);
  p.out_f32 = out32;
  p.plan_m = det_batch ? (int)det_rows(M) : 0;
  NrGemmRoute r;                         // W may be an activation (attention scores): only the kernels that read it as it lies
  LAUNCH_OK(nr_gemm_route_rowmajor(&p, &r));
  const SplitK sk = splitk_scratch(r.ws_bytes);
  float* ws = sk.ws;
  emit([p, r, ws](hipStream_t s) { LAUNCH_OK(nr_launch_gemm(&p, &r, p.w, ws, s)); }, NR_PROF_IGEMM, 2.0 * M * (double)N * K,
       2.0 * ((double)M * K + (double)N * K) + (out32 ? 4.0 : 2.0) * (double)M * N, descf("igemm %s M=%d N=%d K=%d", what, M, N, K));
}

Act nr_net::groupnorm(const Act& x0, const Act* x1, const std::string& prefix, float eps, int silu) {
  const int C = x0.C + (x1 ? x1->C : 0);
  const float* gamma = wts.w_f32(prefix + ".weight", C);
  const float* beta = wts.w_f32(prefix + ".bias", C);
  NrGnParams p = nr_gn_params(x0.ptr, x0.C, x0.ld, x1 ? x1->ptr : nullptr, x1 ? x1->C : 0, x1 ? x1->ld : 0, x0.nimg, x0.H * x0.W, cfg.norm_num_groups, gamma, beta,
                              eps, silu, nullptr, nullptr, C);      // scratch and output: sized by the route below
  if (x1) p.c1 = x1->C;      // whatever x1->ptr is in the sizing pass
  p.plan_nimg = det_batch ? (int)det_rows(x0.nimg) : 0;
  NrGnRoute r;
  LAUNCH_OK(nr_gn_route(&p, &r));
  auto ws = new_tmp((size_t)r.ws_floats * sizeof(float));
  Act out = new_act(x0.nimg, x0.H, x0.W, C);
  p.partial = at<float>(ws->off); p.out = out.ptr;
  if (getenv("NR_OP_TAPS") && keep_all && !x1) {     // debug: what the GroupNorm's input looked like when it ran
    Act snap = new_act(x0.nimg, x0.H, x0.W, x0.C);
    const bf16* src = x0.ptr; bf16* dst = snap.ptr; const size_t nb = (size_t)x0.rows() * x0.C * sizeof(bf16);
    if (x0.ld == x0.C) {
      emit([=](hipStream_t s) { launch_copy16(src, dst, nb, s); });
      op_tap("gn_input_snapshot", snap);
    }
  }
  emit([p, r](hipStream_t s) { LAUNCH_OK(nr_launch_groupnorm(&p, &r, s)); }, NR_PROF_GROUPNORM,
       8.0 * (double)x0.rows() * C, 2.0 * 2.0 * (double)x0.rows() * C,
       "groupnorm nimg=" + std::to_string(x0.nimg) + " hw=" + std::to_string(x0.H * x0.W) + " C=" + std::to_string(C));
  last_op_launches(r.launches);
  op_tap("gn", out);
  return out;
}

Act nr_net::layernorm(const Act& x, const std::string& prefix, const float* pe, int pe_F) {
  const float* g = wts.w_f32(prefix + ".weight", x.C);
  const float* b = wts.w_f32(prefix + ".bias", x.C);
  Act out = new_act(x.nimg, x.H, x.W, x.C);
  const bf16* xp = x.ptr; bf16* op = out.ptr;
  const int ldx = x.ld, ldo = out.ld, M = (int)x.rows(), C = x.C, hw = x.H * x.W;
  emit([=](hipStream_t s) { LAUNCH_OK(nr_launch_layernorm(xp, ldx, op, ldo, M, C, g, b, 1e-5f, pe, hw, pe_F, s)); },
       NR_PROF_LAYERNORM, 8.0 * (double)M * C, 2.0 * 2.0 * (double)M * C,
       "layernorm M=" + std::to_string(M) + " C=" + std::to_string(C));
  op_tap("ln", out);
  return out;
}

// mode 0 spatial self (qkv fused [M][3C]); 1 cross (q [M][C], kv [B2*ctx][2C]); 2 temporal self (qkv fused)
Act nr_net::attention(int mode, const Act& q, const Act* kv, int C, int heads, int causal) {
  Act out = new_act(q.nimg, q.H, q.W, C);
  // e4m3 operands: the U-Net's spatial / cross attention only (nr_net_set_attention_fp8 never changed what a VAE handle computes)
  const bool vae = cfg.kind == NR_KIND_VAE_DECODER || cfg.kind == NR_KIND_VAE_ENCODER;
  const NrAttnParams p = nr_attn_params(mode, q.ptr, kv ? kv->ptr : nullptr, out.ptr, q.ld, kv ? kv->ld : 0, out.ld, q.nimg, q.H * q.W, ctx_len, C, heads, F,
                                        F, causal, (attn_fp8 && mode != 2 && !vae) ? 1 : 0);
  NrAttnRoute r;
  LAUNCH_OK(nr_attn_route(&p, &r));
  const double flops = 4.0 * (double)p.nbatch * p.heads * (double)p.Lq * p.Lk * p.d;
  const double kvrows = mode == 1 ? (double)(p.nbatch / p.kv_div) * p.Lk : (double)p.nbatch * p.Lk;
  const double bytes = 2.0 * ((double)p.nbatch * p.Lq * C * 2.0 + kvrows * C * 2.0);   // q + out + k + v
  emit([p, r](hipStream_t s) { LAUNCH_OK(nr_launch_attention(&p, &r, s)); }, NR_PROF_ATTENTION, flops, bytes,
       descf("attention mode=%d nbatch=%d heads=%d d=%d Lq=%d Lk=%d", mode, p.nbatch, p.heads, p.d, p.Lq, p.Lk));
  op_tap(mode == 2 ? "tattn" : (mode == 1 ? "xattn" : "sattn"), out);
  return out;
}

const float* nr_net::temb_for(const std::string& prefix, int C) {
  for (auto& s : temb_slots) if (s.prefix == prefix) {
    if (s.C != C) throw NrError(NR_ERR_STATE, "temb slot size mismatch for " + prefix);
    return temb_all + s.off;
  }
  throw NrError(NR_ERR_STATE, "no temb slot for " + prefix);
}

// ------------------------------------------------------------------ module builders
// parameter names of one residual block: diffusers-style (animatediff) or sgm-style (openaimodel.py:255-312)
nr_net::ResKeys nr_net::res_keys(const std::string& pre) const {
  if (cfg.kind == NR_KIND_SGM_UNET)
    return ResKeys{pre + ".in_layers.0", pre + ".in_layers.2", pre + ".out_layers.0", pre + ".out_layers.3", pre + ".skip_connection"};
  if (cfg.kind == NR_KIND_VAE_DECODER || cfg.kind == NR_KIND_VAE_ENCODER)   // sgm/modules/diffusionmodules/model.py:94-151
    return ResKeys{pre + ".norm1", pre + ".conv1", pre + ".norm2", pre + ".conv2", pre + ".nin_shortcut"};
  return ResKeys{pre + ".norm1", pre + ".conv1", pre + ".norm2", pre + ".conv2", pre + ".conv_shortcut"};
}

// ResnetBlock3D.forward (resnet.py:182-212) == sgm ResBlock._forward (openaimodel.py:328-354, no up/down, no
// scale-shift): GN+SiLU -> conv (+bias +Linear(SiLU(emb))) -> GN+SiLU -> conv (+bias) + skip(x).
// x1 = skip tensor for the decoder concat.
// 3x3 conv weights in the tap-inner K order of the igemm wherever Cin % 64 == 0; NR_CONV_TAP_INNER=0: tap-major
static bool conv_tap_inner() {
  static const bool on = env_not_0("NR_CONV_TAP_INNER");
  return on;
}
Act nr_net::resnet(const Act& x0, const Act* x1, const std::string& pre, int Cout) {
  const ResKeys k = res_keys(pre);
  const int Cin = x0.C + (x1 ? x1->C : 0);
  const int hw = x0.H * x0.W;
  Act h = groupnorm(x0, x1, k.norm1, cfg.norm_eps, 1);
  GemmOpt o1;
  o1.bias = wts.w_f32(k.conv1 + ".bias", Cout);
  if (cfg.kind != NR_KIND_VAE_DECODER && cfg.kind != NR_KIND_VAE_ENCODER) {   // the VAE's ResnetBlock runs with temb = None (model.py:138-139,727)
    o1.rowvec = temb_for(pre, Cout); o1.rowvec_div = F * hw; o1.rowvec_ld = temb_total;
  }
  const bool ti1 = conv_tap_inner() && Cin % 64 == 0, ti2 = conv_tap_inner() && Cout % 64 == 0;
  o1.tap_inner = ti1 ? 1 : 0;
  Act h1 = conv(h, nullptr, wts.w_conv3(k.conv1 + ".weight", Cout, Cin, ti1), Cout, 3, 1, 0, o1);
  h = Act();
  Act h2 = groupnorm(h1, nullptr, k.norm2, cfg.norm_eps, 1);
  h1 = Act();
  Act sc;
  const bool shortcut = wts.has(k.shortcut + ".weight");
  if (shortcut) {
    GemmOpt os; os.bias = wts.w_f32(k.shortcut + ".bias", Cout);
    sc = conv(x0, x1, wts.w_linear(k.shortcut + ".weight", Cout, Cin), Cout, 1, 1, 0, os);
  } else {
    if (x1 || Cin != Cout) throw NrError(NR_ERR_MISSING_WEIGHT, "missing state-dict entry: " + k.shortcut + ".weight");
    sc = x0;
  }
  GemmOpt o2;
  o2.bias = wts.w_f32(k.conv2 + ".bias", Cout);
  o2.res = &sc;
  o2.tap_inner = ti2 ? 1 : 0;
  Act out = conv(h2, nullptr, wts.w_conv3(k.conv2 + ".weight", Cout, Cout, ti2), Cout, 3, 1, 0, o2);
  tap(pre, out);
  return out;
}

// LayerNorm (+ temporal PE) -> Linear as one launch (LN folded into the igemm) or, with NR_NO_LN_FUSE=1, as the
// layernorm kernel followed by a plain igemm (A/B and fallback path; same results to rounding).
// Neach: rows of each stacked matrix (geglu: the inner width, the matrix has 2*Neach rows).
Act nr_net::ln_linear(const Act& x, const std::string& ln, const std::vector<std::string>& wkeys, const std::vector<std::string>& bkeys,
                      int Neach, bool geglu, int act, bool temporal_pe) {
  static const char* mode = getenv("NR_LN_FUSE");            // "0" never, "1" always, unset: per shape
  const int K = x.C;
  const int N = (geglu ? 2 * Neach : Neach) * (int)wkeys.size();
  // Every n-tile block of the fused GEMM recomputes the row statistics (~1-2 us per block round), so the fusion pays
  // when the LayerNorm launch it removes costs more than that: small M (latency-bound LN) or narrow N.  Measured on
  // BASELINE config 2 (profiles/README.md): wide GEMMs at the 32x32 / 16x16 levels are faster with the separate LN.
  const long long M = det_rows(x.rows());
  bool fuse = !((M >= 8192 && N >= 4 * K) || (M >= 32768 && N >= 3 * K));
  // K = 320 on >= 4096 rows runs on the row-panel kernel (rowpanel.hip): the row statistics come from the register panel once
  // per workgroup, so the folded LayerNorm is free there
  static const bool rowpanel_on = env_not_0("NR_ROWPANEL");
  if (rowpanel_on && K == 320 && M >= 4096) fuse = true;
  // K = 640 wide projections (N >= 3 K) on 2048 .. 8192 rows run on the register-panel form of lin160.hip: statistics from the
  // register-resident rows once per workgroup, so the fold is free there too (and the LayerNorm launch goes)
  if (!temporal_pe && !act && nr_lin160_panel_rule((int)M, N, K) && x.rows() % 128 == 0 && x.ld % 8 == 0) fuse = true;
  if (mode) fuse = mode[0] == '1';
  GemmOpt o;
  o.geglu = geglu ? 1 : 0; o.act = act;
  if (fuse) {
    const auto lw = wts.w_ln_linear(wkeys, bkeys, ln, Neach, K, geglu);
    o.bias = lw.b; o.ln_c = lw.c;
    if (temporal_pe) {
      o.rowvec = wts.pe_projection(wkeys, Neach, K, cfg.motion_pe_max_len);
      o.rowvec_div = x.H * x.W; o.rowvec_ld = N; o.rowvec_mod = F;
    }
    return linear(x, lw.w, N, o);
  }
  Act n = layernorm(x, ln, temporal_pe ? wts.pe_table(K, cfg.motion_pe_max_len) : nullptr, temporal_pe ? F : 1);
  const bf16* w;
  if (geglu) {
    w = wts.w_geglu(wkeys[0], Neach, K);
    if (!bkeys.empty()) o.bias = wts.b_geglu(bkeys[0], Neach);
  } else if (wkeys.size() > 1) {
    w = wts.w_linear_cat(wkeys, Neach, K);
    if (!bkeys.empty()) o.bias = wts.b_cat(bkeys, Neach);
  } else {
    w = wts.w_linear(wkeys[0], Neach, K);
    if (!bkeys.empty()) o.bias = wts.w_f32(bkeys[0], Neach);
  }
  return linear(n, w, N, o);
}

// FeedForward(GEGLU) + residual, in place on t (motion_module_new.py:441-471,497-518)
void nr_net::feed_forward(Act& t, const std::string& ln, const std::string& pre) {
  const int C = t.C, inner = 4 * C;
  Act hmid = ln_linear(t, ln, {pre + ".net.0.proj.weight"}, {pre + ".net.0.proj.bias"}, inner, true, 0, false);
  linear_wb(hmid, pre + ".net.2", C, &t, &t);
}

// The block's LAST FeedForward and the transformer's proj_out as one GEMM (w_fold_ff_proj): x + proj_out(t + FF(t)) =
// x + bc + [t | g] Wc^T with g = GEGLU(net.0(LN(t))).  Removes a launch and the write + read of the post-FF residual stream.
// Needs C % 64 == 0 (the operand switch falls on a k-tile boundary); NR_FOLD_PROJ_OUT=0 keeps the two GEMMs.
Act nr_net::feed_forward_proj_out(const Act& x, Act& t, const std::string& ln, const std::string& ff, const std::string& pre) {
  static const bool fold = env_not_0("NR_FOLD_PROJ_OUT");
  const int C = t.C, inner = 4 * C;
  if (!fold || C % 64 != 0) {
    feed_forward(t, ln, ff);
    return linear_wb(t, pre + ".proj_out", C, &x);
  }
  if (nr_ff_fused_eligible(C, det_rows(t.rows())) && t.ld == C && x.ld == C) return ff_fused_block(x, t, ln, ff, pre + ".proj_out");
  Act g = ln_linear(t, ln, {ff + ".net.0.proj.weight"}, {ff + ".net.0.proj.bias"}, inner, true, 0, false);
  const auto fw = wts.w_fold_ff_proj(ff + ".net.2", pre + ".proj_out", C);
  GemmOpt op; op.bias = fw.b; op.res = &x; op.derived_w = true;
  return conv(t, &g, fw.w, C, 1, 1, 0, op);
}

// Exact classifier-free-guidance de-duplication (U-Net only, cfg_dup): the pipeline feeds cat([latents] * 2) with ONE timestep
// (pipeline_neuroclips.py:435), so the two halves of the batch are identical until the first cross-attention reads the (different) text
// contexts: conv_in, down_blocks[0].resnets[0] and norm / proj_in / norm1 / attn1 of down_blocks[0].attentions[0] (attention.py:256-280) are
// evaluated on B2 / 2 samples and broadcast.  Not in deterministic-batch mode (its plan unit is the CFG pair) and not with debug taps.
bool nr_net::cfg_dedup_active() const {
  static const bool on = env_not_0("NR_CFG_DEDUP");      // A/B switch
  return on && cfg_dup && cfg.kind == NR_KIND_UNET3D && B2 % 2 == 0 && B2 <= 64 && !det_batch && !keep_all && cfg.down_block_has_attn[0];
}
// [h; h]: the half-batch activation repeated for the second half of the batch (one gather launch)
Act nr_net::expand_cfg(const Act& h) {
  if (h.ld != h.C) throw NrError(NR_ERR_STATE, "expand_cfg: strided activation");
  const int Bh = B2 / 2;
  Act f = new_act(h.nimg * 2, h.H, h.W, h.C);
  const long long fe = (long long)(h.nimg / Bh) * h.H * h.W * h.C;      // elements of one sample
  const bf16* sp = h.ptr; bf16* dp = f.ptr; const int b2n = B2;
  std::vector<int> mp(B2);
  for (int i = 0; i < B2; ++i) mp[i] = i % Bh;
  emit([=](hipStream_t s) { LAUNCH_OK(nr_launch_frame_gather(sp, dp, 1, Bh, b2n, fe, mp.data(), s)); }, NR_PROF_OTHER, 0.0, 2.0 * 3.0 * (double)h.rows() * h.C,
       "cfg broadcast rows=" + std::to_string(h.rows()) + " C=" + std::to_string(h.C));
  return f;
}

nr_net::BlockKernel nr_net::cross_attn_kernel(const Act& t, int heads, int hw) const {
  if (cfg.kind == NR_KIND_SGM_UNET || attn_fp8 || t.ld != t.C) return BLOCK_UNFUSED;
  if (nr_xattn_fused_eligible(t.C, heads, ctx_len, hw, det_rows(t.rows()))) return BLOCK_FUSED320;
  return nr_xattnw_eligible(t.C, heads, ctx_len, hw, det_rows(t.rows())) ? BLOCK_HEAD : BLOCK_UNFUSED;
}
nr_net::BlockKernel nr_net::temporal_attn_kernel(const Act& t, int heads, int hw) const {
  if (t.ld != t.C) return BLOCK_UNFUSED;
  if (nr_tattn_fused_eligible(t.C, heads, F, hw, det_rows(t.rows()))) return BLOCK_FUSED320;
  return nr_tattnw_eligible(t.C, heads, F, hw, det_rows(t.rows())) ? BLOCK_HEAD : BLOCK_UNFUSED;
}

// ---- the five fused transformer kernels: each emitter fetches the kernel's weights (WeightStore::X_weights), fills its launch description and emits ONE op ----
// C = 320, >= 4096 rows: LayerNorm + GEGLU projection + the folded net.2 | proj_out GEMM in ONE launch (ffpanel.hip); the 4C-wide hidden activation
// stays in registers; LayerNorm is applied to the register panel.  The weights travel as one pre-arranged stage stream.
Act nr_net::ff_fused_block(const Act& x, const Act& t, const std::string& ln, const std::string& ff, const std::string& po) {
  const int C = t.C, M = (int)t.rows();
  const auto w = wts.ff_fused_weights(ln, ff, po, C);
  Act out = new_act(x.nimg, x.H, x.W, C);
  const NrFfFusedParams p{.t = t.ptr, .ldt = C, .x = x.ptr, .ldx = C, .out = out.ptr, .ldo = C, .M = M, .stream = w.stream, .gamma = w.gamma, .beta = w.beta, .b1 = w.b1,
                          .bc = w.bc, .ln_eps = 1e-5f, .norot = det_batch ? 1 : 0, .waves = nr_ff_waves()};
  emit([p](hipStream_t s) { LAUNCH_OK(nr_launch_ff_fused(&p, s)); }, NR_PROF_IGEMM, 2.0 * M * (double)C * (8.0 * C + 5.0 * C),
       2.0 * (3.0 * M * (double)C + 13.0 * C * (double)C), descf("ff_fused M=%d C=%d (LN + GEGLU 8C + folded net.2|proj_out 5C)", M, C));
  op_tap("ff_fused", out);
  return out;
}
// C = 320, 8 heads, <= 80 context tokens, >= 4096 rows: the whole cross-attention block (LayerNorm, q projection, attention on the cached
// K | V of the clip, to_out + residual) in ONE launch that updates t in place (xattn.hip); q and the attention output never reach HBM
void nr_net::xattn_fused_block(Act& t, const Act& ctx_bf, const std::string& b, int hw) {
  const int C = t.C, nctx = (int)(ctx_bf.rows() / ctx_len), Lk = ctx_len;      // ctx_bf is ONE "image" of B2 * ctx_len token rows
  const double M = (double)t.rows();
  const Act kvs = context_kv(ctx_bf, b, C, nr_xattn_kvstream_bytes(nctx),      // + the per-head LDS images of K | V
                             [=](const bf16* kv, int ldkv, bf16* st, hipStream_t s) { LAUNCH_OK(nr_launch_xattn_kv_pack(kv, ldkv, Lk, nctx, st, s)); });
  const auto w = wts.xattn_fused_weights(b, C);
  const NrXattnFusedParams p{.t = t.ptr, .nimg = t.nimg, .hw = hw, .img_per_ctx = F, .nctx = nctx, .Lk = Lk, .wstream = w.wstream, .kvstream = kvs.ptr, .gamma = w.gamma,
                             .beta = w.beta, .bo = w.bo, .ln_eps = 1e-5f, .norot = det_batch ? 1 : 0};
  emit([p](hipStream_t s) { LAUNCH_OK(nr_launch_xattn_fused(&p, s)); }, NR_PROF_IGEMM, 2.0 * M * C * 2.0 * C + 4.0 * M * (double)Lk * C,
       2.0 * (2.0 * M * C + 2.0 * C * (double)C), descf("xattn_fused M=%d C=%d Lk=%d (LN, q, context attention, to_out + residual)", (int)t.rows(), C, Lk));
  op_tap("xattn_fused", t);
}
// C = 640 / 1280, 8 heads, <= 80 context tokens: LayerNorm (folded), the q projection and the attention on the cached K | V of the row's
// context in ONE launch per block (xattnw.hip); q never reaches HBM.  Returns the attention output: to_out + residual stays the caller's GEMM.
Act nr_net::xattn_head_block(const Act& t, const Act& ctx_bf, const std::string& b, int hw) {
  const int C = t.C, nctx = (int)(ctx_bf.rows() / ctx_len), Lk = ctx_len;
  const Act kvs = context_kv(ctx_bf, b, C, nr_xattnw_kvstream_bytes(C, nctx),      // + the fragment images of K | V
                             [=](const bf16* kv, int ldkv, bf16* st, hipStream_t s) { LAUNCH_OK(nr_launch_xattnw_kv_pack(kv, ldkv, Lk, nctx, C, st, s)); });
  const auto w = wts.xattn_head_weights(b + ".norm2", b + ".attn2.to_q.weight", C);
  Act a = new_act(t.nimg, t.H, t.W, C);
  const NrXattnHeadParams p{.t = t.ptr, .out = a.ptr, .nimg = t.nimg, .hw = hw, .img_per_ctx = F, .nctx = nctx, .Lk = Lk, .C = C, .wstream = w.stream, .kvstream = kvs.ptr,
                            .table = w.table, .ln_eps = 1e-5f};
  const double M = (double)t.rows();
  emit([p](hipStream_t s) { LAUNCH_OK(nr_launch_xattnw(&p, s)); }, NR_PROF_IGEMM, 2.0 * M * C * (double)C + 4.0 * M * (double)Lk * C,
       2.0 * (2.0 * M * C + C * (double)C), descf("xattn_head M=%d C=%d Lk=%d (LN folded, q of 160 columns, context attention)", (int)t.rows(), C, Lk));
  op_tap("xattn_head", a);
  return a;
}
// C = 320, F = 16 or 32: the whole block (LayerNorm + PE, q|k|v, F x F attention per pixel and head, to_out + residual) in ONE launch
// that updates t in place (tattn.hip); q|k|v and the attention output never reach HBM
void nr_net::tattn_fused_block(Act& t, const std::string& nrm, const std::string& ab, int hw, int heads) {
  const int C = t.C; const double M = (double)t.rows();
  const auto w = wts.tattn_fused_weights(nrm, ab, F, C);
  const NrTattnFusedParams p{.t = t.ptr, .nbatch = t.nimg / F, .frames = F, .hw = hw, .stream = w.stream, .gamma = w.gamma, .gb = w.gb, .bo = w.bo, .ln_eps = 1e-5f,
                             .norot = det_batch ? 1 : 0};
  emit([p](hipStream_t s) { LAUNCH_OK(nr_launch_tattn_fused(&p, s)); }, NR_PROF_IGEMM, 2.0 * M * C * 4.0 * C + 4.0 * (M / F) * heads * (double)F * F * (C / heads),
       2.0 * (2.0 * M * C + 4.0 * C * (double)C), descf("tattn_fused M=%d C=%d F=%d (LN+PE, q|k|v, attention, to_out + residual)", (int)t.rows(), C, F));
  op_tap("tattn_fused", t);
}
// C = 640 / 1280, F = 16 or 32: LayerNorm + PE (folded), the q|k|v projection of one head and its F x F attention per (pixel group, head) in
// ONE launch (tattnw.hip); q|k|v never reach HBM.  Returns the attention output: to_out + residual stays the caller's GEMM.
Act nr_net::tattn_head_block(const Act& t, const std::string& nrm, const std::vector<std::string>& wqkv, int hw, int heads) {
  const int C = t.C; const double M = (double)t.rows();
  const auto w = wts.tattn_head_weights(nrm, wqkv, C, F, cfg.motion_pe_max_len);
  Act a = new_act(t.nimg, t.H, t.W, C);
  const NrTattnHeadParams p{.t = t.ptr, .out = a.ptr, .nbatch = t.nimg / F, .frames = F, .hw = hw, .C = C, .stream = w.stream, .table = w.table, .ln_eps = 1e-5f};
  emit([p](hipStream_t s) { LAUNCH_OK(nr_launch_tattnw(&p, s)); }, NR_PROF_IGEMM, 2.0 * M * C * 3.0 * C + 4.0 * (M / F) * heads * (double)F * F * (C / heads),
       2.0 * (2.0 * M * C + 3.0 * C * (double)C), descf("tattn_head M=%d C=%d F=%d (LN+PE folded, q|k|v of one head, FxF attention)", (int)t.rows(), C, F));
  op_tap("tattn_head", a);
  return a;
}

// Transformer3DModel.forward (attention.py:95-142) with one BasicTransformerBlock (:256-300); also sgm
// SpatialTransformer.forward (sgm/modules/attention.py:702-723) with `depth` BasicTransformerBlocks (:551-572):
// same arithmetic and parameter names (proj_in/out are nn.Linear there: same [C][C] matrix).
// cfg_half: x holds the first half of the batch only (cfg_dedup_active); t and x are broadcast behind the self-attention, the result is full-batch;
// *x_full receives the broadcast input (the caller's skip connection)
Act nr_net::spatial_transformer(const Act& x_in, const Act& ctx_bf, const std::string& pre, int depth, bool cfg_half, Act* x_full) {
  Act x = x_in;
  const int C = x.C, heads = cfg.num_head_channels > 0 ? C / cfg.num_head_channels : cfg.num_heads;
  Act t = linear_wb(groupnorm(x, nullptr, pre + ".norm", 1e-6f, 0), pre + ".proj_in", C);      // norm -> proj_in
  for (int dd = 0; dd < depth; ++dd) {
    const std::string b = pre + ".transformer_blocks." + std::to_string(dd);
    {  // self-attention
      Act qkv = ln_linear(t, b + ".norm1", {b + ".attn1.to_q.weight", b + ".attn1.to_k.weight", b + ".attn1.to_v.weight"}, {}, C, false, 0, false);
      Act a = attention(0, qkv, nullptr, C, heads);
      qkv = Act();
      linear_wb(a, b + ".attn1.to_out.0", C, &t, &t);
    }
    if (cfg_half && dd == 0) {      // from here on the two CFG halves differ (their text contexts do)
      t = expand_cfg(t);
      x = expand_cfg(x);
      if (x_full) *x_full = x;
    }
    const BlockKernel xk = cross_attn_kernel(t, heads, x.H * x.W);
    if (xk == BLOCK_FUSED320) xattn_fused_block(t, ctx_bf, b, x.H * x.W);
    else {
      Act a;
      if (xk == BLOCK_HEAD) a = xattn_head_block(t, ctx_bf, b, x.H * x.W);
      else {  // cross-attention on the context (attention.py:100: context repeated per frame)
        Act q = ln_linear(t, b + ".norm2", {b + ".attn2.to_q.weight"}, {}, C, false, 0, false);
        Act kv = context_kv(ctx_bf, b, C);
        a = attention(1, q, &kv, C, heads);
      }
      linear_wb(a, b + ".attn2.to_out.0", C, &t, &t);      // to_out + residual
    }
    if (dd + 1 < depth) feed_forward(t, b + ".norm3", b + ".ff");
  }
  Act out = feed_forward_proj_out(x, t, pre + ".transformer_blocks." + std::to_string(depth - 1) + ".norm3",
                                  pre + ".transformer_blocks." + std::to_string(depth - 1) + ".ff", pre);
  tap(pre, out);
  return out;
}

// VanillaTemporalModule -> TemporalTransformer3DModel.forward (motion_module.py:134-158)
Act nr_net::temporal_module(const Act& x, const std::string& pre0) {
  const std::string pre = pre0 + ".temporal_transformer";
  const int C = x.C, heads = cfg.motion_num_heads;
  if (F > cfg.motion_pe_max_len)
    throw NrError(NR_ERR_ARG, "video_length " + std::to_string(F) + " exceeds temporal_position_encoding_max_len " +
                                  std::to_string(cfg.motion_pe_max_len));
  Act t = linear_wb(groupnorm(x, nullptr, pre + ".norm", 1e-6f, 0), pre + ".proj_in", C);      // norm -> proj_in
  const std::string b = pre + ".transformer_blocks.0";
  for (int k = 0; k < cfg.motion_num_attention_blocks; ++k) {
    const std::string ab = b + ".attention_blocks." + std::to_string(k);
    const std::string nrm = b + ".norms." + std::to_string(k);
    const std::vector<std::string> wqkv = {ab + ".to_q.weight", ab + ".to_k.weight", ab + ".to_v.weight"};
    const BlockKernel tk = temporal_attn_kernel(t, heads, x.H * x.W);
    if (tk == BLOCK_FUSED320) { tattn_fused_block(t, nrm, ab, x.H * x.W, heads); continue; }
    Act a;
    if (tk == BLOCK_HEAD) a = tattn_head_block(t, nrm, wqkv, x.H * x.W, heads);
    else {  // LayerNorm, then + pe[frame] (motion_module.py:212,277): both folded into the q|k|v GEMM
      Act qkv = ln_linear(t, nrm, wqkv, {}, C, false, 0, true);
      a = attention(2, qkv, nullptr, C, heads);
    }
    linear_wb(a, ab + ".to_out.0", C, &t, &t);      // to_out + residual
  }
  Act out = feed_forward_proj_out(x, t, b + ".ff_norm", b + ".ff", pre);
  tap(pre0, out);
  return out;
}

// AttnBlock (model.py:161-201): GroupNorm -> q,k,v 1x1 convs -> single-head softmax(q k^T / sqrt(C)) v -> proj_out
// + x.  The head dimension is the full channel count.  Two forms:
//  * wide: one q|k|v Linear over all images, ONE attention launch on the wide-head flash kernel (attention.hip, NR_ATTN_WIDE: C = 256 / 512) and proj_out;
//    any h*w, no score scratch;
//  * GEMM sequence, per image: S = Q K^T (fp32 scores), row softmax -> bf16 P, O = P V; h*w a multiple of 64.  V is produced already transposed
//    (V^T = Wv . Xn^T, i.e. the igemm with the weight as the "activation" operand); its bias moves to the P V epilogue because every softmax row sums to one.
// Default: wide where the route serves C and either the GEMM sequence refuses the latent (h*w % 64 != 0) or the launch has a workgroup for every CU
// (nimg * ceil(h*w / 64) >= 256: the 16 x 1024-token clip, 0.11 ms against 16 x 0.044 ms).  With fewer workgroups the wide kernel's time is one
// workgroup's walk over all keys whatever the image count: at the 9216-token keyframe (144 workgroups) 0.81 ms against 0.47 ms for the GEMMs, so
// such shapes stay on the GEMM sequence (profiles/r09_vae_attn_wide_ab.txt).  NR_VAE_ATTN_WIDE=0: never wide; =1: wide for every shape the route
// serves.  Read when the launch is described (each plan).
static bool vae_attn_wide(int C, int nimg, int hw) {
  const char* sw = getenv("NR_VAE_ATTN_WIDE");
  if (sw && sw[0] == '0') return false;
  NrAttnParams p{};      // what the route reads of a single-head bf16 self-attention (the tensors come with the real launch, nr_net::attention)
  p.nbatch = nimg; p.heads = 1; p.d = C; p.Lq = p.Lk = hw; p.inner = p.kv_inner = p.kv_div = 1;
  NrAttnRoute r;
  if (nr_attn_route(&p, &r) != 0 || r.cls != NR_ATTN_WIDE) return false;
  if (sw && sw[0] == '1') return true;
  return hw % 64 != 0 || r.grid >= 256u;
}
Act nr_net::vae_attn(const Act& x, const std::string& pre) {
  const int C = x.C, hw = x.H * x.W;
  if (vae_attn_wide(C, x.nimg, hw)) {
    Act hn = groupnorm(x, nullptr, pre + ".norm", cfg.norm_eps, 0);
    GemmOpt oq; oq.bias = wts.b_cat({pre + ".q.bias", pre + ".k.bias", pre + ".v.bias"}, C);
    Act qkv = linear(hn, wts.w_linear_cat({pre + ".q.weight", pre + ".k.weight", pre + ".v.weight"}, C, C), 3 * C, oq);
    hn = Act();
    Act o = attention(0, qkv, nullptr, C, 1);
    qkv = Act();
    Act out = linear_wb(o, pre + ".proj_out", C, &x);
    tap(pre, out);
    return out;
  }
  if (hw % 64 != 0) throw NrError(NR_ERR_UNSUPPORTED, "VAE attention: latent h*w must be a multiple of 64");
  Act hn = groupnorm(x, nullptr, pre + ".norm", cfg.norm_eps, 0);
  Act q = linear_wb(hn, pre + ".q", C);
  Act k = linear_wb(hn, pre + ".k", C);
  const bf16* wv = wts.w_linear(pre + ".v.weight", C, C);
  const float* bv = wts.w_f32(pre + ".v.bias", C);
  Act o = new_act(x.nimg, x.H, x.W, C);
  {
    auto vt = new_tmp((size_t)C * hw * sizeof(bf16));
    auto sc = new_tmp((size_t)hw * hw * sizeof(float));
    auto pr = new_tmp((size_t)hw * hw * sizeof(bf16));
    bf16* vtp = at<bf16>(vt->off); float* scp = at<float>(sc->off); bf16* prp = at<bf16>(pr->off);
    const float scale = 1.0f / std::sqrt((float)C);
    for (int n = 0; n < x.nimg; ++n) {
      const size_t off = (size_t)n * hw * C;
      gemm_raw(wv, C, hn.ptr + off, C, hw, C, nullptr, vtp, hw, nullptr, "vae V^T");
      gemm_raw(q.ptr + off, C, k.ptr + off, hw, hw, C, nullptr, nullptr, 0, scp, "vae QK^T");
      emit([=](hipStream_t s) { LAUNCH_OK(nr_launch_softmax_rows(scp, prp, hw, hw, scale, s)); }, NR_PROF_ATTENTION,
           5.0 * (double)hw * hw, 6.0 * (double)hw * hw, "softmax rows L=" + std::to_string(hw));
      gemm_raw(prp, hw, vtp, hw, C, hw, bv, o.ptr + off, C, nullptr, "vae PV");
    }
  }
  hn = Act(); q = Act(); k = Act();
  Act out = linear_wb(o, pre + ".proj_out", C, &x);
  tap(pre, out);
  return out;
}
