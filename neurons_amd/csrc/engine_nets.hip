// The networks of the engine (engine.h) as launch plans over the emitters of engine_layers.hip, and the two-pass planner.  The plans follow the
// reference module graphs:
//   UNet3DConditionModel.forward        animatediff/models/unet.py:357-475
//   SparseControlNetModel.forward       animatediff/models/sparse_controlnet.py:467-581
//   Cross/Down/Mid/Up blocks            animatediff/models/unet_blocks.py:271-278,382-421,493-521,621-667,735-760
// Host code only.
#include "engine.h"

using namespace nre;

// ------------------------------------------------------------------ topology
// enumerate resnets (prefix, Cout) in definition order: used for the batched time-embedding projection
void nr_net::enumerate_resnets(std::vector<TembSlot>& out) const {
  int off = 0;
  auto add = [&](const std::string& p, int C) { out.push_back(TembSlot{p, off, C}); off += C; };
  const int L = cfg.num_levels;
  for (int i = 0; i < L; ++i)
    for (int j = 0; j < cfg.layers_per_block; ++j)
      add("down_blocks." + std::to_string(i) + ".resnets." + std::to_string(j), cfg.block_out_channels[i]);
  add("mid_block.resnets.0", cfg.block_out_channels[L - 1]);
  add("mid_block.resnets.1", cfg.block_out_channels[L - 1]);
  if (cfg.kind == NR_KIND_UNET3D)
    for (int i = 0; i < L; ++i)
      for (int j = 0; j < cfg.layers_per_block + 1; ++j)
        add("up_blocks." + std::to_string(i) + ".resnets." + std::to_string(j), cfg.block_out_channels[L - 1 - i]);
}

// ---------------------------------------------------------------------------------------------------
// sgm UNetModel (generative_models/sgm/modules/diffusionmodules/openaimodel.py:472; forward :816-853;
// construction order :640-807 fixes the input_blocks / output_blocks numbering used for the key names)
// ---------------------------------------------------------------------------------------------------
nr_net::SgmLayout nr_net::sgm_layout() const {
  SgmLayout l;
  const int L = cfg.num_levels;
  int idx = 0;
  l.in.push_back({idx++, 0, 0, cfg.block_out_channels[0]});
  for (int lev = 0; lev < L; ++lev) {
    for (int r = 0; r < cfg.layers_per_block; ++r) l.in.push_back({idx++, 1, lev, cfg.block_out_channels[lev]});
    if (lev != L - 1) l.in.push_back({idx++, 2, lev, cfg.block_out_channels[lev]});
  }
  idx = 0;
  for (int lev = L - 1; lev >= 0; --lev)
    for (int i = 0; i <= cfg.layers_per_block; ++i)
      l.out.push_back({idx++, lev, cfg.block_out_channels[lev], cfg.down_block_has_attn[lev] != 0,
                       lev > 0 && i == cfg.layers_per_block});
  return l;
}

void nr_net::build_sgm() {
  const int L = cfg.num_levels;
  const int C0 = cfg.block_out_channels[0];
  const int temb_dim = 4 * C0;
  const int nimg = B2 * F;
  if (F != 1) throw NrError(NR_ERR_ARG, "sgm UNetModel is a 2-D network: plan with frames = 1");
  const SgmLayout lay = sgm_layout();
  begin_plan();
  {
    int off = 0;
    auto add = [&](const std::string& p, int C) { temb_slots.push_back(TembSlot{p, off, C}); off += C; };
    for (auto& b : lay.in) if (b.kind == 1) add("input_blocks." + std::to_string(b.idx) + ".0", b.Cout);
    add("middle_block.0", cfg.block_out_channels[L - 1]);
    add("middle_block.2", cfg.block_out_channels[L - 1]);
    for (auto& b : lay.out) add("output_blocks." + std::to_string(b.idx) + ".0", b.Cout);
    temb_total = off;
  }
  // ---- emb = time_embed(sinusoid(t)) + label_emb(y)  (openaimodel.py:836-841); every ResBlock then applies
  // Linear(SiLU(emb)) (emb_layers, :283-289): batched into ONE launch ----
  float* sincos = new_scratch<float>((size_t)B2 * C0);
  float* e1 = new_scratch<float>((size_t)B2 * temb_dim);
  float* et = new_scratch<float>((size_t)B2 * temb_dim);
  float* y1 = new_scratch<float>((size_t)B2 * temb_dim);
  float* emb = new_scratch<float>((size_t)B2 * temb_dim);
  temb_all = new_scratch<float>((size_t)B2 * temb_total);
  {
    const int adm = cfg.adm_in_channels;
    const bf16* w1 = wts.w_linear("time_embed.0.weight", temb_dim, C0);
    const float* b1 = wts.w_f32("time_embed.0.bias", temb_dim);
    const bf16* w2 = wts.w_linear("time_embed.2.weight", temb_dim, temb_dim);
    const float* b2 = wts.w_f32("time_embed.2.bias", temb_dim);
    const bf16* wy1 = wts.w_linear("label_emb.0.0.weight", temb_dim, adm);
    const float* by1 = wts.w_f32("label_emb.0.0.bias", temb_dim);
    const bf16* wy2 = wts.w_linear("label_emb.0.2.weight", temb_dim, temb_dim);
    const float* by2 = wts.w_f32("label_emb.0.2.bias", temb_dim);
    const auto proj = wts.w_temb_projection("sgm", temb_slots, ".emb_layers.1", temb_dim);
    const bf16* wp = proj.w; const float* bp = proj.b;
    float* td = t_dev; float* ta = temb_all;
    const int b2n = B2, tt = temb_total;
    emit([=, this](hipStream_t s) {
      LAUNCH_OK(nr_launch_timestep_sincos(td, b2n, C0, sincos, s));
      LAUNCH_OK(nr_launch_linear_small(sincos, b2n, C0, w1, b1, temb_dim, 0, 1, e1, nullptr, s));
      LAUNCH_OK(nr_launch_linear_small(e1, b2n, temb_dim, w2, b2, temb_dim, 0, 0, et, nullptr, s));
      LAUNCH_OK(nr_launch_linear_small(io.y, b2n, adm, wy1, by1, temb_dim, 0, 1, y1, nullptr, s));
      LAUNCH_OK(nr_launch_linear_small(y1, b2n, temb_dim, wy2, by2, temb_dim, 0, 1, emb, et, s));   // SiLU(time + label)
      LAUNCH_OK(nr_launch_linear_small(emb, b2n, temb_dim, wp, bp, tt, 0, 0, ta, nullptr, s));
    });
    last_op_launches(6);
  }
  // ---- context fp32 -> bf16 ----
  Act ctx_bf = stage_context();
  // ---- input blocks ----
  std::vector<Act> hs;
  Act x;
  for (auto& b : lay.in) {
    const std::string bp = "input_blocks." + std::to_string(b.idx);
    if (b.kind == 0) {
      x = new_act(nimg, H, W, C0);
      const float* wT = wts.w_conv_in(bp + ".0.weight", C0, cfg.in_channels);
      const float* bi = wts.w_f32(bp + ".0.bias", C0);
      bf16* xp = x.ptr; const int ic = cfg.in_channels, b2n = B2, Hn = H, Wn = W;
      emit([=, this](hipStream_t s) {
        LAUNCH_OK(nr_launch_conv_in_small(io.sample, nullptr, ic, 0, b2n, nimg, 1, Hn, Wn, wT, bi, nullptr, C0, xp, io.in_scale, 0.f, s));
      });
      tap(bp, x);
    } else if (b.kind == 1) {
      x = resnet(x, nullptr, bp + ".0", b.Cout);
      if (cfg.down_block_has_attn[b.level]) x = spatial_transformer(x, ctx_bf, bp + ".1", cfg.transformer_depth[b.level]);
    } else {
      GemmOpt o; o.bias = wts.w_f32(bp + ".0.op.bias", b.Cout);
      x = conv(x, nullptr, wts.w_conv3(bp + ".0.op.weight", b.Cout, b.Cout), b.Cout, 3, 2, 0, o);
      tap(bp, x);
    }
    hs.push_back(x);
  }
  // ---- middle block ----
  {
    const int Cm = cfg.block_out_channels[L - 1];
    x = resnet(x, nullptr, "middle_block.0", Cm);
    x = spatial_transformer(x, ctx_bf, "middle_block.1", cfg.transformer_depth[L - 1]);
    x = resnet(x, nullptr, "middle_block.2", Cm);
  }
  // ---- output blocks: h = cat([h, hs.pop()]) -> ResBlock -> [SpatialTransformer] -> [Upsample] ----
  for (auto& b : lay.out) {
    const std::string bp = "output_blocks." + std::to_string(b.idx);
    Act skip = hs.back();
    hs.pop_back();
    x = resnet(x, &skip, bp + ".0", b.Cout);
    skip = Act();
    int sub = 1;
    if (b.attn) { x = spatial_transformer(x, ctx_bf, bp + ".1", cfg.transformer_depth[b.level]); sub = 2; }
    if (b.up) {
      const std::string up = bp + "." + std::to_string(sub) + ".conv";
      GemmOpt o; o.bias = wts.w_f32(up + ".bias", b.Cout);
      x = upsample_conv(x, up + ".weight", b.Cout, o);
      tap(bp + "." + std::to_string(sub), x);
    }
  }
  // ---- out: GroupNorm32 -> SiLU -> conv (openaimodel.py:809-813) ----
  Act hn = groupnorm(x, nullptr, "out.0", cfg.norm_eps, 1);
  {
    const bf16* wo = wts.w_conv3("out.2.weight", cfg.out_channels, C0);
    const float* bo = wts.w_f32("out.2.bias", cfg.out_channels);
    const bf16* hp = hn.ptr; const int Hn = H, Wn = W, oc = cfg.out_channels;
    emit([=, this](hipStream_t s) { LAUNCH_OK(nr_launch_conv_out_small(hp, C0, nimg, 1, Hn, Wn, wo, bo, oc, io.out, 1.f, 0.f, 0, s)); });
  }
}

// AutoencodingEngineLegacy.decode (sgm/models/autoencoder.py:490-494) = post_quant_conv -> Decoder.forward
// (sgm/modules/diffusionmodules/model.py:723-757).  Same network as diffusers AutoencoderKL.decode used by
// decode_latents (pipeline_animation.py:243-256) under different parameter names.
void nr_net::build_vae() {
  const int L = cfg.num_levels, zc = cfg.in_channels, nimg = B2;
  if (F != 1) throw NrError(NR_ERR_ARG, "the VAE decoder is a 2-D network: plan with frames = 1");
  begin_plan();
  const int Cm = cfg.block_out_channels[L - 1];
  float* zq = new_scratch<float>((size_t)nimg * zc * H * W);
  {
    const float* Q = wts.w_f32("post_quant_conv.weight", {zc, zc});
    const float* qb = wts.w_f32("post_quant_conv.bias", zc);
    const int hw = H * W;
    emit([=, this](hipStream_t s) { LAUNCH_OK(nr_launch_post_quant(io.sample, io.in_scale, Q, qb, zq, nimg, zc, hw, s)); });
  }
  Act x = new_act(nimg, H, W, Cm);
  {
    const float* wT = wts.w_conv_in("decoder.conv_in.weight", Cm, zc);
    const float* bi = wts.w_f32("decoder.conv_in.bias", Cm);
    bf16* xp = x.ptr; const int Hn = H, Wn = W;
    emit([=](hipStream_t s) {
      LAUNCH_OK(nr_launch_conv_in_small(zq, nullptr, zc, 0, nimg, nimg, 1, Hn, Wn, wT, bi, nullptr, Cm, xp, 1.f, 0.f, s));
    });
    tap("decoder.conv_in", x);
  }
  x = resnet(x, nullptr, "decoder.mid.block_1", Cm);
  x = vae_attn(x, "decoder.mid.attn_1");
  x = resnet(x, nullptr, "decoder.mid.block_2", Cm);
  for (int lev = L - 1; lev >= 0; --lev) {
    const int Co = cfg.block_out_channels[lev];
    const std::string up = "decoder.up." + std::to_string(lev);
    for (int j = 0; j < cfg.layers_per_block + 1; ++j) x = resnet(x, nullptr, up + ".block." + std::to_string(j), Co);
    if (lev != 0) {
      GemmOpt o; o.bias = wts.w_f32(up + ".upsample.conv.bias", Co);
      x = upsample_conv(x, up + ".upsample.conv.weight", Co, o);   // nearest 2x + conv (model.py:67-71)
      tap(up + ".upsample", x);
    }
  }
  Act hn = groupnorm(x, nullptr, "decoder.norm_out", cfg.norm_eps, 1);
  {
    const int C0 = cfg.block_out_channels[0], oc = cfg.out_channels;
    const bf16* wo = wts.w_conv3("decoder.conv_out.weight", oc, C0);
    const float* bo = wts.w_f32("decoder.conv_out.bias", oc);
    const bf16* hp = hn.ptr; const int Hn = x.H, Wn = x.W;
    emit([=, this](hipStream_t s) { LAUNCH_OK(nr_launch_conv_out_small(hp, C0, nimg, 1, Hn, Wn, wo, bo, oc, io.out, io.out_mul, io.out_add, io.clamp01, s)); });
  }
}


// AutoencodingEngine.encode up to the moments (sgm/models/autoencoder.py:468-488): Encoder.forward
// (sgm/modules/diffusionmodules/model.py:584-609) -> quant_conv.  == diffusers AutoencoderKL.encode(x).latent_dist
// parameters (scripts/neuroclips_video.py:267,282).  Plan h, w are the IMAGE size; moments are [n][2z][h/8][w/8].
void nr_net::build_vae_enc() {
  const int L = cfg.num_levels, zc2 = cfg.out_channels, nimg = B2, ic = cfg.in_channels;
  if (F != 1) throw NrError(NR_ERR_ARG, "the VAE encoder is a 2-D network: plan with frames = 1");
  begin_plan();
  const int C0 = cfg.block_out_channels[0];
  Act x = new_act(nimg, H, W, C0);
  {
    const float* wT = wts.w_conv_in("encoder.conv_in.weight", C0, ic);
    const float* bi = wts.w_f32("encoder.conv_in.bias", C0);
    bf16* xp = x.ptr; const int Hn = H, Wn = W;
    emit([=, this](hipStream_t s) {
      LAUNCH_OK(nr_launch_conv_in_small(io.sample, nullptr, ic, 0, nimg, nimg, 1, Hn, Wn, wT, bi, nullptr, C0, xp, io.in_scale,
                                        io.in_shift, s));
    });
    tap("encoder.conv_in", x);
  }
  for (int lev = 0; lev < L; ++lev) {
    const int Co = cfg.block_out_channels[lev];
    const std::string dn = "encoder.down." + std::to_string(lev);
    for (int j = 0; j < cfg.layers_per_block; ++j) x = resnet(x, nullptr, dn + ".block." + std::to_string(j), Co);
    if (lev != L - 1) {
      // Downsample.forward (model.py:84-91): F.pad (0,1,0,1) then 3x3 stride-2 conv without padding
      GemmOpt o; o.bias = wts.w_f32(dn + ".downsample.conv.bias", Co); o.pad_tl0 = 1;
      x = conv(x, nullptr, wts.w_conv3(dn + ".downsample.conv.weight", Co, Co), Co, 3, 2, 0, o);
      tap(dn + ".downsample", x);
    }
  }
  const int Cm = cfg.block_out_channels[L - 1];
  x = resnet(x, nullptr, "encoder.mid.block_1", Cm);
  x = vae_attn(x, "encoder.mid.attn_1");
  x = resnet(x, nullptr, "encoder.mid.block_2", Cm);
  Act hn = groupnorm(x, nullptr, "encoder.norm_out", cfg.norm_eps, 1);
  {
    const int hw = x.H * x.W;
    float* mraw = new_scratch<float>((size_t)nimg * zc2 * hw);
    const bf16* wo = wts.w_conv3("encoder.conv_out.weight", zc2, Cm);
    const float* bo = wts.w_f32("encoder.conv_out.bias", zc2);
    const float* Q = wts.w_f32("quant_conv.weight", {zc2, zc2});
    const float* qb = wts.w_f32("quant_conv.bias", zc2);
    const bf16* hp = hn.ptr; const int Hn = x.H, Wn = x.W;
    emit([=, this](hipStream_t s) {
      LAUNCH_OK(nr_launch_conv_out_small(hp, Cm, nimg, 1, Hn, Wn, wo, bo, zc2, mraw, 1.f, 0.f, 0, s));
      LAUNCH_OK(nr_launch_post_quant(mraw, 1.f, Q, qb, io.out, nimg, zc2, hw, s));
    });
  }
}


// ------------------------------------------------------------------ CLIP text encoder
// transformers CLIPTextModel.forward -> last_hidden_state, as _encode_prompt calls it (pipeline_neuroclips.py:
// 153-240: text_encoder(ids, attention_mask=None)[0]): CLIPTextEmbeddings -> 12 x CLIPEncoderLayer (pre-LN, causal
// self-attention, quick_gelu MLP) -> final_layer_norm.  Config fields for this kind: block_out_channels[0] =
// hidden_size, num_heads, layers_per_block = num_hidden_layers, cross_attention_dim = intermediate_size,
// in_channels = vocab_size, motion_pe_max_len = max_position_embeddings.  Plan: (batch, 1, 1, seq_len, 0).
void nr_net::build_clip() {
  const int C = cfg.block_out_channels[0], heads = cfg.num_heads, inter = cfg.cross_attention_dim, vocab = cfg.in_channels;
  const int L = W, M = B2 * L;
  if (F != 1 || H != 1) throw NrError(NR_ERR_ARG, "CLIP text encoder: plan with frames = 1, h = 1, w = sequence length");
  if (L > cfg.motion_pe_max_len) throw NrError(NR_ERR_ARG, "sequence longer than max_position_embeddings");
  begin_plan();
  const std::string tm = "text_model.";
  Act x = new_act(B2, 1, L, C);
  {
    const std::string tk = tm + "embeddings.token_embedding.weight", pk = tm + "embeddings.position_embedding.weight";
    const float* tok = wts.w_f32(tk, {vocab, C});
    const float* pos = wts.w_f32(pk, {cfg.motion_pe_max_len, C});
    bf16* xp = x.ptr;
    emit([=, this](hipStream_t s) { LAUNCH_OK(nr_launch_clip_embed(io.ids, tok, pos, xp, M, L, C, vocab, s)); });
    tap("text_model.embeddings", x);
  }
  for (int i = 0; i < cfg.layers_per_block; ++i) {
    const std::string lp = tm + "encoder.layers." + std::to_string(i);
    const std::string ap = lp + ".self_attn";
    Act qkv = ln_linear(x, lp + ".layer_norm1", {ap + ".q_proj.weight", ap + ".k_proj.weight", ap + ".v_proj.weight"},
                        {ap + ".q_proj.bias", ap + ".k_proj.bias", ap + ".v_proj.bias"}, C, false, 0, false);
    Act ao = attention(0, qkv, nullptr, C, heads, 1);      // causal mask (CLIPTextTransformer builds it for every call)
    qkv = Act();
    // residual updates run in place, except in debug mode where every tap keeps its own buffer
    GemmOpt oo; oo.bias = wts.w_f32(ap + ".out_proj.bias", C); oo.res = &x; oo.out = keep_all ? nullptr : &x;
    Act x1 = linear(ao, wts.w_linear(ap + ".out_proj.weight", C, C), C, oo);
    x = x1;
    ao = Act();
    Act hmid = ln_linear(x, lp + ".layer_norm2", {lp + ".mlp.fc1.weight"}, {lp + ".mlp.fc1.bias"}, inter, false, 1, false);
    GemmOpt o2; o2.bias = wts.w_f32(lp + ".mlp.fc2.bias", C); o2.res = &x; o2.out = keep_all ? nullptr : &x;
    Act x2 = linear(hmid, wts.w_linear(lp + ".mlp.fc2.weight", C, inter), C, o2);
    x = x2;
    tap(lp, x);
  }
  Act fin = layernorm(x, tm + "final_layer_norm", nullptr, 1);
  {
    const bf16* fp = fin.ptr; const long long n = (long long)M * C;
    emit([=, this](hipStream_t s) { LAUNCH_OK(nr_launch_bf16_to_f32(fp, io.out, n, s)); });
  }
}

// ------------------------------------------------------------------ leaf modules (test hooks)
// ONE reference module as a network of its own, so that the reference classes' own outputs (tests/golden/leaf_ops.npz) can be
// compared at the row counts where the engine picks its fused kernels:
//   NR_KIND_LEAF_TRANSFORMER3D  Transformer3DModel.forward      (attention.py:95-142; state-dict keys "m.<reference key>")
//   NR_KIND_LEAF_TEMPORAL       VanillaTemporalModule.forward   (motion_module.py:79-86,134-158; keys "m.temporal_transformer...")
// Input / output are the reference's fp32 "b c f h w" tensors; the plan between the two layout converts is exactly the one
// spatial_transformer() / temporal_module() emit inside the U-Net.
void nr_net::build_leaf() {
  const int C = cfg.block_out_channels[0];
  const int nimg = B2 * F;
  begin_plan();
  Act x = new_act(nimg, H, W, C);
  {
    bf16* xp = x.ptr; const int b2n = B2, Fn = F, hw = H * W;
    emit([=, this](hipStream_t s) { LAUNCH_OK(nr_launch_ncfhw_to_nhwc(io.sample, xp, b2n, C, Fn, hw, s)); });
  }
  Act y;
  if (cfg.kind == NR_KIND_LEAF_TRANSFORMER3D) {
    y = spatial_transformer(x, stage_context(), "m");
  } else {
    y = temporal_module(x, "m");
  }
  {
    const bf16* yp = y.ptr; const int b2n = B2, Fn = F, hw = H * W;
    emit([=, this](hipStream_t s) { LAUNCH_OK(nr_launch_nhwc_to_ncfhw(yp, io.out, b2n, C, Fn, hw, s)); });
  }
}

// ---- SparseCtrl image-condition variant: SparseControlNetConditioningEmbedding (sparse_controlnet.py:49-82) added to conv_in (:513-521) ----
// x[b][f] = emb(cat[cond, mask])[b % cond_batch][f] + conv_in.bias (+ conv_in(sample) when the noisy sample is not zeroed).  The embedding
// depends on the condition and mask only: it runs once per condition image (cond_batch of them, read from io at launch; the buffers are
// sized for cond_batch = B2), never per CFG / grouped sample, and with the identical-frame evaluation active (nd > 0) only on the distinct
// frames (a zero condition with a zero mask embeds to the same constant on every other frame), then is broadcast into x.
Act nr_net::embed_conv(const Act& in, int Fe, const std::string& key, int Cout, int stride, int silu, const float* bias) {
  const int Cin = in.C, Hi = in.H, Wi = in.W;
  const int OH = stride == 2 ? (Hi - 1) / 2 + 1 : Hi, OW = stride == 2 ? (Wi - 1) / 2 + 1 : Wi;
  Act o = new_act(in.nimg, OH, OW, Cout);
  const bf16* w = wts.w_condembed(key + ".weight", Cout, Cin);
  const float* b = bias ? bias : wts.w_f32(key + ".bias", Cout);
  const bf16* ip = in.ptr; bf16* op = o.ptr;
  const std::string d = descf("condembed_conv Cin=%d Cout=%d s=%d H=%d W=%d frames=%d", Cin, Cout, stride, OH, OW, Fe);
  emit([=, this](hipStream_t s) { LAUNCH_OK(nr_launch_condembed_conv(ip, io.cond_batch * Fe, Hi, Wi, Cin, stride, w, b, Cout, silu, op, s)); },
       NR_PROF_IGEMM, 2.0 * Fe * OH * OW * Cout * 9.0 * Cin, 2.0 * Fe * ((double)Hi * Wi * Cin + (double)OH * OW * Cout) + 2.0 * Cout * 9.0 * Cin, d);
  return o;
}
void nr_net::cond_embedding(Act& x, int nd, const int* fmap_reduce, const int* fmap_expand) {
  const int L = cfg.cond_embedding_levels, C0 = cfg.block_out_channels[0], cc = cfg.conditioning_channels;
  const int* ch = cfg.cond_embedding_channels;
  const int Hc = H << (L - 1), Wc = W << (L - 1), Fn = F, Hn = H, Wn = W;
  const int Fe = nd > 0 ? nd : F;
  std::vector<int> fsel(Fe), emap(F);
  for (int e = 0; e < Fe; ++e) fsel[e] = nd > 0 ? fmap_reduce[e] : e;
  for (int f = 0; f < F; ++f) emap[f] = nd > 0 ? fmap_expand[f] : f;
  const std::string pre = "controlnet_cond_embedding.";
  // flops / bytes of the op descriptions are per condition image
  Act e = new_act(B2 * Fe, Hc, Wc, ch[0]);
  {
    const float* w = wts.w_conv_in(pre + "conv_in.weight", ch[0], cc + 1);
    const float* b = wts.w_f32(pre + "conv_in.bias", ch[0]);
    bf16* op = e.ptr; const int C = ch[0];
    const std::string d = descf("condembed_in Cin=%d Cout=%d H=%d W=%d frames=%d", cc + 1, C, Hc, Wc, Fe);
    emit([=, this](hipStream_t s) {
      LAUNCH_OK(nr_launch_condembed_in(io.cond, io.mask, cc, io.cond_batch, Fn, Hc, Wc, fsel.data(), Fe, w, b, C, op, s));
    }, NR_PROF_OTHER, 2.0 * Fe * Hc * Wc * C * 9.0 * (cc + 1), 4.0 * Fe * Hc * Wc * (cc + 1) + 2.0 * Fe * Hc * Wc * C, d);
  }
  for (int i = 0; i + 1 < L; ++i) {
    e = embed_conv(e, Fe, pre + "blocks." + std::to_string(2 * i), ch[i], 1, 1, nullptr);
    e = embed_conv(e, Fe, pre + "blocks." + std::to_string(2 * i + 1), ch[i + 1], 2, 1, nullptr);
  }
  if (e.H != H || e.W != W) throw NrError(NR_ERR_STATE, "condition embedding: output size differs from the latent size");
  const bool zero_sample = cfg.set_noisy_sample_input_to_zero;
  const std::string bo_key = pre + "conv_out.bias";
  const float* bo = zero_sample ? wts.w_f32_sum(bo_key, "conv_in.bias", C0) : wts.w_f32(bo_key, C0);    // conv_in(0) = conv_in.bias folded in
  const int cl = ch[L - 1];
  Act eo;
  if (cl % 64 == 0) {
    // conv_out (Cin = 256 at the latent grid) on the implicit-GEMM conv kernel; M follows the condition batch at launch
    eo = new_act(B2 * Fe, H, W, C0);
    NrGemmParams p = nr_gemm_params(e.ptr, cl, cl, nullptr, 0, 0, Fe, H, W, 3, 1, 0, wts.w_conv3(pre + "conv_out.weight", C0, cl), C0, bo, nullptr, 0, eo.ptr, C0);
    size_t wsb = 0;                                  // split-K scratch for the largest need of any cond_batch dividing B2
    std::vector<NrGemmRoute> routes((size_t)B2 + 1); // one route per such cond_batch
    for (int cb = 1; cb <= B2; ++cb)
      if (B2 % cb == 0) { p.M = cb * Fe * H * W; LAUNCH_OK(nr_gemm_route(&p, &routes[cb])); wsb = std::max(wsb, routes[cb].ws_bytes); }
    const SplitK sk = splitk_scratch(wsb);
    float* ws = sk.ws;
    p.M = Fe * H * W;
    const std::string d = descf("igemm ks=3 s=1 ups=0 M=%d N=%d K=%d condembed conv_out frames=%d", p.M, p.N, p.K, Fe);
    const int hw = H * W;
    emit([this, p, routes, ws, Fe, hw](hipStream_t s) {
      NrGemmParams q = p;
      q.M = io.cond_batch * Fe * hw;
      LAUNCH_OK(nr_launch_gemm(&q, &routes[io.cond_batch], q.w, ws, s));
    }, NR_PROF_IGEMM, 2.0 * p.M * (double)p.N * p.K, 2.0 * ((double)p.M * cl + (double)p.N * p.K + (double)p.M * C0), d);
  } else {
    eo = embed_conv(e, Fe, pre + "conv_out", C0, 1, 0, bo);
  }
  e = Act();
  const long long img = (long long)H * W * C0;
  bf16* xp = x.ptr; const bf16* ep = eo.ptr; const int b2n = B2;
  const std::string d = "condembed_bcast frames=" + std::to_string(Fe) + " -> " + std::to_string(F);
  if (zero_sample) {
    emit([=, this](hipStream_t s) { LAUNCH_OK(nr_launch_condembed_bcast(ep, io.cond_batch, Fe, emap.data(), b2n, Fn, img, nullptr, xp, s)); },
         NR_PROF_OTHER, 0.0, 4.0 * B2 * F * img, d);
  } else {
    const float* wT = wts.w_conv_in("conv_in.weight", C0, cfg.in_channels);
    const float* bi = wts.w_f32("conv_in.bias", C0);
    Act x2 = new_act(B2 * F, H, W, C0);
    bf16* x2p = x2.ptr; const int ic = cfg.in_channels, nimg = B2 * F;
    emit([=, this](hipStream_t s) {
      LAUNCH_OK(nr_launch_conv_in_small(io.sample, nullptr, ic, 0, b2n, nimg, Fn, Hn, Wn, wT, bi, nullptr, C0, x2p, 1.f, 0.f, s));
      LAUNCH_OK(nr_launch_condembed_bcast(ep, io.cond_batch, Fe, emap.data(), b2n, Fn, img, x2p, xp, s));
    }, NR_PROF_OTHER, 2.0 * nimg * H * W * C0 * 9.0 * ic, 6.0 * B2 * F * img, d);
    last_op_launches(2);
  }
}

void nr_net::build() {
  if (cfg.kind == NR_KIND_LEAF_TRANSFORMER3D || cfg.kind == NR_KIND_LEAF_TEMPORAL) { build_leaf(); return; }
  if (cfg.kind == NR_KIND_CLIP_TEXT) { build_clip(); return; }
  if (cfg.kind == NR_KIND_VAE_ENCODER) { build_vae_enc(); return; }
  if (cfg.kind == NR_KIND_SGM_UNET) { build_sgm(); return; }
  if (cfg.kind == NR_KIND_VAE_DECODER) { build_vae(); return; }
  const int L = cfg.num_levels;
  const int C0 = cfg.block_out_channels[0];
  const int temb_dim = 4 * C0;
  const int nimg = B2 * F;
  begin_plan();
  enumerate_resnets(temb_slots);
  temb_total = 0;
  for (auto& s : temb_slots) temb_total += s.C;

  // ---- time embedding (unet.py:371-392): sinusoid -> Linear -> SiLU -> Linear ; then every
  // resnet's Linear(SiLU(emb)) (resnet.py:191) in ONE batched launch ----
  float* sincos = new_scratch<float>((size_t)B2 * C0);
  float* emb1 = new_scratch<float>((size_t)B2 * temb_dim);
  float* emb = new_scratch<float>((size_t)B2 * temb_dim);
  temb_all = new_scratch<float>((size_t)B2 * temb_total);
  {
    const bf16* w1 = wts.w_linear("time_embedding.linear_1.weight", temb_dim, C0);
    const float* b1 = wts.w_f32("time_embedding.linear_1.bias", temb_dim);
    const bf16* w2 = wts.w_linear("time_embedding.linear_2.weight", temb_dim, temb_dim);
    const float* b2 = wts.w_f32("time_embedding.linear_2.bias", temb_dim);
    const auto proj = wts.w_temb_projection(std::to_string(cfg.kind), temb_slots, ".time_emb_proj", temb_dim);
    const bf16* wp = proj.w; const float* bp = proj.b;
    float* td = t_dev; float* ta = temb_all;
    const int b2n = B2, tt = temb_total;
    emit([=](hipStream_t s) {
      LAUNCH_OK(nr_launch_timestep_sincos(td, b2n, C0, sincos, s));
      LAUNCH_OK(nr_launch_linear_small(sincos, b2n, C0, w1, b1, temb_dim, 0, 1, emb1, nullptr, s));   // Linear + SiLU
      // every consumer of emb applies SiLU first (resnet.py:191), so store SiLU(emb) once instead of re-evaluating it
      // in each of the ~22k output rows of the batched projection
      LAUNCH_OK(nr_launch_linear_small(emb1, b2n, temb_dim, w2, b2, temb_dim, 0, 1, emb, nullptr, s)); // SiLU(emb)
      LAUNCH_OK(nr_launch_linear_small(emb, b2n, temb_dim, wp, bp, tt, 0, 0, ta, nullptr, s));         // Linear(SiLU(emb)) for all resnets
    });
    last_op_launches(4);
  }

  // ---- text context fp32 -> bf16 [B2*ctx_len][cross_dim] ----
  Act ctx_bf = stage_context();

  // SparseCtrl identical-frame evaluation (see n_cond_frames): distinct frames = the conditioned ones + one representative of the rest
  int nd = 0, fmap_reduce[64], fmap_expand[64];
  if (cfg.kind == NR_KIND_SPARSECTRL && cfg.set_noisy_sample_input_to_zero && cfg.use_motion_module && n_cond_frames >= 0 && !keep_all && F <= 64) {
    int rep = -1;
    for (int f = 0; f < F && rep < 0; ++f) {
      bool is_c = false;
      for (int k = 0; k < n_cond_frames; ++k) is_c = is_c || cond_frames[k] == f;
      if (!is_c) rep = f;
    }
    int nc = 0;
    for (int k = 0; k < n_cond_frames; ++k) if (cond_frames[k] < F) fmap_reduce[nc++] = cond_frames[k];
    if (rep >= 0 && nc + 1 < F) {
      fmap_reduce[nc] = rep;
      nd = nc + 1;
      for (int f = 0; f < F; ++f) {
        fmap_expand[f] = nc;
        for (int k = 0; k < nc; ++k) if (fmap_reduce[k] == f) fmap_expand[f] = k;
      }
    }
  }

  // ---- conv_in ----
  const bool cfg_half = cfg_dedup_active();      // conv_in .. attn1 of the first transformer on the first half of the batch only
  Act x = new_act(cfg_half ? nimg / 2 : nimg, H, W, C0);
  if (cfg.kind == NR_KIND_UNET3D) {
    const float* wT = wts.w_conv_in("conv_in.weight", C0, cfg.in_channels);
    const float* bi = wts.w_f32("conv_in.bias", C0);
    bf16* xp = x.ptr; const int ic = cfg.in_channels, b2n = cfg_half ? B2 / 2 : B2, ni = x.nimg, Fn = F, Hn = H, Wn = W;
    emit([=, this](hipStream_t s) {
      LAUNCH_OK(nr_launch_conv_in_small(io.sample, nullptr, ic, 0, b2n, ni, Fn, Hn, Wn, wT, bi, nullptr, C0, xp, 1.f, 0.f, s));
    });
  } else if (cfg.cond_embedding_levels > 0) {
    cond_embedding(x, nd, fmap_reduce, fmap_expand);
  } else {
    // sparse_controlnet.py:467-521: sample := 0 -> conv_in(0) = bias; + cond_embedding(cat[cond, mask])
    const int cc = cfg.conditioning_channels;
    const float* wTe = wts.w_conv_in("controlnet_cond_embedding.weight", C0, cc + 1);
    const float* be = wts.w_f32("controlnet_cond_embedding.bias", C0);
    const float* bi = wts.w_f32("conv_in.bias", C0);
    bf16* xp = x.ptr; const int Fn = F, Hn = H, Wn = W;
    if (cfg.set_noisy_sample_input_to_zero) {
      emit([=, this](hipStream_t s) {
        LAUNCH_OK(nr_launch_conv_in_small(io.cond, io.mask, cc, 1, io.cond_batch, nimg, Fn, Hn, Wn, wTe, be, bi, C0, xp, 1.f, 0.f, s));
      });
    } else {
      const float* wT = wts.w_conv_in("conv_in.weight", C0, cfg.in_channels);
      Act x2 = new_act(nimg, H, W, C0);
      bf16* x2p = x2.ptr; const int ic = cfg.in_channels, b2n = B2;
      const long long n = (long long)nimg * H * W * C0;
      emit([=, this](hipStream_t s) {
        LAUNCH_OK(nr_launch_conv_in_small(io.sample, nullptr, ic, 0, b2n, nimg, Fn, Hn, Wn, wT, bi, nullptr, C0, xp, 1.f, 0.f, s));
        LAUNCH_OK(nr_launch_conv_in_small(io.cond, io.mask, cc, 1, io.cond_batch, nimg, Fn, Hn, Wn, wTe, be, nullptr, C0, x2p, 1.f, 0.f, s));
        LAUNCH_OK(nr_launch_add_bf16(xp, x2p, xp, n, s));
      });
    }
  }
  tap("conv_in", x);

  // ---- down blocks ----
  std::vector<Act> skips;
  skips.push_back(cfg_half ? expand_cfg(x) : x);          // skip connections are full-batch (the ControlNet residuals added to them differ per half)
  for (int i = 0; i < L; ++i) {
    const int Cout = cfg.block_out_channels[i];
    const std::string bp = "down_blocks." + std::to_string(i);
    for (int j = 0; j < cfg.layers_per_block; ++j) {
      if (i == 0 && j == 0 && nd > 0) {
        // reduce -> resnet + attention on B2 x nd frame-images -> broadcast
        const long long fe = (long long)x.H * x.W * x.C;
        Act xr = new_act(B2 * nd, x.H, x.W, x.C);
        {
          const bf16* sp = x.ptr; bf16* dp = xr.ptr; const int b2n = B2, Fs = F, Fd = nd;
          std::vector<int> mp(fmap_reduce, fmap_reduce + nd);
          emit([=](hipStream_t s) { LAUNCH_OK(nr_launch_frame_gather(sp, dp, b2n, Fs, Fd, fe, mp.data(), s)); });
        }
        const int Fsave = F;
        F = nd;                                           // rows per sample (time-embedding row vector, context per sample) follow the reduced set
        xr = resnet(xr, nullptr, bp + ".resnets.0", Cout);
        if (cfg.down_block_has_attn[0]) xr = spatial_transformer(xr, ctx_bf, bp + ".attentions.0");
        F = Fsave;
        Act xe = new_act(nimg, xr.H, xr.W, xr.C);
        {
          const long long fe2 = (long long)xr.H * xr.W * xr.C;
          const bf16* sp = xr.ptr; bf16* dp = xe.ptr; const int b2n = B2, Fs = nd, Fd = F;
          std::vector<int> mp(fmap_expand, fmap_expand + F);
          emit([=](hipStream_t s) { LAUNCH_OK(nr_launch_frame_gather(sp, dp, b2n, Fs, Fd, fe2, mp.data(), s)); });
        }
        x = xe;
        x = temporal_module(x, bp + ".motion_modules.0");
        skips.push_back(x);
        continue;
      }
      x = resnet(x, nullptr, bp + ".resnets." + std::to_string(j), Cout);
      if (cfg.down_block_has_attn[i]) x = spatial_transformer(x, ctx_bf, bp + ".attentions." + std::to_string(j), 1, cfg_half && i == 0 && j == 0);
      if (cfg.use_motion_module) x = temporal_module(x, bp + ".motion_modules." + std::to_string(j));
      skips.push_back(x);
    }
    if (i != L - 1) {
      GemmOpt o; o.bias = wts.w_f32(bp + ".downsamplers.0.conv.bias", Cout);
      x = conv(x, nullptr, wts.w_conv3(bp + ".downsamplers.0.conv.weight", Cout, Cout), Cout, 3, 2, 0, o);
      tap(bp + ".downsamplers.0", x);
      skips.push_back(x);
    }
  }
  n_res = (int)skips.size();
  res_shapes.clear();
  for (auto& s : skips) res_shapes.push_back(ResShape{s.C, s.H, s.W});

  // ---- mid block (unet_blocks.py:271-278) ----
  Act mid_in = x;
  {
    const int Cm = cfg.block_out_channels[L - 1];
    x = resnet(x, nullptr, "mid_block.resnets.0", Cm);
    x = spatial_transformer(x, ctx_bf, "mid_block.attentions.0");
    if (cfg.use_motion_module && cfg.motion_module_mid_block) x = temporal_module(x, "mid_block.motion_modules.0");
    x = resnet(x, nullptr, "mid_block.resnets.1", Cm);
  }
  res_shapes.push_back(ResShape{x.C, x.H, x.W});
  mid_in = Act();

  if (cfg.kind == NR_KIND_SPARSECTRL) {
    // ---- zero-conv heads (sparse_controlnet.py:551-566): 1x1 conv, * conditioning_scale ----
    for (int i = 0; i <= n_res; ++i) {
      const bool is_mid = i == n_res;
      const Act& src = is_mid ? x : skips[i];
      const std::string key = is_mid ? std::string("controlnet_mid_block") : "controlnet_down_blocks." + std::to_string(i);
      const bf16* w = wts.w_linear(key + ".weight", src.C, src.C);
      const float* bias = wts.w_f32(key + ".bias", src.C);
      NrGemmParams p = nr_gemm_params(src.ptr, src.C, src.ld, nullptr, 0, 0, src.nimg, src.H, src.W, 1, 1, 0, w, src.C, bias, nullptr, 0, nullptr, src.C);   // out: at launch
      p.plan_m = det_batch ? (int)det_rows(p.M) : 0;
      NrGemmRoute r;                     // the epilogue scale arrives at launch: only the kernels that take any
      LAUNCH_OK(nr_gemm_route_rowmajor(&p, &r));
      const SplitK sk = splitk_scratch(r.ws_bytes);
      float* ws = sk.ws;
      emit([this, p, r, i, is_mid, ws](hipStream_t s) {
        NrGemmParams q = p;
        q.out = (bf16*)(is_mid ? io.out_mid : io.out_down[i]);
        q.out_scale = io.scale;
        LAUNCH_OK(nr_launch_gemm(&q, &r, q.w, ws, s));
      }, NR_PROF_IGEMM, 2.0 * p.M * (double)p.N * p.K, 2.0 * (2.0 * p.M * (double)p.N + (double)p.N * p.K));
    }
    return;
  }

  // ---- ControlNet residual adds (unet.py:422-428,436-439).  Everything above is independent of the ControlNet,
  // so segment 0 can run concurrently with it (nr_denoise_step_forward) ----
  split_op = ops.size();
  {
    // all skips but the last have already been consumed by their successor layer -> add in place; the last one is also the
    // mid-block input, which must stay un-added: it was consumed above, so in place is safe too.  One launch for all of them
    // (12 skips + the mid-block output) when every size is a multiple of 8 elements, else one launch each.
    struct AddT { bf16* dst; long long n; };
    std::vector<AddT> adds;
    for (int i = 0; i < n_res; ++i) adds.push_back(AddT{skips[i].ptr, (long long)skips[i].rows() * skips[i].C});
    adds.push_back(AddT{x.ptr, (long long)x.rows() * x.C});
    bool multi = (int)adds.size() <= 16;
    for (auto& a : adds) multi = multi && a.n % 8 == 0;
    if (multi) {
      NrAddMulti am;
      std::memset(&am, 0, sizeof(am));
      long long acc = 0;
      for (size_t i = 0; i < adds.size(); ++i) { am.dst[i] = adds[i].dst; acc += adds[i].n / 8; am.n8_end[i] = acc; }
      am.count = (int)adds.size();
      const int nr = n_res;
      emit([this, am, nr](hipStream_t st) {
        if (!io.has_res) return;
        NrAddMulti q = am;
        for (int i = 0; i < nr; ++i) q.src[i] = (const bf16*)io.down_res[i];
        q.src[nr] = (const bf16*)io.mid_res;
        LAUNCH_OK(nr_launch_add_bf16_multi(&q, st));
      });
    } else {
      for (int i = 0; i < n_res; ++i) {
        bf16* sp = adds[i].dst; const long long n = adds[i].n;
        emit([this, sp, n, i](hipStream_t st) {
          if (io.has_res) LAUNCH_OK(nr_launch_add_bf16(sp, (const bf16*)io.down_res[i], sp, n, st));
        });
      }
      bf16* xp = x.ptr; const long long n = adds.back().n;
      emit([this, xp, n](hipStream_t st) {
        if (io.has_res) LAUNCH_OK(nr_launch_add_bf16(xp, (const bf16*)io.mid_res, xp, n, st));
      });
    }
  }
  split_op2 = ops.size();

  // ---- up blocks (unet_blocks.py:621-667,735-760) ----
  for (int i = 0; i < L; ++i) {
    const int Cout = cfg.block_out_channels[L - 1 - i];
    const std::string bp = "up_blocks." + std::to_string(i);
    for (int j = 0; j < cfg.layers_per_block + 1; ++j) {
      Act skip = skips.back();
      skips.pop_back();
      x = resnet(x, &skip, bp + ".resnets." + std::to_string(j), Cout);
      skip = Act();
      if (cfg.up_block_has_attn[i]) x = spatial_transformer(x, ctx_bf, bp + ".attentions." + std::to_string(j));
      if (cfg.use_motion_module) x = temporal_module(x, bp + ".motion_modules." + std::to_string(j));
    }
    if (i != L - 1) {
      GemmOpt o; o.bias = wts.w_f32(bp + ".upsamplers.0.conv.bias", Cout);
      x = upsample_conv(x, bp + ".upsamplers.0.conv.weight", Cout, o);
      tap(bp + ".upsamplers.0", x);
    }
  }

  // ---- out (unet.py:468-470) ----
  Act hn = groupnorm(x, nullptr, "conv_norm_out", cfg.norm_eps, 1);
  {
    const bf16* wo = wts.w_conv3("conv_out.weight", cfg.out_channels, C0);
    const float* bo = wts.w_f32("conv_out.bias", cfg.out_channels);
    const bf16* hp = hn.ptr; const int Fn = F, Hn = H, Wn = W, oc = cfg.out_channels;
    emit([=, this](hipStream_t s) { LAUNCH_OK(nr_launch_conv_out_small(hp, C0, nimg, Fn, Hn, Wn, wo, bo, oc, io.out, 1.f, 0.f, 0, s)); });
  }
}

void nr_net::plan(int batch, int frames, int h, int w, int ctxl) {
  const bool leaf = cfg.kind == NR_KIND_LEAF_TRANSFORMER3D || cfg.kind == NR_KIND_LEAF_TEMPORAL;
  const bool vae = cfg.kind == NR_KIND_VAE_DECODER || cfg.kind == NR_KIND_VAE_ENCODER || cfg.kind == NR_KIND_CLIP_TEXT || cfg.kind == NR_KIND_LEAF_TEMPORAL;
  if (batch <= 0 || batch > NR_MAX_BATCH || frames <= 0 || h <= 0 || w <= 0 || (ctxl <= 0 && !vae)) throw NrError(NR_ERR_ARG, "plan: bad shape");
  const int down = (cfg.kind == NR_KIND_VAE_DECODER || cfg.kind == NR_KIND_CLIP_TEXT || leaf) ? 1 : 1 << (cfg.num_levels - 1);
  if (h % down != 0 || w % down != 0)
    throw NrError(NR_ERR_ARG, "plan: latent h,w must be multiples of " + std::to_string(down));
  HIP_OK(hipDeviceSynchronize());
  drop_graphs();
  B2 = batch; F = frames; H = h; W = w; ctx_len = ctxl;
  planned = false;
  // pass 1: sizes only
  dry = true;
  char* old = arena_base; arena_base = nullptr;
  main_high = 0;
  try { build(); }
  catch (...) { dry = false; arena_base = old; throw; }      // a shape the network rejects: keep (and later free) the arena of the previous plan
  main_high = Arena::align(arena.high + 256);
  const size_t need_bytes = main_high + parena.high + 256;
  dry = false;
  arena_base = old;
  if (need_bytes > arena_bytes) {
    if (arena_base) { HIP_OK(hipFree(arena_base)); arena_base = nullptr; }
    HIP_OK(hipMalloc((void**)&arena_base, need_bytes));
    arena_bytes = need_bytes;
  }
  // pass 2: real pointers, weights uploaded
  split_op = 0; split_op2 = 0;
  prefetch_valid = false;
  build();
  if (split_op == 0 || split_op > ops.size()) split_op = ops.size();
  if (split_op2 < split_op || split_op2 > ops.size()) split_op2 = ops.size();
  HIP_OK(hipDeviceSynchronize());
  planned = true;
}
