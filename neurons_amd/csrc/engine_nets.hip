// The networks of the engine (engine.h) as launch plans over the emitters of engine_layers.hip, and the two-pass planner.  The plans follow the
// reference module graphs:
//   UNet3DConditionModel.forward        animatediff/models/unet.py:357-475
//   SparseControlNetModel.forward       animatediff/models/sparse_controlnet.py:467-581
//   Cross/Down/Mid/Up blocks            animatediff/models/unet_blocks.py:271-278,382-421,493-521,621-667,735-760
// Host code only.
#include "engine.h"

using namespace nre;

// ------------------------------------------------------------------ emitters the networks share
// The 4-channel stem as a launch: the 3x3 conv <key> of fp32 planes into `out` (+ the vector `addend_key`).  The caller emits it, alone or as one of an op's launches
std::function<void(hipStream_t)> nr_net::stem(const StemIn& in, const std::string& key, const Act& out, const char* addend_key) {
  const bool cond = in.from == StemIn::COND;
  const float* wT = wts.w_conv_in(key + ".weight", out.C, in.C + cond);
  const float* bias = wts.w_f32(key + ".bias", out.C);
  const float* addend = addend_key ? wts.w_f32(addend_key, out.C) : nullptr;
  bf16* op = out.ptr; const int nimg = out.nimg, Fn = F, Hn = out.H, Wn = out.W, Cout = out.C;
  return [=, this](hipStream_t s) {
    const float* src = in.from == StemIn::BUFFER ? in.buf : cond ? io.cond : io.sample;
    LAUNCH_OK(nr_launch_conv_in_small(src, cond ? io.mask : nullptr, in.C, cond, cond ? io.cond_batch : in.batch, nimg, Fn, Hn, Wn, wT, bias, addend, Cout, op,
                                      in.affine ? io.in_scale : 1.f, in.affine ? io.in_shift : 0.f, s));
  };
}

// GroupNorm + SiLU -> the 3x3 conv <conv> to a few fp32 planes: io.out, with the image post-scaling of io (1, 0, off unless the VAE decoder's entry point
// sets it).  With `quant` (the VAE encoder's moments) the conv writes a scratch that the 1x1 conv <quant> maps to io.out: ONE op of two launches
void nr_net::head(const Act& x, const std::string& norm, const std::string& conv, int Cout, const char* quant) {
  Act hn = groupnorm(x, nullptr, norm, cfg.norm_eps, 1);
  const int Cin = x.C, nimg = x.nimg, Fn = F, Hn = x.H, Wn = x.W;
  float* raw = quant ? new_scratch<float>((size_t)nimg * Cout * Hn * Wn) : nullptr;
  const bf16* wo = wts.w_conv3(conv + ".weight", Cout, Cin);
  const float* bo = wts.w_f32(conv + ".bias", Cout);
  const float* Q = quant ? wts.w_f32(std::string(quant) + ".weight", {Cout, Cout}) : nullptr;
  const float* qb = quant ? wts.w_f32(std::string(quant) + ".bias", Cout) : nullptr;
  const bf16* hp = hn.ptr;
  emit([=, this](hipStream_t s) {
    LAUNCH_OK(nr_launch_conv_out_small(hp, Cin, nimg, Fn, Hn, Wn, wo, bo, Cout, raw ? raw : io.out, raw ? 1.f : io.out_mul, raw ? 0.f : io.out_add, raw ? 0 : io.clamp01, s));
    if (raw) LAUNCH_OK(nr_launch_post_quant(raw, 1.f, Q, qb, io.out, nimg, Cout, Hn * Wn, s));
  });
}

// 3x3 stride-2 conv <key> (C -> C) and its tap; pad_tl0: the VAE's Downsample, which pads bottom / right only (model.py:84-91)
Act nr_net::downsample_conv(const Act& x, const std::string& key, const std::string& tap_name, int pad_tl0) {
  GemmOpt o; o.bias = wts.w_f32(key + ".bias", x.C); o.pad_tl0 = pad_tl0;
  Act y = conv(x, nullptr, wts.w_conv3(key + ".weight", x.C, x.C), x.C, 3, 2, 0, o);
  tap(tap_name, y);
  return y;
}

// emb = <l2>(SiLU(<l1>(sinusoid(t)))) (unet.py:371-392) [+ the label branch <label>.0 / <label>.2 on io.y (openaimodel.py:836-841)]; every ResBlock then applies
// Linear(SiLU(emb)) (resnet.py:191, openaimodel.py:283-289): SiLU(emb) is stored once and the Linears `layer` of all temb_slots run as ONE launch into temb_all
void nr_net::time_embedding(const std::string& l1, const std::string& l2, const char* label, const std::string& tag, const std::string& layer) {
  const int C0 = cfg.block_out_channels[0], temb_dim = 4 * C0, adm = cfg.adm_in_channels;
  const bool labelled = label != nullptr;
  float* sincos = new_scratch<float>((size_t)B2 * C0);
  float* e1 = new_scratch<float>((size_t)B2 * temb_dim);
  float* et = labelled ? new_scratch<float>((size_t)B2 * temb_dim) : nullptr;
  float* y1 = labelled ? new_scratch<float>((size_t)B2 * temb_dim) : nullptr;
  float* emb = new_scratch<float>((size_t)B2 * temb_dim);
  temb_all = new_scratch<float>((size_t)B2 * temb_total);
  const bf16* w1 = wts.w_linear(l1 + ".weight", temb_dim, C0);
  const float* b1 = wts.w_f32(l1 + ".bias", temb_dim);
  const bf16* w2 = wts.w_linear(l2 + ".weight", temb_dim, temb_dim);
  const float* b2 = wts.w_f32(l2 + ".bias", temb_dim);
  const std::string lb = labelled ? label : "";
  const bf16* wy1 = labelled ? wts.w_linear(lb + ".0.weight", temb_dim, adm) : nullptr;
  const float* by1 = labelled ? wts.w_f32(lb + ".0.bias", temb_dim) : nullptr;
  const bf16* wy2 = labelled ? wts.w_linear(lb + ".2.weight", temb_dim, temb_dim) : nullptr;
  const float* by2 = labelled ? wts.w_f32(lb + ".2.bias", temb_dim) : nullptr;
  const auto proj = wts.w_temb_projection(tag, temb_slots, layer, temb_dim);
  const bf16* wp = proj.w; const float* bp = proj.b;
  float* td = t_dev; float* ta = temb_all;
  const int b2n = B2, tt = temb_total;
  emit([=, this](hipStream_t s) {
    LAUNCH_OK(nr_launch_timestep_sincos(td, b2n, C0, sincos, s));
    LAUNCH_OK(nr_launch_linear_small(sincos, b2n, C0, w1, b1, temb_dim, 0, 1, e1, nullptr, s));          // Linear + SiLU
    if (labelled) {
      LAUNCH_OK(nr_launch_linear_small(e1, b2n, temb_dim, w2, b2, temb_dim, 0, 0, et, nullptr, s));
      LAUNCH_OK(nr_launch_linear_small(io.y, b2n, adm, wy1, by1, temb_dim, 0, 1, y1, nullptr, s));
      LAUNCH_OK(nr_launch_linear_small(y1, b2n, temb_dim, wy2, by2, temb_dim, 0, 1, emb, et, s));         // SiLU(time + label)
    } else {
      LAUNCH_OK(nr_launch_linear_small(e1, b2n, temb_dim, w2, b2, temb_dim, 0, 1, emb, nullptr, s));      // SiLU(emb)
    }
    LAUNCH_OK(nr_launch_linear_small(emb, b2n, temb_dim, wp, bp, tt, 0, 0, ta, nullptr, s));              // Linear(SiLU(emb)) of every ResBlock
  });
  last_op_launches(labelled ? 6 : 4);
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
  const SgmLayout lay = sgm_layout();
  begin_plan();
  for (auto& b : lay.in) if (b.kind == 1) add_temb_slot("input_blocks." + std::to_string(b.idx) + ".0", b.Cout);
  add_temb_slot("middle_block.0", cfg.block_out_channels[L - 1]);
  add_temb_slot("middle_block.2", cfg.block_out_channels[L - 1]);
  for (auto& b : lay.out) add_temb_slot("output_blocks." + std::to_string(b.idx) + ".0", b.Cout);
  time_embedding("time_embed.0", "time_embed.2", "label_emb.0", "sgm", ".emb_layers.1");
  // ---- context fp32 -> bf16 ----
  Act ctx_bf = stage_context();
  // ---- input blocks ----
  std::vector<Act> hs;
  Act x;
  for (auto& b : lay.in) {
    const std::string bp = "input_blocks." + std::to_string(b.idx);
    if (b.kind == 0) {
      x = new_act(B2, H, W, C0);
      emit(stem(StemIn{StemIn::SAMPLE, cfg.in_channels, B2, nullptr, true}, bp + ".0", x));      // x * c_in(sigma)
      tap(bp, x);
    } else if (b.kind == 1) {
      x = resnet(x, nullptr, bp + ".0", b.Cout);
      if (cfg.down_block_has_attn[b.level]) x = spatial_transformer(x, ctx_bf, bp + ".1", cfg.transformer_depth[b.level]);
    } else {
      x = downsample_conv(x, bp + ".0.op", bp);
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
  head(x, "out.0", "out.2", cfg.out_channels);      // GroupNorm32 -> SiLU -> conv (openaimodel.py:809-813)
}

// AutoencodingEngineLegacy.decode (sgm/models/autoencoder.py:490-494) = post_quant_conv -> Decoder.forward
// (sgm/modules/diffusionmodules/model.py:723-757).  Same network as diffusers AutoencoderKL.decode used by
// decode_latents (pipeline_animation.py:243-256) under different parameter names.
void nr_net::build_vae() {
  const int L = cfg.num_levels, zc = cfg.in_channels, nimg = B2;
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
  emit(stem(StemIn{StemIn::BUFFER, zc, nimg, zq}, "decoder.conv_in", x));
  tap("decoder.conv_in", x);
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
  head(x, "decoder.norm_out", "decoder.conv_out", cfg.out_channels);
}

// AutoencodingEngine.encode up to the moments (sgm/models/autoencoder.py:468-488): Encoder.forward
// (sgm/modules/diffusionmodules/model.py:584-609) -> quant_conv.  == diffusers AutoencoderKL.encode(x).latent_dist
// parameters (scripts/neuroclips_video.py:267,282).  Plan h, w are the IMAGE size; moments are [n][2z][h/8][w/8].
void nr_net::build_vae_enc() {
  const int L = cfg.num_levels;
  begin_plan();
  Act x = new_act(B2, H, W, cfg.block_out_channels[0]);
  emit(stem(StemIn{StemIn::SAMPLE, cfg.in_channels, B2, nullptr, true}, "encoder.conv_in", x));      // x * in_scale + in_shift
  tap("encoder.conv_in", x);
  for (int lev = 0; lev < L; ++lev) {
    const int Co = cfg.block_out_channels[lev];
    const std::string dn = "encoder.down." + std::to_string(lev);
    for (int j = 0; j < cfg.layers_per_block; ++j) x = resnet(x, nullptr, dn + ".block." + std::to_string(j), Co);
    if (lev != L - 1) x = downsample_conv(x, dn + ".downsample.conv", dn + ".downsample", 1);
  }
  const int Cm = cfg.block_out_channels[L - 1];
  x = resnet(x, nullptr, "encoder.mid.block_1", Cm);
  x = vae_attn(x, "encoder.mid.attn_1");
  x = resnet(x, nullptr, "encoder.mid.block_2", Cm);
  head(x, "encoder.norm_out", "encoder.conv_out", cfg.out_channels, "quant_conv");
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
// sized for cond_batch = B2), never per CFG / grouped sample, and with the identical-frame evaluation active (fd.n() > 0) only on the distinct
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
void nr_net::cond_embedding(Act& x, const FrameDedup& fd) {
  const int L = cfg.cond_embedding_levels, C0 = cfg.block_out_channels[0], cc = cfg.conditioning_channels;
  const int* ch = cfg.cond_embedding_channels;
  const int Hc = H << (L - 1), Wc = W << (L - 1), Fn = F;
  const int Fe = fd.n() > 0 ? fd.n() : F;
  std::vector<int> fsel = fd.reduce, emap = fd.expand;      // all frames, each its own, unless the identical-frame evaluation is active
  if (fd.n() == 0) { fsel.resize(F); emap.resize(F); for (int f = 0; f < F; ++f) fsel[f] = emap[f] = f; }
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
  Act x2;                                     // conv_in(sample), when the noisy sample is not zeroed
  std::function<void(hipStream_t)> conv_in;
  if (!zero_sample) {
    x2 = new_act(B2 * F, H, W, C0);
    conv_in = stem(StemIn{StemIn::SAMPLE, cfg.in_channels, B2}, "conv_in", x2);
  }
  const bf16* x2p = x2.ptr;
  emit([=, this](hipStream_t s) {
    if (conv_in) conv_in(s);
    LAUNCH_OK(nr_launch_condembed_bcast(ep, io.cond_batch, Fe, emap.data(), b2n, Fn, img, x2p, xp, s));
  }, NR_PROF_OTHER, zero_sample ? 0.0 : 2.0 * B2 * F * H * W * C0 * 9.0 * cfg.in_channels, (zero_sample ? 4.0 : 6.0) * B2 * F * img, d);
  if (!zero_sample) last_op_launches(2);
}

// SparseCtrl identical-frame evaluation (see n_cond_frames): the distinct frames = the conditioned ones + one representative of the rest.  Empty = off
nr_net::FrameDedup nr_net::identical_frames() const {
  FrameDedup d;
  if (cfg.kind != NR_KIND_SPARSECTRL || !cfg.set_noisy_sample_input_to_zero || !cfg.use_motion_module || n_cond_frames < 0 || keep_all || F > 64) return d;
  int rep = -1;
  for (int f = 0; f < F && rep < 0; ++f) {
    bool is_c = false;
    for (int k = 0; k < n_cond_frames; ++k) is_c = is_c || cond_frames[k] == f;
    if (!is_c) rep = f;
  }
  for (int k = 0; k < n_cond_frames; ++k) if (cond_frames[k] < F) d.reduce.push_back(cond_frames[k]);
  const int nc = d.n();
  if (rep < 0 || nc + 1 >= F) return FrameDedup();
  d.reduce.push_back(rep);
  d.expand.assign(F, nc);
  for (int f = 0; f < F; ++f)
    for (int k = 0; k < nc; ++k) if (d.reduce[k] == f) d.expand[f] = k;
  return d;
}
// y[b][j] = x[b][map[j]]: frames of each sample picked by a map (Fs frames per sample in x)
Act nr_net::frame_gather(const Act& x, int Fs, const std::vector<int>& map) {
  const int Fd = (int)map.size(), b2n = B2;
  Act y = new_act(B2 * Fd, x.H, x.W, x.C);
  const long long fe = (long long)x.H * x.W * x.C;
  const bf16* sp = x.ptr; bf16* dp = y.ptr;
  emit([=](hipStream_t s) { LAUNCH_OK(nr_launch_frame_gather(sp, dp, b2n, Fs, Fd, fe, map.data(), s)); });
  return y;
}

// What the U-Net and SparseCtrl share (unet.py:371-434, sparse_controlnet.py:475-549): time embedding, text context, conv_in, down blocks, mid block.
// Leaves n_res / res_shapes filled
nr_net::Trunk nr_net::down_mid() {
  const int L = cfg.num_levels;
  const int C0 = cfg.block_out_channels[0];
  const int nimg = B2 * F;
  begin_plan();
  // every resnet in definition order: its slice of the batched time-embedding projection
  for (int i = 0; i < L; ++i)
    for (int j = 0; j < cfg.layers_per_block; ++j)
      add_temb_slot("down_blocks." + std::to_string(i) + ".resnets." + std::to_string(j), cfg.block_out_channels[i]);
  add_temb_slot("mid_block.resnets.0", cfg.block_out_channels[L - 1]);
  add_temb_slot("mid_block.resnets.1", cfg.block_out_channels[L - 1]);
  if (cfg.kind == NR_KIND_UNET3D)
    for (int i = 0; i < L; ++i)
      for (int j = 0; j < cfg.layers_per_block + 1; ++j)
        add_temb_slot("up_blocks." + std::to_string(i) + ".resnets." + std::to_string(j), cfg.block_out_channels[L - 1 - i]);
  time_embedding("time_embedding.linear_1", "time_embedding.linear_2", nullptr, std::to_string(cfg.kind), ".time_emb_proj");
  Trunk t;
  t.ctx = stage_context();      // text context fp32 -> bf16 [B2*ctx_len][cross_dim]
  const FrameDedup fd = identical_frames();

  // ---- conv_in ----
  const bool cfg_half = cfg_dedup_active();      // conv_in .. attn1 of the first transformer on the first half of the batch only
  Act x = new_act(cfg_half ? nimg / 2 : nimg, H, W, C0);
  const StemIn sample{StemIn::SAMPLE, cfg.in_channels, cfg_half ? B2 / 2 : B2};
  if (cfg.kind == NR_KIND_UNET3D) {
    emit(stem(sample, "conv_in", x));
  } else if (cfg.cond_embedding_levels > 0) {
    cond_embedding(x, fd);
  } else {
    // sparse_controlnet.py:467-521: conv_in(sample) + controlnet_cond_embedding(cat[cond, mask]); sample := 0 -> conv_in(0) = its bias, added by the one launch
    const StemIn cond{StemIn::COND, cfg.conditioning_channels, 0};
    if (cfg.set_noisy_sample_input_to_zero) {
      emit(stem(cond, "controlnet_cond_embedding", x, "conv_in.bias"));
    } else {
      Act x2 = new_act(nimg, H, W, C0);
      const auto embed = stem(cond, "controlnet_cond_embedding", x2);
      wts.w_f32("conv_in.bias", C0);      // converted before conv_in.weight, as in the zeroed form: the order of the uploads is part of the plan
      const auto conv_in = stem(sample, "conv_in", x);
      bf16* xp = x.ptr; const bf16* x2p = x2.ptr;
      const long long n = (long long)nimg * H * W * C0;
      emit([=](hipStream_t s) { conv_in(s); embed(s); LAUNCH_OK(nr_launch_add_bf16(xp, x2p, xp, n, s)); });
    }
  }
  tap("conv_in", x);

  // ---- down blocks ----
  std::vector<Act>& skips = t.skips;
  skips.push_back(cfg_half ? expand_cfg(x) : x);          // skip connections are full-batch (the ControlNet residuals added to them differ per half)
  for (int i = 0; i < L; ++i) {
    const int Cout = cfg.block_out_channels[i];
    const std::string bp = "down_blocks." + std::to_string(i);
    for (int j = 0; j < cfg.layers_per_block; ++j) {
      if (i == 0 && j == 0 && fd.n() > 0) {
        // reduce -> resnet + attention on B2 x n frame-images -> broadcast
        Act xr = frame_gather(x, F, fd.reduce);
        const int Fsave = F;
        F = fd.n();                                       // rows per sample (time-embedding row vector, context per sample) follow the reduced set
        xr = resnet(xr, nullptr, bp + ".resnets.0", Cout);
        if (cfg.down_block_has_attn[0]) xr = spatial_transformer(xr, t.ctx, bp + ".attentions.0");
        F = Fsave;
        x = frame_gather(xr, fd.n(), fd.expand);
        x = temporal_module(x, bp + ".motion_modules.0");
        skips.push_back(x);
        continue;
      }
      x = resnet(x, nullptr, bp + ".resnets." + std::to_string(j), Cout);
      if (cfg.down_block_has_attn[i]) x = spatial_transformer(x, t.ctx, bp + ".attentions." + std::to_string(j), 1, cfg_half && i == 0 && j == 0);
      if (cfg.use_motion_module) x = temporal_module(x, bp + ".motion_modules." + std::to_string(j));
      skips.push_back(x);
    }
    if (i != L - 1) {
      x = downsample_conv(x, bp + ".downsamplers.0.conv", bp + ".downsamplers.0");
      skips.push_back(x);
    }
  }
  n_res = (int)skips.size();
  res_shapes.clear();
  for (auto& s : skips) res_shapes.push_back(ResShape{s.C, s.H, s.W});

  // ---- mid block (unet_blocks.py:271-278) ----
  const int Cm = cfg.block_out_channels[L - 1];
  x = resnet(x, nullptr, "mid_block.resnets.0", Cm);
  x = spatial_transformer(x, t.ctx, "mid_block.attentions.0");
  if (cfg.use_motion_module && cfg.motion_module_mid_block) x = temporal_module(x, "mid_block.motion_modules.0");
  x = resnet(x, nullptr, "mid_block.resnets.1", Cm);
  res_shapes.push_back(ResShape{x.C, x.H, x.W});
  t.x = x;
  return t;
}

// SparseControlNetModel.forward: the trunk, then the zero-conv heads (sparse_controlnet.py:551-566): 1x1 conv, * conditioning_scale
void nr_net::build_sparsectrl() {
  const Trunk t = down_mid();
  for (int i = 0; i <= n_res; ++i) {
    const bool is_mid = i == n_res;
    const Act& src = is_mid ? t.x : t.skips[i];
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
}

// ControlNet residual adds (unet.py:422-428,436-439): segment 1 of the plan.  Everything before them is independent of the ControlNet, so segment 0 can run
// concurrently with it (nr_denoise_step_forward)
void nr_net::residual_adds(const Trunk& t) {
  split_op = ops.size();
  // all skips but the last have already been consumed by their successor layer -> add in place; the last one is also the
  // mid-block input, which must stay un-added: it was consumed above, so in place is safe too.  One launch for all of them
  // (12 skips + the mid-block output) when every size is a multiple of 8 elements, else one launch each.
  struct AddT { bf16* dst; long long n; };
  std::vector<AddT> adds;
  for (int i = 0; i < n_res; ++i) adds.push_back(AddT{t.skips[i].ptr, (long long)t.skips[i].rows() * t.skips[i].C});
  adds.push_back(AddT{t.x.ptr, (long long)t.x.rows() * t.x.C});
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
    for (int i = 0; i <= n_res; ++i) {      // the last one: the mid-block output
      bf16* dp = adds[i].dst; const long long n = adds[i].n; const bool is_mid = i == n_res;
      emit([this, dp, n, i, is_mid](hipStream_t st) {
        if (io.has_res) LAUNCH_OK(nr_launch_add_bf16(dp, (const bf16*)(is_mid ? io.mid_res : io.down_res[i]), dp, n, st));
      });
    }
  }
  split_op2 = ops.size();
}

// UNet3DConditionModel.forward: the trunk, the residual adds, then the up blocks (unet_blocks.py:621-667,735-760) and conv_norm_out -> SiLU -> conv_out (unet.py:468-470)
void nr_net::build_unet3d() {
  Trunk t = down_mid();
  residual_adds(t);
  Act x = t.x;
  t.x = Act();
  const int L = cfg.num_levels;
  for (int i = 0; i < L; ++i) {
    const int Cout = cfg.block_out_channels[L - 1 - i];
    const std::string bp = "up_blocks." + std::to_string(i);
    for (int j = 0; j < cfg.layers_per_block + 1; ++j) {
      Act skip = t.skips.back();
      t.skips.pop_back();
      x = resnet(x, &skip, bp + ".resnets." + std::to_string(j), Cout);
      skip = Act();
      if (cfg.up_block_has_attn[i]) x = spatial_transformer(x, t.ctx, bp + ".attentions." + std::to_string(j));
      if (cfg.use_motion_module) x = temporal_module(x, bp + ".motion_modules." + std::to_string(j));
    }
    if (i != L - 1) {
      GemmOpt o; o.bias = wts.w_f32(bp + ".upsamplers.0.conv.bias", Cout);
      x = upsample_conv(x, bp + ".upsamplers.0.conv.weight", Cout, o);
      tap(bp + ".upsamplers.0", x);
    }
  }
  head(x, "conv_norm_out", "conv_out", cfg.out_channels);
}

void nr_net::build() {
  switch (cfg.kind) {
    case NR_KIND_UNET3D: return build_unet3d();
    case NR_KIND_SPARSECTRL: return build_sparsectrl();
    case NR_KIND_SGM_UNET: return build_sgm();
    case NR_KIND_VAE_DECODER: return build_vae();
    case NR_KIND_VAE_ENCODER: return build_vae_enc();
    case NR_KIND_CLIP_TEXT: return build_clip();
    default: return build_leaf();      // NR_KIND_LEAF_TRANSFORMER3D / _TEMPORAL
  }
}

// What plan() has to know of a network kind: whether it reads a text context; whether h, w are halved levels - 1 times on the way down (they must divide);
// for a 2-D network, the error text of a plan with frames != 1 (seq: or h != 1)
struct KindFacts { bool ctx, down; const char* two_d; bool seq; };
static constexpr KindFacts kind_facts(int kind) {
  switch (kind) {
    case NR_KIND_SGM_UNET: return {true, true, "sgm UNetModel is a 2-D network: plan with frames = 1", false};
    case NR_KIND_VAE_DECODER: return {false, false, "the VAE decoder is a 2-D network: plan with frames = 1", false};
    case NR_KIND_VAE_ENCODER: return {false, true, "the VAE encoder is a 2-D network: plan with frames = 1", false};
    case NR_KIND_CLIP_TEXT: return {false, false, "CLIP text encoder: plan with frames = 1, h = 1, w = sequence length", true};
    case NR_KIND_LEAF_TRANSFORMER3D: return {true, false, nullptr, false};
    case NR_KIND_LEAF_TEMPORAL: return {false, false, nullptr, false};
    default: return {true, true, nullptr, false};      // the U-Net and SparseCtrl
  }
}

void nr_net::plan(int batch, int frames, int h, int w, int ctxl) {
  const KindFacts kind = kind_facts(cfg.kind);
  if (batch <= 0 || batch > NR_MAX_BATCH || frames <= 0 || h <= 0 || w <= 0 || (ctxl <= 0 && kind.ctx)) throw NrError(NR_ERR_ARG, "plan: bad shape");
  const int down = kind.down ? 1 << (cfg.num_levels - 1) : 1;
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
  try {
    if (kind.two_d && (F != 1 || (kind.seq && H != 1))) throw NrError(NR_ERR_ARG, kind.two_d);
    build();
  } catch (...) { dry = false; arena_base = old; throw; }      // a shape the network rejects: keep (and later free) the arena of the previous plan
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
