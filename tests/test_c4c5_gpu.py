"""GPU parity at the two BASELINE configurations that round 2 only ever ran through bench.py:

  C4  one GPU's share of "8 clips per GPU, enhance mode": EIGHT clips in ONE pipeline call at full SD-1.5 width, (8,4,16,32,32) latents,
      SparseCtrl on (grouped schedule kept at B = 8: 4 DDIM steps x 16 CFG samples = 64 samples per evaluation), CFG 8.5, 12 DDIM steps:
      batched call vs 8 independent B = 1 calls, and clips 0 and 7 vs the fp32 oracle.
      Reference semantics: a batch of clips == B independent B = 1 calls (sparse_controlnet.py:490-521 only broadcasts a batch-1
      condition); scripts/neuroclips_video.py:206,238 run batch_size = 1 per rank.
  C5  "fp8 MFMA attention + 32-frame 512x512 clips": one evaluation of both full-width networks at (2*1,4,32,64,64) with
      temporal_position_encoding_max_len = 32 (motion_module.py:241-243 raises the reference's broadcast error beyond 24 otherwise),
      bf16 attention and the e4m3 variant, vs the fp32 oracle (its attention evaluated a slice of batch*heads at a time).

Stated tolerances: loop level PSNR >= 40 dB and rel-L2 <= 3e-2 vs the fp32 oracle (as test_fullsize_gpu.py); one evaluation
rel-L2 <= 2.5e-2 (bf16) / <= 6e-2 (e4m3 attention operands).  Batched vs independent clips: PSNR >= 40 dB and rel-L2 <= 5e-2 -- the SAME
bar as against fp32, because the two runs are two different bf16 roundings of the same arithmetic, not the same one: the tile plan and split-K
depth depend on M (fp32 summation order) and, more importantly, so does the per-shape choice between the LayerNorm folded into the GEMM and the
separate LayerNorm kernel (engine ln_linear: the 16x16 / 8x8-level q|k|v and GEGLU projections switch form between B = 1 and B = 8), which moves
a bf16 rounding point.  Measured round 3 (6 steps): 45.9-47.2 dB, rel-L2 3.4-4.1e-2 between the two; each is as close to the fp32 oracle."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from test_engine_gpu import metrics  # noqa: E402

LOOP_PSNR_DB, LOOP_REL_L2, FWD_REL_L2, FWD_REL_L2_FP8 = 40.0, 3e-2, 2.5e-2, 6e-2
BATCH_VS_SINGLE_DB, BATCH_VS_SINGLE_REL = 40.0, 5e-2


@pytest.fixture(scope="module")
def nets(cuda):
    """ONE pair of full-width networks for the module.  The U-Net is built with temporal_position_encoding_max_len = 32 (what 32-frame
    clips need); for the 16-frame C4 case that is the SAME network as the default 24 (the sinusoid table is a function of the position
    only, motion_module.py:225-239, and is regenerated at load)."""
    n = _nets(cuda, 32)
    yield n
    n["unet"].set_attention_fp8(False)
    n["ctrl"].set_attention_fp8(False)


def _nets(cuda, pe_max_len_unet):
    from neurons_amd import _lib, NativeSparseCtrl, NativeUNet3D
    from neurons_amd.sparsectrl import controlnet_config_from_unet
    from neurons_amd.synth import gpu_random_state_dict
    from neurons_amd.unet3d import UNet3DConfig, state_dict_schema
    from oracle import animatediff_oracle as O
    kw = {}
    if pe_max_len_unet != 24:
        kw["motion_module_kwargs"] = dict(UNet3DConfig().motion_module_kwargs, temporal_position_encoding_max_len=pe_max_len_unet)
    ucfg = UNet3DConfig(**kw)
    ccfg = controlnet_config_from_unet(ucfg, dict(
        set_noisy_sample_input_to_zero=True, use_simplified_condition_embedding=True, conditioning_channels=4,
        motion_module_kwargs=dict(attention_block_types=["Temporal_Self"], temporal_position_encoding_max_len=32)))
    usd = gpu_random_state_dict(state_dict_schema(ucfg, _lib.NR_KIND_UNET3D), 1, cuda)
    csd = gpu_random_state_dict(state_dict_schema(ccfg, _lib.NR_KIND_SPARSECTRL), 2, cuda)
    unet, ctrl = NativeUNet3D(ucfg).to(cuda), NativeSparseCtrl(ccfg).to(cuda)
    unet.auto_release_host_weights = False        # both handles are driven at several batch sizes here
    ctrl.auto_release_host_weights = False
    unet.load_state_dict({k: v.cpu() for k, v in usd.items()})
    ctrl.load_state_dict({k: v.cpu() for k, v in csd.items()})
    return dict(O=O, unet=unet, ctrl=ctrl, usd=usd, csd=csd, ou=O.OracleConfig.from_native(ucfg), oc=O.OracleConfig.from_native(ccfg),
                ucfg=ucfg)


def test_c4_eight_clips_per_call_full_width(cuda, nets):
    from neurons_amd import DDIMScheduler, NeuroclipsPipeline
    n = nets
    O = n["O"]
    sched = DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="linear", steps_offset=1, clip_sample=False)
    pipe = NeuroclipsPipeline(vae=None, text_encoder=None, tokenizer=None, unet=n["unet"], scheduler=sched, controlnet=n["ctrl"]).to(cuda)
    B, F, L, steps = 8, 16, 32, 12
    import time
    t0 = time.time()
    g = torch.Generator(device=cuda).manual_seed(1000)
    lat = torch.randn(B, 4, F, L, L, generator=g, device=cuda)
    noise = torch.randn(B, 4, F, L, L, generator=g, device=cuda)
    ctx_u = torch.randn(B, 77, n["ucfg"].cross_attention_dim, generator=g, device=cuda)
    ctx_t = torch.randn(B, 77, n["ucfg"].cross_attention_dim, generator=g, device=cuda)
    cimg = torch.randn(B, 4, 1, L, L, generator=g, device=cuda) * 0.18215
    kw = dict(video_length=F, height=L * 8, width=L * 8, num_inference_steps=steps, guidance_scale=8.5, controlnet_image_index=[0],
              low_strength=0.3, output_type="latent")
    both = pipe([""] * B, latents=lat, noise=noise, text_embeddings=torch.cat([ctx_u, ctx_t]), controlnet_images=cimg, **kw).videos.clone()
    assert pipe.last_controlnet_group == 4, "B = 8 must keep the grouped SparseCtrl schedule (12 steps: three groups of 4 x 16 samples)"
    print(f"[C4 timing] batched call {time.time() - t0:.1f} s")
    assert torch.isfinite(both).all()
    worst, worst_rel = 1e9, 0.0
    for i in range(B):
        one = pipe("", latents=lat[i:i + 1], noise=noise[i:i + 1], text_embeddings=torch.cat([ctx_u[i:i + 1], ctx_t[i:i + 1]]),
                   controlnet_images=cimg[i:i + 1], **kw).videos
        rel, psnr = metrics(f"C4: clip {i} of a batch of {B} vs the same clip alone", both[i:i + 1], one)
        worst, worst_rel = min(worst, psnr), max(worst_rel, rel)
    print(f"[C4 timing] + 8 single-clip calls {time.time() - t0:.1f} s")
    assert worst >= BATCH_VS_SINGLE_DB and worst_rel <= BATCH_VS_SINGLE_REL, (worst, worst_rel)
    for i in (0, B - 1):
        with torch.no_grad():
            want, _ = O.neuroclips_denoise(n["usd"], n["ou"], n["csd"], n["oc"], lat[i:i + 1], noise[i:i + 1],
                                           torch.cat([ctx_u[i:i + 1], ctx_t[i:i + 1]]), cimg[i:i + 1], (0,), steps, 8.5)
        rel, psnr = metrics(f"C4: clip {i} of the batched call vs the fp32 oracle ({steps} DDIM steps)", both[i:i + 1], want)
        print(f"[C4 timing] + oracle clip {i} {time.time() - t0:.1f} s")
        assert psnr >= LOOP_PSNR_DB and rel <= LOOP_REL_L2, (i, psnr, rel)


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "e4m3"])
def test_c5_32_frames_64x64_one_evaluation(cuda, nets, fp8):
    n = nets
    O, unet, ctrl = n["O"], n["unet"], n["ctrl"]
    F, L = 32, 64
    g = torch.Generator(device=cuda).manual_seed(5000)
    x = torch.randn(1, 4, F, L, L, generator=g, device=cuda)
    ctx = torch.randn(2, 77, n["ucfg"].cross_attention_dim, generator=g, device=cuda)
    cond = torch.zeros(1, 4, F, L, L, device=cuda)
    cond[:, :, 0] = torch.randn(1, 4, L, L, generator=g, device=cuda) * 0.18215
    mask = torch.zeros(1, 1, F, L, L, device=cuda)
    mask[:, :, 0] = 1
    t = 481
    xin = torch.cat([x] * 2)
    unet.set_attention_fp8(fp8)
    ctrl.set_attention_fp8(fp8)
    down, mid = ctrl(xin, t, encoder_hidden_states=ctx, controlnet_cond=cond, conditioning_mask=mask, return_dict=False)
    eps = unet(xin, t, encoder_hidden_states=ctx, down_block_additional_residuals=down, mid_block_additional_residual=mid).sample
    assert torch.isfinite(eps).all()
    with torch.no_grad():
        rd, rm = O.sparse_controlnet_forward(n["csd"], n["oc"], xin, t, ctx, cond, mask, 1.0)
        ref = O.unet3d_forward(n["usd"], n["ou"], xin, t, ctx, rd, rm)
    tag = "e4m3 attention" if fp8 else "bf16"
    relm, _ = metrics(f"C5 ({tag}): SparseCtrl mid residual, (2,4,32,64,64), full width", mid, rm)
    rel, psnr = metrics(f"C5 ({tag}): eps of SparseCtrl + U-Net, (2,4,32,64,64), full width", eps, ref)
    gate = FWD_REL_L2_FP8 if fp8 else FWD_REL_L2
    assert rel <= gate and psnr >= 30.0, (rel, psnr)


def test_c5_configured_batch_of_four_clips_one_evaluation(cuda, nets):
    """BASELINE config 5 at its CONFIGURED batch: one evaluation of both full-width networks at (2*4, 4, 32, 64, 64) --
    1 048 576 level-0 rows, 256 frame-images -- (a) against four independent B = 1 evaluations of the same clips (layout / offset-width /
    arena-reuse bugs show up exactly here and nowhere smaller), (b) clips 0 and 3 against the fp32 oracle evaluated one clip at a time.
    Largest element offsets at this shape: 1 048 576 rows x 1280 channels (GEGLU output, K = 5C operand halves) = 1.34e9 < 2^31 elements,
    2.7e9 BYTES (> 2^31: every kernel forms byte addresses in 64 bits; the row-panel kernel's 32-bit buffer offsets are gated by
    nr_rowpanel_eligible).  nr_fdiv_small's dividends stay below 2^24 (exact float conversion): 1 048 576 rows, 9 x 5 = 45 k-tiles."""
    n = nets
    O, unet, ctrl = n["O"], n["unet"], n["ctrl"]
    unet.set_attention_fp8(False)
    ctrl.set_attention_fp8(False)
    B, F, L = 4, 32, 64
    g = torch.Generator(device=cuda).manual_seed(5004)
    x = torch.randn(B, 4, F, L, L, generator=g, device=cuda)
    ctx_u = torch.randn(B, 77, n["ucfg"].cross_attention_dim, generator=g, device=cuda)
    ctx_t = torch.randn(B, 77, n["ucfg"].cross_attention_dim, generator=g, device=cuda)
    cond = torch.zeros(B, 4, F, L, L, device=cuda)
    cond[:, :, 0] = torch.randn(B, 4, L, L, generator=g, device=cuda) * 0.18215
    mask = torch.zeros(B, 1, F, L, L, device=cuda)
    mask[:, :, 0] = 1
    t = 481
    xin, ctx = torch.cat([x] * 2), torch.cat([ctx_u, ctx_t])
    down, mid = ctrl(xin, t, encoder_hidden_states=ctx, controlnet_cond=cond, conditioning_mask=mask, return_dict=False)
    eps = unet(xin, t, encoder_hidden_states=ctx, down_block_additional_residuals=down, mid_block_additional_residual=mid).sample.clone()
    mid = mid.float().clone()
    assert torch.isfinite(eps).all() and tuple(eps.shape) == (2 * B, 4, F, L, L)
    del down
    worst_db, worst_rel = 1e9, 0.0
    for i in range(B):
        xi, ci = torch.cat([x[i:i + 1]] * 2), torch.cat([ctx_u[i:i + 1], ctx_t[i:i + 1]])
        d1, m1 = ctrl(xi, t, encoder_hidden_states=ci, controlnet_cond=cond[i:i + 1], conditioning_mask=mask[i:i + 1], return_dict=False)
        e1 = unet(xi, t, encoder_hidden_states=ci, down_block_additional_residuals=d1, mid_block_additional_residual=m1).sample
        both = torch.cat([eps[i:i + 1], eps[B + i:B + i + 1]])
        rel, psnr = metrics(f"C5 B=4: eps of clip {i} in the batch vs the same clip alone", both, e1)
        worst_db, worst_rel = min(worst_db, psnr), max(worst_rel, rel)
        relm, _ = metrics(f"C5 B=4: SparseCtrl mid residual of clip {i} in the batch vs alone", torch.cat([mid[i:i + 1], mid[B + i:B + i + 1]]), m1.float())
        worst_rel = max(worst_rel, relm)
        if i in (0, B - 1):
            with torch.no_grad():
                rd, rm = O.sparse_controlnet_forward(n["csd"], n["oc"], xi, t, ci, cond[i:i + 1], mask[i:i + 1], 1.0)
                ref = O.unet3d_forward(n["usd"], n["ou"], xi, t, ci, rd, rm)
            del rd, rm
            r2, p2 = metrics(f"C5 B=4: eps of clip {i} of the batched evaluation vs the fp32 oracle", both, ref)
            assert r2 <= FWD_REL_L2 and p2 >= 30.0, (i, r2, p2)
            del ref
        del d1, m1, e1
    assert worst_db >= BATCH_VS_SINGLE_DB and worst_rel <= BATCH_VS_SINGLE_REL, (worst_db, worst_rel)


def test_deterministic_batch_mode_makes_a_clip_independent_of_its_neighbours(cuda, nets):
    """nr_net_set_deterministic_batch (NR_DETERMINISTIC_BATCH=1): the LayerNorm-fold / split-K / fused-kernel / GroupNorm-variant choices are
    made for the rows of ONE clip, so the C4 comparison 'clip i of a batch of 8 vs clip i alone' -- 40 dB in the default mode, where those
    choices follow M -- must close to >= 60 dB (every kernel is then row-position independent, so the expectation is
    bit equality, which the test reports).  Full width, (8,4,16,32,32), SparseCtrl on (grouped), CFG 8.5, 6 DDIM steps."""
    from neurons_amd import DDIMScheduler, NeuroclipsPipeline
    n = nets
    unet, ctrl = n["unet"], n["ctrl"]
    unet.set_attention_fp8(False)
    ctrl.set_attention_fp8(False)
    unet.set_deterministic_batch(True)
    ctrl.set_deterministic_batch(True)
    try:
        sched = DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="linear", steps_offset=1, clip_sample=False)
        pipe = NeuroclipsPipeline(vae=None, text_encoder=None, tokenizer=None, unet=unet, scheduler=sched, controlnet=ctrl).to(cuda)
        B, F, L, steps = 8, 16, 32, 6
        g = torch.Generator(device=cuda).manual_seed(1001)
        lat = torch.randn(B, 4, F, L, L, generator=g, device=cuda)
        noise = torch.randn(B, 4, F, L, L, generator=g, device=cuda)
        ctx_u = torch.randn(B, 77, n["ucfg"].cross_attention_dim, generator=g, device=cuda)
        ctx_t = torch.randn(B, 77, n["ucfg"].cross_attention_dim, generator=g, device=cuda)
        cimg = torch.randn(B, 4, 1, L, L, generator=g, device=cuda) * 0.18215
        kw = dict(video_length=F, height=L * 8, width=L * 8, num_inference_steps=steps, guidance_scale=8.5, controlnet_image_index=[0],
                  low_strength=0.3, output_type="latent")
        both = pipe([""] * B, latents=lat, noise=noise, text_embeddings=torch.cat([ctx_u, ctx_t]), controlnet_images=cimg, **kw).videos.clone()
        worst, nequal = 1e9, 0
        for i in (0, 3, 7):
            one = pipe("", latents=lat[i:i + 1], noise=noise[i:i + 1], text_embeddings=torch.cat([ctx_u[i:i + 1], ctx_t[i:i + 1]]),
                       controlnet_images=cimg[i:i + 1], **kw).videos
            nequal += int(torch.equal(both[i:i + 1], one))
            _, psnr = metrics(f"deterministic-batch mode: clip {i} of a batch of {B} vs the same clip alone ({steps} steps)", both[i:i + 1], one)
            worst = min(worst, psnr)
        print(f"[deterministic-batch] bit-identical clips: {nequal} of 3; worst PSNR {worst:.1f} dB")
        assert worst >= 60.0, worst
        assert nequal == 3, "round 4 measured bit equality (every kernel is row-position independent in this mode); a regression to 'close' means a new batch-dependent choice"
    finally:
        unet.set_deterministic_batch(False)
        ctrl.set_deterministic_batch(False)


def test_deterministic_batch_mode_without_guidance(cuda, nets):
    """with guidance off the batch holds ONE sample per clip (pipeline_neuroclips.py:435 does not double the latents), so 'the rows
    of one clip' is half of what the CFG case plans for.  nr_net_set_clip_samples (set by the pipeline per call) tells the engine; a clip of a
    batch of 4 must then equal the same clip alone bit for bit, as in the CFG test above.  Full width, (4,4,16,32,32), 4 DDIM steps."""
    from neurons_amd import DDIMScheduler, NeuroclipsPipeline
    n = nets
    unet, ctrl = n["unet"], n["ctrl"]
    unet.set_attention_fp8(False)
    ctrl.set_attention_fp8(False)
    unet.set_deterministic_batch(True)
    ctrl.set_deterministic_batch(True)
    try:
        sched = DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="linear", steps_offset=1, clip_sample=False)
        pipe = NeuroclipsPipeline(vae=None, text_encoder=None, tokenizer=None, unet=unet, scheduler=sched, controlnet=ctrl).to(cuda)
        B, F, L, steps = 4, 16, 32, 4
        g = torch.Generator(device=cuda).manual_seed(1002)
        lat = torch.randn(B, 4, F, L, L, generator=g, device=cuda)
        noise = torch.randn(B, 4, F, L, L, generator=g, device=cuda)
        ctx = torch.randn(B, 77, n["ucfg"].cross_attention_dim, generator=g, device=cuda)
        cimg = torch.randn(B, 4, 1, L, L, generator=g, device=cuda) * 0.18215
        kw = dict(video_length=F, height=L * 8, width=L * 8, num_inference_steps=steps, guidance_scale=1.0, controlnet_image_index=[0],
                  low_strength=0.3, output_type="latent")
        both = pipe([""] * B, latents=lat, noise=noise, text_embeddings=ctx, controlnet_images=cimg, **kw).videos.clone()
        assert torch.isfinite(both).all()
        nequal = 0
        for i in (0, B - 1):
            one = pipe("", latents=lat[i:i + 1], noise=noise[i:i + 1], text_embeddings=ctx[i:i + 1], controlnet_images=cimg[i:i + 1], **kw).videos
            nequal += int(torch.equal(both[i:i + 1], one))
            _, psnr = metrics(f"deterministic-batch mode, guidance off: clip {i} of a batch of {B} vs the same clip alone", both[i:i + 1], one)
            assert psnr >= 60.0, psnr
        assert nequal == 2, "one sample per clip: the per-clip plan must not depend on the batch"
    finally:
        unet.set_deterministic_batch(False)
        ctrl.set_deterministic_batch(False)
        unet.set_clip_samples(2)
        ctrl.set_clip_samples(2)


def test_c4_full_50_step_loop_two_clips(cuda, nets):
    """BASELINE config 4's loop at its FULL length on the GPU gate (the 8-clip test above stops at 12 steps): two clips in
    one call, (2,4,16,32,32), 50 DDIM steps, CFG 8.5, SparseCtrl on (grouped), against the same clips run alone and clip 1 against the fp32
    oracle's 50-step loop.  Same stated tolerances as every loop-level test."""
    from neurons_amd import DDIMScheduler, NeuroclipsPipeline
    n = nets
    O = n["O"]
    n["unet"].set_attention_fp8(False)
    n["ctrl"].set_attention_fp8(False)
    sched = DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="linear", steps_offset=1, clip_sample=False)
    pipe = NeuroclipsPipeline(vae=None, text_encoder=None, tokenizer=None, unet=n["unet"], scheduler=sched, controlnet=n["ctrl"]).to(cuda)
    B, F, L, steps = 2, 16, 32, 50
    g = torch.Generator(device=cuda).manual_seed(1050)
    lat = torch.randn(B, 4, F, L, L, generator=g, device=cuda)
    noise = torch.randn(B, 4, F, L, L, generator=g, device=cuda)
    ctx_u = torch.randn(B, 77, n["ucfg"].cross_attention_dim, generator=g, device=cuda)
    ctx_t = torch.randn(B, 77, n["ucfg"].cross_attention_dim, generator=g, device=cuda)
    cimg = torch.randn(B, 4, 1, L, L, generator=g, device=cuda) * 0.18215
    kw = dict(video_length=F, height=L * 8, width=L * 8, num_inference_steps=steps, guidance_scale=8.5, controlnet_image_index=[0],
              low_strength=0.3, output_type="latent")
    both = pipe([""] * B, latents=lat, noise=noise, text_embeddings=torch.cat([ctx_u, ctx_t]), controlnet_images=cimg, **kw).videos.clone()
    assert torch.isfinite(both).all()
    for i in range(B):
        one = pipe("", latents=lat[i:i + 1], noise=noise[i:i + 1], text_embeddings=torch.cat([ctx_u[i:i + 1], ctx_t[i:i + 1]]),
                   controlnet_images=cimg[i:i + 1], **kw).videos
        rel, psnr = metrics(f"C4 50 steps: clip {i} of a batch of {B} vs the same clip alone", both[i:i + 1], one)
        assert psnr >= BATCH_VS_SINGLE_DB and rel <= BATCH_VS_SINGLE_REL, (i, psnr, rel)
    i = 1
    with torch.no_grad():
        want, _ = O.neuroclips_denoise(n["usd"], n["ou"], n["csd"], n["oc"], lat[i:i + 1], noise[i:i + 1],
                                       torch.cat([ctx_u[i:i + 1], ctx_t[i:i + 1]]), cimg[i:i + 1], (0,), steps, 8.5)
    rel, psnr = metrics(f"C4 50 steps: clip {i} of the batched call vs the fp32 oracle", both[i:i + 1], want)
    assert psnr >= LOOP_PSNR_DB and rel <= LOOP_REL_L2, (psnr, rel)
