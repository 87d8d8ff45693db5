"""GPU tests of the SparseCtrl image-condition variant (configs/inference/sparsectrl/image_condition.yaml): the condition-embedding
kernels against F.conv2d, the tiny network against the reference fixture (tests/golden/sparsectrl_image_tiny.npz), the full-width
network against the fp32 restatement (tests/sparsectrl_image_ref.py), the identical-frame evaluation, the pipeline schedules and the
converted-weight transport.  Gates as tests/test_engine_gpu.py: rel-L2 <= 2.5e-2 and PSNR >= 35 dB per network evaluation."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "sparsectrl_image_tiny.npz")
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from sparsectrl_image_ref import image_ctrl_config, sparsectrl_image_forward, tiny_image_ctrl_config  # noqa: E402
from test_engine_gpu import _ctrl_descs, metrics  # noqa: E402


def _gate(name, got, want):
    rel, psnr = metrics(name, got, want)
    assert rel <= 2.5e-2 and psnr >= 35.0, (name, rel, psnr)
    return rel


def _rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt()).item()


def _tiny_image(seed=13):
    from neurons_amd import _lib, NativeSparseCtrl
    from neurons_amd.unet3d import random_state_dict
    cfg = tiny_image_ctrl_config()
    ctrl = NativeSparseCtrl(cfg).to("cuda")
    ctrl.load_state_dict(random_state_dict(cfg, _lib.NR_KIND_SPARSECTRL, seed=seed, zero_init_heads=False))
    return ctrl, cfg


def _tiny_unet():
    from neurons_amd import _lib, NativeUNet3D
    from neurons_amd.unet3d import random_state_dict
    from tiny_configs import tiny_unet_config
    ucfg = tiny_unet_config()
    unet = NativeUNet3D(ucfg).to("cuda")
    unet.load_state_dict(random_state_dict(ucfg, _lib.NR_KIND_UNET3D, seed=11))
    return unet


def _golden(cuda):
    g = np.load(GOLD)
    t = {k: torch.from_numpy(g[k]).to(cuda) for k in ("sample", "ctx", "cond", "mask")}
    return g, t


# every (Cin, Cout, stride) of the embedding's table below conv_out, from the condition resolution down
EMBED_CONVS = [(16, 16, 1), (16, 32, 2), (32, 32, 1), (32, 96, 2), (96, 96, 1), (96, 256, 2)]


@pytest.mark.parametrize("lat", [(32, 32), (24, 40), (3, 5)])
def test_condition_embedding_kernels_match_conv2d(cuda, lat):
    from neurons_amd import ops
    g = torch.Generator().manual_seed(7)
    h, w = lat
    H, W = 8 * h, 8 * w
    # conv_in: 3 + 1 -> 16 from the fp32 planes, frames picked by a map
    cond = torch.randn(2, 3, 3, H, W, generator=g)
    mask = (torch.rand(2, 1, 3, H, W, generator=g) > 0.5).float()
    w0, b0 = torch.randn(16, 4, 3, 3, generator=g) / 6, torch.randn(16, generator=g) * 0.1
    frames = [2, 0]
    got = ops.condembed_in(cond.to(cuda), mask.to(cuda), w0.to(cuda), b0.to(cuda), frames=frames)
    x = torch.cat([cond, mask], 1)[:, :, frames].permute(0, 2, 1, 3, 4).reshape(-1, 4, H, W)
    want = F.silu(F.conv2d(x, w0, b0, padding=1)).permute(0, 2, 3, 1)
    rel = _rel(got.float().cpu(), want)
    print(f"condembed_in 4->16 {H}x{W}: rel_l2={rel:.2e}")
    assert rel <= 1e-2
    # the MFMA convs, chained at the sizes the embedding sees them
    size = (H, W)
    for cin, cout, s in EMBED_CONVS:
        x = torch.randn(2, *size, cin, generator=g).to(torch.bfloat16)
        wt = torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5
        b = torch.randn(cout, generator=g) * 0.1
        for silu in (True, False):
            got = ops.condembed_conv(x.to(cuda), wt.to(cuda), b.to(cuda), stride=s, silu=silu)
            want = F.conv2d(x.float().permute(0, 3, 1, 2), wt, b, stride=s, padding=1)
            want = (F.silu(want) if silu else want).permute(0, 2, 3, 1)
            rel = _rel(got.float().cpu(), want)
            print(f"condembed_conv {cin}->{cout} s{s} {size} silu={silu}: rel_l2={rel:.2e}")
            assert tuple(got.shape) == tuple(want.shape) and rel <= 1e-2
        size = tuple(want.shape[1:3])
    assert size == (h, w)
    # conv_out (256 -> C0 = 320 at the latent grid): routed to the implicit-GEMM conv kernel; also the embedding kernel's own form of it
    x = torch.randn(2, h, w, 256, generator=g).to(torch.bfloat16)
    wt, b = torch.randn(320, 256, 3, 3, generator=g) / 48, torch.randn(320, generator=g) * 0.1
    want = F.conv2d(x.float().permute(0, 3, 1, 2), wt, b, padding=1).permute(0, 2, 3, 1)
    got = ops.conv3x3(x.to(cuda), wt.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16).to(cuda), b.to(cuda))
    assert _rel(got.float().cpu(), want) <= 1e-2
    got = ops.condembed_conv(x.to(cuda), wt.to(cuda), b.to(cuda), stride=1, silu=False)
    assert _rel(got.float().cpu(), want) <= 1e-2


def _tap(ctrl, name, shape):
    import ctypes as C
    from neurons_amd import _lib
    lib = _lib.load()
    b, c, f, h, w = shape
    for i in range(lib.nr_net_num_taps(ctrl._h)):
        if lib.nr_net_tap_name(ctrl._h, i).decode() == name:
            buf = np.empty(b * f * h * w * c, dtype=np.float32)
            rows, cc = C.c_int32(), C.c_int32()
            _lib.check(lib.nr_net_read_tap(ctrl._h, i, buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(rows), C.byref(cc)))
            return torch.from_numpy(buf).reshape(b, f, h, w, c).permute(0, 4, 1, 2, 3)
    raise KeyError(name)


def test_tiny_image_sparsectrl_matches_reference_golden(cuda):
    from neurons_amd import _lib
    g, t = _golden(cuda)
    ctrl, cfg = _tiny_image(int(g["ctrl_seed"]))
    T = int(g["t"])

    def run():
        down, mid = ctrl(t["sample"], T, encoder_hidden_states=t["ctx"], controlnet_cond=t["cond"], conditioning_mask=t["mask"],
                         return_dict=False)
        return [d.float().clone() for d in down] + [mid.float().clone()]

    out = run()
    assert len(out) == 13
    for i in range(12):
        _gate(f"image ctrl down_res_{i}", out[i], g[f"down_res_{i}"])
    _gate("image ctrl mid_res", out[12], g["mid_res"])
    descs = _ctrl_descs(ctrl)
    assert sum("condembed_in" in d for d in descs) == 1 and sum("condembed_conv" in d for d in descs) == 6
    assert sum("condembed conv_out" in d for d in descs) == 1
    # the U-Net fed with these residuals
    unet = _tiny_unet()
    eps = unet(t["sample"], T, encoder_hidden_states=t["ctx"], down_block_additional_residuals=out[:12], mid_block_additional_residual=out[12]).sample
    _gate("tiny unet eps (+image ctrl residuals) vs reference", eps, g["eps_ctrl"])
    # bit-identical reruns, and eager launches == hipGraph replay
    assert all(torch.equal(a, b) for a, b in zip(out, run()))
    ctrl.enable_graph(False)
    assert all(torch.equal(a, b) for a, b in zip(out, run()))
    # the embedding itself: the conv_in tap of a debug plan is conv_in(0) + embedding = conv_in.bias + embedding
    _lib.check(_lib.load().nr_net_set_debug(ctrl._handle(), 1))
    ctrl._plan_key = None
    dbg = run()
    emb = torch.from_numpy(g["embedding"])
    got = _tap(ctrl, "conv_in", tuple(emb.shape)) - _conv_in_bias(cfg, int(g["ctrl_seed"])).view(1, -1, 1, 1, 1)
    _gate("image ctrl embedding vs reference", got, emb)
    for i in range(13):
        _gate(f"debug plan residual {i}", dbg[i], out[i].cpu())


def _conv_in_bias(cfg, seed):
    from neurons_amd import _lib
    from neurons_amd.unet3d import random_state_dict
    return random_state_dict(cfg, _lib.NR_KIND_SPARSECTRL, seed=seed, zero_init_heads=False)["conv_in.bias"]


def test_image_condition_size_is_checked(cuda):
    g, t = _golden(cuda)
    ctrl, _ = _tiny_image(int(g["ctrl_seed"]))
    with pytest.raises(ValueError, match="8x the latent"):
        ctrl(t["sample"], int(g["t"]), encoder_hidden_states=t["ctx"], controlnet_cond=t["cond"][..., :8, :8],
             conditioning_mask=t["mask"][..., :8, :8])


@pytest.mark.parametrize("index", [(0,), (0, 5), (3,)])
def test_image_identical_frame_evaluation_is_exact(cuda, index):
    """As test_engine_gpu.py::test_sparsectrl_identical_frame_evaluation_is_exact for the image-condition variant: the embedding runs on
    the conditioned frames + one representative of the rest only."""
    g, t = _golden(cuda)
    ctrl, _ = _tiny_image(int(g["ctrl_seed"]))
    sample, ctx = t["sample"].repeat(2, 1, 1, 1, 1), t["ctx"].repeat(2, 1, 1)        # CFG batch 2, one condition image
    Fr, H, W = sample.shape[2], t["cond"].shape[3], t["cond"].shape[4]
    cond = torch.zeros(1, 3, Fr, H, W, device=cuda)
    mask = torch.zeros(1, 1, Fr, H, W, device=cuda)
    gen = torch.Generator(device=cuda).manual_seed(78)
    for f in index:
        cond[:, :, f] = torch.randn(1, 3, H, W, generator=gen, device=cuda) * 0.5
        mask[:, :, f] = 1

    def run(dedup):
        os.environ["NR_CTRL_DEDUP"] = "1" if dedup else "0"
        ctrl._cframes_key = None
        down, mid = ctrl(sample, int(g["t"]), encoder_hidden_states=ctx, controlnet_cond=cond, conditioning_mask=mask, return_dict=False)
        return [d.float().clone() for d in down] + [mid.float().clone()], _ctrl_descs(ctrl)

    try:
        full, d_full = run(False)
        fast, d_fast = run(True)
    finally:
        os.environ.pop("NR_CTRL_DEDUP", None)
    emb_full = [d for d in d_full if d.startswith("condembed")]
    emb_fast = [d for d in d_fast if d.startswith("condembed")]
    assert len(emb_full) == len(emb_fast) == 8
    assert all(f"frames={Fr}" in d for d in emb_full), emb_full
    assert all(f"frames={len(index) + 1}" in d for d in emb_fast), emb_fast
    for i, (a, b) in enumerate(zip(fast, full)):
        rel, psnr = metrics(f"image identical-frame evaluation, index {index}: residual {i} vs full evaluation", a, b)
        assert (psnr >= 55.0 and rel <= 1.5e-2) or torch.equal(a, b), (i, psnr, rel)


def test_image_sparsectrl_full_width_vs_fp32_restatement(cuda):
    """Config-2 shapes: SD-1.5 widths, one clip of 16 frames at a 32 x 32 latent, 256 x 256 RGB condition on frame 0, CFG batch 2."""
    from neurons_amd import _lib, NativeSparseCtrl
    from neurons_amd.synth import gpu_random_state_dict
    from neurons_amd.unet3d import UNet3DConfig, state_dict_schema
    cfg = image_ctrl_config(UNet3DConfig())
    sd = gpu_random_state_dict(state_dict_schema(cfg, _lib.NR_KIND_SPARSECTRL), 5, cuda)
    ctrl = NativeSparseCtrl(cfg).to(cuda)
    ctrl.load_state_dict({k: v.cpu() for k, v in sd.items()})
    gen = torch.Generator(device=cuda).manual_seed(3)
    Fr, L = 16, 32
    sample = torch.randn(1, 4, Fr, L, L, generator=gen, device=cuda).repeat(2, 1, 1, 1, 1)
    ctx = torch.randn(2, 77, 768, generator=gen, device=cuda)
    cond = torch.zeros(1, 3, Fr, 8 * L, 8 * L, device=cuda)
    mask = torch.zeros(1, 1, Fr, 8 * L, 8 * L, device=cuda)
    cond[:, :, 0] = torch.rand(1, 3, 8 * L, 8 * L, generator=gen, device=cuda) * 2 - 1
    mask[:, :, 0] = 1
    down, mid = ctrl(sample, 601, encoder_hidden_states=ctx, controlnet_cond=cond, conditioning_mask=mask, return_dict=False)
    got = [d.float() for d in down] + [mid.float()]
    with torch.no_grad():
        _, rdown, rmid = sparsectrl_image_forward(sd, cfg, sample, 601, ctx, cond, mask)
    for i, (a, b) in enumerate(zip(got, rdown + [rmid])):
        _gate(f"full-width image ctrl residual {i} vs fp32", a, b)
    descs = _ctrl_descs(ctrl)
    assert [d for d in descs if d.startswith("condembed_in")] == ["condembed_in Cin=4 Cout=16 H=256 W=256 frames=2"]


def _pipe_run(ctrl, unet, mode, g, t):
    from neurons_amd import DDIMScheduler, NeuroclipsPipeline
    sched = DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="linear", steps_offset=1, clip_sample=False)
    pipe = NeuroclipsPipeline(vae=None, text_encoder=None, tokenizer=None, unet=unet, scheduler=sched, controlnet=ctrl).to("cuda")
    if mode == "separate":
        pipe.overlap_controlnet = False
    elif mode == "fused":
        pipe.controlnet_group = 1
        pipe.prefetch_controlnet = True
    else:
        pipe.controlnet_group = 3
    gen = torch.Generator().manual_seed(9)
    lat, noise = torch.randn(1, 4, 8, 8, 8, generator=gen), torch.randn(1, 4, 8, 8, 8, generator=gen)
    ctx = t["ctx"].repeat(2, 1, 1)
    cimg = t["cond"][:, :, [0, 5]]                     # two RGB keyframes at pixel size (no VAE encode)
    out = pipe("", video_length=8, height=64, width=64, num_inference_steps=10, guidance_scale=8.5, latents=lat.cuda(), noise=noise,
               text_embeddings=ctx, controlnet_images=cimg, controlnet_image_index=[0, 5], low_strength=0.3, output_type="latent").videos
    return out.clone(), pipe.last_controlnet_group


def test_image_sparsectrl_pipeline_schedules_agree(cuda):
    g, t = _golden(cuda)
    outs = {}
    for mode in ("separate", "fused", "grouped"):
        ctrl, _ = _tiny_image(int(g["ctrl_seed"]))
        outs[mode], grp = _pipe_run(ctrl, _tiny_unet(), mode, g, t)
        assert torch.isfinite(outs[mode]).all()
        assert grp == (3 if mode == "grouped" else 1)
    for mode in ("fused", "grouped"):
        _, psnr = metrics(f"pipeline {mode} vs separate calls", outs[mode], outs["separate"])
        assert psnr >= 55.0
    # the condition reaches the result: black keyframes -> a different video
    ctrl, _ = _tiny_image(int(g["ctrl_seed"]))
    zero = dict(t, cond=t["cond"] * 0)
    out0, _ = _pipe_run(ctrl, _tiny_unet(), "separate", g, zero)
    assert not torch.equal(out0, outs["separate"])


def test_image_sparsectrl_weight_transport(cuda):
    from neurons_amd import NativeSparseCtrl
    g, t = _golden(cuda)
    ctrl, cfg = _tiny_image(int(g["ctrl_seed"]))
    T = int(g["t"])

    def run(net, sample, ctx, cond, mask):
        down, mid = net(sample, T, encoder_hidden_states=ctx, controlnet_cond=cond, conditioning_mask=mask, return_dict=False)
        return [d.float().clone() for d in down] + [mid.float().clone()]

    ref = run(ctrl, t["sample"], t["ctx"], t["cond"], t["mask"])
    manifest, arena = ctrl.export_weights()
    fresh = NativeSparseCtrl(cfg).to("cuda")
    fresh.import_weights(manifest, arena)
    got = run(fresh, t["sample"], t["ctx"], t["cond"], t["mask"])
    assert all(torch.equal(a, b) for a, b in zip(got, ref))
    # host copies released, then a re-plan to another shape (64 context tokens): equals a handle that kept its host copies
    from neurons_amd import _lib
    _lib.check(_lib.load().nr_net_release_host_weights(ctrl._handle()))
    c2 = t["ctx"][:, :64].contiguous()
    got2 = run(ctrl, t["sample"], c2, t["cond"], t["mask"])
    keep, _ = _tiny_image(int(g["ctrl_seed"]))
    ref2 = run(keep, t["sample"], c2, t["cond"], t["mask"])
    assert all(torch.equal(a, b) for a, b in zip(got2, ref2))
    assert not torch.equal(got2[-1], ref[-1])          # the mid residual sees the context
