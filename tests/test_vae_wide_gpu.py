"""GPU: the full-width first-stage decoder / encoder (mid-block attention with one head of d = 512) on the wide-head attention kernel
(attn_fwd_shared_kernel<WideHead<512>> of attention.hip), at latents the GEMM sequence refuses (6 x 6, 10 x 12: h*w no multiple of 64), where the kernel is the
default, and at latents the GEMM sequence also serves (8 x 8), where the kernel runs under NR_VAE_ATTN_WIDE=1 (the default there stays the
GEMM sequence until a launch has a workgroup for every CU; the switch is read each time a plan is built).

Bounds: those of tests/test_vae_gpu.py at this width: PSNR >= 40 dB (and rel < 2.5e-2) on the decoded pixels and on the encoder moments
against oracle.vae_oracle; two plans of the same images (16-image decode vs four 4-image decodes) agree to >= 50 dB.
The GEMM sequence itself (NR_VAE_ATTN_WIDE=0) measures 61.8 dB on the (2, 4, 8, 8) decode and 54.7 dB on the 64 x 64 encode with these
weights, far from the bound, so the bound is the absolute one and not one relative to that path (the wide kernel: 61.8 / 54.8 dB)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_engine_gpu import metrics  # noqa: E402


def _sd(schema, seed):
    """Seeded weights as tests/test_vae_gpu.py::_gpu_sd, for either half's schema."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    sd = {}
    for k, shape in schema.items():
        z = torch.randn(shape, generator=g, device="cuda")
        if k.endswith(".bias"):
            z = (0.1 if ".norm" in k else 0.02) * z
        elif len(shape) == 1:
            z = 1.0 + 0.1 * z
        else:
            z = z / (int(np.prod(shape[1:])) ** 0.5)
        sd[k] = z
    return sd


@pytest.fixture(scope="module")
def decoder(cuda):
    from neurons_amd.vae import NativeVAEDecoder, VAEDecoderConfig, vae_decoder_state_dict_schema
    cfg = VAEDecoderConfig()
    sd = _sd(vae_decoder_state_dict_schema(cfg), 7)
    dec = NativeVAEDecoder(cfg).to("cuda")
    dec.load_state_dict({k: v.cpu() for k, v in sd.items()})
    return dec, sd


@pytest.fixture(scope="module")
def encoder(cuda):
    from neurons_amd.vae import NativeVAEEncoder, VAEDecoderConfig, vae_encoder_state_dict_schema
    cfg = VAEDecoderConfig()
    sd = _sd(vae_encoder_state_dict_schema(cfg), 12)
    enc = NativeVAEEncoder(cfg).to("cuda")
    enc.load_state_dict({k: v.cpu() for k, v in sd.items()})
    return enc, sd


@pytest.fixture()
def wide(monkeypatch):
    monkeypatch.setenv("NR_VAE_ATTN_WIDE", "1")


@pytest.fixture()
def default_rule(monkeypatch):
    monkeypatch.delenv("NR_VAE_ATTN_WIDE", raising=False)


def _assert_wide_plan(net):
    desc = [d for d in net.op_descriptions() if d]
    attn = [d for d in desc if d.startswith("attention mode=0 ") and " d=512 " in d]
    assert len(attn) == 1, desc
    assert len([d for d in desc if d.startswith("attention")]) == 1, desc
    assert not any("vae QK^T" in d or "softmax rows" in d or "vae PV" in d or "vae V^T" in d for d in desc), desc


@pytest.mark.parametrize("shape", [(2, 4, 8, 8), (1, 4, 6, 6), (1, 4, 10, 12)])
def test_full_width_decode_vs_oracle(decoder, shape, monkeypatch):
    """(2, 4, 8, 8): a latent the GEMM sequence serves too (wide on request); 6 x 6 and 10 x 12: h*w = 36 / 120, refused without the wide kernel
    and on it by default."""
    from neurons_amd.synth import randn
    from oracle import vae_oracle as V
    dec, sd = decoder
    if shape[2] * shape[3] % 64 == 0:
        monkeypatch.setenv("NR_VAE_ATTN_WIDE", "1")
    else:
        monkeypatch.delenv("NR_VAE_ATTN_WIDE", raising=False)
    z = randn(f"vw.z{shape}", shape, 1).cuda()
    img = dec.decode(z, z_scale=1 / 0.18215)
    _assert_wide_plan(dec)
    with torch.no_grad():
        ref = V.decode(sd, z / 0.18215, 4, 2)
    rel, psnr = metrics(f"full-width VAE decode {shape} vs oracle", img, ref)
    assert torch.isfinite(img).all()
    assert psnr >= 40.0 and rel < 2.5e-2


@pytest.mark.parametrize("size", [48, 64])
def test_full_width_encode_vs_oracle(encoder, size, monkeypatch):
    """48 x 48 pixels -> a 6 x 6 latent (36 tokens, wide by default); 64 x 64 -> 8 x 8 (wide on request)."""
    from oracle import vae_oracle as V
    enc, sd = encoder
    if size == 64:
        monkeypatch.setenv("NR_VAE_ATTN_WIDE", "1")
    else:
        monkeypatch.delenv("NR_VAE_ATTN_WIDE", raising=False)
    x = torch.rand(2, 3, size, size, generator=torch.Generator(device="cuda").manual_seed(13 + size), device="cuda")
    mom = enc.moments(x, 2.0, -1.0)
    _assert_wide_plan(enc)
    with torch.no_grad():
        ref = V.encode_moments(sd, 2 * x - 1, 4, 2)
    rel, psnr = metrics(f"full-width VAE encoder moments {size}x{size} vs oracle", mom, ref)
    assert torch.isfinite(mom).all()
    assert psnr >= 40.0 and rel < 2.5e-2


def test_sixteen_image_decode_equals_four_chunks(decoder, wide):
    from neurons_amd.synth import randn
    dec, _ = decoder
    z = randn("vw.z16", (16, 4, 8, 12), 1).cuda()       # a shape of its own: both plans are built under the switch
    whole = dec.decode(z, z_scale=1 / 0.18215)
    _assert_wide_plan(dec)
    parts = dec.decode(z, z_scale=1 / 0.18215, chunk=4)
    _assert_wide_plan(dec)
    _, psnr = metrics("16-image vs 4 x 4-image decode", parts, whole)
    assert psnr >= 50.0


def test_default_rule_keeps_the_gemm_sequence_below_a_full_chip(decoder, default_rule):
    """(2, 4, 16, 8): h*w = 128 is a multiple of 64 and the wide launch would have 4 workgroups for 256 CUs: the GEMM sequence stays the default
    there; NR_VAE_ATTN_WIDE=0 refuses the 6 x 6 latent as the GEMM sequence always did."""
    from neurons_amd.synth import randn
    dec, _ = decoder
    dec.decode(randn("vw.zd", (2, 4, 16, 8), 1).cuda(), z_scale=1 / 0.18215)
    desc = [d for d in dec.op_descriptions() if d]
    assert sum("vae QK^T" in d for d in desc) == 2 and sum(d.startswith("softmax rows") for d in desc) == 2, desc
    assert not any(d.startswith("attention") for d in desc), desc


def test_switch_off_refuses_what_the_gemm_sequence_refuses(decoder, monkeypatch):
    monkeypatch.setenv("NR_VAE_ATTN_WIDE", "0")
    dec, _ = decoder
    with pytest.raises(RuntimeError, match="multiple of 64"):
        dec.decode(torch.zeros(1, 4, 6, 10, device="cuda"))


def test_attention_fp8_request_does_not_reach_the_vae(decoder, default_rule):
    """nr_net_set_attention_fp8 is for the U-Net's attention; a VAE handle accepts it and plans (and computes) as without it."""
    from neurons_amd.synth import randn
    dec, _ = decoder
    z = randn("vw.zf", (1, 4, 6, 8), 1).cuda()
    want = dec.decode(z, z_scale=1 / 0.18215)
    dec.set_attention_fp8(True)                 # the next decode re-plans
    try:
        got = dec.decode(z, z_scale=1 / 0.18215)
        _assert_wide_plan(dec)
    finally:
        dec.set_attention_fp8(False)
    assert torch.equal(got, want)
