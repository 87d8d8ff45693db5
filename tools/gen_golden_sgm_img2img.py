"""Golden vectors of the sgm img2img path from the REFERENCE's own classes -> tests/golden/sgm_img2img_tiny.npz.

What runs is the reference's ``do_img2img`` and ``Img2ImgDiscretizationWrapper`` (generative_models/sgm/inference/helpers.py:77-98,243-305) over its
``LegacyDDPMDiscretization``, ``EulerEDMSampler`` + ``VanillaCFG``, ``DiscreteDenoiser``, ``OpenAIWrapper(UNetModel)``, first-stage ``Encoder`` /
``Decoder`` and ``DiagonalGaussianRegularizer``, at the tiny configurations of sgm_tiny.npz / vae_tiny.npz (tests/tiny_configs.py, synthetic
weights from the Philox recipe: U-Net seed 71, decoder 91, encoder 94).  ``DiffusionEngine`` / ``AutoencodingEngineLegacy`` themselves need
Lightning, so ``do_img2img`` gets a stand-in model holding what it touches, with ``encode_first_stage`` / ``decode_first_stage`` written out as
diffusion.py:118-150 over autoencoder.py:468-494 have them (as oracle/gen_golden.py: gen_unclip does for the decoder); its conditioner hands
back fixed ``c`` / ``uc`` dicts.  Non-arithmetic stand-ins: helpers.py's imports of imwatermark / omegaconf, its prints, and its
``autocast("cpu")``, which would otherwise record bf16 arithmetic: the fixture is fp32.

The file holds
  sig_<steps>_<strength>   pruned sigma tables, steps in {1, 10, 38, 50} x strength in {0, .02, .5, .75, .99, 1}; sigw_50: a wrapper in a wrapper
  img, z_init, ctx, uc_ctx, vec, noise, enc_noise, offset      inputs and the recorded draws (replayed from the seed in the reference's order)
  enc_latent               encode_first_stage(img) with enc_noise
  <case>.start / .z / .img / .calls     noised start handed to the sampler, final latents, images in [0, 1] (fp16), network evaluations;
                           case = "enc" | "skip" + strength in {0, 0.5, 1}, 10 steps, 8x8 latent, 2 samples, offset_noise_level 0.04

Runs only where the reference sources are; the tests read the stored arrays only.

Usage:  python tools/gen_golden_sgm_img2img.py [output path]
"""
import contextlib
import io
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STRENGTHS = (0.0, 0.02, 0.5, 0.75, 0.99, 1.0)
STEPS = (1, 10, 38, 50)
LOOP_STRENGTHS = (0.0, 0.5, 1.0)
LOOP_STEPS = 10
N = 2
OFFSET_LEVEL = 0.04
SCALE_FACTOR = 0.18215


def load_helpers():
    from oracle import gen_golden as G
    G.install_sgm_scaffolding()
    if "imwatermark" not in sys.modules:
        G._mod("imwatermark", WatermarkEncoder=type("WatermarkEncoder", (), {"set_watermark": lambda self, *a: None}))
    helpers = G._load_ref_module("ref_sgm_helpers", f"{G.REF}/generative_models/sgm/inference/helpers.py")
    helpers.autocast = lambda device: contextlib.nullcontext()        # record fp32, not the CPU autocast's bf16
    return helpers


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


class RecordingSampler:
    """What do_img2img touches of a sampler (.discretization, .num_steps, the call), keeping the start it is handed."""

    def __init__(self, sampler):
        self.sampler = sampler
        self.num_steps = sampler.num_steps
        self.start = None

    @property
    def discretization(self):
        return self.sampler.discretization

    def __call__(self, denoiser, x, cond=None, uc=None):
        self.start = x.clone()
        return self.sampler(denoiser, x, cond=cond, uc=uc)


@torch.no_grad()
def main(path):
    from oracle import gen_golden as G
    from neurons_amd.sgm import sgm_random_state_dict
    from neurons_amd.synth import randn
    from neurons_amd.vae import vae_random_state_dict
    from tiny_configs import tiny_sgm_config, tiny_vae_config
    helpers = load_helpers()
    from sgm.modules.autoencoding.regularizers import DiagonalGaussianRegularizer
    from sgm.modules.diffusionmodules.denoiser import DiscreteDenoiser
    from sgm.modules.diffusionmodules.discretizer import LegacyDDPMDiscretization
    from sgm.modules.diffusionmodules.model import Decoder, Encoder
    from sgm.modules.diffusionmodules.sampling import EulerEDMSampler
    from sgm.modules.diffusionmodules.wrappers import OpenAIWrapper
    W = helpers.Img2ImgDiscretizationWrapper
    out = {}

    # ---- pruned tables -------------------------------------------------------------------------------------------------------------
    for steps in STEPS:
        for s in STRENGTHS:
            out[f"sig_{steps}_{s}"] = quiet(W(LegacyDDPMDiscretization(), s), steps).numpy()
    out["sigw_50"] = quiet(W(W(LegacyDDPMDiscretization(), 0.75), 0.5), 50).numpy()

    # ---- the networks --------------------------------------------------------------------------------------------------------------
    cfg, vcfg = tiny_sgm_config(), tiny_vae_config()
    net = G.build_reference_sgm(cfg, sgm_random_state_dict(cfg, seed=71))
    dd = dict(ch=vcfg.ch, out_ch=vcfg.out_ch, ch_mult=vcfg.ch_mult, num_res_blocks=vcfg.num_res_blocks, attn_resolutions=[], in_channels=3,
              resolution=64, z_channels=vcfg.z_channels, attn_type="vanilla", double_z=True)
    vsd, esd = vae_random_state_dict(vcfg, seed=91), vae_random_state_dict(vcfg, seed=94, encoder=True)
    dec, enc = Decoder(**dd), Encoder(**dd)
    dec.load_state_dict({k[len("decoder."):]: v for k, v in vsd.items() if k.startswith("decoder.")}, strict=True)
    enc.load_state_dict({k[len("encoder."):]: v for k, v in esd.items() if k.startswith("encoder.")}, strict=True)
    dec.eval(), enc.eval()
    pq = torch.nn.Conv2d(vcfg.embed_dim, vcfg.z_channels, 1)
    pq.load_state_dict({"weight": vsd["post_quant_conv.weight"], "bias": vsd["post_quant_conv.bias"]})
    qc = torch.nn.Conv2d(2 * vcfg.z_channels, 2 * vcfg.embed_dim, 1)
    qc.load_state_dict({"weight": esd["quant_conv.weight"], "bias": esd["quant_conv.bias"]})
    reg = DiagonalGaussianRegularizer()                  # AutoencoderKL's regularizer with its default sample=True (autoencoder.py:508-520)

    ctx = randn("i2i.ctx", (N, 24, cfg.context_dim), 81)
    uc_ctx = randn("i2i.uc_ctx", (N, 24, cfg.context_dim), 82)
    vec = randn("i2i.vec", (N, cfg.adm_in_channels), 83)
    img = torch.rand(torch.Size((N, 3, 64, 64)), generator=torch.Generator().manual_seed(84)) * 2 - 1
    z_init = randn("i2i.z_init", (N, 4, 8, 8), 85) * 0.7
    c = {"crossattn": ctx, "vector": vec}
    uc = {"crossattn": uc_ctx, "vector": vec}
    calls = [0]

    class CountingWrapper(OpenAIWrapper):
        def forward(self, *a, **k):
            calls[0] += 1
            return super().forward(*a, **k)

    dcfg = {"target": "sgm.modules.diffusionmodules.discretizer.LegacyDDPMDiscretization"}
    model = types.SimpleNamespace(
        ema_scope=contextlib.nullcontext,
        conditioner=types.SimpleNamespace(embedders=[], get_unconditional_conditioning=lambda batch, batch_uc=None, force_uc_zero_embeddings=None:
                                          (dict(c), dict(uc))),
        denoiser=DiscreteDenoiser(scaling_config={"target": "sgm.modules.diffusionmodules.denoiser_scaling.EpsScaling"}, num_idx=1000,
                                  discretization_config=dcfg),
        model=CountingWrapper(net),
        encode_first_stage=lambda x: SCALE_FACTOR * reg(qc(enc(x)))[0],        # diffusion.py:137-150 over autoencoder.py:468-488
        decode_first_stage=lambda z: dec(pq(z / SCALE_FACTOR)))               # diffusion.py:118-135 over autoencoder.py:490-494
    seed = 321
    # the draws in the order do_img2img makes them: posterior sample (encode only), noise = randn_like(z), offset = randn(n)
    torch.manual_seed(seed)
    enc_noise = torch.randn(N, 4, 8, 8)
    noise = torch.randn(N, 4, 8, 8)
    offset = torch.randn(N)
    out.update(img=img.numpy(), z_init=z_init.numpy(), ctx=ctx.numpy(), uc_ctx=uc_ctx.numpy(), vec=vec.numpy(), noise=noise.numpy(),
               enc_noise=enc_noise.numpy(), offset=offset.numpy(), num_steps=np.array(LOOP_STEPS), offset_noise_level=np.array(OFFSET_LEVEL),
               scale_factor=np.array(SCALE_FACTOR))
    torch.manual_seed(seed)
    out["enc_latent"] = model.encode_first_stage(img).numpy()

    for skip in (False, True):
        for s in LOOP_STRENGTHS:
            tag = f"{'skip' if skip else 'enc'}{s}"
            sampler = EulerEDMSampler(num_steps=LOOP_STEPS, discretization_config=dcfg, device="cpu",
                                      guider_config={"target": "sgm.modules.diffusionmodules.guiders.VanillaCFG", "params": {"scale": 5.0}})
            sampler.discretization = W(sampler.discretization, s)
            rec = RecordingSampler(sampler)
            calls[0] = 0
            torch.manual_seed(seed)
            if skip:
                torch.randn(N, 4, 8, 8)                   # no posterior draw with skip_encode: keep noise / offset the recorded ones
            samples, samples_z = quiet(helpers.do_img2img, z_init if skip else img, model, rec, {}, N, offset_noise_level=OFFSET_LEVEL,
                                       return_latents=True, skip_encode=skip, device="cpu")
            pruned = out[f"sig_{LOOP_STEPS}_{s}"]
            assert calls[0] == len(pruned) - 1, (tag, calls[0], len(pruned))
            assert tuple(samples.shape) == (N, 3, 64, 64) and tuple(samples_z.shape) == (N, 4, 8, 8)
            out[f"{tag}.start"] = rec.start.numpy()
            out[f"{tag}.z"] = samples_z.numpy()
            out[f"{tag}.img"] = samples.numpy().astype(np.float16)
            out[f"{tag}.img_mean"] = np.array(samples.double().mean().item())
            out[f"{tag}.calls"] = np.array(calls[0])
            print(f"sgm_img2img: {tag}: {calls[0]} network calls, start std {rec.start.std().item():.3f}, z std {samples_z.std().item():.3f}, "
                  f"image mean {samples.mean().item():.4f}, clamped {((samples == 0) | (samples == 1)).float().mean().item():.3f}", flush=True)
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    torch.manual_seed(0)
    torch.set_num_threads(8)
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "sgm_img2img_tiny.npz"))
