"""DDIM-50 against DPM-Solver++ 2M at 25 and 20 steps on the headline configuration of bench.py (1 clip, 16 frames, 32x32 latent, CFG 8.5,
SparseCtrl on, random-init weights of the reference architecture): ms per step and seconds per clip, the arms alternating in one process on
one GPU, and the distance of the 25-step results of both rules to a 200-step DDIM run of the same engine.

Networks, weights and inputs are built as bench.py's main() builds them (its gpu_random_state_dict by import, the same seeds and shapes).
Nothing here is gated; the report goes to --out.  Synthetic weights say nothing about the quality a real checkpoint gives at 20 - 25 steps.

Usage:  python tools/dpmpp_ab.py [--rounds 3] [--clips 2] [--out profiles/dpmpp_ab.txt]
"""
import argparse
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F, L = 16, 32
KW = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="linear", steps_offset=1, clip_sample=False)
ARMS = (("DDIM-50", "ddim", 50), ("DPM++-25", "dpm", 25), ("DPM++-20", "dpm", 20))


def distance(got, ref):
    mse = ((got.double() - ref.double()) ** 2).mean().item()
    rng = (ref.max() - ref.min()).item()
    return math.sqrt(mse) / math.sqrt((ref.double() ** 2).mean().item()), 10 * math.log10(rng * rng / max(mse, 1e-30))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--clips", type=int, default=2, help="timed clips per arm and round")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dpmpp_ab.txt"))
    args = ap.parse_args()
    from bench import gpu_random_state_dict
    from neurons_amd import _lib, DDIMScheduler, DPMSolverMultistepScheduler, NativeSparseCtrl, NativeUNet3D, NeuroclipsPipeline
    from neurons_amd.sparsectrl import controlnet_config_from_unet
    from neurons_amd.unet3d import UNet3DConfig, state_dict_schema
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ucfg = UNet3DConfig()
    ccfg = controlnet_config_from_unet(ucfg, dict(
        set_noisy_sample_input_to_zero=True, use_simplified_condition_embedding=True, conditioning_channels=4,
        motion_module_kwargs=dict(attention_block_types=["Temporal_Self"], temporal_position_encoding_max_len=32)))
    unet, ctrl = NativeUNet3D(ucfg).to(dev), NativeSparseCtrl(ccfg).to(dev)
    for net, cfg, kind, seed in ((unet, ucfg, _lib.NR_KIND_UNET3D, 1), (ctrl, ccfg, _lib.NR_KIND_SPARSECTRL, 2)):
        net.load_state_dict({k: v.cpu() for k, v in gpu_random_state_dict(state_dict_schema(cfg, kind), seed, dev).items()})
    torch.cuda.empty_cache()
    scheds = dict(ddim=DDIMScheduler(**KW), dpm=DPMSolverMultistepScheduler(**KW))
    pipe = NeuroclipsPipeline(vae=None, text_encoder=None, tokenizer=None, unet=unet, scheduler=scheds["ddim"], controlnet=ctrl).to(dev)
    g = torch.Generator(device=dev).manual_seed(1000)
    clips = [dict(latents=torch.randn(1, 4, F, L, L, generator=g, device=dev), noise=torch.randn(1, 4, F, L, L, generator=g, device=dev),
                  ctx=torch.randn(2, 77, ucfg.cross_attention_dim, generator=g, device=dev),
                  cimg=torch.randn(1, 4, 1, L, L, generator=g, device=dev) * 0.18215) for _ in range(1 + args.clips)]

    def run(kind, steps, c):
        pipe.scheduler = scheds[kind]
        return pipe("", video_length=F, height=L * 8, width=L * 8, num_inference_steps=steps, guidance_scale=8.5, latents=c["latents"],
                    noise=c["noise"], text_embeddings=c["ctx"], controlnet_images=c["cimg"], controlnet_image_index=[0], low_strength=0.3,
                    output_type="latent").videos

    lines = [f"DPM-Solver++ 2M (nr_cfg_dpmpp_step) against DDIM on the headline configuration: 1 clip, {F} frames, {L}x{L} latent, CFG 8.5, SparseCtrl on",
             f"one process, one GPU, arms alternating; per arm and round one untimed clip (plans, graphs), then {args.clips} timed clips",
             "weights are seeded random tensors: the distances below compare solvers on this engine and say NOTHING about the quality a real",
             "checkpoint gives at 20 - 25 steps", ""]

    def flush():
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    per = {name: [] for name, _, _ in ARMS}
    for r in range(args.rounds):
        for name, kind, steps in ARMS:
            run(kind, steps, clips[0])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for c in clips[1:]:
                out = run(kind, steps, c)
            torch.cuda.synchronize()
            s_clip = (time.perf_counter() - t0) / args.clips
            per[name].append((s_clip, 1e3 * s_clip / steps))
            lines.append(f"round {r} {name:9s} {s_clip:7.4f} s/clip  {1e3 * s_clip / steps:7.3f} ms/step  SparseCtrl group {pipe.last_controlnet_group}"
                         f"  finite {bool(torch.isfinite(out).all())}")
            print(lines[-1], flush=True)
            flush()
    lines += ["", "mean over rounds (min .. max):"]
    base_s = sum(v[0] for v in per["DDIM-50"]) / args.rounds
    base_m = sum(v[1] for v in per["DDIM-50"]) / args.rounds
    for name, _, steps in ARMS:
        s = [v[0] for v in per[name]]
        m = [v[1] for v in per[name]]
        mean_s, mean_m = sum(s) / len(s), sum(m) / len(m)
        lines.append(f"  {name:9s} {mean_s:7.4f} s/clip ({min(s):.4f} .. {max(s):.4f})   {mean_m:7.3f} ms/step ({min(m):.3f} .. {max(m):.3f})"
                     f"   per step vs DDIM-50 {100 * (mean_m / base_m - 1):+.2f} %   clips/s vs DDIM-50 x{base_s / mean_s:.2f}")
    flush()

    lines += ["", "distance of the final latents to a 200-step DDIM run of the same engine (clip 1; rel-L2, PSNR over the reference's range).",
              "Each run is noised to its own first timestep (low_strength: DDIM-200 996, DDIM-25 961, DDIM-20 951, DPM++ 999), as the pipeline does:"]
    ref = run("ddim", 200, clips[1]).clone()
    for name, kind, steps in (("DDIM-25", "ddim", 25), ("DPM++-25", "dpm", 25), ("DDIM-20", "ddim", 20), ("DPM++-20", "dpm", 20), ("DDIM-50", "ddim", 50)):
        rel, psnr = distance(run(kind, steps, clips[1]), ref)
        lines.append(f"  {name:9s} rel-L2 {rel:.4e}   PSNR {psnr:6.2f} dB")
        print(lines[-1], flush=True)
    flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
