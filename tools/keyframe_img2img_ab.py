"""Keyframes/s of the sgm keyframe path started from an init image, on the configuration of ``bench.py --workload keyframe`` (one keyframe per
Euler loop, 64x64 latent = 512x512 pixels, 50 Euler steps, CFG 5.0, context 256x1664, unclip6.yaml width, random-init weights).

Arms, one fresh process each, alternating, every arm ``--rounds`` times:
  plain    the call bench.py times: ``sampler(net, z, cond=, uc=)`` from pure noise (the figure to hold against ``bench.py --workload keyframe`` of
           the parent commit, run from a checkout of it on the same box)
  s1.0 / s0.75 / s0.5
           ``unclip_sample(engine, ..., init=<512x512 image>, strength=s)``: one first-stage encode, the start kernel (nr_edm_img2img_start),
           then len(pruned sigma table) - 1 Euler steps.  No decode, as in bench.py
Every img2img arm also times the encode alone at 512x512 and 768x768.  Nothing here is gated; the report goes to --out.

Usage:  python tools/keyframe_img2img_ab.py [--rounds 2] [--steps 3] [--warmup 1] [--out profiles/keyframe_img2img_ab.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LATENT, EULER_STEPS = 64, 50
ARMS = ("plain", "s1.0", "s0.75", "s0.5")


def child(args):
    import numpy as np
    import torch
    from neurons_amd.sgm import NativeDiffusionEngine, SGMUNetConfig, sgm_state_dict_schema, unclip_sample
    from neurons_amd.synth import gpu_random_state_dict
    from neurons_amd.vae import VAEDecoderConfig, vae_encoder_state_dict_schema
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg = SGMUNetConfig()
    g = torch.Generator(device=dev).manual_seed(3)
    sd = {}
    for k, shape in sgm_state_dict_schema(cfg).items():          # bench.py: keyframe_main's weights
        z = torch.randn(shape, generator=g, device=dev)
        if k.endswith(".bias"):
            z = 0.02 * z
        elif len(shape) == 1:
            z = 1.0 + 0.1 * z
        else:
            z = z / (int(np.prod(shape[1:])) ** 0.5)
        sd[k] = z.cpu()
    eng = NativeDiffusionEngine(network_config=cfg, num_steps=EULER_STEPS, scale=5.0).to(dev)
    net = eng.model.diffusion_model
    net.load_state_dict(sd)
    del sd
    L = LATENT
    items = []
    for _ in range(args.warmup + args.steps):
        items.append(dict(z=torch.randn(1, 4, L, L, generator=g, device=dev), noise=torch.randn(1, 4, L, L, generator=g, device=dev),
                          enc_noise=torch.randn(1, 4, L, L, generator=g, device=dev), offset=torch.randn(1, generator=g, device=dev),
                          img=torch.rand(1, 3, 8 * L, 8 * L, generator=g, device=dev) * 2 - 1,
                          tokens=torch.randn(1, 256, 1664, generator=g, device=dev), uc_tokens=torch.randn(1, 256, 1664, generator=g, device=dev),
                          vec=torch.randn(1, 1024, generator=g, device=dev)))
    res = {"arm": args.arm}
    if args.arm == "plain":
        def run(it):
            return eng.sampler(net, it["z"], cond={"crossattn": it["tokens"], "vector": it["vec"]}, uc={"crossattn": it["uc_tokens"], "vector": it["vec"]})
        res["euler_steps"] = EULER_STEPS
    else:
        from neurons_amd.sgm import Img2ImgDiscretizationWrapper
        s = float(args.arm[1:])
        eng.first_stage_encoder.load_state_dict({k: v.cpu() for k, v in gpu_random_state_dict(vae_encoder_state_dict_schema(VAEDecoderConfig()), 9, dev).items()})
        res["euler_steps"] = len(Img2ImgDiscretizationWrapper(eng.sampler.discretization, s)(EULER_STEPS)) - 1

        def run(it):
            return unclip_sample(eng, it["tokens"], it["vec"], None, it["noise"], it["uc_tokens"], eng.sampler, offset_noise=it["offset"],
                                 offset_noise_level=0.04, init=it["img"], strength=s, enc_noise=it["enc_noise"])
    for it in items[:args.warmup]:
        run(it)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for it in items[args.warmup:]:
        out = run(it)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    res.update(keyframes_per_s=round(args.steps / el, 4), ms_per_keyframe=round(1e3 * el / args.steps, 2), finite=bool(torch.isfinite(out).all()))
    if args.arm != "plain":
        for px in (512, 768):
            x = torch.rand(1, 3, px, px, generator=g, device=dev) * 2 - 1
            eng.encode_first_stage_moments(x)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(5):
                eng.encode_first_stage_moments(x)
            torch.cuda.synchronize()
            res[f"encode_{px}_ms"] = round(1e3 * (time.perf_counter() - t0) / 5, 2)
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", choices=ARMS)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--steps", type=int, default=3, help="timed keyframes per process")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keyframe_img2img_ab.txt"))
    ap.add_argument("--child-timeout", type=int, default=400)
    args = ap.parse_args()
    if args.arm:
        return child(args)
    lines = [f"# keyframe img2img A/B: {LATENT}x{LATENT} latent, {EULER_STEPS} Euler steps, one keyframe per loop; {args.steps} timed keyframes after "
             f"{args.warmup} warm-up per process"]
    results = []
    for r in range(args.rounds):
        for arm in ARMS:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--arm", arm, "--steps", str(args.steps), "--warmup", str(args.warmup)],
                               capture_output=True, text=True, timeout=args.child_timeout)
            got = [ln[len("RESULT "):] for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not got:
                lines.append(f"round {r} arm {arm}: FAILED rc={p.returncode}: {p.stderr.strip().splitlines()[-3:]}")
                open(args.out, "w").write("\n".join(lines) + "\n")
                print(lines[-1], flush=True)
                return 1                                          # nothing more is started on the GPU after a failed arm
            res = json.loads(got[0])
            results.append(res)
            lines.append(f"round {r} " + json.dumps(res))
            print(lines[-1], flush=True)
            open(args.out, "w").write("\n".join(lines) + "\n")
    lines.append("# per arm: keyframes/s of every round; ms per keyframe (mean); Euler steps")
    for arm in ARMS:
        rs = [x for x in results if x["arm"] == arm]
        lines.append(f"{arm:6s} " + "  ".join(f"{x['keyframes_per_s']:.4f}" for x in rs) + f"   {sum(x['ms_per_keyframe'] for x in rs) / len(rs):9.2f} ms"
                     f"   {rs[0]['euler_steps']} steps")
    open(args.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines[-5:]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
