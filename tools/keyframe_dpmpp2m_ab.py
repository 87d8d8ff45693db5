"""ms per step and ms per keyframe of the sgm keyframe loop under its two samplers, on the configuration of ``bench.py --workload keyframe`` (BASELINE
config 3: one keyframe per loop, 64x64 latent = 512x512 pixels, CFG 5.0, context 256x1664, unclip6.yaml width, random-init weights; no decode, as in
bench.py).

Arms, in ONE process on one network handle, alternating, every arm ``--rounds`` times after one warm-up keyframe each:
  euler38    ``EulerEDMSampler(38)(net, z, cond=, uc=)``: the call bench.py times, i.e. the parent commit's code path; the yardstick of this run
  dpmpp2m38  ``DPMPP2MSampler(38)``: same table, same network evaluations, nr_edm_cfg_dpmpp2m_step instead of nr_edm_cfg_euler_step per step
  dpmpp2m19  ``DPMPP2MSampler(19)``: half the evaluations
  euler19    ``EulerEDMSampler(19)``: the control for dpmpp2m19's ms per step.  Whatever a keyframe pays once, outside its steps, 19 steps amortise half as well
             as 38 under either sampler; the report separates the two from the pairs of step counts
The 2M step reads and writes one more fp32 array of n floats than the Euler step; its ms per step is expected inside the spread of the repeated
Euler arms.  Nothing here is gated and nothing is said about image quality (random weights); the report goes to --out.

Usage:  python tools/keyframe_dpmpp2m_ab.py [--rounds 4] [--keyframes 1] [--out profiles/keyframe_dpmpp2m_ab.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LATENT = 64
ARMS = (("euler38", "EulerEDMSampler", 38), ("dpmpp2m38", "DPMPP2MSampler", 38), ("dpmpp2m19", "DPMPP2MSampler", 19),
        ("euler19", "EulerEDMSampler", 19))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--keyframes", type=int, default=1, help="timed keyframes per arm and round")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keyframe_dpmpp2m_ab.txt"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from neurons_amd import sgm
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg = sgm.SGMUNetConfig()
    g = torch.Generator(device=dev).manual_seed(3)
    sd = {}
    for k, shape in sgm.sgm_state_dict_schema(cfg).items():          # bench.py: keyframe_main's weights
        z = torch.randn(shape, generator=g, device=dev)
        if k.endswith(".bias"):
            z = 0.02 * z
        elif len(shape) == 1:
            z = 1.0 + 0.1 * z
        else:
            z = z / (int(np.prod(shape[1:])) ** 0.5)
        sd[k] = z.cpu()
    net = sgm.NativeSGMUNet(cfg).to(dev)
    net.load_state_dict(sd)
    del sd
    L = LATENT
    it = dict(z=torch.randn(1, 4, L, L, generator=g, device=dev),
              c={"crossattn": torch.randn(1, 256, 1664, generator=g, device=dev), "vector": torch.randn(1, 1024, generator=g, device=dev)},
              uc={"crossattn": torch.randn(1, 256, 1664, generator=g, device=dev), "vector": torch.randn(1, 1024, generator=g, device=dev)})
    samplers = {name: getattr(sgm, cls)(num_steps=steps, scale=5.0) for name, cls, steps in ARMS}
    steps_of = {name: steps for name, _, steps in ARMS}
    finite = {}
    for name, s in samplers.items():                                 # warm-up: plans, and the per-step graph slots of both tables
        finite[name] = bool(torch.isfinite(s(net, it["z"], cond=it["c"], uc=it["uc"])).all())
    torch.cuda.synchronize()
    ms = {name: [] for name in samplers}
    for _ in range(args.rounds):
        for name, s in samplers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.keyframes):
                s(net, it["z"], cond=it["c"], uc=it["uc"])
            torch.cuda.synchronize()
            ms[name].append(1e3 * (time.perf_counter() - t0) / args.keyframes)
    lines = [f"# keyframe sampler A/B (BASELINE config 3 shape): {L}x{L} latent, one keyframe per loop, CFG 5.0, random-init weights; one process, arms "
             f"alternating, {args.rounds} rounds of {args.keyframes} keyframe(s) per arm after one warm-up keyframe each",
             "# arm         steps   ms per keyframe, every round" + " " * max(0, 9 * args.rounds - 28) + "    mean ms/keyframe   ms/step (mean)   min .. max ms/step"]
    per_step = {}
    for name in samplers:
        n = steps_of[name]
        per_step[name] = [v / n for v in ms[name]]
        mean = sum(ms[name]) / len(ms[name])
        lines.append(f"{name:11s} {n:5d}   " + " ".join(f"{v:8.2f}" for v in ms[name]) + f"   {mean:12.2f}   {mean / n:12.3f}        "
                     f"{min(per_step[name]):.3f} .. {max(per_step[name]):.3f}   finite={finite[name]}")
    e = per_step["euler38"]
    e_mean, spread = sum(e) / len(e), max(e) - min(e)
    for name in ("dpmpp2m38", "dpmpp2m19"):
        d = sum(per_step[name]) / len(per_step[name]) - e_mean
        lines.append(f"# {name}: ms/step minus euler38's {d:+.3f} ms; spread (max - min) of the repeated euler38 arms {spread:.3f} ms: "
                     f"{'inside' if abs(d) <= spread else 'OUTSIDE'} it")
    d = sum(per_step["dpmpp2m19"]) / len(per_step["dpmpp2m19"]) - sum(per_step["euler19"]) / len(per_step["euler19"])
    e19 = per_step["euler19"]
    lines.append(f"# dpmpp2m19: ms/step minus euler19's {d:+.3f} ms; spread of the repeated euler19 arms {max(e19) - min(e19):.3f} ms: "
                 f"{'inside' if abs(d) <= max(e19) - min(e19) else 'OUTSIDE'} it")
    for a, b in (("euler38", "euler19"), ("dpmpp2m38", "dpmpp2m19")):
        ka, kb = sum(ms[a]) / len(ms[a]), sum(ms[b]) / len(ms[b])
        step = (ka - kb) / (steps_of[a] - steps_of[b])
        lines.append(f"# {a} against {b}: {step:.3f} ms per additional step, {kb - steps_of[b] * step:.2f} ms per keyframe outside the steps")
    k38, k19 = sum(ms["euler38"]) / len(ms["euler38"]), sum(ms["dpmpp2m19"]) / len(ms["dpmpp2m19"])
    lines.append(f"# ms per keyframe: dpmpp2m19 / euler38 = {k19 / k38:.3f} (evaluations 19 / 38 = 0.500).  Which step count keeps keyframe quality is not "
                 "measured here: no trained checkpoint; see DESIGN section 7")
    open(args.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
