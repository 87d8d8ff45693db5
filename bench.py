#!/usr/bin/env python
"""bench.py — headline benchmark of the NEURONS video-denoising hot path on MI355X.

Metric (BASELINE.json): denoising frames/sec on 16-frame 256x256 clips, 50 DDIM steps.
One "step" of this script = ONE CLIP through the whole hot path: 50 x {SparseCtrl forward, temporal U-Net
forward on the CFG-doubled batch, CFG combine + DDIM update} on a (1,4,16,32,32) latent — BASELINE config 2.
Inputs (latents, noise, text context, keyframe latent) are synthetic and resident in HBM before the timed
region; weights are seeded random tensors of the reference architecture (1 277 M + 497 M parameters).

    python bench.py --gpus N --steps K --warmup W
N > 1: either under torch.distributed.run (one rank per GPU), or bare (`python bench.py --gpus N`): the script then starts its own N
rank processes before touching a GPU (self_launch) and forwards rank 0's line.  Clips shard across ranks with no data-path
collective (weak scaling); rank 0 converts the weights once and broadcasts the bf16 arenas device-to-device over RCCL before timing.

Prints ONE JSON line (rank 0).  A plain run does only what that line's headline needs: set up, warm up, time --steps clips, print.
SparseCtrl is evaluated several (50 steps: 5) DDIM steps at a time (pipeline.controlnet_group_size): all 50 evaluations per clip are
computed inside the timed region.

    --dump-outputs DIR   after the timed steps, the arrays the timed path returned in its last step go to DIR/<name>.npy (float32, at most
                         64 MB in all; a larger output is written as a fixed seeded sample).  Inputs and weights are seeded: the same
                         arguments give the same inputs on every run, so two builds can be compared output for output.
    --full               everything else the benchmark measures, each leg after the timed region (--no-op-profile, --no-psnr,
                         --no-cpu-baseline, --no-end-to-end leave single legs out).  Extra objects:
  roofline     dominant kernel class = the MFMA implicit-GEMM (conv/Linear): algorithmic FLOPs / summed launch
               time, measured with one HIP event pair per launch on the launch stream (nr_net_profile_last, a replay of its own).
  cpu_baseline the oracle (fp32 torch restatement of the reference graph, eager, math attention) timed on the host
               cores for a bounded sample and scaled to the clip.  The same oracle leg also CHECKS the clip just timed
               (config.psnr_c2_vs_fp32_oracle_db: final latents vs the oracle run in fp32 on the GPU, outside the timed region);
               --no-cpu-baseline skips the whole leg.
  end_to_end   the same clips through the whole __call__ (native CLIP -> loop -> native VAE decode -> .videos).
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_BF16_TFLOPS = 2500.0   # MI355X dense bf16 MFMA (guides/MI355X_MICROARCH.md)
PEAK_HBM_GBS = 8000.0


def current_round():
    """Label of the newest round that has ANY evidence file under profiles/ ("r06" from profiles/r06_*): a committed traffic file whose
    label is older than that (a round that kept profiles but forgot its PMC pass) is reported as historical.  Derived, not a constant to edit."""
    import glob
    import re
    labels = [m.group(1) for f in glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_*"))
              for m in [re.match(r"(r\d\d)_", os.path.basename(f))] if m]
    return max(labels) if labels else None


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3, help="timed clips per GPU")
    ap.add_argument("--warmup", type=int, default=1, help="untimed clips per GPU")
    ap.add_argument("--ddim-steps", type=int, default=50)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--latent", type=int, default=32, help="latent side (pixels/8)")
    ap.add_argument("--batch", type=int, default=1, help="clips per pipeline call (BASELINE config 4 runs 8 clips/GPU; headline = 1); "
                                                         "--workload keyframe: keyframes per Euler loop (utils.unclip_recon's num_samples)")
    ap.add_argument("--full", action="store_true",
                    help="also run what the headline does not need, after the timed region: the per-launch event pass (roofline), the PSNR legs, "
                         "the CPU baseline and the end-to-end leg (the --no-* switches below leave single legs out)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the arrays the timed path returned in its last step to DIR/<name>.npy (float32, at most 64 MB in all)")
    ap.add_argument("--no-end-to-end", action="store_true",
                    help="with --full: skip the end-to-end leg of the headline run (native CLIP _encode_prompt -> loop -> native VAE decode -> .videos, SURVEY 8d)")
    ap.add_argument("--attn-fp8", action="store_true", help="BASELINE config 5: spatial/cross attention on OCP e4m3 MFMA operands (bf16 is the default)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline (and the oracle check of the timed clip)")
    ap.add_argument("--no-psnr", action="store_true", help="with --full: skip the PSNR runs (profiling passes: keeps tiny-network launches out)")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--no-controlnet", action="store_true",
                    help="DIAGNOSTIC (not BASELINE config 2): the loop without SparseCtrl, to read what the second stream costs the U-Net's chain; "
                         "the line says so in config.workload")
    ap.add_argument("--no-op-profile", action="store_true",
                    help="with --full: skip the per-launch HIP-event pass and every other leg after the timed region, as a plain run does "
                         "(rocprofv3 runs: keeps the launch counts of the trace at exactly the timed steps); the roofline object is then omitted")
    ap.add_argument("--workload", choices=["video", "keyframe", "vae", "enhance"], default="video",
                    help="video = BASELINE config 2 (headline); keyframe = config 3: sgm unCLIP U-Net, Euler-EDM + CFG 5.0; "
                         "vae = the first-stage round trip of one clip (SURVEY 8f rank 1): encode 16 frames + decode 16 frames; "
                         "enhance = one GPU's share of BASELINE config 4: --batch keyframes in one Euler loop, then --batch clips in one call, decoded")
    ap.add_argument("--keyframe-steps", type=int, default=50)
    ap.add_argument("--keyframe-latent", type=int, default=64, help="64 = BASELINE config 3 (512 px); 96 = reference-faithful (768 px, 38 steps)")
    ap.add_argument("--self-launch", action="store_true",
                    help="start the rank processes from this process even for --gpus 1 (tests/test_dist_gpu.py: the N > 1 launcher with a world of one)")
    ap.add_argument("--launch-dry-run", action="store_true",
                    help="rank processes only rendezvous (gloo, CPU), shard a clip list, reduce a timing scalar and exit: the launcher and the "
                         "rank logic without a GPU (tests/test_bench_launch.py)")
    ap.add_argument("--launch-timeout", type=float, default=3600.0, help="self-launch: seconds before the rank processes are stopped")
    return ap.parse_args()


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir, arrays, limit=DUMP_LIMIT_BYTES):
    """--dump-outputs: each tensor of `arrays` (name -> tensor) as out_dir/<name>.npy in float32.  Every array gets an equal share of
    `limit` bytes; one larger than its share is written as a sample of its flattened elements at fixed seeded positions (the same
    positions on every run), so two builds compare the same elements."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    share = limit // len(arrays)
    for name, t in arrays.items():
        a = t.detach().float().cpu().numpy()
        if a.nbytes > share:
            idx = np.sort(np.random.default_rng(0).choice(a.size, share // a.itemsize, replace=False))
            print(f"bench.py: {name} {list(a.shape)} written as a seeded sample of {idx.size} of its {a.size} elements", file=sys.stderr)
            a = a.reshape(-1)[idx]
        np.save(os.path.join(out_dir, name + ".npy"), a)


def count_gpus_without_runtime(topology="/sys/class/kfd/kfd/topology/nodes"):
    """GPUs this process would see, from the KFD topology (nodes with simd_count > 0) cut down by HIP_VISIBLE_DEVICES /
    ROCR_VISIBLE_DEVICES / CUDA_VISIBLE_DEVICES — no HIP runtime call (torch.cuda.device_count() may fall back to hipGetDeviceCount,
    which initialises the runtime).  None when the topology cannot be read."""
    try:
        n = 0
        for node in sorted(os.listdir(topology)):
            with open(os.path.join(topology, node, "properties")) as f:
                props = dict(ln.split(None, 1) for ln in f.read().splitlines() if " " in ln)
            if int(props.get("simd_count", "0").strip()) > 0:
                n += 1
    except (OSError, ValueError):
        return None
    for var in ("ROCR_VISIBLE_DEVICES", "HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        v = os.environ.get(var)
        if v is not None:
            n = min(n, len([x for x in v.split(",") if x.strip() != ""]))
    return n


def self_launch(args):
    """`python bench.py --gpus N` with no launcher around it: start N FRESH rank processes of this same script (one per GPU, the layout
    `accelerate launch` gives the reference: /root/reference/train_neurons.sh:92-96, scripts/neuroclips_video.py:39-40,323) and wait.
    This parent makes no HIP-runtime call at all, not even through torch (GPUs are counted from the KFD topology in sysfs; when that is unreadable the check is
    skipped and a rank fails instead) and never exec's: the ranks are children, rank 0's stdout (the ONE JSON line) is forwarded, every
    other stream goes to stderr, the exit code is non-zero if any rank failed.  Do not run the self-launcher under rocprofv3: the
    profiler's preloaded library initialises the GPU in this parent before the ranks exist (profile a rank: `--gpus 1`, or torchrun)."""
    import signal
    import socket
    import subprocess
    import threading
    n = args.gpus
    if not args.launch_dry_run:
        have = count_gpus_without_runtime()
        if have is not None and have < n:
            raise SystemExit(f"--gpus {n} but this node shows {have} GPU(s)")
    # the rendezvous port: probed free here, bound by rank 0 a moment later (a small window another process could take it in: the ranks then
    # fail the rendezvous and the launcher reports it; a caller that needs certainty sets MASTER_PORT itself)
    if os.environ.get("MASTER_PORT", "").isdigit() and "RANK" not in os.environ:
        port = int(os.environ["MASTER_PORT"])
    else:
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
    argv = [a for a in sys.argv[1:] if a != "--self-launch"]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0", NR_BENCH_RANK_PROCESS="1")
        if n == 1:
            env["NR_DIST_FORCE"] = "1"        # a world of one still takes the RCCL path (init, broadcasts, all-reduce, barriers)
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv, env=env, cwd=os.getcwd(),
                                      stdout=subprocess.PIPE if r == 0 else sys.stderr, stderr=sys.stderr, text=True))

    def _stop(signum, frame):                # the launcher is told to stop (driver timeout): take exactly our own ranks along
        for p in procs:
            if p.poll() is None:
                p.terminate()
        raise SystemExit(128 + signum)
    signal.signal(signal.SIGTERM, _stop)
    signal.signal(signal.SIGINT, _stop)
    out0 = []
    reader = threading.Thread(target=lambda: out0.extend(procs[0].stdout.readlines()), daemon=True)
    reader.start()
    deadline = time.time() + args.launch_timeout
    failed = None
    while True:
        codes = [p.poll() for p in procs]
        bad = [(r, c) for r, c in enumerate(codes) if c not in (None, 0)]
        if bad:
            failed = f"rank {bad[0][0]} exited with code {bad[0][1]}"
            break
        if all(c == 0 for c in codes):
            break
        if time.time() > deadline:
            failed = f"rank processes still running after {args.launch_timeout:.0f} s"
            break
        time.sleep(0.2)
    if failed:
        for p in procs:                      # exactly the PIDs started above
            if p.poll() is None:
                p.terminate()
        for p in procs:
            try:
                p.wait(timeout=20)
            except subprocess.TimeoutExpired:
                p.kill()
    reader.join(timeout=10)
    lines = [ln for ln in out0 if ln.startswith("{")]
    for ln in out0:
        if not ln.startswith("{"):
            sys.stderr.write(ln)
    if failed:
        sys.stderr.write(f"bench.py self-launch: {failed}\n")
        raise SystemExit(1)
    if len(lines) != 1:
        sys.stderr.write(f"bench.py self-launch: rank 0 printed {len(lines)} JSON lines, expected one\n")
        raise SystemExit(1)
    sys.stdout.write(lines[0])
    sys.stdout.flush()


def launch_dry_run(args):
    """One rank of `--launch-dry-run`: the rendezvous, the clip sharding and the timing reduction of the real run on gloo / CPU tensors."""
    import torch.distributed as dist
    from neurons_amd.distributed import clip_indices_for_rank, max_over_ranks
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    if os.environ.get("NR_LAUNCH_DRY_RUN_FAIL_RANK") == str(rank):      # test hook: a rank that dies before the rendezvous
        raise SystemExit(3)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    seen = torch.ones(1)
    dist.all_reduce(seen)
    mine = clip_indices_for_rank(world * args.steps, rank, world)
    slowest = max_over_ranks(1.0 + rank)
    gathered = [None] * world
    dist.all_gather_object(gathered, (rank, int(os.environ["LOCAL_RANK"]), mine))
    dist.barrier()
    dist.destroy_process_group()
    if rank == 0:
        print(json.dumps({"metric": "launcher dry run (no GPU work)", "value": 0.0, "unit": "frames/s", "n_gpus": world, "steps": args.steps,
                          "warmup": args.warmup, "ranks_seen": int(seen.item()), "slowest_rank_time": slowest,
                          "ranks": [{"rank": r, "local_rank": lr, "clips": c} for r, lr, c in gathered]}))


def vae_main(args):
    """SURVEY §8f rank 1 (single GPU): one step = encode the clip's 16 blurry frames (scripts/neuroclips_video.py:267) and
    decode its 16 denoised frames (decode_latents), both through the C ABI.  Prints one JSON line with frames/s."""
    from neurons_amd.vae import NativeVAEDecoder, NativeVAEEncoder, VAEDecoderConfig, vae_decoder_state_dict_schema, vae_encoder_state_dict_schema
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg = VAEDecoderConfig()
    dsd = gpu_random_state_dict(vae_decoder_state_dict_schema(cfg), 3, dev)
    esd = gpu_random_state_dict(vae_encoder_state_dict_schema(cfg), 4, dev)
    dec, enc = NativeVAEDecoder(cfg).to(dev), NativeVAEEncoder(cfg).to(dev)
    dec.load_state_dict({k: v.cpu() for k, v in dsd.items()})
    enc.load_state_dict({k: v.cpu() for k, v in esd.items()})
    F, L = args.frames, args.latent
    g = torch.Generator(device=dev).manual_seed(5)
    items = [(torch.rand(F, 3, L * 8, L * 8, generator=g, device=dev), torch.randn(1, 4, F, L, L, generator=g, device=dev) * 0.18215)
             for _ in range(args.warmup + args.steps)]

    def step(img, lat):
        z = enc.encode(img, in_mul=2.0, in_add=-1.0).sample(generator=g, scale=0.18215)
        return z, dec.decode_latents(lat)

    for it in items[:args.warmup]:
        step(*it)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    for it in items[args.warmup:]:
        z, vid = step(*it)
    torch.cuda.synchronize()
    el = time.perf_counter() - t1
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, {"latents": z, "decoded": vid})
    res = {
        "metric": "first-stage VAE frames/sec (encode + decode of a 16f x 256^2 clip)", "value": round(args.steps * F / el, 3), "unit": "frames/s",
        "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(1e3 * el / args.steps, 3), "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
        "config": {"workload": f"SURVEY 8f rank 1: encode {F} x 3x{L * 8}x{L * 8} images + decode ({F},4,{L},{L}) latents, SD-1.5 VAE "
                               f"(ch 128, mult 1,2,4,4), random-init weights", "output_finite": bool(torch.isfinite(vid).all() and torch.isfinite(z).all())}}
    if args.full:
        pd, pe = dec.profile_last(), enc.profile_last()
        ig_ms = pd["igemm"]["ms"] + pe["igemm"]["ms"]
        ig_fl = pd["igemm"]["flops"] + pe["igemm"]["flops"]
        res["roofline"] = {"bound": "mfma", "kernel": "igemm_bf16_kernel (3x3 conv)", "achieved": round(ig_fl / (ig_ms * 1e-3) / 1e12, 2),
                           "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s", "frac": round(ig_fl / (ig_ms * 1e-3) / 1e12 / PEAK_BF16_TFLOPS, 4), "traffic": None,
                           "per_class_ms": {"decode": {k: round(v["ms"], 3) for k, v in pd.items()}, "encode": {k: round(v["ms"], 3) for k, v in pe.items()}}}
    if args.full and not args.no_cpu_baseline:
        from oracle import vae_oracle as V
        hd = {k: v.cpu() for k, v in dsd.items()}
        he = {k: v.cpu() for k, v in esd.items()}
        with torch.no_grad():
            t0 = time.perf_counter()
            V.encode_moments(he, 2 * items[0][0][:1].cpu() - 1, 4, 2)
            V.decode(hd, items[0][1][:, :, 0].cpu() / 0.18215, 4, 2)
            dt = time.perf_counter() - t0
        res["cpu_baseline"] = {"value": round(1.0 / dt, 4), "unit": "frames/s", "cores": torch.get_num_threads(), "kind": "port",
                               "sample": f"oracle encode + decode of ONE {L * 8}x{L * 8} frame took {dt:.2f} s on {torch.get_num_threads()} threads"}
    print(json.dumps(res))


def keyframe_main(args):
    """BASELINE config 3 (single GPU): one keyframe = `keyframe_steps` x {sgm UNetModel on the CFG batch of 2 + fused
    EDM/CFG/Euler update}.  Prints one JSON line with keyframes/s."""
    import numpy as np
    from neurons_amd.sgm import EulerEDMSampler, NativeSGMUNet, SGMUNetConfig, sgm_state_dict_schema
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg = SGMUNetConfig()
    g = torch.Generator(device=dev).manual_seed(3)
    sd = {}
    for k, shape in sgm_state_dict_schema(cfg).items():
        z = torch.randn(shape, generator=g, device=dev)
        if k.endswith(".bias"):
            z = 0.02 * z
        elif len(shape) == 1:
            z = 1.0 + 0.1 * z
        else:
            z = z / (int(np.prod(shape[1:])) ** 0.5)
        sd[k] = z.cpu()
    net = NativeSGMUNet(cfg).to(dev)
    net.load_state_dict(sd)
    cpu_leg = args.full and not args.no_cpu_baseline
    if not cpu_leg:
        del sd
    L = args.keyframe_latent
    B = args.batch          # keyframes per Euler loop = CFG batch 2B (utils.unclip_recon's num_samples, utils.py:302-303,316-321)
    sampler = EulerEDMSampler(num_steps=args.keyframe_steps, scale=5.0)
    items = []
    for _ in range(args.warmup + args.steps):
        items.append(dict(z=torch.randn(B, 4, L, L, generator=g, device=dev),
                          c={"crossattn": torch.randn(B, 256, 1664, generator=g, device=dev), "vector": torch.randn(B, 1024, generator=g, device=dev)},
                          uc={"crossattn": torch.randn(B, 256, 1664, generator=g, device=dev), "vector": torch.randn(B, 1024, generator=g, device=dev)}))
    for it in items[:args.warmup]:
        sampler(net, it["z"], cond=it["c"], uc=it["uc"])
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    for it in items[args.warmup:]:
        out = sampler(net, it["z"], cond=it["c"], uc=it["uc"])
    torch.cuda.synchronize()
    el = time.perf_counter() - t1
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, {"samples": out})
    cpu = None
    if cpu_leg:
        # the oracle's UNetModel forward (fp32, eager) on the host cores: ONE full Euler step of this configuration (CFG batch of 2),
        # scaled by the step count only
        from oracle import sgm_oracle as S
        it = items[-1]
        x2 = torch.cat([it["z"][:1], it["z"][:1]]).cpu()
        ctx2 = torch.cat([it["uc"]["crossattn"][:1], it["c"]["crossattn"][:1]]).cpu()
        y2 = torch.cat([it["uc"]["vector"][:1], it["c"]["vector"][:1]]).cpu()
        ts = torch.full((2,), 500.0)
        with torch.no_grad():
            t0 = time.perf_counter()
            S.unet_forward(sd, cfg, x2, ts, ctx2, y2)
            dt = time.perf_counter() - t0
        cpu = {"value": round(1.0 / (dt * args.keyframe_steps), 5), "unit": "keyframes/s", "cores": torch.get_num_threads(), "kind": "port",
               "sample": f"one full Euler step (oracle/sgm_oracle.py unet_forward, CFG batch 2, ({L},{L}) latent, context 256x1664) = {dt:.1f} s, "
                         f"x {args.keyframe_steps} steps"}
        del sd
    res = {
        "metric": "unCLIP keyframes/sec (sgm UNetModel, Euler-EDM, CFG 5.0)", "value": round(args.steps * B / el, 4), "unit": "keyframes/s",
        "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(1e3 * el / args.steps, 2),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
        "config": {"workload": f"BASELINE config 3: {B} keyframe(s) per Euler loop, ({B},4,{L},{L}) latent (CFG batch {2 * B}), {args.keyframe_steps} Euler steps, "
                               f"context 256x1664, 2 501 M-parameter UNetModel, random-init weights",
                   "keyframes_per_call": B, "ms_per_euler_step": round(1e3 * el / args.steps / args.keyframe_steps, 3),
                   "ms_per_keyframe_step": round(1e3 * el / args.steps / args.keyframe_steps / B, 3), "output_finite": bool(torch.isfinite(out).all()),
                   "resident_weight_gb": round(net.weight_bytes() / 1e9, 2)}}
    if args.full:
        p = net.profile_last()
        ig = p["igemm"]
        res["roofline"] = {"bound": "mfma", "kernel": "igemm_bf16_kernel", "achieved": round(ig["flops"] / (ig["ms"] * 1e-3) / 1e12, 2),
                           "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s", "frac": round(ig["flops"] / (ig["ms"] * 1e-3) / 1e12 / PEAK_BF16_TFLOPS, 4),
                           # the event pass launches eagerly (one HIP event pair per launch): with ~730 launches of ~10 us the HOST can be the slower side,
                           # and the intervals then contain idle time (their sum exceeds the replayed graph's step).  Second reading: the class keeps its
                           # share of the event pass, applied to the step as the timed region ran it.
                           "event_pass_ms_per_step": round(sum(v["ms"] for v in p.values()), 3),
                           "replayed_graph_ms_per_step": round(1e3 * el / args.steps / args.keyframe_steps, 3),
                           "frac_of_replayed_step_share": round(ig["flops"] / (1e-3 * (1e3 * el / args.steps / args.keyframe_steps) * ig["ms"] /
                                                                               max(sum(v["ms"] for v in p.values()), 1e-9)) / 1e12 / PEAK_BF16_TFLOPS, 4),
                           "traffic": keyframe_traffic(B, L), "per_class_ms_per_step": {k: round(v["ms"], 3) for k, v in p.items()},
                           "launches_per_step": int(sum(v["launches"] for v in p.values())),
                           "algorithmic_gbytes_per_step": round(sum(v["bytes"] for v in p.values()) / 1e9, 2),
                           "algorithmic_tflop_per_step": round(sum(v["flops"] for v in p.values()) / 1e12, 3)}
    if cpu:
        res["cpu_baseline"] = cpu
    print(json.dumps(res))


from neurons_amd.synth import gpu_random_state_dict  # noqa: E402

class _BenchTokenizer:
    """Stand-in for the CLIP BPE tokenizer (no vocabulary files offline): fixed-length ids, BOS / EOS framing, one hashed id per word.
    Tokenisation is host string work outside the measured path; what the pipeline needs is the call surface (pipeline_neuroclips.py:156-166)."""
    model_max_length = 77

    def __call__(self, text, padding=None, max_length=None, truncation=None, return_tensors=None):
        import types
        import zlib
        texts = [text] if isinstance(text, str) else list(text)
        L = self.model_max_length
        ids = torch.full((len(texts), L), 49407, dtype=torch.long)
        for i, t in enumerate(texts):
            words = [1000 + zlib.crc32(w.encode()) % 40000 for w in t.split()][:L - 2]
            ids[i, 0] = 49406
            if words:
                ids[i, 1:1 + len(words)] = torch.tensor(words)
        return types.SimpleNamespace(input_ids=ids, attention_mask=torch.ones_like(ids))

    def batch_decode(self, ids):
        return ["" for _ in ids]


def build_text_and_vae(dev):
    """native CLIP text encoder (f3) and first-stage decoder (f1) at SD-1.5 size with seeded random weights"""
    from neurons_amd.clip import CLIPTextConfig, NativeCLIPTextModel, clip_state_dict_schema
    from neurons_amd.vae import NativeVAEDecoder, VAEDecoderConfig, vae_decoder_state_dict_schema
    tcfg, vcfg = CLIPTextConfig(), VAEDecoderConfig()
    te, vae = NativeCLIPTextModel(tcfg).to(dev), NativeVAEDecoder(vcfg).to(dev)
    te.load_state_dict({k: v.cpu() for k, v in gpu_random_state_dict(clip_state_dict_schema(tcfg), 7, dev).items()})
    vae.load_state_dict({k: v.cpu() for k, v in gpu_random_state_dict(vae_decoder_state_dict_schema(vcfg), 8, dev).items()})
    return te, vae


def end_to_end_leg(args, dev, unet, ctrl, sched, clips):
    """SURVEY 8d "also report end-to-end (__call__) time separately": the reference call includes _encode_prompt (pipeline_neuroclips.py:373-375)
    and decode_latents (:492, :242-255) around the denoising loop.  Same clips, same networks, all three stages native: CLIP text encoder ->
    50-step loop -> VAE decode -> .videos (a CPU fp32 tensor, as the reference returns it: the D2H copy of the pixels is inside)."""
    from neurons_amd import NeuroclipsPipeline
    F, L, Bc = args.frames, args.latent, args.batch
    te, vae = build_text_and_vae(dev)
    pipe = NeuroclipsPipeline(vae=vae, text_encoder=te, tokenizer=_BenchTokenizer(), unet=unet, scheduler=sched, controlnet=ctrl).to(dev)
    prompt = "a man rides a bicycle along the beach at sunset while seagulls circle above the waves"

    def run(c):
        return pipe([prompt] * Bc if Bc > 1 else prompt, video_length=F, height=L * 8, width=L * 8, num_inference_steps=args.ddim_steps,
                    guidance_scale=8.5, negative_prompt=None, latents=c["latents"], noise=c["noise"], controlnet_images=c["cimg"],
                    controlnet_image_index=[0], low_strength=0.3, output_type="tensor").videos

    run(clips[0])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for c in clips[args.warmup:]:
        vid = run(c)
    torch.cuda.synchronize()
    el = (time.perf_counter() - t0) / max(1, len(clips) - args.warmup)
    # stage shares (device time, events on the current stream)
    e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    e[0].record()
    pipe._encode_prompt(prompt, dev, 1, True, None)
    e[1].record()
    lat = clips[-1]["latents"]
    e[2].record()
    pipe.decode_latents(lat)
    e[3].record()
    torch.cuda.synchronize()
    return {"frames_per_s": round(Bc * F / el, 4), "ms_per_clip": round(1e3 * el, 2),
            "stages_ms": {"clip_text_encode_2x77_tokens": round(e[0].elapsed_time(e[1]), 3),
                          "vae_decode_incl_d2h_copy": round(e[2].elapsed_time(e[3]), 3)},
            "videos_shape": list(vid.shape), "videos_finite": bool(torch.isfinite(vid).all()),
            "what": "NeuroclipsPipeline.__call__(prompt, ..., output_type='tensor'): native CLIP _encode_prompt -> SparseCtrl + U-Net loop -> native VAE decode "
                    "-> .videos on the host (pipeline_neuroclips.py:321-501); random-init SD-1.5-size CLIP / VAE"}


def keyframe_traffic(B, L):
    """HBM bytes per Euler step of the keyframe path from the committed rocprofv3 --pmc passes (a profiler measurement of the same
    command, not a live counter read), or null when no pass of this batch / latent size is committed."""
    import glob
    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", f"r*_keyframe_b{B}_l{L}_traffic_pmc.json")), reverse=True):
        d = json.load(open(f))
        return {"hbm_gbytes_per_euler_step": round(d["whole_step_hbm_bytes"] / 1e9, 2),
                "igemm_hbm_gbytes_per_euler_step": round(d["igemm_hbm_bytes_per_ddim_step"] / 1e9, 2), "source": os.path.basename(f),
                "measured_in_this_run": False}
    return None


def enhance_main(args):
    """One GPU's share of BASELINE config 4 ("8 clips per GPU, 'enhance' inference mode end to end"), all stages native and resident on ONE
    GPU: B keyframes in ONE Euler loop (recon_keyframe_neurons_enhance.py:458-462 loops one image at a time; utils.unclip_recon's
    num_samples makes it a batch) + their first-stage decode, then the B clips in ONE pipeline call (CLIP -> loop -> VAE decode -> .videos).
    Wall times per stage; `value` = clips per second of the whole chain."""
    import numpy as np
    from neurons_amd import _lib, DDIMScheduler, NativeSparseCtrl, NativeUNet3D, NeuroclipsPipeline
    from neurons_amd.sgm import EulerEDMSampler, NativeSGMUNet, SGMUNetConfig, sgm_state_dict_schema
    from neurons_amd.sparsectrl import controlnet_config_from_unet
    from neurons_amd.unet3d import UNet3DConfig, state_dict_schema
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B = args.batch if args.batch > 1 else 8
    F, L, KL = args.frames, args.latent, args.keyframe_latent
    t_setup = time.time()
    scfg = SGMUNetConfig()
    knet = NativeSGMUNet(scfg).to(dev)
    knet.load_state_dict({k: v.cpu() for k, v in gpu_random_state_dict(sgm_state_dict_schema(scfg), 3, dev).items()})
    ucfg = UNet3DConfig()
    ccfg = controlnet_config_from_unet(ucfg, dict(
        set_noisy_sample_input_to_zero=True, use_simplified_condition_embedding=True, conditioning_channels=4,
        motion_module_kwargs=dict(attention_block_types=["Temporal_Self"], temporal_position_encoding_max_len=32)))
    unet, ctrl = NativeUNet3D(ucfg).to(dev), NativeSparseCtrl(ccfg).to(dev)
    unet.load_state_dict({k: v.cpu() for k, v in gpu_random_state_dict(state_dict_schema(ucfg, _lib.NR_KIND_UNET3D), 1, dev).items()})
    ctrl.load_state_dict({k: v.cpu() for k, v in gpu_random_state_dict(state_dict_schema(ccfg, _lib.NR_KIND_SPARSECTRL), 2, dev).items()})
    te, vae = build_text_and_vae(dev)
    torch.cuda.empty_cache()
    sched = DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="linear", steps_offset=1, clip_sample=False)
    pipe = NeuroclipsPipeline(vae=vae, text_encoder=te, tokenizer=_BenchTokenizer(), unet=unet, scheduler=sched, controlnet=ctrl).to(dev)
    sampler = EulerEDMSampler(num_steps=args.keyframe_steps, scale=5.0)
    g = torch.Generator(device=dev).manual_seed(11)
    prompt = "a man rides a bicycle along the beach at sunset while seagulls circle above the waves"

    def chain():
        ts = [time.perf_counter()]
        z = torch.randn(B, 4, KL, KL, generator=g, device=dev)
        c = {"crossattn": torch.randn(B, 256, 1664, generator=g, device=dev), "vector": torch.randn(B, 1024, generator=g, device=dev)}
        uc = {"crossattn": torch.randn(B, 256, 1664, generator=g, device=dev), "vector": torch.randn(B, 1024, generator=g, device=dev)}
        kz = sampler(knet, z, cond=c, uc=uc)
        torch.cuda.synchronize(); ts.append(time.perf_counter())
        kimg = vae.decode_keyframe(kz)                                   # utils.py:343-348
        torch.cuda.synchronize(); ts.append(time.perf_counter())
        # the keyframe enters the video stage as its latent (scripts/neuroclips_video_enhance.py:268,283 encode it; here the sampled latent is used directly)
        cimg = (kz[:, :, :L, :L] if KL >= L else torch.nn.functional.interpolate(kz, size=(L, L))).unsqueeze(2).contiguous() * 0.18215
        vid = pipe([prompt] * B, video_length=F, height=L * 8, width=L * 8, num_inference_steps=args.ddim_steps, guidance_scale=8.5,
                   latents=torch.randn(B, 4, F, L, L, generator=g, device=dev), noise=torch.randn(B, 4, F, L, L, generator=g, device=dev),
                   controlnet_images=cimg, controlnet_image_index=[0], low_strength=0.3, output_type="tensor").videos
        torch.cuda.synchronize(); ts.append(time.perf_counter())
        return ts, kimg, vid

    setup_s = time.time() - t_setup
    for _ in range(args.warmup):
        chain()
    tot, stages = 0.0, np.zeros(3)
    for _ in range(args.steps):
        ts, kimg, vid = chain()
        tot += ts[-1] - ts[0]
        stages += np.diff(ts)
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, {"keyframes": kimg, "videos": vid})
    tot /= args.steps
    stages /= args.steps
    print(json.dumps({
        "metric": "'enhance' chain clips/sec on one GPU (keyframes + video, BASELINE config 4 share)", "value": round(B / tot, 4), "unit": "clips/s",
        "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(1e3 * tot, 1), "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
        "config": {"workload": f"BASELINE config 4, one GPU's share: {B} keyframes ({KL}x{KL} latent, {args.keyframe_steps} Euler steps, CFG 5.0) in one loop + decode, "
                               f"then {B} clips ({F} f, {L}x{L} latent, {args.ddim_steps} DDIM steps, CFG 8.5, SparseCtrl) in one call incl. CLIP and VAE decode",
                   "stage_s": {"keyframes_euler_loop": round(float(stages[0]), 3), "keyframes_vae_decode": round(float(stages[1]), 3),
                               "video_call_clip_loop_vae": round(float(stages[2]), 3)},
                   "video_frames_per_s_incl_keyframes": round(B * F / tot, 2), "setup_s": round(setup_s, 1),
                   "output_finite": bool(torch.isfinite(vid).all() and torch.isfinite(kimg).all()),
                   "resident_weight_gb": round((knet.weight_bytes() + unet.weight_bytes() + ctrl.weight_bytes() + te.weight_bytes() + vae.weight_bytes()) / 1e9, 2)}}))



def main():
    args = parse()
    if args.workload == "keyframe":
        return keyframe_main(args)
    if args.workload == "vae":
        return vae_main(args)
    if args.workload == "enhance":
        return enhance_main(args)
    # No launcher around us (`python bench.py --gpus N`, the driver's SCALE command): this process becomes the launcher of N rank processes.
    # Under torch.distributed.run (RANK / WORLD_SIZE in the environment) it IS a rank.
    if "RANK" not in os.environ and (args.gpus > 1 or args.self_launch or args.launch_dry_run):
        return self_launch(args)
    if args.launch_dry_run:
        return launch_dry_run(args)
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: the launcher's world and --gpus must agree")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist, rccl_ranks_seen = None, None
    # NR_DIST_FORCE=1 under torchrun with ONE rank: the same NCCL (= RCCL) init / broadcast / all-reduce / barrier calls as N > 1
    # (tests/test_dist_gpu.py runs this on the single-GPU box)
    use_dist = world > 1 or (os.environ.get("NR_DIST_FORCE") == "1" and "RANK" in os.environ)
    if use_dist:
        import torch.distributed as dist_mod
        dist = dist_mod
        dist.init_process_group("nccl", device_id=dev)
        seen = torch.ones(1, device=dev)
        dist.all_reduce(seen)                 # every rank's GPU answers over RCCL before anything is timed
        rccl_ranks_seen = int(seen.item())

    from neurons_amd import _lib, DDIMScheduler, NativeSparseCtrl, NativeUNet3D, NeuroclipsPipeline
    from neurons_amd.sparsectrl import controlnet_config_from_unet
    from neurons_amd.unet3d import UNet3DConfig, state_dict_schema

    ucfg = UNet3DConfig()
    if args.frames > 24:   # the v3 motion module's PE table has 24 rows; longer clips need a 32-row config
        ucfg.motion_module_kwargs = dict(ucfg.motion_module_kwargs, temporal_position_encoding_max_len=32)
    ccfg = controlnet_config_from_unet(ucfg, dict(
        set_noisy_sample_input_to_zero=True, use_simplified_condition_embedding=True, conditioning_channels=4,
        motion_module_kwargs=dict(attention_block_types=["Temporal_Self"], temporal_position_encoding_max_len=32)))
    unet = NativeUNet3D(ucfg).to(dev)
    ctrl = NativeSparseCtrl(ccfg).to(dev)
    if args.no_graph:
        unet.enable_graph(False)
        ctrl.enable_graph(False)
    if args.attn_fp8:
        unet.set_attention_fp8(True)
        ctrl.set_attention_fp8(True)
    headline = args.batch == 1 and args.frames == 16 and args.latent == 32 and not args.attn_fp8 and not args.no_controlnet

    # ---- weights: rank 0 generates + converts once; the converted bf16 arenas travel device to device over RCCL/xGMI ----
    t0 = time.time()
    from neurons_amd.distributed import broadcast_native_weights, max_over_ranks
    host_sd = {}
    F, L = args.frames, args.latent
    for net, cfg, kind, seed in ((unet, ucfg, _lib.NR_KIND_UNET3D, 1), (ctrl, ccfg, _lib.NR_KIND_SPARSECTRL, 2)):
        if rank == 0:
            sd = {k: v.cpu() for k, v in gpu_random_state_dict(state_dict_schema(cfg, kind), seed, dev).items()}
            net.load_state_dict(sd)
            if args.full:               # the oracle legs after the timed region read the host weights
                host_sd[kind] = sd
            if use_dist:
                # converts the weights for the shape every rank will run: SparseCtrl is evaluated `grp` DDIM steps at a time (pipeline.py)
                from neurons_amd.pipeline import controlnet_group_size
                grp0 = controlnet_group_size(args.ddim_steps, 2 * args.batch, F, L, L,
                                             int(os.environ["NR_CTRL_GROUP"]) if os.environ.get("NR_CTRL_GROUP") else "auto")
                if kind == _lib.NR_KIND_SPARSECTRL and os.environ.get("NR_CTRL_DEDUP", "1") != "0":
                    # the plan every rank will run: condition on frame 0 only (controlnet_image_index=[0]) -> identical-frame evaluation
                    import ctypes
                    _lib.check(_lib.load().nr_sparsectrl_set_condition_frames(net._handle(), (ctypes.c_int32 * 1)(0), 1))
                    net._cframes = (0,)
                net._ensure_plan(2 * args.batch * (grp0 if kind == _lib.NR_KIND_SPARSECTRL else 1), F, L, L, 77)
        if use_dist:
            broadcast_native_weights(net, src=0)
    torch.cuda.empty_cache()

    sched = DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="linear", steps_offset=1, clip_sample=False)
    pipe = NeuroclipsPipeline(vae=None, text_encoder=None, tokenizer=None, unet=unet, scheduler=sched, controlnet=ctrl).to(dev)

    n_clips = args.warmup + args.steps
    g = torch.Generator(device=dev).manual_seed(1000 + rank)
    clips = []
    Bc = args.batch
    for _ in range(n_clips):   # synthetic inputs, resident in HBM before timing
        clips.append(dict(
            latents=torch.randn(Bc, 4, F, L, L, generator=g, device=dev),
            noise=torch.randn(Bc, 4, F, L, L, generator=g, device=dev),
            ctx=torch.randn(2 * Bc, 77, ucfg.cross_attention_dim, generator=g, device=dev),
            cimg=torch.randn(Bc, 4, 1, L, L, generator=g, device=dev) * 0.18215))

    # NR_BENCH_STEP_EVENTS=1 (diagnostic): one event per DDIM step through the pipeline's callback; the per-step milliseconds of the last
    # clip go to stderr after the timed region (where inside a clip the time goes: first step, group boundaries, steady state)
    step_events = [] if os.environ.get("NR_BENCH_STEP_EVENTS") == "1" else None

    def _mark(i, t, lat):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        step_events.append(e)

    def run_clip(c):
        extra = {}
        if step_events is not None:
            step_events.clear()
            _mark(-1, None, None)
            extra = dict(callback=_mark, callback_steps=1)
        return pipe([""] * Bc if Bc > 1 else "", video_length=F, height=L * 8, width=L * 8, num_inference_steps=args.ddim_steps, guidance_scale=8.5,
                    latents=c["latents"], noise=c["noise"], text_embeddings=c["ctx"], controlnet_images=None if args.no_controlnet else c["cimg"],
                    controlnet_image_index=[0], low_strength=0.3, output_type="latent", **extra).videos

    for i in range(args.warmup):
        run_clip(clips[i])
    torch.cuda.synchronize()
    setup_s = time.time() - t0
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    for i in range(args.warmup, n_clips):
        out = run_clip(clips[i])
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t1
    elapsed = max_over_ranks(elapsed, device=dev)
    if step_events:
        ms = [step_events[i].elapsed_time(step_events[i + 1]) for i in range(len(step_events) - 1)]
        print("per-step ms of the last clip (first entry: call start -> end of step 0): " + " ".join(f"{m:.2f}" for m in ms) +
              f" | sum {sum(ms):.1f} ms, wall per clip {1e3 * elapsed / args.steps:.1f} ms", file=sys.stderr)
    finite = bool(torch.isfinite(out).all().item())
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, {"videos": out})

    result = None
    if rank == 0:
        total_frames = world * args.steps * F * Bc
        value = total_frames / elapsed
        # SparseCtrl is evaluated `grp` DDIM steps at a time (pipeline.controlnet_group): its per-launch profile covers grp steps
        grp = getattr(pipe, "last_controlnet_group", 1)
        result = {
            "metric": "denoising frames/sec, 16f x 256^2 clip, 50 DDIM steps",
            "value": round(value, 4), "unit": "frames/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(1e3 * elapsed / args.steps, 2), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "bf16" if not args.attn_fp8 else "bf16 (attention operands e4m3)", "data": "synthetic",
            "rccl_ranks_seen": rccl_ranks_seen,
            "config": {"workload": f"BASELINE config {5 if (Bc, F, L) == (4, 32, 64) else 4 if Bc > 1 else 2}: {Bc} clip(s) per call, ({Bc},4,{F},{L},{L}) latent, {args.ddim_steps} DDIM steps, CFG 8.5 "
                                   f"(batch {2 * Bc}), SparseCtrl + temporal U-Net per step, random-init weights" +
                                   (" -- DIAGNOSTIC RUN WITHOUT SparseCtrl (--no-controlnet): not the configured workload" if args.no_controlnet else ""),
                       "clips_per_gpu": args.steps * Bc, "frame_steps_per_s": round(value * args.ddim_steps, 2),
                       "ddim_steps": args.ddim_steps, "ms_per_ddim_step": round(1e3 * elapsed / args.steps / args.ddim_steps, 3),
                       "sparsectrl_steps_per_evaluation": grp,
                       "hip_graph": not args.no_graph, "output_finite": finite, "setup_s": round(setup_s, 1),
                       "resident_weight_gb": round((unet.weight_bytes() + ctrl.weight_bytes()) / 1e9, 2),
                       "attention": "e4m3 spatial/cross (fp32 softmax/accumulate), bf16 temporal" if args.attn_fp8 else "bf16"},
        }
        if args.full and not args.no_op_profile:
            full_legs(args, result, dev, world, headline, elapsed, grp, host_sd, ucfg, ccfg, unet, ctrl, sched, pipe, clips)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        print(json.dumps(result))


def full_legs(args, result, dev, world, headline, elapsed, grp, host_sd, ucfg, ccfg, unet, ctrl, sched, pipe, clips):
    """--full on rank 0, after the timed region: the per-launch event pass (roofline), the PSNR legs, the CPU baseline and the
    end-to-end leg, added to `result`."""
    # ---- roofline of the dominant kernel class (MFMA implicit GEMM), HIP events per launch ----
    pu = unet.profile_last()
    pc = ctrl.profile_last() if not args.no_controlnet else {k: {f: 0.0 for f in v} for k, v in pu.items()}
    pc = {k: {f: v[f] / grp for f in v} for k, v in pc.items()}
    ig_ms = pu["igemm"]["ms"] + pc["igemm"]["ms"]
    ig_fl = pu["igemm"]["flops"] + pc["igemm"]["flops"]
    ig_n = pu["igemm"]["launches"] + pc["igemm"]["launches"]
    achieved = ig_fl / (ig_ms * 1e-3) / 1e12 if ig_ms > 0 else 0.0
    breakdown = {k: round(pu[k]["ms"] + pc[k]["ms"], 3) for k in pu}
    step_flops = sum(pu[k]["flops"] + pc[k]["flops"] for k in pu)
    step_bytes = sum(pu[k]["bytes"] + pc[k]["bytes"] for k in pu)
    # whole-step algorithmic HBM bytes (every kernel's operands counted once) / measured wall time of a DDIM step
    result["config"]["achieved_hbm_gbs"] = round(step_bytes / (elapsed / args.steps / args.ddim_steps) / 1e9, 1)
    result["config"]["achieved_tflops"] = round(step_flops / (elapsed / args.steps / args.ddim_steps) / 1e12, 1)
    result["roofline"] = {"bound": "mfma", "kernel": "igemm_bf16_kernel (3x3/1x1 conv + Linear)", "achieved": round(achieved, 2),
                          "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s", "frac": round(achieved / PEAK_BF16_TFLOPS, 4),
                          # HBM bytes of the igemm class per DDIM step (GB) from the committed rocprofv3 PMC passes, next to the
                          # class's algorithmic bytes: traffic >> algorithmic = operand re-reads / split-K slabs
                          "traffic": (pmc_traffic() or {}).get("igemm_hbm_gbytes_per_ddim_step") if headline else None,
                          "traffic_unit": "GB per DDIM step (igemm class, PMC FETCH_SIZE x2 + WRITE_SIZE)",
                          "traffic_detail": pmc_traffic() if headline else None,
                          "algorithmic_gbytes_per_ddim_step": round((pu["igemm"]["bytes"] + pc["igemm"]["bytes"]) / 1e9, 2),
                          "launches_per_ddim_step": round(ig_n, 1), "ms_per_ddim_step": round(ig_ms, 3),
                          # kernels enqueued per DDIM step, both networks (split-K reduces, multi-pass norms and the time-embedding MLP counted
                          # per kernel; + set_timesteps and the CFG/DDIM update; SparseCtrl's share is 1/grp of an evaluation)
                          "whole_step_launches_sparsectrl_counted_at_1_over_group": round(sum(pu[k]["launches"] + pc[k]["launches"] for k in pu) + 2 + 1.0 / grp, 1),
                          "sparsectrl_steps_per_evaluation": grp,
                          "algorithmic_tflop_per_ddim_step": round(ig_fl / 1e12, 3),
                          "per_class_ms_per_ddim_step": breakdown,
                          "whole_step_algorithmic": {"tflop": round(step_flops / 1e12, 3), "gbytes": round(step_bytes / 1e9, 2)}}
    # "PSNR vs ref" half of the metric: (a) the reference-generated C1 fixture (tiny networks, 10 steps) and (b) THIS configuration:
    # the clip just timed, final latents against the fp32 oracle run on the same GPU, same weights and inputs (outside the timed region)
    result["config"]["psnr_c1_fixture_db"] = None if args.no_psnr else psnr_vs_reference(dev)
    # The oracle leg (rank 0, N = 1, headline configuration only; `--no-cpu-baseline` skips all of it): oracle/ is used here as
    # the CHECKER of the clip just timed (b) and as the timed CPU baseline -- never as anything measured in `value` or shipped.
    # Larger configurations (4 / 5) take their parity from tests/test_fullsize_gpu.py and tests/test_engine_gpu.py.
    oracle_leg = (not args.no_cpu_baseline) and world == 1 and headline
    result["config"]["psnr_c2_vs_fp32_oracle_db"] = psnr_headline(dev, host_sd, ucfg, ccfg, pipe, clips[-1], args) if (oracle_leg and not args.no_psnr) else None
    if oracle_leg:
        result["cpu_baseline"] = cpu_baseline(host_sd, ucfg, ccfg, args)
    # end-to-end __call__ (CLIP -> loop -> VAE decode -> .videos) beside the loop-only headline; N = 1 only
    if world == 1 and not args.no_end_to_end and not args.attn_fp8:
        result["end_to_end"] = end_to_end_leg(args, dev, unet, ctrl, sched, clips)


def psnr_headline(dev, host_sd, ucfg, ccfg, pipe, clip, args):
    """PSNR (and rel-L2) of the timed configuration itself: the last timed clip re-run through the HIP pipeline vs the fp32 oracle
    (reference module graph restated in PyTorch, pinned by tests/golden) on the same GPU, weights, latents, noise, context."""
    import numpy as np
    from neurons_amd import _lib
    from oracle import animatediff_oracle as O
    if clip["latents"].shape[0] != 1:
        return None
    F, L = args.frames, args.latent
    got = pipe("", video_length=F, height=L * 8, width=L * 8, num_inference_steps=args.ddim_steps, guidance_scale=8.5, latents=clip["latents"],
               noise=clip["noise"], text_embeddings=clip["ctx"], controlnet_images=clip["cimg"], controlnet_image_index=[0], low_strength=0.3,
               output_type="latent").videos
    usd = {k: v.to(dev) for k, v in host_sd[_lib.NR_KIND_UNET3D].items()}
    csd = {k: v.to(dev) for k, v in host_sd[_lib.NR_KIND_SPARSECTRL].items()}
    with torch.no_grad():
        want, _ = O.neuroclips_denoise(usd, O.OracleConfig.from_native(ucfg), csd, O.OracleConfig.from_native(ccfg), clip["latents"], clip["noise"],
                                       clip["ctx"], clip["cimg"], (0,), args.ddim_steps, 8.5)
    mse = ((got.float() - want) ** 2).mean().item()
    rng = (want.max() - want.min()).item()
    rel = mse ** 0.5 / (want.pow(2).mean().item() ** 0.5 + 1e-12)
    return {"psnr_db": round(10.0 * float(np.log10(rng * rng / (mse + 1e-20))), 2), "rel_l2": round(rel, 5), "ddim_steps": args.ddim_steps}


def psnr_vs_reference(dev):
    """"PSNR vs ref" half of BASELINE.json's metric, measured live: the reference-generated C1 fixture (tests/golden/
    c1_loop.npz: 8-frame 64x64 clip, 10 DDIM steps, CFG 8.5, SparseCtrl on, produced by the reference's own classes in fp32)
    run through the same pipeline code path on the tiny full-topology networks it was recorded with."""
    import numpy as np
    from neurons_amd import _lib, DDIMScheduler, NativeSparseCtrl, NativeUNet3D, NeuroclipsPipeline
    from neurons_amd.sparsectrl import controlnet_config_from_unet
    from neurons_amd.unet3d import UNet3DConfig, random_state_dict
    path = os.path.join(ROOT, "tests", "golden", "c1_loop.npz")
    if not os.path.exists(path):
        return None
    g = np.load(path)
    ucfg = UNet3DConfig(sample_size=8, block_out_channels=(64, 64, 128, 128), cross_attention_dim=64)
    ccfg = controlnet_config_from_unet(ucfg, dict(
        set_noisy_sample_input_to_zero=True, use_simplified_condition_embedding=True, conditioning_channels=4,
        motion_module_kwargs=dict(num_attention_heads=8, num_transformer_block=1, attention_block_types=["Temporal_Self"],
                                  temporal_position_encoding=True, temporal_position_encoding_max_len=32, temporal_attention_dim_div=1)))
    unet, ctrl = NativeUNet3D(ucfg).to(dev), NativeSparseCtrl(ccfg).to(dev)
    unet.load_state_dict(random_state_dict(ucfg, _lib.NR_KIND_UNET3D, seed=11))
    ctrl.load_state_dict(random_state_dict(ccfg, _lib.NR_KIND_SPARSECTRL, seed=12))
    sched = DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="linear", steps_offset=1, clip_sample=False)
    pipe = NeuroclipsPipeline(None, None, None, unet, sched, ctrl).to(dev)
    out = pipe("", video_length=8, height=64, width=64, num_inference_steps=int(g["steps"]), guidance_scale=float(g["guidance"]),
               latents=torch.from_numpy(g["latents"]).to(dev), noise=torch.from_numpy(g["noise"]), text_embeddings=torch.from_numpy(g["ctx"]).to(dev),
               controlnet_images=torch.from_numpy(g["cimg"]).to(dev), controlnet_image_index=[0], low_strength=0.3, output_type="latent").videos
    want = torch.from_numpy(g["final"])
    mse = ((out.float().cpu() - want) ** 2).mean().item()
    rng = (want.max() - want.min()).item()
    return round(10.0 * float(np.log10(rng * rng / (mse + 1e-20))), 2)


def pmc_traffic():
    """HBM bytes of the igemm kernel class per DDIM step from the committed rocprofv3 --pmc passes (FETCH_SIZE and
    WRITE_SIZE in separate runs, FETCH_SIZE doubled as MI355X_MICROARCH.md prescribes for gfx950): bench.py cannot
    run the profiler itself, so it reports the most recent committed measurement, or null."""
    import glob
    files = sorted(f for f in glob.glob(os.path.join(ROOT, "profiles", "r*_traffic_pmc.json")) if "keyframe" not in os.path.basename(f))
    if not files:
        return None
    with open(files[-1]) as f:
        d = json.load(f)
    name = os.path.basename(files[-1])
    return {"igemm_hbm_gbytes_per_ddim_step": round(d["igemm_hbm_bytes_per_ddim_step"] / 1e9, 2),
            "whole_step_hbm_gbytes": round(d["whole_step_hbm_bytes"] / 1e9, 2), "source": name,
            "traffic_source_round": name.split("_")[0], "historical": name.split("_")[0] != current_round(),
            "measured_in_this_run": False}      # a committed profiler measurement of the same command, not a live counter read


def cpu_baseline(host_sd, ucfg, ccfg, args):
    """The oracle (reference module graph, fp32, eager, math attention) on the host cores, as BASELINE.md section 4 states it:
    (1) BASELINE config 1 end to end (8 frames, 8x8 latent, 10 DDIM steps, tiny full-topology networks), best of 2;
    (2) ONE full denoising step of the headline config (SparseCtrl + U-Net forward, CFG batch 2, all 16 frames, full width) --
        no frame extrapolation -- scaled by the step count only.  `value` is (2).  Fixed thread count (all host cores torch uses)."""
    import numpy as np
    from neurons_amd import _lib
    from neurons_amd.sparsectrl import controlnet_config_from_unet
    from neurons_amd.unet3d import UNet3DConfig, random_state_dict
    from oracle import animatediff_oracle as O
    threads = torch.get_num_threads()
    # (1) C1 end to end
    c1 = None
    path = os.path.join(ROOT, "tests", "golden", "c1_loop.npz")
    if os.path.exists(path):
        g = np.load(path)
        tu = UNet3DConfig(sample_size=8, block_out_channels=(64, 64, 128, 128), cross_attention_dim=64)
        tc = controlnet_config_from_unet(tu, dict(
            set_noisy_sample_input_to_zero=True, use_simplified_condition_embedding=True, conditioning_channels=4,
            motion_module_kwargs=dict(num_attention_heads=8, num_transformer_block=1, attention_block_types=["Temporal_Self"],
                                      temporal_position_encoding=True, temporal_position_encoding_max_len=32, temporal_attention_dim_div=1)))
        tus, tcs = random_state_dict(tu, _lib.NR_KIND_UNET3D, seed=11), random_state_dict(tc, _lib.NR_KIND_SPARSECTRL, seed=12)
        best = 1e30
        with torch.no_grad():
            for _ in range(2):
                t0 = time.perf_counter()
                O.neuroclips_denoise(tus, O.OracleConfig.from_native(tu), tcs, O.OracleConfig.from_native(tc), torch.from_numpy(g["latents"]),
                                     torch.from_numpy(g["noise"]), torch.from_numpy(g["ctx"]), torch.from_numpy(g["cimg"]), (0,), int(g["steps"]), 8.5)
                best = min(best, time.perf_counter() - t0)
        c1 = {"seconds": round(best, 3), "frames_per_s": round(8 / best, 4), "what": "C1: 8 f x 64^2, 10 DDIM steps, tiny networks, best of 2"}
    # (2) one full C2 step
    F, L = args.frames, args.latent
    uc, cc = O.OracleConfig.from_native(ucfg), O.OracleConfig.from_native(ccfg)
    usd, csd = host_sd[_lib.NR_KIND_UNET3D], host_sd[_lib.NR_KIND_SPARSECTRL]
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 4, F, L, L, generator=g)
    ctx = torch.randn(2, 77, ucfg.cross_attention_dim, generator=g)
    cond = torch.zeros(1, 4, F, L, L)
    mask = torch.zeros(1, 1, F, L, L)
    mask[:, :, 0] = 1
    with torch.no_grad():
        t0 = time.perf_counter()
        down, mid = O.sparse_controlnet_forward(csd, cc, x, 500, ctx, cond, mask, 1.0)
        O.unet3d_forward(usd, uc, x, 500, ctx, down, mid)
        dt = time.perf_counter() - t0
    clip_s = dt * args.ddim_steps
    return {"value": round(F / clip_s, 6), "unit": "frames/s", "cores": threads, "kind": "port",
            "sample": f"ONE full DDIM step (SparseCtrl + U-Net forward, CFG batch 2, {F} frames, {L}x{L} latent, full width) took {dt:.2f} s on "
                      f"{threads} threads ({os.cpu_count()} logical CPUs); x{args.ddim_steps} steps = {clip_s:.0f} s per clip",
            "c1_end_to_end": c1, "logical_cpus": os.cpu_count()}


if __name__ == "__main__":
    main()
