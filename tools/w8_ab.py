"""A/B of the e4m3-weight form of the small-M GEMM (smallm.hip, NR_W8=1) against its bf16 form on the M = 512 Linears of the U-Net 4x4 level and the
keyframe model: the same inputs and the same SmallmPlan, NR_W8 unset vs 1, rel-L2 of the outputs, and the time per launch inside a replayed graph of
48 launches that walk a pool of distinct weight tensors larger than the Infinity Cache (every launch streams its weights from HBM, as in the
denoiser).  Both arms run in this one process, alternating, ROUNDS times; the line gives each arm's median and its min .. max over the rounds.
The second block repeats it with NR_SMALLM=2 on the several-slabs-per-workgroup plans (N = 3840: J > 1) that the shipped rule leaves to the tiled
igemm, with the igemm (NR_SMALLM=0) as a third arm: halving the weight bytes a CU requests is what that rule's argument rests on.
Usage (on an MI355X): python tools/w8_ab.py > profiles/w8_smallm_ab.txt"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neurons_amd import ops  # noqa: E402

dev = torch.device("cuda", 0)
# (M, N, K, kind) kind: res | ln
SHIPPED = [(512, 1280, 1280, "res"), (512, 1280, 1280, "ln"), (512, 1280, 5120, "res"), (512, 640, 640, "res"), (256, 1280, 1280, "res")]
SLABS = [(512, 3840, 1280, "ln"), (512, 3840, 5120, "res"), (512, 1920, 640, "ln")]
NCALL = 48
REPLAYS = 100
ROUNDS = 5


def make(M, N, K, kind, npool):
    a = torch.randn(M, K, device=dev).to(torch.bfloat16)
    ws = [(torch.randn(N, K, device=dev) * K ** -0.5).to(torch.bfloat16) for _ in range(npool)]
    b = torch.randn(N, device=dev)
    r = torch.randn(M, N, device=dev).to(torch.bfloat16)
    if kind == "res":
        return [lambda w=w: ops.gemm(a, w, b, r) for w in ws]
    gamma, beta = 1.0 + 0.1 * torch.randn(K, device=dev), 0.1 * torch.randn(K, device=dev)
    fns = []
    lib = ops._lib.load()
    for w in ws:      # LayerNorm folded: the folded operands once per weight (the engine does this at plan time)
        wf = w.float()
        wsc = (wf * gamma[None]).to(torch.bfloat16).contiguous()
        c = wsc.float().sum(dim=1).contiguous()
        bb = ((wf.double() @ beta.double()).float() + b).contiguous()

        def fn(wsc=wsc, c=c, bb=bb):
            out = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
            ops._lib.check(lib.nr_op_gemm_ex(ops._stream(), ops._ptr(a), K, ops._ptr(wsc), ops._ptr(bb), ops._ptr(c), 1e-5, None, 1, 0, 0, ops._ptr(r), N,
                                             ops._ptr(out), N, M, N, K, 0, 0, 1.0))
            return out
        fns.append(fn)
    return fns


def capture(fns):
    for f in fns:      # every packed copy exists before the capture (NR_OP_FM_CACHE)
        f()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            for i in range(NCALL):
                fns[i % len(fns)]()
    torch.cuda.synchronize()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    return g


def timed(g):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(REPLAYS):
        g.replay()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / (REPLAYS * NCALL) * 1e3


def setenv(env):
    for k in ("NR_SMALLM", "NR_W8"):
        os.environ.pop(k, None)
    os.environ.update(env)


def ab(shapes, arms):
    for (M, N, K, kind) in shapes:
        npool = max(2, min(NCALL, int(600e6 / (N * K * 2))))
        fns = make(M, N, K, kind, npool)
        graphs, outs = {}, {}
        for name, env in arms:      # the environment is read when a launch is described, i.e. at capture: a replay runs what was captured
            setenv(env)
            outs[name] = fns[0]().float()
            graphs[name] = capture(fns)
        t = {name: [] for name, _ in arms}
        for _ in range(ROUNDS):
            for name, _ in arms:
                t[name].append(timed(graphs[name]))
        base = arms[0][0]
        line = f"M={M:4d} N={N:5d} K={K:5d} {kind:4s}"
        for name, _ in arms:
            line += f" | {name} {statistics.median(t[name]):6.2f}us ({min(t[name]):.2f}..{max(t[name]):.2f})"
        for name, _ in arms[1:]:
            rel = ((outs[name] - outs[base]).norm() / outs[base].norm()).item()
            line += f" | {base}/{name} x{statistics.median(t[base]) / statistics.median(t[name]):4.2f} rel-L2 {rel:.1e}"
        print(line, flush=True)
        torch.cuda.synchronize()
        del fns, graphs
        ops._lib.load().nr_op_fm_cache_clear()


os.environ["NR_OP_FM_CACHE"] = "1"       # one packed copy per (weight tensor, layout) of the pool, made outside the capture
print(f"# us per launch, median (min..max) of {ROUNDS} alternating rounds of {REPLAYS} replays of a {NCALL}-launch graph; {torch.cuda.get_device_name(0)}")
print("# shipped plans (one slab per workgroup): bf16 weights vs e4m3 weights, same SmallmPlan")
ab(SHIPPED, [("bf16", {}), ("e4m3", {"NR_W8": "1"})])
print("# several slabs per workgroup (NR_SMALLM=2; the shipped rule sends these to the tiled igemm): igemm vs smallm bf16 vs smallm e4m3")
ab(SLABS, [("igemm", {"NR_SMALLM": "0"}), ("bf16", {"NR_SMALLM": "2"}), ("e4m3", {"NR_SMALLM": "2", "NR_W8": "1"})])
