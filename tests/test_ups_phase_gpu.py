"""Phase form of the nearest-2x upsample convs on the GPU: ops.conv3x3_ups_phase (four 2x2 phase convs on the source, NrGemmParams::ups == 2)
against fp32 torch on the same bf16 operands, with ops.conv3x3(ups=True) -- the 3x3 conv on the replicated image -- held to the same criterion
beside it; and the engine's switch NR_UPS_PHASE on the tiny U-Net: the plan, and the two forwards against the fp32 oracle."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)


def _cmp(name, out, ref, max_tol=2e-2, mean_tol=4e-3):      # the criterion of tests/test_ops_gpu.py
    out = out.float()
    ref = ref.float()
    assert out.shape == ref.shape, (name, out.shape, ref.shape)
    assert torch.isfinite(out).all(), f"{name}: non-finite output"
    err = (out - ref).abs()
    mx, mean = err.max().item(), err.mean().item()
    rmx, rmean = ref.abs().max().item(), ref.abs().mean().item()
    print(f"[{name}] max_err={mx:.4e} (ref max {rmx:.3e})  mean_err={mean:.4e} (ref mean {rmean:.3e})")
    assert mx <= max_tol * rmx + 1e-6, f"{name}: max err {mx} vs ref max {rmx}"
    assert mean <= mean_tol * rmean + 1e-7, f"{name}: mean err {mean} vs ref mean {rmean}"


def _case(shape, seed=0):
    """seeded bf16 operands and the fp32 reference: F.interpolate(nearest, 2x) + conv2d(padding=1) on the bf16 values, NHWC"""
    nimg, H, W, Cin, Cout = shape
    g = torch.Generator(device="cpu").manual_seed(1000 + seed + nimg * 7 + H * 11 + Cin)
    x = torch.randn(nimg, H, W, Cin, generator=g).to(torch.bfloat16).cuda()
    w = (torch.randn(Cout, 3, 3, Cin, generator=g) * (9 * Cin) ** -0.5).to(torch.bfloat16).cuda()
    b = torch.randn(Cout, generator=g).cuda()
    up = F.interpolate(x.float().permute(0, 3, 1, 2), scale_factor=2, mode="nearest")
    ref = F.conv2d(up, w.float().permute(0, 3, 1, 2), b, padding=1).permute(0, 2, 3, 1).contiguous()
    return x, w, b, ref


def _check(shape, tag=""):
    from neurons_amd import ops
    x, w, b, ref = _case(shape)
    got = ops.conv3x3_ups_phase(x, w, b)
    base = ops.conv3x3(x, w, b, ups=True)
    torch.cuda.synchronize()
    _cmp(f"ups_phase {shape}{tag}", got, ref)
    _cmp(f"ups 3x3   {shape}{tag}", base, ref)


# (nimg, H, W, Cin, Cout)
SHAPES = [
    (1, 1, 1, 64, 64),           # every tap but one is padding, Mp = 1
    (3, 5, 7, 64, 96),           # odd sizes, Mp = 105 straddles tiles, N no multiple of 64
    (2, 3, 2, 128, 160),         # H != W
    (2, 4, 4, 1280, 1280),       # the headline's Cin / Cout on two images
    # the two (tile, split-K) plans choose_plan_phase (gemm.hip) gives the three headline shapes, each at the fewest images that still get it:
    (1, 4, 4, 1280, 1280),       # 4x4 -> 8x8 (M <= 2048, K = 5120): 128 x 160 tiles, four K slices + reduce
    (31, 8, 8, 1280, 1280),      # 8x8 -> 16x16: 128 x 160 tiles, one slice, from 31 images on (512 tiles); Mp = 1984 is no multiple of 128
    (1, 16, 16, 640, 640),       # 16x16 -> 32x32 (K = 2560): 128 x 160 tiles, one slice, at any image count
]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_phase_conv_vs_fp32_torch(cuda, shape):
    _check(shape)


def test_phase_conv_split_k_reduce_maps_rows(cuda):
    """split-K > 1 forced (the override is read per route, the other kernel classes look at it once per process: a fresh child), so the
    reduce kernel's row mapping runs: Mp = 105 rows per phase on 64-row tiles, three K slices of a K = 512 loop"""
    env = dict(os.environ, NR_IGEMM_FORCE="64,64,3,-1,-1")
    r = subprocess.run([sys.executable, "-c",
                        "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_ups_phase_gpu as t; t._check((3, 5, 7, 128, 96), ' splitk=3')" % (ROOT, HERE)],
                       env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0
    assert r.stdout.count("max_err=") == 2


# ---------------------------------------------------------------------------------------------------------------------------------------
# engine: NR_UPS_PHASE is read when a plan is built
# ---------------------------------------------------------------------------------------------------------------------------------------
def _descs(unet):
    from neurons_amd import _lib
    lib = _lib.load()
    return [lib.nr_net_op_desc(unet._h, i).decode() for i in range(lib.nr_net_num_ops(unet._h))]


def test_engine_switch_is_per_plan_and_both_forms_match_the_oracle(cuda):
    import numpy as np
    from neurons_amd import _lib, NativeUNet3D
    from neurons_amd.unet3d import random_state_dict
    from oracle import animatediff_oracle as O
    from tiny_configs import tiny_unet_config
    g = np.load(os.path.join(HERE, "golden", "tiny_networks.npz"))
    ucfg = tiny_unet_config()
    sd = random_state_dict(ucfg, _lib.NR_KIND_UNET3D, seed=11)
    sample, ctx = torch.from_numpy(g["sample"]).cuda(), torch.from_numpy(g["ctx"]).cuda()
    outs, plans = {}, {}
    old = os.environ.get("NR_UPS_PHASE")
    try:
        for mode in ("0", "1"):      # two handles in one process, each planned (at its first forward) under its own setting
            os.environ["NR_UPS_PHASE"] = mode
            unet = NativeUNet3D(ucfg).to("cuda")
            unet.load_state_dict(sd)
            outs[mode] = unet(sample, int(g["t"]), encoder_hidden_states=ctx).sample.float()
            plans[mode] = _descs(unet)
    finally:
        if old is None:
            os.environ.pop("NR_UPS_PHASE", None)
        else:
            os.environ["NR_UPS_PHASE"] = old
    ups0 = [d for d in plans["0"] if " ups=1 " in d or " ups=2 " in d]
    ups1 = [d for d in plans["1"] if " ups=1 " in d or " ups=2 " in d]
    print("NR_UPS_PHASE=0:", ups0)
    print("NR_UPS_PHASE=1:", ups1)
    assert len(ups0) == 3 and all(" ups=1 " in d for d in ups0)
    assert len(ups1) == 3 and all(" ups=2 " in d for d in ups1)
    # nothing else in the plan moved, and the phase launches describe the launched work (K = 4 Cin against 9 Cin)
    assert [d for d in plans["0"] if d not in ups0] == [d for d in plans["1"] if d not in ups1]
    for a, b in zip(ups0, ups1):
        ka, kb = int(a.split(" K=")[1].split()[0]), int(b.split(" K=")[1].split()[0])
        assert ka * 4 == kb * 9 and a.split(" K=")[0].replace("ups=1", "ups=2") == b.split(" K=")[0]
    with torch.no_grad():
        ref = O.unet3d_forward({k: v.cuda() for k, v in sd.items()}, O.OracleConfig.from_native(ucfg), sample, int(g["t"]), ctx).float()

    def rel(a, b):
        return ((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt()).item()
    d01, d0, d1 = rel(outs["1"], outs["0"]), rel(outs["0"], ref), rel(outs["1"], ref)
    print(f"rel-L2: phase vs 3x3 {d01:.3e}   3x3 vs fp32 oracle {d0:.3e}   phase vs fp32 oracle {d1:.3e}")
    assert d01 < d0 and d01 < d1
