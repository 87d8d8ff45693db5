"""The 32-frame form of the temporal attention head kernel (tattnw.hip, ``tattn_head_kernel<D, 32>``): BASELINE config 5's clips on the C = 640 / 1280 levels.

Op level against the fp32 torch composition of the reference (the recipe and the tolerances of tests/test_ops_gpu.py for the 16-frame kernel), the
16-frame kernel against a recording made on the commit before this one, the reference's own VanillaTemporalModule at 32 frames through a leaf handle
(tests/golden/leaf_tm_f32.npz, tools/gen_golden_leaf_tm_f32.py; gate of tests/test_leaf_gpu.py), a U-Net + SparseCtrl pair with the head path on and off,
and the 16 -> 32 -> 16 re-plan of one handle."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)


def _reference(t, nbatch, F, hw, gamma, beta, wq, wk, wv):
    """tests/test_ops_gpu.py: test_temporal_attention_head_kernel_matches_torch, for F frames"""
    from neurons_amd import ops
    C, H = t.shape[1], 8
    x = t.float().view(nbatch, F, hw, C)
    n = torch.nn.functional.layer_norm(x, (C,), gamma, beta, 1e-5) + ops.temporal_pe_table(F, C, t.device)[None, :, None, :]
    seq = n.permute(0, 2, 1, 3).reshape(nbatch * hw, F, C)                     # (b d) f c
    q, k, v = (torch.nn.functional.linear(seq, w).view(-1, F, H, C // H).transpose(1, 2) for w in (wq, wk, wv))
    a = torch.softmax(q @ k.transpose(-1, -2) * (C // H) ** -0.5, dim=-1) @ v
    return a.transpose(1, 2).reshape(nbatch, hw, F, C).permute(0, 2, 1, 3)


# mean |error| / mean |reference| of the THREE-LAUNCH path (LayerNorm-folded q|k|v GEMM + temporal attention core) of the commit before the 32-frame head
# kernel, measured on an MI355X on exactly the inputs of the op test below (plain variant), keyed by (C, nbatch, hw)
THREE_LAUNCH_MEAN_REL = {(640, 1, 8): 3.9834e-3, (640, 2, 64): 4.0578e-3, (640, 3, 24): 4.0363e-3,
                         (1280, 1, 4): 4.0831e-3, (1280, 2, 64): 3.9720e-3, (1280, 3, 12): 4.0557e-3}


def _cmp32(name, out, ref, max_tol, mean_tol):
    """tests/test_ops_gpu.py: _cmp with the bounds given as fractions of the reference's max / mean"""
    out, ref = out.float(), ref.float()
    assert out.shape == ref.shape, (name, out.shape, ref.shape)
    assert torch.isfinite(out).all(), f"{name}: non-finite output"
    err = (out - ref).abs()
    mx, mean = err.max().item(), err.mean().item()
    rmx, rmean = ref.abs().max().item(), ref.abs().mean().item()
    print(f"[{name}] max_err={mx:.4e} (ref max {rmx:.3e}, ratio {mx / rmx:.4e}, bound {max_tol:.3e})  mean_err={mean:.4e} (ref mean {rmean:.3e}, ratio {mean / rmean:.4e}, bound {mean_tol:.3e})")
    assert mx <= max_tol * rmx + 1e-6, f"{name}: max err {mx} vs ref max {rmx}"
    assert mean <= mean_tol * rmean + 1e-7, f"{name}: mean err {mean} vs ref mean {rmean}"


@pytest.mark.parametrize("C,nbatch,hw", [(640, 1, 8), (640, 2, 64), (640, 3, 24), (1280, 1, 4), (1280, 2, 64), (1280, 3, 12)])
def test_temporal_attention_head_kernel_32_frames_matches_torch(cuda, C, nbatch, hw):
    """norm -> (+ positional encoding) -> to_q|k|v -> softmax(q k^T / sqrt(d)) v over the 32 frames of each pixel, d = 80 / 160, 8 heads, one launch,
    against the fp32 torch composition of the reference (motion_module.py:210-218, :270-329, :225-243; motion_module_new.py:201-287).  Shapes: the
    smallest hw the kernel takes at each width, the 8 x 8 level of the leaf fixtures at two clips, pixel-group counts that are not a multiple of
    8 (the other workgroup -> XCD mapping at C = 640), an odd batch.

    Tolerances: those tests/test_ops_gpu.py applies to the 16-frame kernel -- 2e-2 of the reference's max and 4e-3 of its mean; 4e-2 / 8e-3 with the rows
    offset by 6 sigma -- with ONE exception: the mean bound of the plain variant.  With 32 keys it is missed by the three-launch path of the previous
    commit (LayerNorm-folded q|k|v GEMM + attention core) just as by the head kernel.  Measured on an MI355X on these six inputs, mean error / mean |reference|:
        three launches, previous commit: 3.97e-3 .. 4.08e-3 (plain; per case THREE_LAUNCH_MEAN_REL), 3.93e-3 .. 4.10e-3 (offset)
        head kernel, 32 frames:          3.97e-3 .. 4.08e-3 (plain),                                 3.93e-3 .. 4.10e-3 (offset)
    (per case the two agree to three digits: the error is the bf16 rounding of q, k, v and P, which both paths share; max error / max |reference| is
    7.1e-3 .. 1.03e-2 for both).  So the plain mean bound is 1.25 x the recorded three-launch error of the case: 4.97e-3 .. 5.10e-3.  The margin covers
    another fp32 summation order, nothing else.  The other three bounds are those of the 16-frame test, unchanged."""
    from neurons_amd import ops
    F = 32
    g = torch.Generator(device="cuda").manual_seed(C + nbatch * 1000 + hw + 32)
    t = (torch.randn(nbatch * F * hw, C, generator=g, device="cuda") * 1.1 + 0.1).to(torch.bfloat16)
    gamma = 1.0 + 0.2 * torch.randn(C, generator=g, device="cuda")
    beta = 0.1 * torch.randn(C, generator=g, device="cuda")
    wq, wk, wv = (torch.randn(C, C, generator=g, device="cuda") * C ** -0.5 for _ in range(3))
    wq = wq * 2.0                                  # sharper softmax: exercises the max subtraction
    out = ops.tattn_head(t, nbatch, hw, gamma, beta, wq, wk, wv, frames=F)
    _cmp32(f"temporal attention head kernel F=32 C={C} nbatch={nbatch} hw={hw}", out.view(nbatch, F, hw, C), _reference(t, nbatch, F, hw, gamma, beta, wq, wk, wv),
           2e-2, 1.25 * THREE_LAUNCH_MEAN_REL[(C, nbatch, hw)])
    assert torch.equal(out, ops.tattn_head(t, nbatch, hw, gamma, beta, wq, wk, wv, frames=F))
    # row statistics under a large common offset (|mean| >> std: the cancellation case of the folded LayerNorm)
    t2 = (t.float() + 6.0).to(torch.bfloat16)
    _cmp32(f"temporal attention head kernel F=32 C={C} (rows offset by 6 sigma)", ops.tattn_head(t2, nbatch, hw, gamma, beta, wq, wk, wv, frames=F).view(nbatch, F, hw, C),
           _reference(t2, nbatch, F, hw, gamma, beta, wq, wk, wv), 4e-2, 8e-3)


def test_each_frame_attends_to_all_32_frames(cuda):
    """Flat logits (to_q = to_k = 0): every query's output is the MEAN of the value rows of all 32 frames.  Catches a kernel that normalises or sums over
    one 16-frame half only (off by a factor of two, or the mean of the wrong frames: far outside the tolerance of the op test above)."""
    from neurons_amd import ops
    C, F, hw = 640, 32, 8
    g = torch.Generator(device="cuda").manual_seed(7)
    base = torch.randn(F * hw, C, generator=g, device="cuda").to(torch.bfloat16)
    ones, zeros = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
    wv = torch.randn(C, C, generator=g, device="cuda") * C ** -0.5
    wz = torch.zeros(C, C, device="cuda")          # q = k = pe-free zero: flat softmax; v = LayerNorm(t) Wv^T + pe Wv^T
    out = ops.tattn_head(base, 1, hw, ones, zeros, wz, wz, wv, frames=F).float().view(F, hw, C)
    n = torch.nn.functional.layer_norm(base.float().view(F, hw, C), (C,)) + ops.temporal_pe_table(F, C, base.device)[:, None, :]
    want = torch.nn.functional.linear(n, wv).mean(0, keepdim=True).expand(F, hw, C)
    err = (out - want).abs().max().item()
    print(f"[flat softmax over 32 frames] max_err={err:.3e} (ref max {want.abs().max().item():.3e})")
    assert err <= 2e-2 * want.abs().max().item() + 1e-6


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_16_frame_kernel_is_bit_identical_to_the_recording_of_the_previous_commit(cuda):
    """No existing behaviour changes: ``ops.tattn_head`` with the default frame count and with ``frames=16`` return the same bits, and those are the bits
    the kernel returned on the commit before the 32-frame form existed (tests/golden/tattn_head_f16_c640.npz, tools/record_tattn_head_f16.py: one
    C = 640 output on Philox-seeded inputs)."""
    from neurons_amd import ops
    rec = _tool("record_tattn_head_f16")
    t, gamma, beta, wq, wk, wv = rec.inputs(cuda)
    a = ops.tattn_head(t, rec.NBATCH, rec.HW, gamma, beta, wq, wk, wv)
    b = ops.tattn_head(t, rec.NBATCH, rec.HW, gamma, beta, wq, wk, wv, frames=16)
    assert torch.equal(a, b)
    g = np.load(os.path.join(GOLD, "tattn_head_f16_c640.npz"))
    assert tuple(a.shape) == tuple(g["shape"])
    got = a.view(torch.int16).cpu().numpy().view(np.uint16)
    ndiff = int((got != g["a"]).sum())
    print(f"[16-frame head kernel vs the recording] differing bf16 values: {ndiff} of {got.size}")
    assert ndiff == 0


@pytest.mark.parametrize("C,seed", [(640, 81), (1280, 85)])
def test_temporal_module_32_frames_runs_the_head_kernel_and_matches_reference(cuda, C, seed):
    """The reference's VanillaTemporalModule (temporal_position_encoding_max_len = 32, two Temporal_Self blocks) on (1, C, 32, 8, 8) = 2048 rows through
    a leaf handle = the launch sequence temporal_module() emits inside the U-Net at this shape.  Plan asserted: per temporal attention ONE
    ``tattn_head ... F=32`` launch + the to_out GEMM, no q|k|v GEMM, no attention core.  Gate: that of tests/test_leaf_gpu.py for the 16-frame fixtures
    at these widths (rel-L2 < 1.5e-2, PSNR > 40 dB)."""
    from neurons_amd.ops import NativeLeaf
    from neurons_amd.synth import randn
    from neurons_amd.unet3d import _motion_keys
    from test_leaf_gpu import _compare, _fill
    g = np.load(os.path.join(GOLD, "leaf_tm_f32.npz"))
    F, hw = 32, 8
    M = F * hw * hw
    tag = f"tm{C}f32"
    leaf = NativeLeaf("temporal", channels=C, heads=8, num_attention_blocks=2, pe_max_len=32)
    leaf.load_state_dict(_fill({k[2:]: v for k, v in _motion_keys("m", C, 2).items()}, tag, seed))
    x = randn(f"{tag}.x", (1, C, F, hw, hw), seed + 1).cuda()
    y = leaf(x)
    desc = [d for d in leaf.op_descriptions() if d]
    print("\n".join(desc))
    assert sum(d.startswith(f"tattn_head M={M} C={C} F=32") for d in desc) == 2, desc
    assert not any(d.startswith("attention") for d in desc), desc
    assert not any(f"N={3 * C} K={C}" in d for d in desc), desc                      # no q|k|v projection of its own, on any GEMM kernel
    assert not any(d.startswith(("tattn_fused", "ff_fused")) for d in desc), desc
    _compare(f"VanillaTemporalModule (1,{C},32,{hw},{hw}) vs reference", y, g, tag)
    assert torch.equal(y, leaf(x, graph=False))
    assert torch.equal(y, leaf(x))


def test_one_handle_replanned_16_32_16_frames(cuda):
    """The packed epilogue table holds one row per frame: a handle planned at 16 frames and re-planned at 32 must not reuse the 16-position table (and
    back).  The two 16-frame runs agree bit for bit, the 32-frame run equals a fresh handle's, and every plan names its own frame count."""
    from neurons_amd.ops import NativeLeaf
    from neurons_amd.synth import randn
    from neurons_amd.unet3d import _motion_keys
    from test_leaf_gpu import _fill
    C, hw = 640, 8
    sd = _fill({k[2:]: v for k, v in _motion_keys("m", C, 2).items()}, "tm640f32", 81)
    x16 = randn("replan.x16", (2, C, 16, hw, hw), 91).cuda()
    x32 = randn("replan.x32", (1, C, 32, hw, hw), 92).cuda()
    leaf = NativeLeaf("temporal", channels=C, heads=8, num_attention_blocks=2, pe_max_len=32)
    leaf.load_state_dict(sd)
    y16a = leaf(x16).clone()
    assert sum(d.startswith(f"tattn_head M=2048 C={C} F=16") for d in leaf.op_descriptions()) == 2, leaf.op_descriptions()
    y32 = leaf(x32).clone()
    assert sum(d.startswith(f"tattn_head M=2048 C={C} F=32") for d in leaf.op_descriptions()) == 2, leaf.op_descriptions()
    y16b = leaf(x16).clone()
    assert sum(d.startswith(f"tattn_head M=2048 C={C} F=16") for d in leaf.op_descriptions()) == 2, leaf.op_descriptions()
    assert torch.equal(y16a, y16b)
    fresh = NativeLeaf("temporal", channels=C, heads=8, num_attention_blocks=2, pe_max_len=32)
    fresh.load_state_dict(sd)
    assert torch.equal(y32, fresh(x32))
    assert torch.equal(y16a, fresh(x16))
    # frames 16 .. 31 of the 32-frame run carry their own positions: the second half is not a copy of a 16-position evaluation
    assert not torch.equal(y32[:, :, :16], y32[:, :, 16:])


def _networks_one_evaluation(dev):
    """One evaluation of a U-Net + SparseCtrl pair at 32 frames, condition on frame 0.  tests/tiny_configs.py's widths (64 .. 128) never reach the head
    kernel, so this is the tiny configuration with its SECOND level widened to 640 channels: the narrowest configuration with a C = 640 level (latent
    16 x 16 -> that level is 8 x 8: 2 x 32 x 64 = 4096 rows per temporal attention)."""
    from neurons_amd import _lib, NativeSparseCtrl, NativeUNet3D
    from neurons_amd.sparsectrl import controlnet_config_from_unet
    from neurons_amd.synth import randn
    from neurons_amd.unet3d import UNet3DConfig, random_state_dict
    ucfg = UNet3DConfig(sample_size=16, block_out_channels=(64, 640, 128, 128), cross_attention_dim=64,
                        motion_module_kwargs=dict(UNet3DConfig().motion_module_kwargs, temporal_position_encoding_max_len=32))
    ccfg = controlnet_config_from_unet(ucfg, dict(
        set_noisy_sample_input_to_zero=True, use_simplified_condition_embedding=True, conditioning_channels=4,
        motion_module_kwargs=dict(attention_block_types=["Temporal_Self"], temporal_position_encoding_max_len=32)))
    unet, ctrl = NativeUNet3D(ucfg).to(dev), NativeSparseCtrl(ccfg).to(dev)
    unet.load_state_dict(random_state_dict(ucfg, _lib.NR_KIND_UNET3D, seed=21))
    ctrl.load_state_dict(random_state_dict(ccfg, _lib.NR_KIND_SPARSECTRL, seed=22, zero_init_heads=False))
    F, L = 32, 16
    x = randn("net32.x", (1, 4, F, L, L), 23).to(dev)
    ctx = randn("net32.ctx", (2, 77, 64), 24).to(dev)
    cond = torch.zeros(1, 4, F, L, L, device=dev)
    cond[:, :, 0] = randn("net32.cond", (1, 4, L, L), 25).to(dev) * 0.18215
    mask = torch.zeros(1, 1, F, L, L, device=dev)
    mask[:, :, 0] = 1
    xin = torch.cat([x] * 2)
    down, mid = ctrl(xin, 481, encoder_hidden_states=ctx, controlnet_cond=cond, conditioning_mask=mask, return_dict=False)
    eps = unet(xin, 481, encoder_hidden_states=ctx, down_block_additional_residuals=down, mid_block_additional_residual=mid).sample
    torch.cuda.synchronize()
    return dict(eps=eps.float().cpu(), mid=mid.float().cpu(), down1=down[4].float().cpu(), unet_desc=[d for d in unet.op_descriptions() if d],
                ctrl_desc=[d for d in ctrl.op_descriptions() if d])


def test_networks_at_32_frames_head_path_on_and_off_agree(cuda, tmp_path):
    """The U-Net and SparseCtrl (whose identical-frame shortcut reduces the frame set of its first per-frame layers only: every temporal attention sees
    all 32 frames) with the head kernel on, against the same evaluation in a child process with NR_TATTN_HEAD=0 (q|k|v GEMM + attention core).  Gate:
    that of tests/test_c4c5_gpu.py: test_c5_32_frames_64x64_one_evaluation (rel-L2 <= 2.5e-2, PSNR >= 30 dB)."""
    from test_c4c5_gpu import FWD_REL_L2
    from test_engine_gpu import metrics
    if os.environ.get("NR_TATTN_HEAD", "")[:1] == "0":
        pytest.fail("NR_TATTN_HEAD=0 in the environment of the test run: the head path under test is switched off")
    on = _networks_one_evaluation(cuda)
    for name in ("unet_desc", "ctrl_desc"):
        heads = [d for d in on[name] if d.startswith("tattn_head")]
        print(name, len(heads), "tattn_head launches:", sorted(set(h.split(" (")[0] for h in heads)))
        assert heads and all("C=640 F=32" in h for h in heads), on[name]
    # SparseCtrl's temporal attentions run on ALL 32 frames x 64 pixels of every sample, not on the reduced frame set of its first layers
    ctrl_rows = [int(d.split("M=")[1].split()[0]) for d in on["ctrl_desc"] if d.startswith("tattn_head")]
    assert len(ctrl_rows) >= 2 and all(m >= 32 * 64 and m % (32 * 64) == 0 for m in ctrl_rows), ctrl_rows
    out = str(tmp_path / "off.pt")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=dict(os.environ, NR_TATTN_HEAD="0"), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    off = torch.load(out)
    assert not any(d.startswith("tattn_head") for d in off["unet_desc"] + off["ctrl_desc"])
    assert any(d.startswith("attention mode=2") for d in off["unet_desc"]) and any(d.startswith("attention mode=2") for d in off["ctrl_desc"])
    for key in ("mid", "down1", "eps"):
        rel, psnr = metrics(f"32 frames, head kernel on vs NR_TATTN_HEAD=0: {key}", on[key], off[key])
        assert rel <= FWD_REL_L2 and psnr >= 30.0, (key, rel, psnr)


if __name__ == "__main__":           # the NR_TATTN_HEAD=0 arm of the network test (the switch is read once per process)
    torch.save(_networks_one_evaluation(torch.device("cuda", 0)), sys.argv[1])
