"""The elementwise bound of tests/norm_cases.py has teeth and fits a correct kernel: CPU only.

An fp32 emulation of norm.hip's arithmetic stands in for the kernels.  GroupNorm: one-pass statistics (sum and sum of squares in fp32, summed as a
tree and as running sums of the length the kernels keep, see _sum32; var = max(q / n - mean^2, 0)), rstd = 1 / sqrt(var + eps), the fold into scale = gamma rstd, shift = beta - mean scale,
one multiply-add per element, SiLU in fp32, bf16 result.  LayerNorm: two-pass statistics in fp32, (x - mean) rstd gamma + beta (+ pe), bf16 result.
The correct emulation must be inside the bound on every shape; each deliberately wrong one (the mistakes this code invites: a group normalised
with its neighbour's statistics, the last image with image 0's, the last pixel left out of the sums; a LayerNorm row with the previous row's
statistics) must be outside it on every shape where the mistake changes anything."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import norm_cases as nc  # noqa: E402

# (nimg, hw, C, silu, eps), 32 groups
GN_SHAPES = [(3, 1, 64, True, 1e-5), (2, 65, 320, False, 1e-6), (4, 1024, 320, True, 1e-5), (1, 5000, 128, True, 1e-6), (1, 64, 5120, False, 1e-5),
             (2, 1633, 2560, True, 1e-5)]
GN_VARIANTS = ("neighbour_group", "image0_stats", "last_pixel_dropped")
LN_SHAPES = [(33, 40, None), (17, 128, (4, 3, 4)), (19, 200, None), (7, 776, (4, 2, 2)), (2, 4096, None), (105, 320, (24, 5, 7))]


RUN = 256      # the longest running sum of norm.hip: gn_slab_kernel<32> adds 32 chunks x 8 elements into one register before any tree step


def _sum32(t, sequential):
    """fp32 sum over the last dim: torch's tree, or running fp32 sums in element order over runs of RUN elements whose totals are then added as a
    tree (strictly sequential up to RUN elements).  No kernel keeps one running sum longer than RUN: over the 20 000 .. 130 000 elements of the two
    largest shapes a single running fp32 sum reaches 1.08 x and 10.9 x the bound (a random walk of sqrt(n) 2^-24 on a mean of up to 16 sd), which
    says something about that order of summation and nothing about the kernels."""
    if not sequential:
        return t.sum(dim=-1)
    n = t.shape[-1]
    pad = torch.nn.functional.pad(t, (0, -n % RUN)).reshape(*t.shape[:-1], -1, RUN)
    return torch.from_numpy(np.ascontiguousarray(np.cumsum(pad.numpy(), axis=-1, dtype=np.float32)[..., -1])).sum(dim=-1)


def gn_emulate(x, gamma, beta, groups, eps, silu, sequential=False, variant=None):
    nimg, hw, C = x.shape
    cg = C // groups
    xg = x.float().view(nimg, hw, groups, cg)
    xs = xg[:, :hw - 1] if variant == "last_pixel_dropped" else xg      # the sums miss the pixel, the count does not
    xs = xs.permute(0, 2, 1, 3).reshape(nimg, groups, -1).contiguous()
    s, q = _sum32(xs, sequential), _sum32(xs * xs, sequential)
    inv = torch.tensor(1.0, dtype=torch.float32) / (torch.tensor(float(cg), dtype=torch.float32) * torch.tensor(float(hw), dtype=torch.float32))
    mean = s * inv
    rstd = 1.0 / torch.sqrt((q * inv - mean * mean).clamp_min(0.0) + torch.tensor(eps, dtype=torch.float32))
    if variant == "neighbour_group":
        g = groups // 2
        mean[:, g], rstd[:, g] = mean[:, g + 1].clone(), rstd[:, g + 1].clone()
    elif variant == "image0_stats":
        mean[-1], rstd[-1] = mean[0].clone(), rstd[0].clone()
    scale = gamma.view(1, groups, cg) * rstd.unsqueeze(-1)                # [nimg, groups, cg]
    shift = beta.view(1, groups, cg) - mean.unsqueeze(-1) * scale
    y = xg * scale.unsqueeze(1) + shift.unsqueeze(1)
    if silu:
        y = y * (1.0 / (1.0 + torch.exp(-y)))
    assert y.dtype == torch.float32
    return y.view(nimg, hw, C).to(torch.bfloat16)


def ln_emulate(x, gamma, beta, eps, pe=None, pe_hw=1, pe_F=1, variant=None):
    M, C = x.shape
    xf = x.float()
    mean = xf.sum(dim=1, keepdim=True) / float(C)
    d = xf - mean
    rstd = 1.0 / torch.sqrt((d * d).sum(dim=1, keepdim=True) / float(C) + torch.tensor(eps, dtype=torch.float32))
    if variant == "previous_row":
        mean, rstd = torch.cat([mean[:1], mean[:-1]]), torch.cat([rstd[:1], rstd[:-1]])
    y = (xf - mean) * rstd * gamma + beta
    if pe is not None:
        y = y + pe[(torch.arange(M) // pe_hw) % pe_F]
    assert y.dtype == torch.float32
    return y.to(torch.bfloat16)


@pytest.mark.parametrize("nimg,hw,C,silu,eps", GN_SHAPES, ids=[f"{s[0]}x{s[1]}x{s[2]}" for s in GN_SHAPES])
def test_groupnorm_bound_fits_the_fp32_emulation_and_rejects_wrong_kernels(nimg, hw, C, silu, eps):
    x, gamma, beta = nc.gn_inputs(nimg, hw, C, 32, seed=101)
    ref, _, mag = nc.gn_reference(x, gamma, beta, 32, eps, silu)
    for sequential in (False, True):
        w = nc.worst_ratio(gn_emulate(x, gamma, beta, 32, eps, silu, sequential), ref, mag, gamma)
        print(f"[gn-emulation {nimg}x{hw}x{C} {'sequential' if sequential else 'tree'} sums] worst |err| / bound = {w:.3f}")
        assert w <= 1.0, "a correct fp32 one-pass GroupNorm must be inside the bound"
    meaningful = {"neighbour_group": True, "image0_stats": nimg > 1, "last_pixel_dropped": hw > 1}
    for v in GN_VARIANTS:
        if meaningful[v]:
            w = nc.worst_ratio(gn_emulate(x, gamma, beta, 32, eps, silu, variant=v), ref, mag, gamma)
            print(f"[gn-emulation {nimg}x{hw}x{C} {v}] worst |err| / bound = {w:.3g}")
            assert w > 1.0, f"{v}: a wrong kernel inside the bound"


@pytest.mark.parametrize("M,C,pe", LN_SHAPES, ids=[f"{s[0]}x{s[1]}" for s in LN_SHAPES])
def test_layernorm_bound_fits_the_fp32_emulation_and_rejects_wrong_kernels(M, C, pe):
    rows, pe_hw, pe_F = pe if pe else (0, 1, 1)
    x, gamma, beta, table = nc.ln_inputs(M, C, rows, seed=101)
    ref, _, mag = nc.ln_reference(x, gamma, beta, 1e-5, table, pe_hw, pe_F)
    w = nc.worst_ratio(ln_emulate(x, gamma, beta, 1e-5, table, pe_hw, pe_F), ref, mag, gamma)
    print(f"[ln-emulation {M}x{C} pe{int(bool(pe))}] worst |err| / bound = {w:.3f}")
    assert w <= 1.0, "a correct fp32 two-pass LayerNorm must be inside the bound"
    w = nc.worst_ratio(ln_emulate(x, gamma, beta, 1e-5, table, pe_hw, pe_F, variant="previous_row"), ref, mag, gamma)
    print(f"[ln-emulation {M}x{C} previous_row] worst |err| / bound = {w:.3g}")
    assert w > 1.0, "previous_row: a wrong kernel inside the bound"


def test_case_tables_are_well_formed():
    """every GroupNorm case divides into its groups in 16-byte chunks; silu and both eps values occur in every form; the inputs keep |mu| / sd <= 16"""
    kinds = {}
    for c in nc.GN_CASES:
        C = c.c0 + c.c1
        assert C % 8 == 0 and C % c.groups == 0 and c.c0 % 8 == 0 and c.groups <= 64, c
        kinds.setdefault(c.form["kind"], set()).add((c.silu, c.eps))
    for kind in ("small", "slab", "chunked3"):
        assert kinds[kind] == {(True, 1e-5), (False, 1e-5), (True, 1e-6), (False, 1e-6)}, (kind, kinds[kind])
    assert {s for s, _ in kinds["chunked2"]} == {True, False}
    x, _, _ = nc.gn_inputs(4, 1024, 320, 32, seed=5)
    xg = x.double().view(4, 1024, 32, 10)
    mu, sd = xg.mean(dim=(1, 3)), xg.std(dim=(1, 3))
    assert (mu.abs() / sd).max() <= 16 * 1.1 and 0.2 < sd.min() and sd.max() < 4.4 and mu.abs().max() <= 8.3
    assert len({round(v, 3) for v in sd.flatten().tolist()}) >= 120, "every (image, group) has its own scale"
