"""norm.hip through nr_op_groupnorm / nr_op_layernorm, every kernel form, against a float64 reference under an ELEMENTWISE bound.

Cases, inputs, reference and bound are in tests/norm_cases.py: every (image, group) / row has its own mean and scale, so statistics taken from
the wrong group, image, row or pixel range show (tests/test_norm_bound_host.py proves that on an fp32 emulation), and the GroupNorm table reaches
every instantiation of the slab, small-image and chunked forms (tests/test_launch_routes_host.py proves that on the route and the launcher).
Every case runs twice into NaN-pre-filled results: nothing left unwritten, all finite, the same bits both times, and
    |out - ref| <= 2^-8 |ref| + 2^-10 mag + 2^-14 |gamma|       (mag = |gamma| |xhat| + |beta| (+ |pe|))
at every element; each case prints its worst |err| / bound.

Measured on an MI355X: the largest ratio of the GroupNorm table is 0.796 (64 x 100 x 640 and 1 x 2100 x 2048; the smallest 0.641 at 3 x 1 x 64) and
of the LayerNorm table 0.793 (37 x 192, 7 x 776, 77 x 1280); the fp32 emulation of tests/test_norm_bound_host.py reaches 0.67 .. 0.79.  SiLU through
the hardware exp / rcp of silu_f pushes no case over the bound (the largest SiLU case: 0.791), so the bound's second term is as stated.  The chunked
case with 64 groups (2 x 128 x 256) failed before gn_stats_kernel's group reduce covered groups 32 .. 63, which were normalised from uninitialised
scratch (worst ratio 2.3e7), and reaches 0.770 since."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import norm_cases as nc  # noqa: E402


@pytest.mark.parametrize("case", nc.GN_CASES, ids=[nc.gn_id(c) for c in nc.GN_CASES])
def test_groupnorm_elementwise(cuda, case):
    from neurons_amd import ops
    c = case
    x, gamma, beta = (t.to(cuda) for t in nc.gn_case_inputs(c))
    ref, _, mag = nc.gn_reference(x, gamma, beta, c.groups, c.eps, c.silu)
    if c.const:
        img, g, _ = c.const
        cg = (c.c0 + c.c1) // c.groups
        b = beta[g * cg:(g + 1) * cg].double()
        assert torch.equal(ref[img, :, g * cg:(g + 1) * cg], (b * torch.sigmoid(b) if c.silu else b).expand(c.hw, cg)), "a constant group: ref = beta"
    x4 = x.view(c.nimg, c.hw, 1, c.c0 + c.c1)
    x0 = x4[..., :c.c0].contiguous()
    x1 = x4[..., c.c0:].contiguous() if c.c1 else None
    nc.run(f"groupnorm {nc.gn_id(c)}", lambda o: ops.groupnorm(x0, gamma, beta, groups=c.groups, eps=c.eps, silu=c.silu, x1=x1, out=o),
           (c.nimg, c.hw, 1, c.c0 + c.c1), ref, mag, gamma, cuda)


@pytest.mark.parametrize("with_pe", [False, True], ids=["plain", "pe"])
@pytest.mark.parametrize("case", nc.LN_CASES, ids=[nc.ln_id(c) for c in nc.LN_CASES])
def test_layernorm_elementwise(cuda, case, with_pe):
    from neurons_amd import ops
    rows, pe_hw, pe_F = case.pe if with_pe else (0, 1, 1)
    x, gamma, beta, pe = (None if t is None else t.to(cuda) for t in nc.ln_inputs(case.M, case.C, rows))
    ref, _, mag = nc.ln_reference(x, gamma, beta, 1e-5, pe, pe_hw, pe_F)
    nc.run(f"layernorm {nc.ln_id(case)} pe{int(with_pe)}", lambda o: ops.layernorm(x, gamma, beta, pe=pe, pe_hw=pe_hw, pe_F=pe_F, out=o),
           (case.M, case.C), ref, mag, gamma, cuda)


@pytest.mark.parametrize("C", [4104, 12])
def test_layernorm_unserved_width_raises(cuda, C):
    """more than 512 16-byte chunks per row, and a row that is no whole number of them: no kernel, and no launch"""
    from neurons_amd import ops
    x, gamma, beta, _ = (None if t is None else t.to(cuda) for t in nc.ln_inputs(3, C))
    out = torch.full((3, C), float("nan"), dtype=torch.bfloat16, device=cuda)
    with pytest.raises(RuntimeError):
        ops.layernorm(x, gamma, beta, out=out)
    torch.cuda.synchronize()
    assert torch.isnan(out).all(), "nothing may be written for a width that raises"
