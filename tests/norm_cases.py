"""The cases, inputs, float64 references and the elementwise bound of the GroupNorm / LayerNorm op tests (a helper module: no test functions).
Shared by tests/test_norm_bound_host.py (the bound against an fp32 emulation of the kernels' arithmetic and against deliberately wrong variants),
tests/test_norm_gpu.py (norm.hip itself) and tests/test_launch_routes_host.py (the GroupNorm table reaches every instantiation).

Inputs, drawn on the CPU from a seeded torch.Generator (the same numbers on every machine): every (image, group) of a GroupNorm and every row of a
LayerNorm has its own scale sd = 2^u, u ~ U[-2, 2], and its own mean mu = clamp(U[-1, 1] * 16 sd, -8, 8); x = mu + sd * N(0, 1), rounded to bf16.
|mu| / sd <= 16 holds by construction: a stated condition of the inputs, under which the fp32 one-pass variance E[x^2] - mean^2 of norm.hip stays
well inside the bound (it is not a test of that design choice).  gamma, beta and the pe table ~ N(0, 1) in fp32.

Reference: float64 torch on the same bf16 values (biased variance, eps inside the sqrt, SiLU as x * sigmoid(x), pe added after the affine), which
also returns xhat and the pre-activation magnitude mag = |gamma| |xhat| + |beta| (+ |pe|).

Bound, elementwise:   |out - ref| <= 2^-8 |ref| + 2^-10 mag + 2^-14 |gamma|
  2^-8 |ref|     the half-ulp of the bf16 result
  2^-10 mag      about 1e-3 of relative slack on rstd and the affine
  2^-14 |gamma|  the fp32 error of the mean, visible where the result is near zero
A case's figure is its worst ratio max(|out - ref| / bound); <= 1 passes."""
from collections import namedtuple

import torch

# ------------------------------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------------------------------
# form: what nr_gn_route makes of the case, as tests/test_launch_routes_host.py reads it from the launch trace: kind "small" / "slab" / "chunked2" /
# "chunked3" and, where the case is in the table for one of them, maxp (small), nv / gs (slab), pl1 (chunked: one pixel lane, C / 8 >= 256).
# const: (image, group, value) of one constant group.
GnCase = namedtuple("GnCase", "nimg hw c0 c1 groups silu eps form const note", defaults=(None, ""))


def _gn(nimg, hw, c0, c1, groups, form, note="", eps=None, const=None):
    i = len(_GN)      # silu alternates down the table, eps 1e-5 / 1e-6 in pairs, so the four combinations all occur in every form
    _GN.append(GnCase(nimg, hw, c0, c1, groups, i % 2 == 0, eps if eps is not None else (1e-5 if (i // 2) % 2 == 0 else 1e-6), form, const, note))


_GN = []
# small image: one workgroup per (image, group)
_gn(3, 1, 64, 0, 32, dict(kind="small", maxp=8), "hw = 1")
_gn(3, 1, 1280, 1280, 32, dict(kind="small", maxp=8), "hw = 1, concat")
_gn(2, 4, 128, 64, 32, dict(kind="small", maxp=8), "concat split inside a group")
_gn(2, 64, 1280, 0, 32, dict(kind="small", maxp=8))
_gn(2, 64, 1280, 1280, 32, dict(kind="small", maxp=16))
_gn(1, 64, 5120, 0, 32, dict(kind="small", maxp=48))
_gn(2, 40, 256, 0, 64, dict(kind="small"), "64 groups")
# slab: one workgroup per (image, set of GS groups)
_gn(2, 65, 256, 0, 32, dict(kind="slab", gs=1, nv=2), "one chunk per pixel")
_gn(2, 65, 320, 0, 32, dict(kind="slab", gs=4, nv=2), "every chunk straddles two groups, 2 idle threads")
_gn(2, 70, 200, 120, 32, dict(kind="slab"), "concat split on a group edge")
_gn(2, 70, 328, 312, 32, dict(kind="slab", gs=2), "concat split inside a group")
_gn(2, 72, 640, 320, 32, dict(kind="slab", nv=4), "cg = 30")
_gn(2, 144, 1280, 640, 32, dict(kind="slab", nv=8), "cg = 60")
_gn(2, 900, 320, 0, 32, dict(kind="slab", nv=12))
_gn(2, 1300, 320, 0, 32, dict(kind="slab", nv=16))
_gn(1, 2200, 320, 0, 32, dict(kind="slab", nv=24))
_gn(1, 1700, 2304, 0, 32, dict(kind="slab", nv=32), "cg = 72")
_gn(64, 100, 640, 0, 32, dict(kind="slab", gs=8), "12 idle threads")
_gn(64, 100, 1280, 0, 32, dict(kind="slab", gs=8, nv=12), "40 chunks per pixel")
_gn(3, 100, 64, 0, 4, dict(kind="slab", grid=12), "grid of 12: the non-remapped block order")
_gn(3, 100, 320, 0, 32, dict(kind="slab", grid=24), "grid of 24: the remapped order, odd image count")
_gn(2, 100, 64, 0, 1, dict(kind="slab"), "one group")
_gn(2, 100, 512, 0, 64, dict(kind="slab"), "64 groups")
# chunked, two launches
_gn(32, 128, 64, 0, 32, dict(kind="chunked2"))
_gn(32, 100, 96, 0, 32, dict(kind="chunked2"), "last chunk of 4 px, 21 pixel lanes, 4 idle threads")
# chunked, three launches (gn_finalize)
_gn(2, 65, 64, 0, 32, dict(kind="chunked3"), "last chunk of 1 px")
_gn(1, 300, 224, 0, 32, dict(kind="chunked3"), "idle threads")
_gn(1, 5000, 128, 0, 32, dict(kind="chunked3"), "313 chunks: gn_finalize's second stride")
_gn(1, 20000, 128, 0, 32, dict(kind="chunked3"), "64 px per block = 4 pixel-lane rounds: the unrolled apply loop; the VAE's own form")
_gn(1, 2100, 2048, 0, 32, dict(kind="chunked3", pl1=True), "one pixel lane; unrolled loop twice per chunk, then the tail chunk")
_gn(2, 1633, 2560, 0, 32, dict(kind="chunked3", pl1=True), "C / 8 > 256: strided channel loop, scale / shift from LDS")
_gn(1, 1700, 1280, 1280, 32, dict(kind="chunked3", pl1=True), "C / 8 > 256 with concat")
_gn(2, 128, 256, 0, 64, dict(kind="chunked3"), "chunked with more than 32 groups")
_gn(2, 65, 64, 0, 32, dict(kind="chunked3"), "one constant group: ref = beta, or silu(beta)", eps=1e-6, const=(0, 3, 0.75))
GN_CASES = tuple(_GN)

# pe: (table rows, pe_hw, pe_F) of the with-pe run
LnCase = namedtuple("LnCase", "M C pe")
LN_CASES = tuple(LnCase(M, C, pe) for M, C, pe in [
    (1, 8, (3, 1, 3)), (33, 40, (4, 3, 4)), (17, 128, (4, 3, 4)), (5, 136, (2, 2, 2)), (37, 192, (8, 2, 5)), (19, 200, (4, 3, 4)), (16, 384, (4, 3, 4)),
    (9, 392, (4, 2, 3)), (8, 768, (4, 1, 4)), (7, 776, (4, 2, 2)), (5, 1536, (4, 1, 3)), (3, 1544, (4, 1, 2)), (2, 4096, (2, 1, 2)),
    (105, 320, (24, 5, 7)), (50, 640, (16, 1, 16)), (77, 1280, (8, 4, 8))])


def gn_id(c):
    return f"{c.nimg}x{c.hw}x{c.c0}+{c.c1}-g{c.groups}-silu{int(c.silu)}-eps{c.eps:g}" + ("-const" if c.const else "")


def ln_id(c):
    return f"{c.M}x{c.C}"


# ------------------------------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------------------------------
def _draw(gen, nset, nper_shape):
    """[nset, *nper_shape] fp32: set i ~ mu_i + sd_i N(0, 1) with sd_i = 2^U[-2, 2], mu_i = clamp(U[-1, 1] 16 sd_i, -8, 8)."""
    sd = torch.exp2(torch.rand(nset, generator=gen) * 4 - 2)
    mu = ((torch.rand(nset, generator=gen) * 2 - 1) * 16 * sd).clamp(-8, 8)
    bc = (nset,) + (1,) * len(nper_shape)
    return mu.view(bc) + sd.view(bc) * torch.randn(nset, *nper_shape, generator=gen)


def gn_inputs(nimg, hw, C, groups, seed=0, const=None):
    """x bf16 [nimg, hw, C], gamma fp32 [C], beta fp32 [C] (CPU)."""
    gen = torch.Generator().manual_seed(1000003 * seed + 7919 * nimg + 31 * hw + C + groups)
    cg = C // groups
    x = _draw(gen, nimg * groups, (hw, cg)).view(nimg, groups, hw, cg).permute(0, 2, 1, 3).reshape(nimg, hw, C)
    if const is not None:
        img, g, val = const
        x[img, :, g * cg:(g + 1) * cg] = val
    return x.to(torch.bfloat16).contiguous(), torch.randn(C, generator=gen), torch.randn(C, generator=gen)


def gn_case_inputs(c):
    return gn_inputs(c.nimg, c.hw, c.c0 + c.c1, c.groups, seed=GN_CASES.index(c), const=c.const)


def ln_inputs(M, C, pe_rows=0, seed=0):
    """x bf16 [M, C], gamma, beta fp32 [C], pe fp32 [pe_rows, C] or None (CPU)."""
    gen = torch.Generator().manual_seed(1000003 * seed + 7919 * M + C)
    x = _draw(gen, M, (C,)).to(torch.bfloat16).contiguous()
    gamma, beta = torch.randn(C, generator=gen), torch.randn(C, generator=gen)
    return x, gamma, beta, (torch.randn(pe_rows, C, generator=gen) if pe_rows else None)


# ------------------------------------------------------------------------------------------------------------------------------------------------
# float64 references: (ref, xhat, mag)
# ------------------------------------------------------------------------------------------------------------------------------------------------
def gn_reference(x, gamma, beta, groups, eps, silu):
    nimg, hw, C = x.shape
    xg = x.double().view(nimg, hw, groups, C // groups)
    mean = xg.mean(dim=(1, 3), keepdim=True)
    var = ((xg - mean) ** 2).mean(dim=(1, 3), keepdim=True)
    xhat = ((xg - mean) / torch.sqrt(var + eps)).view(nimg, hw, C)
    g, b = gamma.double(), beta.double()
    y = xhat * g + b
    return (y * torch.sigmoid(y) if silu else y), xhat, g.abs() * xhat.abs() + b.abs()


def ln_reference(x, gamma, beta, eps, pe=None, pe_hw=1, pe_F=1):
    M, C = x.shape
    xd = x.double()
    mean = xd.mean(dim=1, keepdim=True)
    var = ((xd - mean) ** 2).mean(dim=1, keepdim=True)
    xhat = (xd - mean) / torch.sqrt(var + eps)
    g, b = gamma.double(), beta.double()
    ref, mag = xhat * g + b, g.abs() * xhat.abs() + b.abs()
    if pe is not None:
        rows = pe.double()[(torch.arange(M, device=x.device) // pe_hw) % pe_F]
        ref, mag = ref + rows, mag + rows.abs()
    return ref, xhat, mag


# ------------------------------------------------------------------------------------------------------------------------------------------------
# the bound
# ------------------------------------------------------------------------------------------------------------------------------------------------
def bound(ref, mag, gamma):
    return 2.0 ** -8 * ref.abs() + 2.0 ** -10 * mag + 2.0 ** -14 * gamma.double().abs()


def worst_ratio(out, ref, mag, gamma):
    """max over the elements of |out - ref| / bound (inf if out holds a NaN)."""
    r = (out.double() - ref).abs() / bound(ref, mag, gamma)
    return float("inf") if torch.isnan(r).any() else r.max().item()


def check(name, out, ref, mag, gamma):
    assert tuple(out.shape) == tuple(ref.shape), (name, out.shape, ref.shape)
    assert not torch.isnan(out).any(), f"{name}: elements of the NaN-filled result were left unwritten (or NaN was computed)"
    assert torch.isfinite(out).all(), f"{name}: non-finite output"
    w = worst_ratio(out, ref, mag, gamma)
    print(f"[{name}] worst |err| / bound = {w:.3f}")
    assert w <= 1.0, f"{name}: |out - ref| reaches {w:.3f} x (2^-8 |ref| + 2^-10 mag + 2^-14 |gamma|)"
    return w


def run(name, call, shape, ref, mag, gamma, dev):
    """call(out) writes the op's result into out.  Twice into NaN-filled results: all written, finite, same bits, within the bound."""
    outs = []
    for _ in range(2):
        out = torch.full(shape, float("nan"), dtype=torch.bfloat16, device=dev)
        got = call(out)
        assert got.data_ptr() == out.data_ptr()
        outs.append(out)
    torch.cuda.synchronize()
    w = check(name, outs[0].view(ref.shape), ref, mag, gamma)
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), f"{name}: two calls on the same inputs differ"
    return w
