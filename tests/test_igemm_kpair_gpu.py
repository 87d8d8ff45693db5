"""Arithmetic of the K-pair kernel of the tiled igemm (gemm.hip: igemm_kpair_kernel, TiledPlan::waves == 82) under forced plans
NR_IGEMM_FORCE=128,160,<slabs>,2,<order>,82: two K slices of one 128 x 160 output tile in one 8-wave workgroup, summed through LDS.

Exact regime (the integer operands of tests/igemm_forms.py): the result must equal bf16(fp64 reference) bit for bit inside 256 NaN guard rows.
  * kinds: linear, linear_2src, conv3x3, conv3x3_2src, conv3x3_s2, conv3x3_tap_inner; N = 160, 320 and 352 (a last column tile of 32); M = 300 (a last row tile of 44 rows) and M = 80 (less than one tile)
  * k-tiles per pair that make the two groups differ: nk = 2 (one k-tile per group), 3 and 5 (unequal halves), 49; a two-source boundary c0 inside a
    half and exactly on the half boundary; tap-inner halves that start on a tap that is not 0
  * slab counts: 1 (direct epilogue: bias, row vector, a residual in +-2000), 2 (the kernel writes slabs, splitk_reduce_kernel runs), and a count
    whose doubled slice count does not divide nk
  * tile orders 0 / 1 / 8
Every exact case with a residual draws it in +-2000 (output steps of 8 and 16: round to nearest even, ties).

Real-valued regime (Gaussian operands, one Linear and one conv): with one slab the partial sums and their order are those of the two-slice plan on
free workgroups (128,160,2,2,ord,4) and the result must be bit-identical to it; with two slabs the summation tree differs from split-K 4, so the
result meets the tolerance tests/test_ops_gpu.py asks of the tiled conv (_cmp's defaults) against the fp64 reference.

Mutation (compiled for gfx950, never run): with the `acc[i][j] + xch[...]` add of the kernel dropped, group 0 finishes with the sums of slice 2 j
alone; every one-slab case here has at least one k-tile in slice 2 j + 1 whose integer operands are not all zero, so every one-slab case must fail."""
import pytest
import torch

import igemm_forms as forms
from igemm_forms import Shape
from test_igemm_forms_gpu import _assert_equal, _run_guarded
from test_ops_gpu import _cmp

pytestmark = pytest.mark.gpu

# per kind: the (c0, c1) of its K variants.  Linears: nk = (c0 + c1) / 64; convs: nk = 9 (c0 + c1) / 64
CHANNELS = {
    "linear": [(128, 0), (192, 0), (320, 0), (3136, 0)],                       # nk = 2, 3, 5, 49
    "linear_2src": [(128, 128), (64, 192), (192, 128)],                        # c0 on the half boundary (nk 4) | inside half 0 | inside half 1 of [0, 2) [2, 5)
    "conv3x3": [(64, 0), (192, 0)],                                            # nk = 9 (4 | 5), 27 (13 | 14)
    "conv3x3_2src": [(64, 64), (128, 64)],                                     # nk = 18: tile 9 = (tap 4, c0): on the half boundary | nk = 27: inside
    "conv3x3_s2": [(64, 0)],
    "conv3x3_tap_inner": [(64, 0), (128, 0)],                                  # nk = 9: the second half starts at tap 4 | nk = 18: at chunk 1, tap 0
}
# per kind: (nimg, H, W) of the M = 300 shape (the kind's short shape in igemm_forms) and of the M = 80 shape
GEOMETRY = {
    "linear": ((300, 1, 1), (80, 1, 1)), "linear_2src": ((300, 1, 1), (80, 1, 1)), "conv3x3": ((5, 6, 10), (1, 8, 10)),
    "conv3x3_2src": ((5, 6, 10), (1, 8, 10)), "conv3x3_s2": ((15, 7, 9), (1, 16, 20)), "conv3x3_tap_inner": ((5, 6, 10), (1, 8, 10)),
}


def _register(kind, m_idx, c0, c1, N):
    """the shape under a key of its own in igemm_forms' table of further shapes, so build_exact / shape_of serve it"""
    nimg, H, W = GEOMETRY[kind][m_idx]
    key = f"kp-m{(300, 80)[m_idx]}-c{c0}+{c1}-n{N}"
    forms.EXTRA_SHAPES[(kind, key)] = Shape(nimg, H, W, c0, c1, N)
    return key


def _cases():
    """(id, kind, shape key, slabs, order)"""
    out = []
    for kind, chans in CHANNELS.items():
        for ci, (c0, c1) in enumerate(chans):
            nk = (1 if kind.startswith("linear") else 9) * (c0 + c1) // 64
            for N in (160, 320):
                for m_idx in (0, 1):
                    key = _register(kind, m_idx, c0, c1, N)
                    assert forms.gemm_mnk(kind, forms.shape_of(kind, key))[0] == (300, 80)[m_idx], (kind, key)
                    out.append((kind, key, 1, 0))
                    if N == 320 and m_idx == 0:
                        # two slabs; a slab count whose 2 s slices do not divide nk (3 slabs, or 2 where nk < 6)
                        for slabs in (2, 3):
                            if 2 * slabs <= nk and (slabs == 2 or nk % 6 != 0):
                                out.append((kind, key, slabs, 0))
                        if ci == len(chans) - 1:      # the tile orders on the kind's longest K, without and with slabs
                            for order in (1, 8):
                                out.append((kind, key, 1, order))
                                if nk >= 4:
                                    out.append((kind, key, 2, order))
            # N = 352: a last column tile of 32 columns (the W rows past N, the column guard of the stores), without and with slabs
            key = _register(kind, 0, c0, c1, 352)
            out.append((kind, key, 1, 0))
            if nk >= 4:
                out.append((kind, key, 2, 0))
    return [(f"{kind}-{key}-slabs{slabs}-ord{order}", kind, key, slabs, order) for kind, key, slabs, order in out]


CASES = _cases()


def _force(slabs, order, waves=82):
    return f"128,160,{slabs},2,{order},{waves}"


def _route(kind, key, force, monkeypatch):
    monkeypatch.setenv("NR_IGEMM_FORCE", force)
    plan = forms.route_of(kind, forms.shape_of(kind, key))
    assert plan.status == 0 and plan.cls == "tiled", plan
    return plan


@pytest.fixture(scope="module")
def operands(cuda):
    """operands and bf16(fp64 reference) per (kind, key), built on the CPU once, on the device; never modified afterwards"""
    cache = {}

    def get(kind, key):
        if (kind, key) not in cache:
            t = forms.build_exact(kind, key, "bigres")
            ref = t.pop("ref")
            cache[(kind, key)] = ({n: v.to(cuda) for n, v in t.items()}, tuple(ref.shape), ref.to(torch.bfloat16).to(cuda))
        return cache[(kind, key)]
    return get


def test_case_list_covers_what_it_claims():
    """the k-tile counts, the unequal halves and the slab counts the docstring names are in CASES"""
    nks, slab_nondiv, orders = set(), 0, set()
    for _, kind, key, slabs, order in CASES:
        nk = forms.gemm_mnk(kind, forms.shape_of(kind, key))[2] // 64
        nks.add(nk)
        assert 2 * slabs <= nk
        slab_nondiv += slabs > 1 and nk % (2 * slabs) != 0
        orders.add(order)
    assert {2, 3, 5, 49, 9, 18, 27} <= nks and slab_nondiv >= 6 and orders == {0, 1, 8}
    assert sum(1 for c in CASES if c[3] == 2) >= 12


@pytest.mark.parametrize("cid,kind,key,slabs,order", CASES, ids=[c[0] for c in CASES])
def test_exact(operands, monkeypatch, cuda, cid, kind, key, slabs, order):
    plan = _route(kind, key, _force(slabs, order), monkeypatch)
    assert (plan.bm, plan.bn, plan.waves, plan.stages, plan.splitk, plan.adma, plan.m_fast) == (128, 160, 82, 2, slabs, 1, order), plan
    t, shape, want = operands(kind, key)
    out = _run_guarded(kind, t, shape, cuda)
    _assert_equal(cid, out, want)
    again = _run_guarded(kind, t, shape, cuda)
    _assert_equal(cid + " (second run)", again, out)


def _gaussian(kind, cuda):
    g = torch.Generator().manual_seed(82 + len(kind))
    if kind == "linear":
        M, K, N = 300, 1536, 320
        t = {"a0": torch.randn(M, K, generator=g).to(torch.bfloat16), "w": (torch.randn(N, K, generator=g) * K ** -0.5).to(torch.bfloat16),
             "bias": torch.randn(N, generator=g), "res": torch.randn(M, N, generator=g).to(torch.bfloat16)}
        ref = t["a0"].double() @ t["w"].double().t() + t["bias"].double() + t["res"].double()
        key = _register(kind, 0, K, 0, N)
    else:
        nimg, H, W, Cin, N = 5, 6, 10, 192, 320
        t = {"a0": torch.randn(nimg, H, W, Cin, generator=g).to(torch.bfloat16),
             "w": (torch.randn(N, 3, 3, Cin, generator=g) * (9 * Cin) ** -0.5).to(torch.bfloat16), "bias": torch.randn(N, generator=g),
             "rowvec": torch.randn(nimg, N, generator=g), "res": torch.randn(nimg, H, W, N, generator=g).to(torch.bfloat16)}
        ref = forms._conv_ref(kind, t["a0"], t["w"]) + t["bias"].double() + t["rowvec"].double()[:, None, None, :] + t["res"].double()
        key = _register(kind, 0, Cin, 0, N)
    return key, {n: v.to(cuda) for n, v in t.items()}, tuple(ref.shape), ref.float().to(cuda)


@pytest.mark.parametrize("kind", ["linear", "conv3x3"])
def test_real_valued(monkeypatch, cuda, kind):
    key, t, shape, ref = _gaussian(kind, cuda)
    for order in (0, 1, 8):
        plan = _route(kind, key, _force(1, order), monkeypatch)
        assert (plan.waves, plan.splitk) == (82, 1), plan
        pair = _run_guarded(kind, t, shape, cuda)
        _cmp(f"{kind} K pair, order {order}", pair, ref)
        plan = _route(kind, key, _force(2, order, waves=4), monkeypatch)
        assert (plan.bm, plan.bn, plan.waves, plan.splitk) == (128, 160, 4, 2), plan
        free = _run_guarded(kind, t, shape, cuda)
        _assert_equal(f"{kind}: one slab against two slices on free workgroups, order {order}", pair, free)
    plan = _route(kind, key, _force(2, 0), monkeypatch)
    assert (plan.waves, plan.splitk) == (82, 2), plan
    _cmp(f"{kind} K pairs, two slabs", _run_guarded(kind, t, shape, cuda), ref)
