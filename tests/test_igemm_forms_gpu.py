"""Arithmetic of every instantiation of the tiled igemm (gemm.hip: igemm_bf16_kernel, splitk_reduce_kernel) under forced plans: the case lists of
tests/igemm_forms.py -- every (form, tile, wave grid, ring depth, adma, lin) the route can name, each conv form on every table row, split-K depths that
do not divide the k-tiles or leave one k-tile per slice, the grouped tile order with a short last band, the phase form under split-K and the grouped
order -- each through its op wrapper into a result with 256 guard rows of NaN on either side.

Exact kinds (Linear, two-source, the 3x3 conv forms, the phase form): integer operands, so every partial sum is exact in fp32 in any order and the one
rounding of the epilogue must give bf16(fp64 reference) BIT FOR BIT; tests/test_igemm_forms_host.py asserts from the reference alone that the operands
stay in that regime.  No tolerance: one wrong k-tile, tap, border column or channel chunk changes an integer by at least 1, which bf16 shows wherever
|ref| <= 256 (>= 99 % of every reference).

GEGLU and the LayerNorm-folded form (erf; row statistics) are not exact: Gaussian operands as tests/test_ops_gpu.py draws them, its _cmp with its
default tolerances against the fp64 reference, and bit identity across ring depths on one tile: the ring depth and the A-operand load path (adma) change
buffering, never the order in which a lane accumulates, and the staged and the direct epilogue apply the same operations in the same order.
  * geglu: adma follows K (>= 24 k-tiles), so the adma = 1 member of the group is the K = 1536 request whose first 256 columns are the K = 256 operands
    and whose further activation columns are zero: the same sums plus exact zeros.
  * ln_linear / ln_geglu: the folded form is one instantiation per ring with the builtin DMA (the route sets adma = 0), so there is no adma pair;
    the rings of one tile must agree.

Split-K and tile-order cases must also equal the same request at split-K 1 / order 0 and themselves on a second run.  Each case first asks the route,
under its force string, that the plan is the one its id names.  Every shape has M <= 720 but one phase shape (M = 1800: eight row tiles per phase)."""
import pytest
import torch

import igemm_forms as forms
from test_ops_gpu import _cmp

pytestmark = pytest.mark.gpu
GUARD = 256
M_ROWS = forms.M0


@pytest.fixture(scope="module")
def operands(cuda):
    """operands and fp64 reference per (kind, shape key, variant), built on the CPU once and moved to the device; never modified afterwards"""
    cache = {}

    def get(kind, key, variant=""):
        k = (kind, key, variant)
        if k not in cache:
            if forms.KINDS[kind].exact:
                t = forms.build_exact(kind, key, variant)
            else:
                t = forms.build_tolerance(kind, key, zero_extend_from="short" if variant == "zext" else None)
            # (operands on the device; the reference: its shape, as bf16 on the device for the exact kinds, as fp32 on the device for _cmp)
            ref = t.pop("ref")
            dev = {n: v.to(cuda) for n, v in t.items()}
            cache[k] = (dev, tuple(ref.shape), ref.to(torch.bfloat16).to(cuda) if forms.KINDS[kind].exact else None, ref.float().to(cuda))
        return cache[k]
    return get


def _run_guarded(kind, t, ref_shape, cuda):
    """the op into rows [GUARD, GUARD + M) of a NaN buffer; the guard rows must stay NaN"""
    No = ref_shape[-1]
    M = 1
    for d in ref_shape[:-1]:
        M *= d
    buf = torch.full((GUARD + M + GUARD, No), float("nan"), dtype=torch.bfloat16, device=cuda)
    out = buf[GUARD:GUARD + M].view(ref_shape)
    forms.run_op(kind, t, out=out)
    torch.cuda.synchronize()
    assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[GUARD + M:]).all(), "rows outside the result were written"
    return out


def _assert_equal(name, out, want):
    """bit equality with a message that shows where: count, first (m, n), row and column range of the mismatches"""
    a, b = out.reshape(-1, out.shape[-1]), want.reshape(-1, want.shape[-1])
    assert a.shape == b.shape, (name, a.shape, b.shape)
    if torch.equal(a.view(torch.int16), b.view(torch.int16)):
        return
    bad = (a.view(torch.int16) != b.view(torch.int16)).nonzero()
    m, n = bad[0].tolist()
    rows, cols = bad[:, 0], bad[:, 1]
    raise AssertionError(f"{name}: {bad.shape[0]} of {a.numel()} elements differ; first at (m={m}, n={n}): got {a[m, n].item()} want {b[m, n].item()}; "
                         f"rows {rows.min().item()} .. {rows.max().item()}, columns {cols.min().item()} .. {cols.max().item()}")


def _check_route(case, monkeypatch, force=None):
    monkeypatch.setenv("NR_IGEMM_FORCE", case.force if force is None else force)
    plan = forms.route_of(case.kind, forms.shape_of(case.kind, case.shape_key))
    if force is None:
        assert plan == case.plan, f"{case.id}: the route answers {plan}"
    return plan


def _run_case(case, operands, monkeypatch, cuda):
    t, shape, want, ref = operands(case.kind, case.shape_key, case.variant)
    _check_route(case, monkeypatch)
    out = _run_guarded(case.kind, t, shape, cuda)
    if want is not None:
        _assert_equal(case.id, out, want)
    else:
        _cmp(case.id, out, ref)
    return out, t, shape


@pytest.mark.parametrize("case", forms.INSTANTIATION_CASES, ids=lambda c: c.id)
def test_instantiation(operands, monkeypatch, cuda, case):
    _run_case(case, operands, monkeypatch, cuda)


def _against_base(case, operands, monkeypatch, cuda):
    out, t, shape = _run_case(case, operands, monkeypatch, cuda)
    again = _run_guarded(case.kind, t, shape, cuda)
    _assert_equal(case.id + " (second run)", again, out)
    base = _check_route(case, monkeypatch, forms.base_force(case))
    assert base._replace(adma=0) == case.plan._replace(splitk=1, m_fast=0, adma=0), (case.id, base)
    first = _run_guarded(case.kind, t, shape, cuda)
    _assert_equal(case.id + " (against split-K 1, order 0)", out, first)


@pytest.mark.parametrize("case", forms.SPLITK_CASES, ids=lambda c: c.id)
def test_split_k(operands, monkeypatch, cuda, case):
    assert case.plan.splitk > 1
    _against_base(case, operands, monkeypatch, cuda)


@pytest.mark.parametrize("case", forms.ORDER_CASES, ids=lambda c: c.id)
def test_tile_order(operands, monkeypatch, cuda, case):
    _against_base(case, operands, monkeypatch, cuda)


# (kind, bm, bn, waves): 256 x 128 runs the direct epilogue at ring depth 2 and the staged one at 3; 128 x 64 and 64 x 64 the staged one at every depth
RING_GROUPS = [("geglu", 256, 128, 8), ("geglu", 64, 64, 4), ("ln_linear", 128, 64, 8), ("ln_linear", 64, 160, 4), ("ln_geglu", 128, 64, 4), ("ln_geglu", 128, 160, 41)]


@pytest.mark.parametrize("kind,bm,bn,waves", RING_GROUPS)
def test_ring_depth_and_load_path_do_not_change_a_bit(operands, monkeypatch, cuda, kind, bm, bn, waves):
    members = [c for c in forms.INSTANTIATION_CASES if c.kind == kind and (c.plan.bm, c.plan.bn, c.plan.waves) == (bm, bn, waves)]
    assert len(members) >= 2 and len({c.plan.stages for c in members}) >= 2, members
    assert {c.plan.adma for c in members} == ({0, 1} if kind == "geglu" else {0})
    outs = []
    for c in members:
        # a long-K (adma = 1) member runs the short-K operands extended with zero activation columns
        variant = "zext" if c.shape_key == "long" else ""
        t, shape, _, ref = operands(c.kind, c.shape_key, variant)
        _check_route(c, monkeypatch)
        outs.append((c.id, _run_guarded(c.kind, t, shape, cuda)))
        _cmp(c.id, outs[-1][1], ref)
    for cid, o in outs[1:]:
        _assert_equal(f"{cid} against {outs[0][0]}", o, outs[0][1])


def test_out_argument_of_the_wrappers(operands, monkeypatch, cuda):
    """out= is the caller's tensor, checked like the attention wrappers' (contiguous bf16, exact shape); without it the result is the same"""
    from neurons_amd import ops
    monkeypatch.delenv("NR_IGEMM_FORCE", raising=False)
    for kind in ("linear", "linear_2src", "conv3x3", "conv3x3_tap_inner", "ups_phase", "ln_linear"):
        t, shape, want, _ = operands(kind, "short")
        out = torch.empty(shape, dtype=torch.bfloat16, device=cuda)
        assert forms.run_op(kind, t, out=out) is out
        fresh = forms.run_op(kind, t)
        assert tuple(fresh.shape) == shape
        _assert_equal(f"{kind}: out= against a fresh result", out, fresh)
        if want is not None:
            _assert_equal(kind, fresh, want)
        with pytest.raises(ValueError):
            forms.run_op(kind, t, out=torch.empty(shape[:-1] + (shape[-1] + 8,), dtype=torch.bfloat16, device=cuda))
        with pytest.raises(AssertionError):
            forms.run_op(kind, t, out=torch.empty(shape, dtype=torch.float32, device=cuda))
        with pytest.raises(AssertionError):
            forms.run_op(kind, t, out=torch.empty(shape[:-1] + (2 * shape[-1],), dtype=torch.bfloat16, device=cuda)[..., ::2])
    t, _, _, _ = operands("linear", "short")
    with pytest.raises(ValueError):
        ops.gemm(t["a0"], t["w"], out=torch.empty(M_ROWS + 1, forms.N0, dtype=torch.bfloat16, device=cuda))
