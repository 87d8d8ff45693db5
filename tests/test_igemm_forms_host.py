"""The case lists of tests/igemm_forms.py, host side (route queries through ctypes on the built library and CPU arithmetic; no GPU): the forced plans
of INSTANTIATION_CASES reach every instantiation of igemm_bf16_kernel but the two LayerNorm-folded 64 x 32 kernels the route never names
(tests/test_igemm_table_host.py: LN_UNROUTED); every case of the three lists is a launch of the tiled class; and the integer operands of the exact
kinds stay in the regime where tests/test_igemm_forms_gpu.py may ask for bit equality.

Instantiations only reachable through a GEGLU request: none.  (GEGLU is a run-time flag of the LIN kernels; the `geglu` cases run its epilogue on
the tiles a GEGLU projection can be forced to -- bn 64 / 128 and the row-wave tile -- which the `linear` cases reach as well.)"""
import pytest
import torch

import igemm_forms as forms
from test_igemm_table_host import LN_UNROUTED, TABLE


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ("NR_SMALLM", "NR_IGEMM_FORCE", "NR_DETERMINISTIC_BATCH", "NR_G8P", "NR_W8", "NR_IGEMM_FORCE_MAXM", "NR_IGEMM_FORCE_MINM", "NR_IGEMM_FORCE_KS",
              "NR_IGEMM_FORCE_N", "NR_IGEMM_FORCE_K"):
        monkeypatch.delenv(k, raising=False)


def _table_kernels():
    """(form, row, ring, adma, lin) of all 160 instantiations (gemm.hip: launch_inst)"""
    out = set()
    for row, (rings, ln_rings, phase) in TABLE.items():
        for ns in rings:
            out |= {("plain", row, ns, adma, lin) for adma in (0, 1) for lin in ((0, 1) if ns <= 4 else (0,))}
        out |= {("ln", row, ns, 0, 1) for ns in ln_rings}
        if phase:
            out |= {("phase", row, 2, adma, 0) for adma in (0, 1)}
    return out


def test_the_instantiation_cases_reach_every_kernel_but_the_two_unrouted_ones():
    table = _table_kernels()
    assert len(table) == 160
    reached = {forms.inst_key(c.plan) for c in forms.INSTANTIATION_CASES}
    unrouted = {("ln", row, ns, 0, 1) for row, ns in LN_UNROUTED}
    print(f"{len(reached)} of {len(table)} kernels reached; not reached: {sorted(table - reached)}")
    assert reached <= table, sorted(reached - table)
    assert table - reached == unrouted, (sorted(table - reached - unrouted), sorted(unrouted - (table - reached)))
    assert len(reached) == 158
    # what each kind is there for
    by_kind = {}
    for c in forms.INSTANTIATION_CASES:
        by_kind.setdefault(c.kind, set()).add(forms.inst_key(c.plan))
    assert by_kind["linear"] == {k for k in table if k[0] == "plain" and k[4] == 1}
    assert by_kind["conv3x3"] == {k for k in table if k[0] == "plain" and k[4] == 0}
    assert by_kind["ups_phase"] == {k for k in table if k[0] == "phase"}
    assert by_kind["ln_linear"] | by_kind["ln_geglu"] == {k for k in table if k[0] == "ln"} - unrouted
    assert by_kind["geglu"] <= by_kind["linear"] | by_kind["conv3x3"], "an instantiation only GEGLU reaches: name it in the module text"
    shallow = {(row, min(rings), adma) for row, (rings, _, _) in TABLE.items() for adma in (0, 1)}
    for kind in ("linear_2src", "conv3x3_2src", "conv3x3_s2", "conv3x3_ups", "conv3x3_tap_inner"):
        got = {(k[1], k[2], k[3]) for k in by_kind[kind]}
        assert shallow <= got and all(k[4] == 0 for k in by_kind[kind]), kind
    assert {c.kind for c in forms.INSTANTIATION_CASES if c.variant == "bigres"} == set(forms.RES_KINDS)


def test_every_case_is_a_launch_of_the_tiled_class_and_names_its_plan():
    for cases in (forms.INSTANTIATION_CASES, forms.SPLITK_CASES, forms.ORDER_CASES):
        assert len({c.id for c in cases}) == len(cases)
        for c in cases:
            assert c.plan.status == 0 and c.plan.cls == "tiled", c
            assert forms.route_of(c.kind, forms.shape_of(c.kind, c.shape_key), c.force) == c.plan, c.id
            assert c.id.startswith(f"{c.kind}-{c.plan.bm}x{c.plan.bn}-w{c.plan.waves}-r{c.plan.stages}-adma{c.plan.adma}-sk{c.plan.splitk}-ord{c.plan.m_fast}"), c.id


def test_the_grids_exercise_the_block_id_remap_at_every_remainder():
    """nr_xcd_bid spreads the block ids over the 8 XCDs: the grids of the cases leave every remainder mod 8"""
    rem = set()
    for cases in (forms.INSTANTIATION_CASES, forms.SPLITK_CASES, forms.ORDER_CASES):
        for c in cases:
            M, N, _ = forms.gemm_mnk(c.kind, forms.shape_of(c.kind, c.shape_key))
            ntm = 4 * -(-(M // 4) // c.plan.bm) if c.plan.form == "phase" else -(-M // c.plan.bm)
            rem.add(ntm * -(-N // c.plan.bn) * c.plan.splitk % 8)
    assert rem == set(range(8)), rem


def test_the_split_k_cases_are_the_depths_they_are_there_for():
    by = {}
    for c in forms.SPLITK_CASES:
        assert (c.plan.bm, c.plan.bn) in {t[:2] for t in forms.SPLITK_TILES} and c.plan.m_fast == 0, c.id
        nk = forms.gemm_mnk(c.kind, forms.shape_of(c.kind, c.shape_key))[2] // 64
        by.setdefault((c.kind, c.shape_key, c.plan.bm, c.plan.bn), []).append((c.plan.splitk, nk))
    for key, depths in by.items():
        sks, nk = sorted(set(d[0] for d in depths)), depths[0][1]
        if key[1] == "k3136":
            assert sks == [2] and nk == 49, key
            continue
        assert 2 in sks and nk in sks and any(1 < s < nk and nk % s for s in sks), (key, sks, nk)
    assert all(c.plan.adma == 1 for c in forms.SPLITK_CASES if c.shape_key == "k3136")
    assert any(c.kind == "ups_phase" and c.shape_key == "short" and c.plan.splitk == 3 for c in forms.SPLITK_CASES)      # slices of 1, 1 and 2 k-tiles


def test_the_order_cases_have_a_short_last_band_and_the_phase_fallback():
    for c in forms.ORDER_CASES:
        M = forms.gemm_mnk(c.kind, forms.shape_of(c.kind, c.shape_key))[0]
        if c.kind != "ups_phase":
            ntm = -(-M // c.plan.bm)
            assert M == 720 and ntm % 8 != 0 and c.plan.splitk == 1, c.id
    assert sorted(c.plan.m_fast for c in forms.ORDER_CASES if c.kind != "ups_phase") == sorted([0, 1, 8] * 6)
    phase = {c.shape_key: c.plan for c in forms.ORDER_CASES if c.kind == "ups_phase"}
    assert phase["p450"].m_fast == 8 and (450 + phase["p450"].bm - 1) // phase["p450"].bm == 8
    assert phase["short"].m_fast in (0, 1), "3 row tiles per phase: the route answers a plain order"


@pytest.mark.parametrize("kind", forms.EXACT_KINDS)
def test_integer_operands_keep_the_reference_exact_in_bf16(kind):
    """the two conditions of the exact regime, from the reference alone: >= 99 % of the elements within 256 (there bf16 holds every integer, so an
    error of one is visible) and every element below 2^24 (every partial sum is an integer fp32 holds)"""
    keys = ["short", "long"] + [k for (kd, k) in forms.EXTRA_SHAPES if kd == kind]
    for key in keys:
        t = forms.build_exact(kind, key)
        ref = t["ref"]
        assert ref.dtype == torch.float64 and torch.equal(ref, ref.round())
        within = (ref.abs() <= 256).double().mean().item()
        print(f"{kind} {key}: max |ref| {ref.abs().max().item():.0f}, {100 * within:.3f} % within 256")
        assert within >= 0.99 and ref.abs().max().item() < 2 ** 24, (kind, key)
        # |activation| <= 2, |weight| <= 4 (a phase weight sums up to four taps): the sum of absolute terms bounds every partial sum in any order
        K = forms.gemm_mnk(kind, forms.shape_of(kind, key))[2]
        assert 2 * 4 * K + 8 + 8 + 2000 < 2 ** 24
        for name in ("a0", "a1", "w", "res"):
            if name in t:
                assert t[name].dtype == torch.bfloat16 and torch.equal(t[name].double(), t[name].double().round())
    if kind in forms.RES_KINDS:
        t = forms.build_exact(kind, "short", "bigres")
        ref = t["ref"]
        assert torch.equal(ref, ref.round()) and ref.abs().max().item() < 2 ** 24
        got = ref.to(torch.bfloat16).double()
        assert (ref.abs() > 1024).double().mean().item() > 0.3 and not torch.equal(got, ref), "the big residual makes the single rounding visible"


def test_torch_rounds_fp64_to_bf16_to_nearest_even():
    x = torch.tensor([257.0, 259.0, 258.0, -257.0, 1028.0, 1036.0, 2056.0, 2072.0], dtype=torch.float64)
    assert x.to(torch.bfloat16).tolist() == [256.0, 260.0, 258.0, -256.0, 1024.0, 1040.0, 2048.0, 2080.0]
