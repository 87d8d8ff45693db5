"""The route of the K-pair kernel of the tiled igemm (gemm.hip: TiledPlan::waves == 82, splitk = slabs written), asked of the built library: host
code, no GPU.  NR_IGEMM_KPAIR is read once per process, so the two arms of the rule are asked in one child process each."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

import igemm_forms as forms
from igemm_forms import Shape

HERE = os.path.dirname(os.path.abspath(__file__))

# the launches of the headline workload (32 frames, 64 x 64 latents) that the parent's choose_plan gives the 128 x 160 tile with an even split-K:
# (kind, shape, K slices, admitted by the K-pair rule)
HEADLINE = [
    ("conv3x3_tap_inner", Shape(32, 16, 16, 640, 0, 640), 2, True),       # 16x16 level: M = 8192, N = 640, K = 5760
    ("conv3x3_2src", Shape(32, 16, 16, 640, 640, 640), 2, True),          #   K = 11520 (skip concat)
    ("conv3x3_2src", Shape(32, 16, 16, 1280, 640, 640), 2, True),         #   K = 17280
    ("conv3x3_tap_inner", Shape(32, 8, 8, 1280, 0, 1280), 4, True),       # 8x8 level: M = 2048, N = 1280, K = 11520
    ("conv3x3_2src", Shape(32, 8, 8, 1280, 1280, 1280), 4, True),         #   K = 23040
    ("conv3x3_s2", Shape(32, 16, 16, 1280, 0, 1280), 4, True),            #   the downsample conv into the 8x8 level
    ("linear", Shape(2048, 1, 1, 6400, 0, 1280), 4, True),                #   the folded FeedForward.net.2 | proj_out Linear
    ("conv3x3_2src", Shape(32, 4, 4, 1280, 1280, 1280), 16, True),        # 4x4 level: M = 512, K = 23040
    ("conv3x3_tap_inner", Shape(32, 4, 4, 1280, 0, 1280), 8, False),      #   K = 11520: four pairs a tile would leave half the CUs idle (measured slower)
    ("conv3x3_ups", Shape(32, 4, 4, 1280, 0, 1280), 4, False),            # the replicated upsample gather: no form of the K-pair kernel
]
# the one-slice Linear the rule admits on its own measurement: M = 8192, N = 640, K = 3200
LONG_K_LINEAR = ("linear", Shape(8192, 1, 1, 3200, 0, 640))

_CHILD = """
import json, sys
sys.path.insert(0, %r)
import ctypes as C
import igemm_forms as forms
from igemm_forms import Shape
out = []
for kind, shape in json.loads(sys.argv[1]):
    s = Shape(*shape)
    lib = forms._route_lib()
    p, r = forms.params_of(kind, s), forms.NrGemmRoute()
    status = lib.nr_gemm_route(C.byref(p), C.byref(r))
    out.append([status, r.cls, r.m_fast, r.ws_bytes, r.weight_layout] + list(r.tiled))
print(json.dumps(out))
"""


def _routes(queries, **env):
    """[status, cls, m_fast, ws_bytes, weight_layout, bm, bn, splitk, stages, waves, adma, lin] per (kind, shape), from a child process under `env`"""
    e = dict(os.environ)
    for k in ("NR_IGEMM_FORCE", "NR_IGEMM_KPAIR", "NR_G8P"):
        e.pop(k, None)
    e.update(env)
    r = subprocess.run([sys.executable, "-c", _CHILD % HERE, json.dumps([(k, list(s)) for k, s in queries])], capture_output=True, text=True, env=e,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def arms():
    q = [(k, s) for k, s, _, _ in HEADLINE] + [LONG_K_LINEAR]
    return _routes(q), _routes(q, NR_IGEMM_KPAIR="0")


def test_the_admitted_headline_shapes_run_as_k_pairs_with_half_the_slabs(arms):
    on, off = arms
    for (kind, s, slices, admitted), a, b in zip(HEADLINE, on, off):
        M, N, _ = forms.gemm_mnk(kind, s)
        # the parent's plan: the two-stage 128 x 160 tile on 4 waves, `slices` K slices, one fp32 slab each
        assert b[0] == 0 and b[1] == forms.NR_GEMM_TILED and b[5:10] == [128, 160, slices, 2, 4], (kind, s, b)
        assert b[3] == slices * M * N * 4
        if not admitted:
            assert a == b, (kind, s, a, b)
            continue
        assert a[0] == 0 and a[1] == forms.NR_GEMM_TILED and a[5:10] == [128, 160, slices // 2, 2, 82], (kind, s, a)
        assert a[3] == (b[3] // 2 if slices > 2 else 0), (kind, s, a, b)
        assert a[2] == b[2] and a[4] == b[4] and a[10] == 1 and a[11] == b[11], "tile order, weight layout and the Linear form are the parent's"
    a, b = on[-1], off[-1]
    assert b[0] == 0 and b[1] == forms.NR_GEMM_TILED and b[7] == 1 and b[3] == 0 and b[9] != 82, b
    assert a[0] == 0 and a[1] == forms.NR_GEMM_TILED and a[5:12] == [128, 160, 1, 2, 82, 1, 1] and a[3] == 0, a


def test_switched_off_the_route_is_the_parents(arms):
    _, off = arms
    assert all(r[9] != 82 for r in off)
    # shapes the rule does not touch answer the same in both arms
    other = [("linear", Shape(8192, 1, 1, 640, 0, 640)), ("conv3x3", Shape(32, 32, 32, 320, 0, 320)), ("geglu", Shape(2048, 1, 1, 1280, 0, 10240)),
             ("ups_phase", Shape(32, 8, 8, 1280, 0, 1280)), ("ln_linear", Shape(2048, 1, 1, 1280, 0, 3840)),
             # one-slice long-K Linears other than the measured M = 8192, N = 640, K = 3200: also 256 tiles of 128 x 160, not admitted
             ("linear", Shape(4096, 1, 1, 3200, 0, 1280)), ("linear", Shape(8192, 1, 1, 4096, 0, 640)), ("linear", Shape(8192, 1, 1, 3136, 0, 640))]
    assert _routes(other) == _routes(other, NR_IGEMM_KPAIR="0")


@pytest.mark.parametrize("force", ["128,160,2,2,0,4", "128,160,-1,-1,-1,-1", "-1,-1,-1,-1,1,-1", "128,160,4,2,-1,41", "128,64,2,2,0,8", "-1,-1,2", "64,64"])
def test_a_force_string_that_does_not_name_82_never_gives_a_k_pair(force):
    for kind, s, _, _ in HEADLINE:
        plan = forms.route_of(kind, s, force)
        assert plan.status == 0 and plan.waves != 82, (kind, s, force, plan)


def test_a_forced_k_pair_is_the_slab_count_it_names():
    kind, s, _, _ = HEADLINE[3]      # nk = 180
    for slabs in (1, 2, 3, 8):
        plan = forms.route_of(kind, s, f"128,160,{slabs},2,0,82")
        assert (plan.status, plan.bm, plan.bn, plan.waves, plan.stages, plan.splitk, plan.adma) == (0, 128, 160, 82, 2, slabs, 1), plan
    # more slabs than pairs of k-tiles: one k-tile per group at the most
    plan = forms.route_of("linear", Shape(300, 1, 1, 320, 0, 320), "128,160,7,2,0,82")
    assert (plan.waves, plan.splitk) == (82, 2), plan
    # one k-tile cannot be split
    plan = forms.route_of("linear", Shape(300, 1, 1, 64, 0, 320), "128,160,1,2,0,82")
    assert plan.status == 0 and plan.waves == 4 and plan.splitk == 1, plan
    # another tile named with 82: the tile's own wave grid
    plan = forms.route_of(kind, s, "128,64,2,2,0,82")
    assert plan.status == 0 and (plan.bm, plan.bn) == (128, 64) and plan.waves in (4, 8), plan


@pytest.mark.parametrize("kind", ["ln_linear", "ln_geglu", "geglu", "ups_phase"])
def test_a_k_pair_request_for_a_form_the_kernel_lacks_is_an_existing_instantiation(kind):
    from test_igemm_table_host import TABLE
    for key in ("short", "long"):
        if getattr(forms.KINDS[kind], key) is None:
            continue
        plan = forms.route_of(kind, forms.shape_of(kind, key), "128,160,1,2,0,82")
        assert plan.status == 0 and plan.cls == "tiled" and plan.waves != 82, plan
        forms.table_row(plan)      # a row of the table of instantiations
        assert plan.stages in TABLE[forms.table_row(plan)][0] or kind.startswith("ln") or kind == "ups_phase", plan
        base = forms.route_of(kind, forms.shape_of(kind, key), "128,160,1,2,0,4")
        assert plan == base, "what the same request gets when it names the 2 x 2 grid"


def test_a_raw_fp32_result_is_never_a_k_pair():
    lib = forms._route_lib()
    for kind, s, _, _ in HEADLINE[:2]:
        p, r = forms.params_of(kind, s), forms.NrGemmRoute()
        p.out_f32 = 256
        os.environ["NR_IGEMM_FORCE"] = "128,160,1,2,0,82"
        try:
            status = lib.nr_gemm_route(C.byref(p), C.byref(r))
        finally:
            os.environ.pop("NR_IGEMM_FORCE", None)
        assert status == 0 and list(r.tiled)[4] == 4 and list(r.tiled)[2] == 1 and r.ws_bytes == 0, list(r.tiled)
