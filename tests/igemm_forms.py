"""The request kinds, the forced plans and the operands of tests/test_igemm_forms_host.py / _gpu.py (a helper module: no test functions), and the ONE
ctypes mirror of NrGemmParams / NrGemmRoute that the host tests share.

route_of() fills NrGemmParams the way the op hook of a request kind does (engine_ops.hip) and asks nr_gemm_route under an NR_IGEMM_FORCE string: host
code, no GPU.  The three case lists are built from its answers when first asked for (the built library must exist) and never written by hand,
so a case's name is the plan the route reports for its force string:

  INSTANTIATION_CASES  one case per (form, table row, ring depth, adma, lin) of igemm_bf16_kernel that a forced plan reaches: `conv3x3` on the plain
                       kernels, `linear` on the LIN ones, `ups_phase` on the phase form, `ln_linear` / `ln_geglu` on the LayerNorm-folded rings, `geglu`
                       (the GEGLU epilogue of the LIN kernels on the tiles it can be forced to); the other conv / two-source kinds on every table row
                       at the row's shallowest ring with adma 0 and 1; and per kind with a residual two cases whose residual is in +-2000 (the
                       staged and the direct epilogue).
  SPLITK_CASES         split-K 2, a depth that does not divide the k-tiles, and one k-tile per slice, on four tiles; the +-2000 residual once per kind.
  ORDER_CASES          tile orders 0 / 1 / 8 where the grouped order has a short last band; the phase form under order 8.

Operands: the exact kinds get small integers (activations in -2 .. 2, weights in -1 .. 1, bias / row vector / residual in -8 .. 8), so every partial
sum is an integer below 2^24, exact in fp32 in any order, and the kernel's single rounding must give bf16(reference) bit for bit.  GEGLU and the
LayerNorm-folded form (erf, row statistics) get Gaussian operands and the tolerance of tests/test_ops_gpu.py."""
import ctypes as C
import os
from collections import namedtuple

import torch
import torch.nn.functional as F

from neurons_amd import _lib

NR_GEMM_TILED = 4      # NrGemmClass of neurons_amd/csrc/gemm_route.h
GEMM_CLASS_NAMES = ("smallm", "lin160", "rowpanel", "gemm8p", "tiled")


class NrGemmParams(C.Structure):      # neurons_amd/csrc/common.h
    _fields_ = [("a0", C.c_void_p), ("a1", C.c_void_p), ("c0", C.c_int), ("c1", C.c_int), ("lda0", C.c_int), ("lda1", C.c_int), ("H", C.c_int),
                ("W", C.c_int), ("OH", C.c_int), ("OW", C.c_int), ("ksize", C.c_int), ("stride", C.c_int), ("ups", C.c_int), ("w", C.c_void_p),
                ("M", C.c_int), ("N", C.c_int), ("K", C.c_int), ("bias", C.c_void_p), ("rowvec", C.c_void_p), ("rowvec_div", C.c_int),
                ("rowvec_mod", C.c_int), ("rowvec_ld", C.c_int), ("res", C.c_void_p), ("ldr", C.c_int), ("out", C.c_void_p), ("ldo", C.c_int),
                ("out_scale", C.c_float), ("geglu", C.c_int), ("ln_c", C.c_void_p), ("ln_eps", C.c_float), ("act", C.c_int), ("pad_tl0", C.c_int),
                ("w8", C.c_int), ("out_f32", C.c_void_p), ("plan_m", C.c_int), ("tap_inner", C.c_int), ("w_fm", C.c_void_p)]


class NrGemmRoute(C.Structure):       # neurons_amd/csrc/gemm_route.h
    _fields_ = [("cls", C.c_int), ("weight_layout", C.c_int), ("m_fast", C.c_int), ("ws_bytes", C.c_size_t), ("tiled", C.c_int * 7),
                ("smallm", C.c_int * 4), ("lin160", C.c_int * 4), ("rowpanel", C.c_int * 1), ("g8p", C.c_int * 2)]


# ------------------------------------------------------------------------------------------------------------------------------------------------
# request kinds
# ------------------------------------------------------------------------------------------------------------------------------------------------
# nimg images of H x W source pixels (a Linear: nimg = M, H = W = 1), c0 (+ c1) input channels, N output columns of the GEMM (GEGLU: value | gate)
Shape = namedtuple("Shape", "nimg H W c0 c1 N")
# form: which family of instantiations serves the kind; exact: integer operands, compared bit for bit
Kind = namedtuple("Kind", "form exact ksize stride ups two_src tap_inner geglu ln bias rowvec res short long")
M0, N0 = 300, 352
KINDS = {
    "linear":            Kind("plain", True, 1, 1, 0, False, False, False, False, True, False, True, Shape(M0, 1, 1, 256, 0, N0), Shape(M0, 1, 1, 1536, 0, N0)),
    "linear_2src":       Kind("plain", True, 1, 1, 0, True, False, False, False, True, False, True, Shape(M0, 1, 1, 128, 128, N0), Shape(M0, 1, 1, 1024, 512, N0)),
    "conv3x3":           Kind("plain", True, 3, 1, 0, False, False, False, False, True, True, True, Shape(5, 6, 10, 64, 0, N0), Shape(5, 6, 10, 192, 0, N0)),
    "conv3x3_2src":      Kind("plain", True, 3, 1, 0, True, False, False, False, True, False, False, Shape(5, 6, 10, 64, 64, N0), Shape(5, 6, 10, 128, 64, N0)),
    "conv3x3_s2":        Kind("plain", True, 3, 2, 0, False, False, False, False, True, False, False, Shape(15, 7, 9, 64, 0, N0), Shape(15, 7, 9, 192, 0, N0)),
    "conv3x3_ups":       Kind("plain", True, 3, 1, 1, False, False, False, False, True, False, False, Shape(5, 3, 5, 64, 0, N0), Shape(5, 3, 5, 192, 0, N0)),
    "conv3x3_tap_inner": Kind("plain", True, 3, 1, 0, False, True, False, False, True, True, True, Shape(5, 6, 10, 64, 0, N0), Shape(5, 6, 10, 192, 0, N0)),
    "ups_phase":         Kind("phase", True, 3, 1, 2, False, False, False, False, True, False, False, Shape(3, 5, 10, 64, 0, N0), Shape(3, 5, 10, 384, 0, N0)),
    "geglu":             Kind("plain", False, 1, 1, 0, False, False, True, False, True, False, False, Shape(M0, 1, 1, 256, 0, 640), Shape(M0, 1, 1, 1536, 0, 640)),
    "ln_linear":         Kind("ln", False, 1, 1, 0, False, False, False, True, True, False, True, Shape(M0, 1, 1, 256, 0, N0), None),
    "ln_geglu":          Kind("ln", False, 1, 1, 0, False, False, True, True, True, False, False, Shape(M0, 1, 1, 256, 0, 640), None),
}
EXACT_KINDS = tuple(k for k, v in KINDS.items() if v.exact)
RES_KINDS = tuple(k for k, v in KINDS.items() if v.exact and v.res)
# further shapes of the split-K and tile-order cases
EXTRA_SHAPES = {
    ("linear", "k3136"): Shape(M0, 1, 1, 3136, 0, N0),          # 49 k-tiles: two slices of 24 and 25, both on the ADMA path
    ("linear", "m720"): Shape(720, 1, 1, 256, 0, N0),            # 12 / 6 row tiles of 64 / 128 rows: a short last band under the grouped order
    ("conv3x3", "m720"): Shape(12, 6, 10, 64, 0, N0),
    # 450 source pixels per phase = 8 row tiles of 64 (the last with 2 rows): the only phase shape here above M = 720, the grouped order needs 8 row tiles a phase
    ("ups_phase", "p450"): Shape(5, 9, 10, 64, 0, N0),
}


def shape_of(kind, key):
    if key in ("short", "long"):
        s = getattr(KINDS[kind], key)
        assert s is not None, (kind, key)
        return s
    return EXTRA_SHAPES[(kind, key)]


def out_hw(kind, s):
    k = KINDS[kind]
    OH, OW = (2 * s.H, 2 * s.W) if k.ups else (s.H, s.W)
    if k.stride == 2:
        OH, OW = (OH - 1) // 2 + 1, (OW - 1) // 2 + 1
    return OH, OW


def gemm_mnk(kind, s):
    k = KINDS[kind]
    OH, OW = out_hw(kind, s)
    return s.nimg * OH * OW, s.N, (4 if k.ups == 2 else k.ksize * k.ksize) * (s.c0 + s.c1)


_PTR = 256      # any non-null pointer: the route never dereferences


def params_of(kind, s):
    """NrGemmParams as nr_gemm_params and the kind's op hook fill them"""
    k = KINDS[kind]
    p = NrGemmParams()
    p.a0, p.c0, p.lda0, p.w, p.out = _PTR, s.c0, s.c0, _PTR, _PTR
    if k.two_src:
        p.a1, p.c1, p.lda1 = _PTR, s.c1, s.c1
    p.H, p.W = s.H, s.W
    p.OH, p.OW = out_hw(kind, s)
    p.ksize, p.stride, p.ups = k.ksize, k.stride, k.ups
    p.M, p.N, p.K = gemm_mnk(kind, s)
    No = p.N // 2 if k.geglu else p.N
    p.rowvec_div, p.ldo, p.out_scale = 1, No, 1.0
    if k.bias:
        p.bias = _PTR
    if k.res:
        p.res = _PTR
    if k.form != "phase":
        p.ldr = No                                  # the hooks pass the row strides whether or not there is a residual / row vector
    if k.ksize == 3 and k.form != "phase":
        p.rowvec_ld = p.N
    if k.rowvec:
        p.rowvec, p.rowvec_div = _PTR, p.OH * p.OW
    p.geglu, p.tap_inner = int(k.geglu), int(k.tap_inner)
    if k.ln:
        p.ln_c, p.ln_eps = _PTR, 1e-5
    return p


# what a route query answers: status of nr_gemm_route, class name, the tiled plan, the tile order and the form of the instantiation
Plan = namedtuple("Plan", "status cls bm bn stages waves splitk adma lin m_fast form")
_UNSET = object()
_lib_handle = None


def _route_lib():
    global _lib_handle
    if _lib_handle is None:
        _lib_handle = _lib.load()
        _lib_handle.nr_gemm_route.restype = C.c_int
        _lib_handle.nr_gemm_route.argtypes = [C.POINTER(NrGemmParams), C.POINTER(NrGemmRoute)]
    return _lib_handle


def route_of(kind, shape, force=_UNSET):
    """The route of a request of this kind and shape under NR_IGEMM_FORCE = force (None: unset; left out: the environment as it is)"""
    lib = _route_lib()
    saved = os.environ.get("NR_IGEMM_FORCE")
    if force is not _UNSET:
        if force is None:
            os.environ.pop("NR_IGEMM_FORCE", None)
        else:
            os.environ["NR_IGEMM_FORCE"] = force
    try:
        p, r = params_of(kind, shape), NrGemmRoute()
        status = lib.nr_gemm_route(C.byref(p), C.byref(r))
    finally:
        if force is not _UNSET:
            if saved is None:
                os.environ.pop("NR_IGEMM_FORCE", None)
            else:
                os.environ["NR_IGEMM_FORCE"] = saved
    bm, bn, splitk, stages, waves, adma, lin = list(r.tiled)
    return Plan(status, GEMM_CLASS_NAMES[r.cls], bm, bn, stages, waves, splitk, adma, lin, r.m_fast, KINDS[kind].form)


# ------------------------------------------------------------------------------------------------------------------------------------------------
# case lists
# ------------------------------------------------------------------------------------------------------------------------------------------------
# variant "bigres": the residual is in +-2000 (output steps of 8 and 16: round-to-nearest-even and ties)
Case = namedtuple("Case", "id kind shape_key variant force plan")


def table_row(plan):
    """(bm, bn, wgm, wgn) of tests/test_igemm_table_host.py::TABLE that a plan's tile and wave count name"""
    from test_igemm_table_host import TABLE
    rows = [r for r in TABLE if r[:2] == (plan.bm, plan.bn) and (41 if r[3] == 1 else r[2] * r[3]) == plan.waves]
    assert len(rows) == 1, plan
    return rows[0]


def inst_key(plan):
    return (plan.form, table_row(plan), plan.stages, plan.adma, plan.lin)


def _force(bm, bn, splitk=-1, stages=-1, order=-1, waves=-1):
    return f"{bm},{bn},{splitk},{stages},{order},{waves}"


def _case_id(kind, plan):
    return f"{kind}-{plan.bm}x{plan.bn}-w{plan.waves}-r{plan.stages}-adma{plan.adma}-sk{plan.splitk}-ord{plan.m_fast}"


def _finish(cases):
    """unique ids: cases whose plans agree differ in the shape (or the variant)"""
    seen, out = {}, []
    for c in cases:
        seen.setdefault(c.id, []).append(c)
    for c in cases:
        cid = c.id
        if len(seen[cid]) > 1:
            cid += f"-{c.shape_key}"
        if c.variant:
            cid += f"-{c.variant}"
        out.append(c._replace(id=cid))
    assert len({c.id for c in out}) == len(out), sorted(c.id for c in out)
    return out


def _instantiation_cases():
    from test_igemm_table_host import TABLE
    cases, seen = [], set()

    def sweep(kind, keep):
        for key in ("short", "long"):
            if getattr(KINDS[kind], key) is None:
                continue
            for bm in (64, 128, 256):
                for bn in (32, 64, 128, 160):
                    for stages in range(2, 9):
                        for waves in (4, 8, 41):
                            force = _force(bm, bn, stages=stages, waves=waves)
                            plan = route_of(kind, shape_of(kind, key), force)
                            if plan.status != 0 or plan.cls != "tiled" or not keep(plan):
                                continue
                            k = (kind,) + inst_key(plan)
                            if k not in seen:
                                seen.add(k)
                                cases.append(Case(_case_id(kind, plan), kind, key, "", force, plan))

    sweep("conv3x3", lambda pl: True)               # the plain kernels (lin = 0), every ring
    sweep("linear", lambda pl: pl.lin == 1)         # the LIN kernels: rings up to 4 (deeper rings run a Linear on the plain kernel: conv3x3 has them)
    sweep("ups_phase", lambda pl: True)
    sweep("ln_linear", lambda pl: True)
    sweep("ln_geglu", lambda pl: True)
    sweep("geglu", lambda pl: True)
    # the other conv / two-source kinds: every table row at its shallowest ring, adma 0 (short K) and 1 (long K)
    for kind in ("linear_2src", "conv3x3_2src", "conv3x3_s2", "conv3x3_ups", "conv3x3_tap_inner"):
        for (bm, bn, wgm, wgn), (rings, _, _) in TABLE.items():
            for key in ("short", "long"):
                force = _force(bm, bn, stages=min(rings), waves=41 if wgn == 1 else wgm * wgn)
                plan = route_of(kind, shape_of(kind, key), force)
                cases.append(Case(_case_id(kind, plan), kind, key, "", force, plan))
    # the residual in +-2000 through the staged epilogue (128 x 64) and the direct one (256 x 160); SPLITK_CASES has it through the reduce kernel
    for kind in RES_KINDS:
        for bm, bn in ((128, 64), (256, 160)):
            force = _force(bm, bn, stages=2, waves=4)
            plan = route_of(kind, shape_of(kind, "short"), force)
            cases.append(Case(_case_id(kind, plan), kind, "short", "bigres", force, plan))
    return _finish(cases)


SPLITK_TILES = ((128, 160, 4), (128, 64, 8), (64, 64, 4), (256, 128, 8))


def _splitk_cases():
    cases = []
    for kind in ("linear", "conv3x3", "conv3x3_tap_inner", "ups_phase"):
        for key in ("short", "long"):
            s = shape_of(kind, key)
            nk = gemm_mnk(kind, s)[2] // 64
            for bm, bn, waves in SPLITK_TILES:
                for sk in (2, 3 if nk % 3 else 5, nk):
                    force = _force(bm, bn, splitk=sk, order=0, waves=waves)
                    plan = route_of(kind, s, force)
                    cases.append(Case(_case_id(kind, plan), kind, key, "", force, plan))
    for bm, bn, waves in SPLITK_TILES:
        force = _force(bm, bn, splitk=2, order=0, waves=waves)
        plan = route_of("linear", shape_of("linear", "k3136"), force)
        cases.append(Case(_case_id("linear", plan), "linear", "k3136", "", force, plan))
    for kind in ("linear", "conv3x3", "conv3x3_tap_inner"):      # the rounding of splitk_reduce_kernel behind a residual in +-2000
        force = _force(64, 64, splitk=2, order=0, waves=4)
        plan = route_of(kind, shape_of(kind, "short"), force)
        cases.append(Case(_case_id(kind, plan), kind, "short", "bigres", force, plan))
    return _finish(cases)


def _order_cases():
    cases = []
    for kind in ("linear", "conv3x3"):
        for bm, bn in ((64, 32), (64, 64), (128, 64)):
            for order in (0, 1, 8):
                force = _force(bm, bn, splitk=1, order=order, waves=4)
                plan = route_of(kind, shape_of(kind, "m720"), force)
                cases.append(Case(_case_id(kind, plan), kind, "m720", "", force, plan))
    # the phase form under the grouped order: 8 row tiles per phase (kept), 3 row tiles per phase (the route falls back to a plain order)
    for key in ("p450", "short"):
        force = _force(64, 64, splitk=1, order=8)
        plan = route_of("ups_phase", shape_of("ups_phase", key), force)
        cases.append(Case(_case_id("ups_phase", plan), "ups_phase", key, "", force, plan))
    return _finish(cases)


def base_force(case):
    """the force string of the same tile, ring and wave grid at split-K 1 and tile order 0"""
    pl = case.plan
    return _force(pl.bm, pl.bn, splitk=1, stages=pl.stages, order=0, waves=pl.waves)


_LISTS = {"INSTANTIATION_CASES": _instantiation_cases, "SPLITK_CASES": _splitk_cases, "ORDER_CASES": _order_cases}


def __getattr__(name):      # the lists are built (once) when first asked for: importing the ctypes mirrors alone queries nothing
    if name in _LISTS:
        globals()[name] = _LISTS[name]()
        return globals()[name]
    raise AttributeError(name)


# ------------------------------------------------------------------------------------------------------------------------------------------------
# operands and references (CPU; the GPU test moves them to the device)
# ------------------------------------------------------------------------------------------------------------------------------------------------
def _seed(kind, key, variant):
    return 1000 * list(KINDS).index(kind) + sum(ord(ch) for ch in key + variant)


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g)


def _conv_ref(kind, x, w_tap):
    """fp64 conv of the NHWC image x (all sources concatenated) with taps [Cout][3][3][Cin], the kind's stride / upsample -> [nimg][OH][OW][Cout]"""
    k = KINDS[kind]
    xi = x.double().permute(0, 3, 1, 2)
    if k.ups:
        xi = F.interpolate(xi, scale_factor=2.0, mode="nearest")
    return F.conv2d(xi, w_tap.double().permute(0, 3, 1, 2), None, stride=k.stride, padding=1).permute(0, 2, 3, 1).contiguous()


def build_exact(kind, key, variant=""):
    """Seeded integer operands of an exact kind and the fp64 reference: dict of CPU tensors (bf16 operands, fp32 bias / rowvec, `ref` fp64 in the
    shape of the op's result)"""
    k, s = KINDS[kind], shape_of(kind, key)
    assert k.exact
    g = torch.Generator().manual_seed(_seed(kind, key, variant))
    M, N, K = gemm_mnk(kind, s)
    OH, OW = out_hw(kind, s)
    Cin = s.c0 + s.c1
    t = {}
    if k.ksize == 1:
        a = _ints(g, -2, 2, M, Cin)
        w = _ints(g, -1, 1, N, Cin)
        ref = a.double() @ w.double().t()
        oshape = (M, N)
    else:
        a = _ints(g, -2, 2, s.nimg, s.H, s.W, Cin)
        w = _ints(g, -1, 1, N, 3, 3, Cin)
        ref = _conv_ref(kind, a, w)
        oshape = (s.nimg, OH, OW, N)
    assert tuple(ref.shape) == oshape
    if k.two_src:
        t["a0"], t["a1"] = a[..., :s.c0].contiguous().to(torch.bfloat16), a[..., s.c0:].contiguous().to(torch.bfloat16)
    else:
        t["a0"] = a.to(torch.bfloat16)
    t["w"] = w.to(torch.bfloat16)
    if k.bias:
        t["bias"] = _ints(g, -8, 8, N).float()
        ref = ref + t["bias"].double()
    if k.rowvec:
        t["rowvec"] = _ints(g, -8, 8, s.nimg, N).float()
        ref = ref + t["rowvec"].double()[:, None, None, :]
    if k.res:
        big = 2000 if variant == "bigres" else 8
        t["res"] = _ints(g, -big, big, *oshape).to(torch.bfloat16)
        assert torch.equal(t["res"].double().round(), t["res"].double())
        ref = ref + t["res"].double()
    t["ref"] = ref
    return t


def build_tolerance(kind, key="short", zero_extend_from=None):
    """Gaussian operands of geglu / ln_linear / ln_geglu as tests/test_ops_gpu.py::test_gemm_geglu / ::test_ln_gemm_... draw them, fp64 reference.
    zero_extend_from (geglu, long K): the operands of that shorter-K build in the first columns, zero activations behind them and random weights
    there: the same sums with exact zeros added, so the result must be the shorter build's bit for bit."""
    k, s = KINDS[kind], shape_of(kind, key)
    assert not k.exact
    g = torch.Generator().manual_seed(_seed(kind, key, ""))
    M, N, K = gemm_mnk(kind, s)
    t = {}
    if k.ln:
        a = (torch.randn(M, K, generator=g) * 2.0 + 0.7).to(torch.bfloat16)      # non-zero mean rows
        w = torch.randn(N, K, generator=g) * K ** -0.5
        t["gamma"], t["beta"] = 1.0 + 0.2 * torch.randn(K, generator=g), 0.1 * torch.randn(K, generator=g)
        t["bias"] = 0.1 * torch.randn(N, generator=g)
        h = F.linear(F.layer_norm(a.double(), (K,), t["gamma"].double(), t["beta"].double(), 1e-5), w.double(), t["bias"].double())
    else:
        a = torch.randn(M, K, generator=g).to(torch.bfloat16)
        w = (torch.randn(N, K, generator=g) * K ** -0.5).to(torch.bfloat16)
        t["bias"] = torch.randn(N, generator=g) * 0.1
        if zero_extend_from is not None:
            base = build_tolerance(kind, zero_extend_from)
            K0 = base["a0"].shape[1]
            a[:, :K0], a[:, K0:], w[:, :K0], t["bias"] = base["a0"], 0, base["w"], base["bias"]
        h = a.double() @ w.double().t() + t["bias"].double()
    t["a0"], t["w"] = a, w
    if k.geglu:
        val, gate = h.chunk(2, dim=-1)
        ref = val * F.gelu(gate)
    else:
        ref = h
    if k.res:
        t["res"] = torch.randn(M, N, generator=g).to(torch.bfloat16)
        ref = ref + t["res"].double()
    t["ref"] = ref
    return t


def run_op(kind, t, out=None):
    """the op wrapper of the kind on the (device) operands of build_exact / build_tolerance (`ref` not needed)"""
    from neurons_amd import ops
    k = KINDS[kind]
    if kind == "linear":
        return ops.gemm(t["a0"], t["w"], t["bias"], t["res"], out=out)
    if kind == "linear_2src":
        return ops.gemm2(t["a0"], t["a1"], t["w"], t["bias"], t["res"], out=out)
    if kind == "ups_phase":
        return ops.conv3x3_ups_phase(t["a0"], t["w"], t["bias"], out=out)
    if kind == "geglu":
        wp, bp = ops.geglu_permute(t["w"], t["bias"])
        return ops.gemm(t["a0"], wp, bp, geglu=True, out=out)
    if k.ln:
        return ops.ln_gemm(t["a0"], t["w"], t["gamma"], t["beta"], t["bias"], t.get("res"), geglu=k.geglu, out=out)
    OH, OW = (2 * t["a0"].shape[1], 2 * t["a0"].shape[2]) if k.ups else t["a0"].shape[1:3]
    rowvec_div = OH * OW      # one row of the row vector per image (stride 1 wherever a kind has one)
    return ops.conv3x3(t["a0"], t["w"], t["bias"], x1=t.get("a1"), stride=k.stride, ups=bool(k.ups), rowvec=t.get("rowvec"), rowvec_div=rowvec_div,
                       res=t.get("res"), tap_inner=k.tap_inner, out=out)
