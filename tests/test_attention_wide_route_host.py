"""nr_attn_route (neurons_amd/csrc/attention.hip) through ctypes with mirrored structs, host only: the wide class serves d = 256 / 512 and
nothing else changes its answer.

The wide kernel's tile is 64 queries of one (image, head) per workgroup, so its grid is nbatch * heads * ceil(Lq / 64); its LDS image is two
buffers of a 32-key K tile (rows of d + 8 elements) and V tile (rows of d + 16): 2 * 32 * (2 d + 24) * 2 bytes, under the 160 KiB of a CU.
The d = 40 / 80 / 160 routes are compared field by field with the values the routing rule gave before the wide class existed."""
import ctypes as C

import pytest

from neurons_amd import _lib

NR_ATTN_WAVE, NR_ATTN_SHARED, NR_ATTN_WIDE = 0, 1, 2


class NrAttnParams(C.Structure):      # neurons_amd/csrc/common.h
    _fields_ = [("q", C.c_void_p), ("k", C.c_void_p), ("v", C.c_void_p), ("out", C.c_void_p),
                ("q_outer", C.c_longlong), ("q_inner_stride", C.c_longlong), ("q_seq", C.c_longlong),
                ("kv_outer", C.c_longlong), ("kv_inner_stride", C.c_longlong), ("kv_seq", C.c_longlong),
                ("o_outer", C.c_longlong), ("o_inner_stride", C.c_longlong), ("o_seq", C.c_longlong),
                ("inner", C.c_int), ("kv_inner", C.c_int), ("kv_div", C.c_int),
                ("nbatch", C.c_int), ("heads", C.c_int), ("d", C.c_int), ("Lq", C.c_int), ("Lk", C.c_int),
                ("scale", C.c_float), ("causal", C.c_int), ("fp8", C.c_int)]


class NrAttnRoute(C.Structure):       # neurons_amd/csrc/launchers.h
    _fields_ = [("cls", C.c_int), ("dk", C.c_int), ("dt", C.c_int), ("fp8", C.c_int), ("ones", C.c_int), ("grid", C.c_uint), ("lds_bytes", C.c_size_t)]


@pytest.fixture()
def lib(monkeypatch):
    monkeypatch.delenv("NR_ATTN_ROWSUM", raising=False)
    lib = _lib.load()
    lib.nr_attn_route.restype = C.c_int
    lib.nr_attn_route.argtypes = [C.POINTER(NrAttnParams), C.POINTER(NrAttnRoute)]
    return lib


def _self(nimg, L, heads, d, causal=0, fp8=0):
    """mode 0 of nr_attn_params: fused q|k|v rows of 3C."""
    Cc = heads * d
    p = NrAttnParams()
    p.nbatch, p.heads, p.d, p.Lq, p.Lk, p.scale, p.causal, p.fp8 = nimg, heads, d, L, L, d ** -0.5, causal, fp8
    p.inner, p.kv_inner, p.kv_div = 1, 1, 1
    p.q_outer = p.kv_outer = L * 3 * Cc
    p.q_seq = p.kv_seq = 3 * Cc
    p.o_outer, p.o_seq = L * Cc, Cc
    return p


def _cross(nimg, L, Lk, heads, d, kv_div):
    Cc = heads * d
    p = _self(nimg, L, heads, d)
    p.Lk, p.kv_div = Lk, kv_div
    p.q_outer, p.q_seq, p.kv_outer, p.kv_seq = L * Cc, Cc, Lk * 2 * Cc, 2 * Cc
    return p


def _temporal(nimg, hw, frames, heads, d):
    Cc = heads * d
    p = _self(nimg, frames, heads, d)
    p.nbatch, p.inner, p.kv_inner = (nimg // frames) * hw, hw, hw
    p.q_outer = p.kv_outer = frames * hw * 3 * Cc
    p.q_inner_stride = p.kv_inner_stride = 3 * Cc
    p.q_seq = p.kv_seq = hw * 3 * Cc
    p.o_outer, p.o_inner_stride, p.o_seq = frames * hw * Cc, Cc, hw * Cc
    return p


def _route(lib, p):
    r = NrAttnRoute()
    return lib.nr_attn_route(C.byref(p), C.byref(r)), r


@pytest.mark.parametrize("p,units", [(_self(16, 1024, 1, 512), 16 * 16), (_self(1, 9216, 1, 512), 144), (_self(2, 36, 1, 512), 2), (_self(1, 65, 1, 512), 2),
                                     (_self(3, 100, 2, 256), 3 * 2 * 2), (_cross(3, 64, 77, 2, 256, 2), 3 * 2), (_cross(5, 130, 77, 1, 512, 2), 5 * 3)])
def test_wide_widths_route_to_the_wide_class(lib, p, units):
    rc, r = _route(lib, p)
    assert rc == 0
    assert r.cls == NR_ATTN_WIDE and r.fp8 == 0 and r.ones == 0
    assert r.grid == units == p.nbatch * p.heads * ((p.Lq + 63) // 64)
    assert r.lds_bytes == 2 * 32 * (2 * p.d + 24) * 2 <= 160 * 1024
    assert (r.dk, r.dt) == (p.d // 32, p.d // 16)


@pytest.mark.parametrize("p", [_self(2, 64, 2, 168), _self(2, 64, 1, 512, causal=1), _self(2, 64, 1, 512, fp8=1), _self(2, 64, 2, 256, causal=1),
                               _temporal(8, 3, 4, 1, 512), _self(2, 64, 1, 384), _self(2, 64, 1, 1024), _self(2, 64, 2, 104), _self(2, 64, 2, 144)])
def test_what_no_kernel_serves_is_refused(lib, p):
    rc, _ = _route(lib, p)
    assert rc != 0


# (params, (cls, dk, dt, fp8, ones, grid, lds_bytes)) as the rule answered before NR_ATTN_WIDE: block-shared K/V tiles of 64 keys from 48 queries on
# (K rows of 64 elements swizzled up to d = 64, else 32 dk + 8; V rows of 16 dt [+ 16]; the ones column at d = 40), per-wave tiles of 32 keys below,
# for causal and for temporal calls
PARENT = [
    (_self(2, 1024, 8, 40), (NR_ATTN_SHARED, 2, 3, 0, 1, 256, 2 * 64 * (64 + 48) * 2)),
    (_self(2, 1024, 8, 80), (NR_ATTN_SHARED, 3, 5, 0, 0, 256, 2 * 64 * (104 + 80) * 2)),
    (_self(2, 1024, 8, 160), (NR_ATTN_SHARED, 5, 10, 0, 0, 256, 2 * 64 * (168 + 176) * 2)),
    (_self(2, 100, 8, 80, fp8=1), (NR_ATTN_SHARED, 3, 5, 1, 0, 32, 2 * 64 * (104 + 80) * 2)),
    (_cross(32, 256, 77, 8, 160, 16), (NR_ATTN_SHARED, 5, 10, 0, 0, 32 * 8 * 4, 2 * 64 * (168 + 176) * 2)),
    (_self(2, 16, 8, 40), (NR_ATTN_WAVE, 2, 3, 0, 0, 4, 4 * 32 * 48 * 2)),
    (_self(2, 40, 8, 80), (NR_ATTN_WAVE, 3, 5, 0, 0, 12, 4 * 32 * 80 * 2)),
    (_self(2, 77, 8, 160, causal=1), (NR_ATTN_WAVE, 5, 10, 0, 0, 20, 4 * 32 * 176 * 2)),
    (_temporal(32, 64, 16, 8, 40), (NR_ATTN_WAVE, 2, 3, 0, 0, 2 * 64 * 8 // 4, 4 * 32 * 48 * 2)),
    (_temporal(32, 64, 16, 8, 160), (NR_ATTN_WAVE, 5, 10, 0, 0, 2 * 64 * 8 // 4, 4 * 32 * 176 * 2)),
    # every other instantiated dt (1, 2, 4, 6, 8) once per class, and a second width of dt = 3, 5, 10: the numbers the rule answered while the
    # route still retyped the kernels' LDS strides (recorded from that commit's nr_attn_route)
    (_self(2, 1024, 8, 16), (NR_ATTN_SHARED, 1, 1, 0, 0, 256, 20480)),
    (_self(2, 40, 8, 16), (NR_ATTN_WAVE, 1, 1, 0, 0, 12, 4096)),
    (_self(2, 100, 8, 8, fp8=1), (NR_ATTN_SHARED, 1, 1, 1, 0, 32, 20480)),
    (_self(2, 1024, 8, 32), (NR_ATTN_SHARED, 1, 2, 0, 0, 256, 28672)),
    (_self(2, 40, 8, 32), (NR_ATTN_WAVE, 1, 2, 0, 0, 12, 12288)),
    (_self(2, 1024, 8, 24), (NR_ATTN_SHARED, 1, 2, 0, 0, 256, 28672)),
    (_self(2, 1024, 8, 48), (NR_ATTN_SHARED, 2, 3, 0, 0, 256, 28672)),
    (_self(2, 40, 8, 48), (NR_ATTN_WAVE, 2, 3, 0, 0, 12, 12288)),
    (_self(2, 1024, 8, 64), (NR_ATTN_SHARED, 2, 4, 0, 0, 256, 36864)),
    (_self(2, 40, 8, 64), (NR_ATTN_WAVE, 2, 4, 0, 0, 12, 20480)),
    (_self(2, 100, 8, 56, fp8=1), (NR_ATTN_SHARED, 2, 4, 1, 0, 32, 36864)),
    (_self(2, 1024, 8, 72), (NR_ATTN_SHARED, 3, 5, 0, 0, 256, 47104)),
    (_self(2, 40, 8, 72), (NR_ATTN_WAVE, 3, 5, 0, 0, 12, 20480)),
    (_self(2, 1024, 8, 96), (NR_ATTN_SHARED, 3, 6, 0, 0, 256, 55296)),
    (_self(2, 40, 8, 96), (NR_ATTN_WAVE, 3, 6, 0, 0, 12, 28672)),
    (_self(2, 100, 8, 88, fp8=1), (NR_ATTN_SHARED, 3, 6, 1, 0, 32, 55296)),
    (_self(2, 1024, 8, 128), (NR_ATTN_SHARED, 4, 8, 0, 0, 256, 71680)),
    (_self(2, 40, 8, 128), (NR_ATTN_WAVE, 4, 8, 0, 0, 12, 36864)),
    (_self(2, 100, 8, 120, fp8=1), (NR_ATTN_SHARED, 4, 8, 1, 0, 32, 71680)),
    (_self(2, 1024, 8, 152), (NR_ATTN_SHARED, 5, 10, 0, 0, 256, 88064)),
    (_self(2, 40, 8, 152), (NR_ATTN_WAVE, 5, 10, 0, 0, 12, 45056)),
    (_self(2, 100, 1, 256), (NR_ATTN_WIDE, 8, 16, 0, 0, 4, 68608)),
    (_self(2, 100, 1, 512), (NR_ATTN_WIDE, 16, 32, 0, 0, 4, 134144)),
]


@pytest.mark.parametrize("p,want", PARENT)
def test_narrow_widths_route_as_before(lib, p, want):
    rc, r = _route(lib, p)
    assert rc == 0
    assert (r.cls, r.dk, r.dt, r.fp8, r.ones, r.grid, r.lds_bytes) == want
