"""Phase form of the nearest-2x upsample convs (NrGemmParams::ups == 2), host side, through ctypes on the built library (no GPU): the weight
packer against the four tap sums computed in torch, and the route -- ups = 2 is served by the tiled class with dense split-K slabs, every
combination the form has no path for is refused, and ups = 1 launches route exactly as they did before the form existed."""
import ctypes as C

import pytest
import torch

from igemm_forms import NR_GEMM_TILED, NrGemmParams, NrGemmRoute      # the ctypes mirrors of common.h / gemm_route.h
from neurons_amd import _lib, ops

# the three upsample convs of the headline step: (nimg, H, W, Cin, Cout)
HEADLINE = ((32, 4, 4, 1280, 1280), (32, 8, 8, 1280, 1280), (32, 16, 16, 640, 640))


@pytest.fixture()
def lib(monkeypatch):
    for k in ("NR_SMALLM", "NR_IGEMM_FORCE", "NR_DETERMINISTIC_BATCH", "NR_G8P", "NR_W8", "NR_IGEMM_GROUPED", "NR_IGEMM_GROUPED_MINW", "NR_IGEMM_T64X160",
              "NR_IGEMM_ADMA_MINK", "NR_IGEMM_LIN", "NR_UPS_PHASE"):
        monkeypatch.delenv(k, raising=False)
    lib = _lib.load()
    lib.nr_gemm_route.restype = C.c_int
    lib.nr_gemm_route.argtypes = [C.POINTER(NrGemmParams), C.POINTER(NrGemmRoute)]
    return lib


def _conv(nimg, H, W, Cin, Cout, ups):
    p = NrGemmParams()
    p.c0, p.lda0, p.H, p.W, p.OH, p.OW, p.ksize, p.stride, p.ups = Cin, Cin, H, W, 2 * H, 2 * W, 3, 1, ups
    p.M, p.N, p.K, p.rowvec_div, p.ldo, p.out_scale = nimg * 4 * H * W, Cout, (4 if ups == 2 else 9) * Cin, 1, Cout, 1.0
    return p


def _phase_reference(w):
    """w fp32 [Cout][3][3][Cin] -> [4][Cout][4][Cin] bf16: Wp[py][px][a][b] = sum of the taps ky in R(py, a), kx in R(px, b)"""
    R = {(0, 0): (0,), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2,)}
    Cout, _, _, Cin = w.shape
    out = torch.empty(4, Cout, 4, Cin, dtype=torch.bfloat16)
    for py in range(2):
        for px in range(2):
            for a in range(2):
                for b in range(2):
                    acc = torch.zeros(Cout, Cin, dtype=torch.float32)
                    for ky in R[(py, a)]:
                        for kx in R[(px, b)]:
                            acc = acc + w[:, ky, kx, :]
                    out[2 * py + px, :, 2 * a + b, :] = acc.to(torch.bfloat16)
    return out


@pytest.mark.parametrize("Cout,Cin", [(32, 64), (96, 128)])
def test_packer_sums_the_taps_in_fp32_and_rounds_once(Cout, Cin):
    g = torch.Generator().manual_seed(100 + Cout)
    w = torch.randn(Cout, 3, 3, Cin, generator=g, dtype=torch.float32) * 0.05
    got = ops.ups_phase_weights(w)
    ref = _phase_reference(w)
    assert got.shape == (4, Cout, 4, Cin) and got.dtype == torch.bfloat16
    assert torch.equal(got.view(torch.int16), ref.view(torch.int16))
    # the sums are not the bf16 sums of bf16 taps: rounding happens once, after the fp32 sum
    twice = _phase_reference(w.to(torch.bfloat16).float())
    assert not torch.equal(got.view(torch.int16), twice.view(torch.int16))


@pytest.mark.parametrize("shape", HEADLINE + ((3, 5, 7, 64, 96), (1, 1, 1, 64, 64)))
def test_route_accepts_the_phase_form_in_the_tiled_class(lib, shape):
    p = _conv(*shape, ups=2)
    r = NrGemmRoute()
    assert lib.nr_gemm_route(C.byref(p), C.byref(r)) == 0
    bm, bn, splitk, stages, waves, adma, lin = list(r.tiled)
    assert r.cls == NR_GEMM_TILED and r.weight_layout == 0 and lin == 0 and stages == 2 and splitk >= 1
    assert r.ws_bytes == (splitk * p.M * p.N * 4 if splitk > 1 else 0)      # dense slabs [slice][phase * Mp + r][N]


def test_route_phase_form_keeps_dense_slabs_under_forced_split_k(lib, monkeypatch):
    monkeypatch.setenv("NR_IGEMM_FORCE", "64,64,3,-1,-1")
    p = _conv(3, 5, 7, 64, 96, ups=2)
    r = NrGemmRoute()
    assert lib.nr_gemm_route(C.byref(p), C.byref(r)) == 0
    assert r.cls == NR_GEMM_TILED and list(r.tiled)[:3] == [64, 64, 3]
    assert r.ws_bytes == 3 * p.M * p.N * 4


def test_route_refuses_what_the_phase_form_has_no_path_for(lib):
    one = C.c_void_p(256)      # any non-null pointer: the route never dereferences

    def second_source(p): p.a1, p.c1, p.lda1, p.K = one, 64, 64, 4 * (p.c0 + 64)
    def stride2(p): p.stride = 2
    def tap_inner(p): p.tap_inner = 1
    def pad_tl0(p): p.pad_tl0 = 1
    def geglu(p): p.geglu = 1
    def ln_c(p): p.ln_c = one
    def out_f32(p): p.out_f32 = one
    def res(p): p.res, p.ldr = one, p.N
    def rowvec(p): p.rowvec, p.rowvec_ld = one, p.N
    def k_of_the_3x3_form(p): p.K = 9 * p.c0
    def not_a_2x_upsample(p): p.OH = p.H
    def ksize1(p): p.ksize = 1

    for spoil in (second_source, stride2, tap_inner, pad_tl0, geglu, ln_c, out_f32, res, rowvec, k_of_the_3x3_form, not_a_2x_upsample, ksize1):
        p = _conv(2, 4, 4, 1280, 1280, ups=2)
        r = NrGemmRoute()
        assert lib.nr_gemm_route(C.byref(p), C.byref(r)) == 0
        spoil(p)
        assert lib.nr_gemm_route(C.byref(p), C.byref(r)) != 0, spoil.__name__


# NrGemmRoute of the three headline upsample convs as ups = 1 launches, recorded from the library before the phase form existed
UPS1_ROUTE_BYTES = {
    (32, 4, 4, 1280, 1280): "04000000000000000800000000000000000080020000000080000000a000000004000000020000000400000001000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000002000000",
    (32, 8, 8, 1280, 1280): "040000000000000008000000000000000000000000000000800000008000000001000000020000000800000001000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000002000000",
    (32, 16, 16, 640, 640): "040000000000000008000000000000000000000000000000800000008000000001000000020000000800000001000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000002000000",
}


@pytest.mark.parametrize("shape", HEADLINE)
def test_route_of_the_3x3_form_is_unchanged(lib, shape):
    p = _conv(*shape, ups=1)
    r = NrGemmRoute()
    assert lib.nr_gemm_route(C.byref(p), C.byref(r)) == 0
    assert bytes(r).hex() == UPS1_ROUTE_BYTES[shape]
