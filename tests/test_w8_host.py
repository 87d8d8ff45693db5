"""Weight-only e4m3 storage for the small-M Linear kernel (nr_net_set_weight_fp8), host side: the format's exactness properties on the
reference quantiser of neurons_amd/w8.py, and -- through ctypes on the built library, no GPU needed -- the size of the packed form and the
route: the request bit changes the weight layout smallm.hip is handed and nothing else, and a launch smallm.hip does not take ignores it."""
import ctypes as C

import pytest
import torch

from igemm_forms import NrGemmParams, NrGemmRoute      # the ctypes mirrors of common.h / gemm_route.h
from neurons_amd import _lib, w8

# NrWeightLayout / NrGemmClass of neurons_amd/csrc/gemm_route.h
NR_W_FRAGMAJOR, NR_W_FRAGMAJOR_E4M3 = 2, 5
NR_GEMM_SMALLM = 0


def _rows():
    """[16][128] bf16: rows spanning 1e-4 .. 10 in scale, then a row with values far below its amax (subnormal codes), a row whose amax scales to
    (224, 232) so that its largest code rounds DOWN to 224, a row whose amax is 448 * 2^-3 exactly, and a zero row."""
    g = torch.Generator().manual_seed(7)
    w = torch.randn(16, 128, generator=g)
    w[:12] *= torch.logspace(-4, 1, 12)[:, None]
    w[12] = 2e-5 * torch.randn(128, generator=g)
    w[12, 5] = 1.0
    w[13] = w[13].clamp(-1, 1) * 100 * 2.0 ** -10
    w[13, 9] = -225 * 2.0 ** -10
    w[14] = w[14].clamp(-3, 3) * 10
    w[14, 77] = 448 * 2.0 ** -3
    w[15] = 0
    return w.to(torch.bfloat16)


def test_row_exponent_is_the_ceiling_of_log2_amax_over_448():
    w = _rows()
    e = w8.row_exponents(w)
    amax = w.double().abs().amax(1)
    nz = amax > 0
    s = torch.ldexp(torch.ones(16, dtype=torch.float64), e)
    assert (amax[nz] <= 448 * s[nz]).all() and (amax[nz] > 224 * s[nz]).all()      # 2^(e-1) < amax / 448 <= 2^e, in exact products
    assert e[15] == 0                                                             # all-zero row
    assert e[14] == -3                                                            # amax / 448 already a power of two: kept
    assert e[12] == -8


def test_codes_never_overflow_and_match_the_plain_torch_cast():
    w = _rows()
    q, e = w8.quantize(w)
    scaled = torch.ldexp(w.float(), -e[:, None])
    assert torch.equal(scaled.double(), w.double() * torch.ldexp(torch.ones(16, dtype=torch.float64), -e)[:, None])      # the scaling is exact
    assert scaled.abs().max() <= w8.E4M3_MAX
    assert torch.equal(q.view(torch.uint8), scaled.to(torch.float8_e4m3fn).view(torch.uint8))
    qf = q.float()
    assert torch.isfinite(qf).all()
    assert (qf.abs().amax(1)[:15] >= 224).all()
    sub = (qf[12] != 0) & (qf[12].abs() < 2.0 ** -6)
    assert sub.sum() > 10, "the small-value row must reach subnormal codes"
    assert qf[13].abs().max() == 224


def test_dequantised_weights_are_bf16_values_and_requantise_losslessly():
    w = _rows()
    q, e = w8.quantize(w)
    d32 = w8.dequantize(q, e, torch.float32)
    d = w8.dequantize(q, e)
    assert d.dtype == torch.bfloat16 and torch.equal(d.float(), d32)
    q2, e2 = w8.quantize(d)
    assert torch.equal(w8.dequantize(q2, e2), d)
    low = q.float().abs().amax(1) == 224          # amax * 2^-e lies in (224, 448]: a largest code of 224 was rounded down to
    assert low[13] and not low[14] and not low[15]
    assert torch.equal(e2, e - low.to(torch.int32)), "a row whose largest code rounded to 224 requantises one exponent lower, every other row keeps its own"
    assert torch.equal(q2.float()[13], 2 * q.float()[13])


def test_scaling_the_fp32_accumulator_equals_accumulating_the_dequantised_weights():
    w = _rows()
    q, e = w8.quantize(w)
    g = torch.Generator().manual_seed(8)
    x = torch.randn(33, 128, generator=g).to(torch.bfloat16).float()
    s = torch.ldexp(torch.ones(16), e)
    lhs = torch.zeros(33, 16)
    rhs = torch.zeros(33, 16)
    d = w8.dequantize(q, e, torch.float32)
    qf = q.float()
    for k in range(128):      # one fixed fp32 summation order for both
        lhs += x[:, k, None] * qf[None, :, k]
        rhs += x[:, k, None] * d[None, :, k]
    assert torch.equal(lhs * s[None], rhs)


def test_pack_reference_puts_every_code_where_the_kernel_reads_it():
    g = torch.Generator().manual_seed(9)
    w = (torch.randn(32, 192, generator=g) * 0.03).to(torch.bfloat16)
    codes, scale = w8.pack_reference(w)
    q, e = w8.quantize(w)
    qb = q.view(torch.uint8)
    assert codes.shape == (2, 3, 64, 16) and codes.dtype == torch.uint8
    for T in range(2):
        for kp in range(3):
            for lane in range(64):
                fr, fg = lane & 15, lane >> 4
                for j in range(2):
                    k0 = 32 * (2 * kp + j) + 8 * fg
                    assert torch.equal(codes[T, kp, lane, 8 * j:8 * j + 8], qb[16 * T + fr, k0:k0 + 8])
    assert torch.equal(scale, torch.ldexp(torch.ones(32), e)) and scale.dtype == torch.float32


# ---------------------------------------------------------------------------------------------------------------------------------------
# the built library through ctypes: sizes and the route (host functions; nothing here touches a device)
# ---------------------------------------------------------------------------------------------------------------------------------------


@pytest.fixture()
def lib(monkeypatch):
    for k in ("NR_SMALLM", "NR_IGEMM_FORCE", "NR_DETERMINISTIC_BATCH", "NR_G8P", "NR_W8"):
        monkeypatch.delenv(k, raising=False)
    lib = _lib.load()
    lib.nr_gemm_packed_bytes.restype = C.c_size_t
    lib.nr_gemm_packed_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.nr_gemm_route.restype = C.c_int
    lib.nr_gemm_route.argtypes = [C.POINTER(NrGemmParams), C.POINTER(NrGemmRoute)]
    return lib


def _linear(M, N, K, w8_request):
    p = NrGemmParams()
    p.c0, p.lda0, p.H, p.W, p.OH, p.OW, p.ksize, p.stride = K, K, 1, 1, 1, 1, 1, 1
    p.M, p.N, p.K, p.rowvec_div, p.ldo, p.out_scale, p.w8 = M, N, K, 1, N, 1.0, w8_request
    return p


def _route(lib, p):
    r = NrGemmRoute()
    assert lib.nr_gemm_route(C.byref(p), C.byref(r)) == 0
    return r


def test_packed_bytes_of_the_e4m3_layout(lib):
    for N, K in ((80, 640), (1280, 1280), (1920, 2560)):
        assert lib.nr_gemm_packed_bytes(NR_W_FRAGMAJOR_E4M3, N, K) == N * K + 4 * N
        assert lib.nr_gemm_packed_bytes(NR_W_FRAGMAJOR, N, K) == 2 * N * K
    assert lib.nr_gemm_packed_bytes(NR_W_FRAGMAJOR_E4M3, 72, 640) == 0      # N % 16
    assert lib.nr_gemm_packed_bytes(NR_W_FRAGMAJOR_E4M3, 80, 608) == 0      # K % 64


def test_the_request_changes_the_weight_layout_of_a_smallm_launch_and_nothing_else(lib):
    for M, N, K in ((512, 1280, 1280), (512, 1280, 5120), (33, 64, 640)):
        r0, r1 = _route(lib, _linear(M, N, K, 0)), _route(lib, _linear(M, N, K, 1))
        assert r0.cls == r1.cls == NR_GEMM_SMALLM
        assert list(r0.smallm) == list(r1.smallm) and r0.smallm[0] in (4, 5)
        assert (r0.weight_layout, r1.weight_layout) == (NR_W_FRAGMAJOR, NR_W_FRAGMAJOR_E4M3)
        r1.weight_layout = r0.weight_layout
        assert bytes(r0) == bytes(r1)


def test_a_launch_smallm_does_not_take_ignores_the_request(lib):
    # K = 768 (the text context projections), > 512 rows, several slabs per workgroup under the shipped rule
    for M, N, K in ((512, 1280, 768), (1024, 1280, 1280), (512, 3840, 1280)):
        r0, r1 = _route(lib, _linear(M, N, K, 0)), _route(lib, _linear(M, N, K, 1))
        assert r0.cls != NR_GEMM_SMALLM
        assert bytes(r0) == bytes(r1)
