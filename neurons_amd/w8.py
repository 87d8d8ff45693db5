"""Host reference of the weight-only e4m3 format behind ``nr_net_set_weight_fp8`` (smallm.hip, ``NR_W_FRAGMAJOR_E4M3``), in plain torch: for
tests and tools, never on the product path.

One power-of-two scale per row n of W ``[N, K]``: ``e[n] = ceil(log2(amax_n / 448))`` (448 = the largest OCP e4m3fn value), from frexp, so a ratio
that already is a power of two keeps it and an all-zero row gets 0.  Codes ``q = e4m3_rne(w * 2^-e)``: the scaling is exact and ``|w * 2^-e| <= 448``,
so the cast never overflows.  Every dequantised weight ``q * 2^e`` is a bf16 value (4 significant bits), and quantising it again gives it back.
"""
import torch

E4M3_MAX = 448.0


def row_exponents(w):
    """int32 ``[N]``: ``ceil(log2(amax_n / 448))``, exactly.  frexp: amax = m 2^x with 1/2 <= m < 1, so amax / 448 = (m / 0.875) 2^(x - 9)."""
    amax = w.detach().float().abs().amax(dim=1)
    m, x = torch.frexp(amax)
    e = torch.where(m > 0.875, x - 8, x - 9)
    return torch.where(amax > 0, e, torch.zeros_like(e)).to(torch.int32)


def quantize(w):
    """``(codes, e)``: ``codes`` float8_e4m3fn ``[N, K]`` and the row exponents int32 ``[N]`` of a bf16 / fp32 ``[N, K]`` matrix."""
    e = row_exponents(w)
    return torch.ldexp(w.detach().float(), -e[:, None]).to(torch.float8_e4m3fn), e


def dequantize(codes, e, dtype=torch.bfloat16):
    """``codes * 2^e`` per row; exact in bf16."""
    return torch.ldexp(codes.float(), e[:, None].to(codes.device)).to(dtype)


def pack_reference(w):
    """``(codes, scale)`` as ``ops.w8_pack``: uint8 ``[N/16, K/64, 64, 16]`` -- lane (fr, fg) = fr + 16 fg of block (T, kp) holds, for j = 0, 1, the
    eight codes of ``W[16 T + fr][32 (2 kp + j) + 8 fg .. + 7]`` -- and the fp32 row scales ``2^e`` ``[N]``."""
    N, K = w.shape
    assert N % 16 == 0 and K % 64 == 0, (N, K)
    q, e = quantize(w)
    b = q.view(torch.uint8).view(N // 16, 16, K // 64, 2, 4, 8)          # T, fr, kp, j, fg, byte
    codes = b.permute(0, 2, 4, 1, 3, 5).reshape(N // 16, K // 64, 64, 16).contiguous()   # T, kp, (fg, fr), (j, byte)
    return codes, torch.ldexp(torch.ones_like(e, dtype=torch.float32), e)
