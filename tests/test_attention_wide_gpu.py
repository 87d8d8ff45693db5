"""The wide-head attention kernel (the WideHead instantiations of attn_fwd_shared_kernel in attention.hip, d = 256 / 512) through neurons_amd.ops: the VAE mid-block shape class (one head of
d = 512 over h*w tokens), a strided two-head cross-attention at d = 256, the rescale of a non-empty accumulator, batch independence and
the calls the wide route refuses.

Reference: float64 softmax attention on the same bf16-rounded inputs, head split as test_attention_gpu._ref.
Tolerance: the project's attention bound of that file, max |err| <= 3e-2 max|ref| and mean |err| <= 8e-3 mean|ref|.  A CPU emulation of
the kernel's arithmetic (bf16 operands, fp32 logits, P rounded to bf16, the denominator summed from the rounded P, fp32 accumulation,
bf16 output) at these shapes sits at <= 3.3e-3 / 2.2e-3, so the bound has a 4-9x margin; every case prints its measured ratios.
Every case also asserts: finite output, no element of a NaN-pre-filled result left unwritten, a second call giving the same bits.
The kernel's tile: one workgroup = 64 queries of one (image, head), key tiles of 32."""
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_attention_gpu import _bits, _cross, _randn, _self  # noqa: E402


# ---------------------------------------------------------------- self-attention, d = 512, one head
@pytest.mark.parametrize("nimg,L", [(1, 16),       # below one key tile
                                    (2, 36),       # the 6 x 6 latent: query and key tails
                                    (3, 64),       # exactly one workgroup per image
                                    (1, 65),       # one query in the second workgroup
                                    (2, 100),
                                    (1, 1296)])    # 36 x 36: many tiles plus a tail
def test_self_attention_d512(cuda, nimg, L):
    _self(f"wide self d=512 nimg={nimg} L={L}", cuda, _randn(2000 + 7 * nimg + L, nimg, L, 3 * 512), 1)


# ---------------------------------------------------------------- cross-attention, d = 256, two heads
def test_cross_attention_d256_two_heads(cuda):
    # three images on two contexts of 77 keys: the last context serves one image; q rows of C, k|v rows of 2C, heads at stride d
    _cross("wide cross d=256", cuda, _randn(2100, 3, 64, 2 * 256), _randn(2101, 2, 77, 2 * 2 * 256), 2, 2)


# ---------------------------------------------------------------- rescale after the first key tile
def test_self_attention_d512_staircase_of_tile_maxima(cuda):
    # The construction of test_attention_gpu's staircase: q rows near sqrt(d) u for a unit vector u, the k rows of tile t = b_t u + noise
    # with b_t log2(e) = 0, 6, 16, 22 over tiles of 32 keys, so the row maximum rises tile by tile and the accumulator that is rescaled
    # is never empty.  Accuracy alone is asserted: the rescale policy is the kernel's.
    d, L, nimg = 512, 128, 2
    g = torch.Generator().manual_seed(2200)
    u = torch.randn(d, generator=g)
    u = u / u.norm()
    steps = torch.tensor([0.0, 6.0, 16.0, 22.0]) / math.log2(math.e)
    q = math.sqrt(d) * u + 0.3 * torch.randn(nimg, L, d, generator=g)
    k = steps.repeat_interleave(32)[None, :, None] * u + 0.3 * torch.randn(nimg, L, d, generator=g)
    v = torch.randn(nimg, L, d, generator=g)
    qkv = torch.cat([q, k, v], dim=-1).to(torch.bfloat16)
    s = torch.matmul(qkv[..., :d].double(), qkv[..., d:2 * d].double().transpose(-1, -2)) * (d ** -0.5 * math.log2(math.e))
    tmax = s.reshape(nimg, L, 4, 32).amax(dim=-1)
    rise = (tmax[..., 1:] - tmax[..., :-1]).reshape(-1, 3).median(dim=0).values
    print(f"[wide staircase] median rises of the log2-domain tile maxima {rise.tolist()}")
    assert ((rise - torch.tensor([6.0, 10.0, 6.0], dtype=rise.dtype)).abs() <= 1.0).all()
    _self("wide staircase d=512", cuda, qkv, 1)


# ---------------------------------------------------------------- batch independence
def test_image_zero_does_not_depend_on_the_batch(cuda):
    from neurons_amd import ops
    qkv = _randn(2300, 3, 100, 3 * 512).to(cuda)
    three = ops.attention_self(qkv, 1)
    one = ops.attention_self(qkv[:1].contiguous(), 1)
    torch.cuda.synchronize()
    assert torch.isfinite(three).all()
    assert torch.equal(_bits(three[0]), _bits(one[0])), "image 0 of the 3-image call differs from the 1-image call"


# ---------------------------------------------------------------- refusals
@pytest.mark.parametrize("what", ["causal", "fp8", "temporal"])
def test_wide_route_refusals_leave_the_result_untouched(cuda, what):
    from neurons_amd import ops
    frames, hw = 4, 3
    shape = (2 * frames, hw, 512) if what == "temporal" else (2, 64, 512)
    qkv = _randn(2400, shape[0], shape[1], 3 * 512).to(cuda)
    out = torch.full(shape, float("nan"), dtype=torch.bfloat16, device=cuda)
    with pytest.raises(RuntimeError, match="nr_launch_attention"):
        if what == "temporal":
            ops.attention_temporal(qkv, 1, frames, out=out)
        else:
            ops.attention_self(qkv, 1, causal=what == "causal", fp8=what == "fp8", out=out)
    torch.cuda.synchronize()
    assert torch.isnan(out).all(), "a refused call wrote to its result"
