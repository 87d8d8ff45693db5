"""attention.hip through nr_op_attention at the shapes the other op tests leave out: every instantiated head width (pad
columns, the 16-deep second k-step of d = 40 / 48), head counts that make the workgroup remap's remainder branch and the
idle wave of the per-wave kernel run, every key / query tile edge, the causal mask, and inputs that make the block-shared
kernel's lazy running maximum move AFTER the first key tile (the rescale of a non-empty accumulator).

Reference: softmax attention in float64 torch on the same bf16-rounded inputs, head split as test_ops_gpu._attn_ref.
Tolerance: the project's attention bound, max |err| <= 3e-2 max|ref| and mean |err| <= 8e-3 mean|ref| (the error
sources are the bf16 rounding of P and of the output, neither of which grows with the size of the logits).
Every case also asserts: finite output, no element of a NaN-pre-filled result left unwritten, and a second call with
the same inputs returning the same bits."""
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_ops_gpu import FP8_ATTN_REL_L2  # noqa: E402

MAX_TOL, MEAN_TOL = 3e-2, 8e-3
WIDTHS = (8, 16, 24, 32, 40, 48, 56, 64, 72, 80, 88, 96, 120, 128, 152, 160)


# ---------------------------------------------------------------- inputs, reference, comparison
def _randn(seed, *shape, scale=1.0):
    """N(0, scale^2) drawn on the CPU (the same numbers on every machine), rounded to bf16."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16)


def _ref(q, k, v, heads, causal=False):
    """q [B, Lq, C], k / v [B, Lk, C] (bf16 values) -> float64 softmax(q k^T / sqrt(d)) v per head, [B, Lq, C]."""
    q, k, v = q.double(), k.double(), v.double()
    B, Lq, C = q.shape
    d = C // heads

    def split(t):
        return t.reshape(B, -1, heads, d).permute(0, 2, 1, 3)
    s = torch.matmul(split(q), split(k).transpose(-1, -2)) * (d ** -0.5)
    if causal:
        Lk = k.shape[1]
        s = s.masked_fill(torch.ones(Lq, Lk, dtype=torch.bool, device=s.device).triu(1), float("-inf"))
    o = torch.matmul(s.softmax(dim=-1), split(v))
    return o.permute(0, 2, 1, 3).reshape(B, Lq, C)


def _temporal_ref(qkv, heads, B, Fr, hw):
    """"(b f) d c -> (b d) f c" regroup, attention over f, and back."""
    C = qkv.shape[-1] // 3
    t = qkv.double().reshape(B, Fr, hw, 3 * C).permute(0, 2, 1, 3).reshape(B * hw, Fr, 3 * C)
    q, k, v = t.chunk(3, dim=-1)
    return _ref(q, k, v, heads).reshape(B, hw, Fr, C).permute(0, 2, 1, 3).reshape(B * Fr, hw, C)


def _bits(t):
    return t.view(torch.int16)


def _cmp(name, out, ref):
    assert out.shape == ref.shape, (name, out.shape, ref.shape)
    assert not torch.isnan(out).any(), f"{name}: elements of the NaN-filled result were left unwritten (or NaN was computed)"
    assert torch.isfinite(out).all(), f"{name}: non-finite output"
    err = (out.double() - ref).abs()
    mx, mean = err.max().item(), err.mean().item()
    rmx, rmean = ref.abs().max().item(), ref.abs().mean().item()
    print(f"[{name}] max_ratio={mx / rmx:.3e} mean_ratio={mean / rmean:.3e}")
    assert mx <= MAX_TOL * rmx + 1e-6, f"{name}: max err {mx} vs ref max {rmx}"
    assert mean <= MEAN_TOL * rmean + 1e-7, f"{name}: mean err {mean} vs ref mean {rmean}"


def _run(name, call, shape, ref, dev):
    """call(out) writes the op's result into out.  Twice into NaN-filled results: all written, same bits, within tolerance."""
    outs = []
    for _ in range(2):
        out = torch.full(shape, float("nan"), dtype=torch.bfloat16, device=dev)
        got = call(out)
        assert got.data_ptr() == out.data_ptr()
        outs.append(out)
    torch.cuda.synchronize()
    _cmp(name, outs[0], ref)
    assert torch.equal(_bits(outs[0]), _bits(outs[1])), f"{name}: two calls on the same inputs differ"
    return outs[0]


def _self(name, dev, qkv, heads, causal=False):
    from neurons_amd import ops
    qkv = qkv.to(dev)
    q, k, v = qkv.chunk(3, dim=-1)
    nimg, L, C3 = qkv.shape
    out = _run(name, lambda o: ops.attention_self(qkv, heads, causal=causal, out=o), (nimg, L, C3 // 3), _ref(q, k, v, heads, causal), dev)
    return out, v


def _cross(name, dev, q, kv, heads, kv_div):
    from neurons_amd import ops
    q, kv = q.to(dev), kv.to(dev)
    k, v = (t.repeat_interleave(kv_div, dim=0)[:q.shape[0]] for t in kv.chunk(2, dim=-1))
    out = _run(name, lambda o: ops.attention_cross(q, kv, heads, kv_div, out=o), tuple(q.shape), _ref(q, k, v, heads), dev)
    return out, v


def _temporal(name, dev, qkv, heads, B, Fr, hw):
    from neurons_amd import ops
    qkv = qkv.to(dev)
    C = qkv.shape[-1] // 3
    return _run(name, lambda o: ops.attention_temporal(qkv, heads, Fr, out=o), (B * Fr, hw, C), _temporal_ref(qkv, heads, B, Fr, hw), dev)


# ---------------------------------------------------------------- A. head widths
@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("L", [100, 40])
def test_self_attention_every_head_width(cuda, d, L):
    # L = 100: block-shared kernel, partial query block, 36-key last tile; L = 40: per-wave kernel, 8-key last tile, 8-row last query tile
    _self(f"A self d={d} L={L}", cuda, _randn(100 + d + L, 2, L, 3 * 2 * d), 2)


@pytest.mark.parametrize("d", WIDTHS)
def test_cross_attention_every_head_width(cuda, d):
    # three images on two contexts: the last context serves one image only
    _cross(f"A cross d={d}", cuda, _randn(200 + d, 3, 64, 2 * d), _randn(300 + d, 2, 77, 2 * 2 * d), 2, 2)


# ---------------------------------------------------------------- B. refusals
@pytest.mark.parametrize("d", [104, 112, 136, 144, 168, 12])
def test_head_width_without_a_kernel_is_refused_before_any_launch(cuda, d):
    from neurons_amd import ops
    qkv = _randn(400 + d, 2, 64, 3 * 2 * d).to(cuda)
    out = torch.full((2, 64, 2 * d), float("nan"), dtype=torch.bfloat16, device=cuda)
    with pytest.raises(RuntimeError, match="nr_launch_attention"):
        ops.attention_self(qkv, 2, out=out)
    torch.cuda.synchronize()
    assert torch.isnan(out).all(), "a refused call wrote to its result"


@pytest.mark.parametrize("mode", [17, 18, 24])
def test_causal_bit_is_for_plain_self_attention_only(cuda, mode):
    from neurons_amd import _lib
    qkv = _randn(450, 2, 64, 3 * 32).to(cuda)
    kv = _randn(451, 2, 64, 2 * 32).to(cuda)
    out = torch.full((2, 64, 32), float("nan"), dtype=torch.bfloat16, device=cuda)
    st = _lib.load().nr_op_attention(torch.cuda.current_stream().cuda_stream, mode, qkv.data_ptr(), kv.data_ptr(), out.data_ptr(),
                                     2, 64, 64, 32, 2, 2 if mode == 18 else 1, 1)
    assert st == 1, st                         # NR_ERR_ARG (include/neurons_amd.h)
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


# ---------------------------------------------------------------- C. head counts (d = 64)
@pytest.mark.parametrize("heads,nimg,L,units", [(1, 1, 64, 1), (5, 1, 192, 15), (10, 3, 64, 30), (12, 1, 192, 36), (20, 1, 64, 20),   # workgroups
                                                (5, 1, 40, 15)])                                                                    # waves
def test_self_attention_head_counts_off_the_multiple_of_eight(cuda, heads, nimg, L, units):
    # block-shared kernel (L >= 48): `units` workgroups, none a multiple of 8, so the remap's remainder branch places them;
    # per-wave kernel (L = 40): 15 work units on 4 blocks of 4 waves, the last wave idle and clamped
    per = (L + 63) // 64 if L >= 48 else (L + 15) // 16
    assert nimg * heads * per == units and units % (8 if L >= 48 else 4) != 0
    _self(f"C self heads={heads} nimg={nimg} L={L}", cuda, _randn(500 + heads + L, nimg, L, 3 * heads * 64), heads)


def test_temporal_attention_with_an_idle_wave(cuda):
    # C = 40, 5 heads, one pixel, 16 frames: 5 work units, 3 idle waves in the second block
    _temporal("C temporal heads=5", cuda, _randn(520, 16, 1, 3 * 40), 5, 1, 16, 1)


# ---------------------------------------------------------------- D. key / query edges
def _assert_rows_are_the_single_value_row(out, v):
    # softmax over one key is exactly 1: every output row is that key's V row, bit for bit
    assert torch.equal(_bits(out), _bits(v[:, :1].expand_as(out).contiguous()))


@pytest.mark.parametrize("d", [40, 80])
@pytest.mark.parametrize("L", [1, 16, 17, 31, 32, 33, 47, 48, 63, 64, 65, 127, 128, 129])
def test_self_attention_sequence_edges(cuda, d, L):
    out, v = _self(f"D self d={d} L={L}", cuda, _randn(600 + d + L, 2, L, 3 * 2 * d), 2)
    if L == 1:
        _assert_rows_are_the_single_value_row(out, v)


@pytest.mark.parametrize("d", [40, 80])
@pytest.mark.parametrize("Lq", [16, 64])
@pytest.mark.parametrize("Lk", [1, 31, 32, 33, 63, 64, 65, 77, 128, 129])
def test_cross_attention_key_edges(cuda, d, Lq, Lk):
    # Lq = 16: per-wave kernel; Lq = 64: block-shared kernel, with the denominator on the ones column at d = 40
    out, v = _cross(f"D cross d={d} Lq={Lq} Lk={Lk}", cuda, _randn(700 + d + Lq + Lk, 3, Lq, 2 * d), _randn(800 + d + Lq + Lk, 2, Lk, 2 * 2 * d), 2, 2)
    if Lk == 1:
        _assert_rows_are_the_single_value_row(out, v)


@pytest.mark.parametrize("hw", [1, 3])
@pytest.mark.parametrize("Fr", [1, 8, 17, 32, 33, 48])
def test_temporal_attention_frame_count_edges(cuda, Fr, hw):
    _temporal(f"D temporal F={Fr} hw={hw}", cuda, _randn(900 + Fr + hw, 2 * Fr, hw, 3 * 80), 2, 2, Fr, hw)


# ---------------------------------------------------------------- E. rescale of a non-empty accumulator (block-shared kernel, bf16)
def _lazy_maximum_replay(q, k, heads):
    """The block-shared kernel's running-maximum policy replayed on the REFERENCE scores scale * log2(e) * q k^T (float64): 64-key
    tiles, the reference maximum of a query starts at -inf and moves to the tile maximum only when that exceeds it by more than 8.
    Returns, over the tiles after the first, boolean [B, heads, Lq, tiles - 1] maps: the reference moved / the tile maximum
    was above the reference but within the margin (probabilities in (1, 256])."""
    q, k = q.double(), k.double()
    B, Lq, C = q.shape
    d = C // heads
    s = torch.matmul(q.reshape(B, Lq, heads, d).permute(0, 2, 1, 3), k.reshape(B, -1, heads, d).permute(0, 2, 3, 1)) * (d ** -0.5 * math.log2(math.e))
    assert s.shape[-1] % 64 == 0
    tmax = s.reshape(B, heads, Lq, -1, 64).amax(dim=-1)
    m = tmax[..., 0]
    moved, stale = [], []
    for t in range(1, tmax.shape[-1]):
        mv = tmax[..., t] > m + 8.0
        moved.append(mv)
        stale.append((tmax[..., t] > m) & ~mv)
        m = torch.where(mv, tmax[..., t], m)
    return torch.stack(moved, dim=-1), torch.stack(stale, dim=-1), tmax


def _mixed_groups(moved):
    """Share of (16-query group = one wave, tile) pairs in which some queries move their reference and others keep it."""
    B, H, Lq, T = moved.shape
    g = moved.reshape(B, H, Lq // 16, 16, T)
    return (g.any(dim=3) & ~g.all(dim=3)).double().mean().item()


@pytest.mark.parametrize("d", [40, 48, 64, 80, 160])
@pytest.mark.parametrize("L", [128, 256])
def test_self_attention_large_logits_rescale_after_the_first_tile(cuda, d, L):
    # q scaled by 6 before the bf16 rounding (logits of the size real weights produce).  d = 40: the denominator rides in the
    # accumulator through the rescale (ones column); d = 48: the same tile shape with the fp32 partial sums
    g = torch.Generator().manual_seed(1000 + d + L)
    qkv = torch.randn(2, L, 3 * 2 * d, generator=g)
    qkv[..., :2 * d] *= 6.0
    qkv = qkv.to(torch.bfloat16)
    q, k, _ = qkv.chunk(3, dim=-1)
    moved, stale, _ = _lazy_maximum_replay(q, k, 2)
    f_moved, f_stale, f_mixed = moved.double().mean().item(), stale.double().mean().item(), _mixed_groups(moved)
    print(f"[E d={d} L={L}] reference moves {f_moved:.3f}, stale {f_stale:.3f}, mixed 16-query groups {f_mixed:.3f}")
    assert f_moved >= 0.02 and f_stale >= 0.20 and f_mixed >= 0.20
    _self(f"E self d={d} L={L}", cuda, qkv, 2)


@pytest.mark.parametrize("d", [40, 48, 64, 80, 160])
def test_self_attention_staircase_of_tile_maxima(cuda, d):
    # q rows near sqrt(d) u for a unit vector u, k rows of tile t = b_t u + noise with b_t log2(e) = 0, 6, 16, 22: the log2-domain tile
    # maxima rise by +6 (inside the margin: the reference stays, probabilities up to 2^6), +10 (the reference moves by 16 under
    # an accumulator holding those probabilities), +6
    L, heads, nimg = 256, 2, 2
    g = torch.Generator().manual_seed(1100 + d)
    u = torch.randn(heads, d, generator=g)
    u = u / u.norm(dim=-1, keepdim=True)
    steps = torch.tensor([0.0, 6.0, 16.0, 22.0]) / math.log2(math.e)
    q = math.sqrt(d) * u + 0.3 * torch.randn(nimg, L, heads, d, generator=g)
    k = steps.repeat_interleave(64)[None, :, None, None] * u + 0.3 * torch.randn(nimg, L, heads, d, generator=g)
    v = torch.randn(nimg, L, heads, d, generator=g)
    qkv = torch.cat([t.reshape(nimg, L, heads * d) for t in (q, k, v)], dim=-1).to(torch.bfloat16)
    q, k, _ = qkv.chunk(3, dim=-1)
    moved, stale, tmax = _lazy_maximum_replay(q, k, heads)
    rise = (tmax[..., 1:] - tmax[..., :-1]).reshape(-1, 3).median(dim=0).values
    f_moved, f_stale = moved.double().mean(dim=(0, 1, 2)), stale.double().mean(dim=(0, 1, 2))
    print(f"[E staircase d={d}] median rises {rise.tolist()}, moved per tile {f_moved.tolist()}, stale per tile {f_stale.tolist()}")
    assert ((rise - torch.tensor([6.0, 10.0, 6.0], dtype=rise.dtype)).abs() <= 1.0).all()
    assert f_stale[0] >= 0.9 and f_moved[1] >= 0.9 and f_stale[2] >= 0.9
    _self(f"E staircase d={d}", cuda, qkv, heads)


@pytest.mark.parametrize("kind,d,heads,L,Lk", [("self", 80, 2, 100, 0), ("self", 64, 5, 192, 0), ("cross", 40, 2, 64, 65)])
def test_fp8_variant_shapes(cuda, kind, d, heads, L, Lk):
    # the check and ordering of test_ops_gpu.test_attention_fp8_variant (e4m3 keeps the exact running maximum, so N(0,1) inputs reach its rescale)
    from neurons_amd import ops
    C = heads * d
    if kind == "self":
        qkv = _randn(1200 + d, 2, L, 3 * C).to(cuda)
        q, k, v = qkv.chunk(3, dim=-1)
        call = lambda fp8: lambda o: ops.attention_self(qkv, heads, fp8=fp8, out=o)  # noqa: E731
    else:
        q, kv = _randn(1200 + d, 3, L, C).to(cuda), _randn(1300 + d, 2, Lk, 2 * C).to(cuda)
        k, v = (t.repeat_interleave(2, dim=0)[:3] for t in kv.chunk(2, dim=-1))
        call = lambda fp8: lambda o: ops.attention_cross(q, kv, heads, 2, fp8=fp8, out=o)  # noqa: E731
    ref = _ref(q, k, v, heads)
    outs = {}
    for fp8 in (True, False):
        a, b = (call(fp8)(torch.full(tuple(ref.shape), float("nan"), dtype=torch.bfloat16, device=cuda)) for _ in range(2))
        torch.cuda.synchronize()
        assert torch.isfinite(a).all() and torch.equal(_bits(a), _bits(b))
        outs[fp8] = a
    rel8 = ((outs[True].double() - ref).norm() / ref.norm()).item()
    rel16 = ((outs[False].double() - ref).norm() / ref.norm()).item()
    print(f"[E fp8 {kind} d={d} heads={heads} L={L} Lk={Lk}] rel_l2 fp8={rel8:.3e} bf16={rel16:.3e}")
    assert not torch.equal(outs[True], outs[False])
    assert rel16 < rel8 <= FP8_ATTN_REL_L2


# ---------------------------------------------------------------- F. causal
@pytest.mark.parametrize("heads,d", [(12, 64), (5, 8)])
@pytest.mark.parametrize("L", [16, 17, 33, 77, 100])
def test_causal_self_attention(cuda, heads, d, L):
    # L >= 48 without the mask would take the block-shared kernel: a causal call has to stay on the per-wave one
    from neurons_amd import ops
    qkv = _randn(1400 + d + L, 2, L, 3 * heads * d)
    out, v = _self(f"F causal heads={heads} d={d} L={L}", cuda, qkv, heads, causal=True)
    assert torch.equal(_bits(out[:, 0]), _bits(v[:, 0])), "query 0 sees key 0 only"
    plain = ops.attention_self(qkv.to(cuda), heads)
    assert not torch.equal(_bits(out[:, :-1]), _bits(plain[:, :-1])), "the causal flag changed nothing"


# ---------------------------------------------------------------- G. guard rows around the result
@pytest.mark.parametrize("mode", ["self", "self-per-wave", "causal", "cross", "temporal"])
def test_result_stays_inside_its_rows(cuda, mode):
    from neurons_amd import ops
    heads, d, slack = 2, 40, 64
    C = heads * d
    if mode == "cross":
        q, kv = _randn(1500, 3, 100, C).to(cuda), _randn(1501, 2, 77, 2 * C).to(cuda)
        k, v = (t.repeat_interleave(2, dim=0)[:3] for t in kv.chunk(2, dim=-1))
        shape, ref = (3, 100, C), _ref(q, k, v, heads)
        call = lambda o: ops.attention_cross(q, kv, heads, 2, out=o)  # noqa: E731
    elif mode == "temporal":
        qkv = _randn(1502, 2 * 17, 3, 3 * C).to(cuda)
        shape, ref = (2 * 17, 3, C), _temporal_ref(qkv, heads, 2, 17, 3)
        call = lambda o: ops.attention_temporal(qkv, heads, 17, out=o)  # noqa: E731
    else:
        L = 40 if mode == "self-per-wave" else 100
        qkv = _randn(1503, 2, L, 3 * C).to(cuda)
        q, k, v = qkv.chunk(3, dim=-1)
        shape, ref = (2, L, C), _ref(q, k, v, heads, mode == "causal")
        call = lambda o: ops.attention_self(qkv, heads, causal=mode == "causal", out=o)  # noqa: E731
    rows = shape[0] * shape[1]
    buf = torch.full((slack + rows + slack, C), float("nan"), dtype=torch.bfloat16, device=cuda)
    out = buf[slack:slack + rows].view(shape)
    call(out)
    torch.cuda.synchronize()
    _cmp(f"G {mode}", out, ref)
    assert torch.isnan(buf[:slack]).all() and torch.isnan(buf[slack + rows:]).all(), "rows outside the result were written"
