"""Weight-only e4m3 storage for the small-M Linear kernel on the GPU (nr_net_set_weight_fp8 / NR_W8): the pack kernel against the torch reference
byte for byte; the e4m3 instantiations of smallm.hip against the bf16 ones run on the dequantised matrix, bit for bit (same MFMAs, same order,
same operand values: only the load and the conversion differ); one case against fp32 torch; the engine flag on a C = 1280 transformer leaf."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _dq(w):
    """dequantize(quantize(w)) of a bf16 CUDA matrix, through the host reference"""
    from neurons_amd import w8
    q, e = w8.quantize(w.cpu())
    return w8.dequantize(q, e).cuda()


@pytest.mark.parametrize("N,K", [(80, 640), (64, 1280), (1920, 2560)])
def test_pack_kernel_matches_the_torch_reference_byte_for_byte(cuda, N, K):
    from neurons_amd import ops, w8
    g = torch.Generator().manual_seed(N + K)
    w = torch.randn(N, K, generator=g) * K ** -0.5
    w[: N // 2] *= torch.logspace(-3, 1, N // 2)[:, None]      # row scales over four decades
    w[3] = 0                                                    # a zero row
    w[5, 17] = 448 * 2.0 ** -4                                  # amax / 448 a power of two (the other values of the row are far below it)
    w[5, :17] *= 1e-3
    w[5, 18:] *= 1e-3
    w = w.to(torch.bfloat16)
    codes, scale = ops.w8_pack(w.cuda())
    rcodes, rscale = w8.pack_reference(w)
    assert codes.shape == rcodes.shape and codes.dtype == torch.uint8
    assert torch.equal(codes.cpu(), rcodes)
    assert torch.equal(scale.cpu(), rscale)


CASES = [
    (1, 80, 640, "plain"),          # one chunk, NT = 5, row mask
    (33, 64, 640, "res"),           # NT = 4, second row tile ragged
    (512, 1280, 1280, "res"),       # the shipped plan, both register banks
    (100, 160, 2560, "ln"),         # 4 chunks: the streaming ring
    (64, 128, 1280, "geglu"),       # value / gate pairs, scales of both
    (96, 128, 640, "lngeglu"),      # LayerNorm + GEGLU
    (512, 1920, 640, "rv"),         # J = 2: scale index across slabs
    (40, 80, 1280, "cat"),          # two sources, 640 + 640
]


@pytest.mark.parametrize("M,N,K,kind", CASES)
def test_e4m3_kernel_equals_the_bf16_kernel_on_the_dequantised_weights(cuda, monkeypatch, M, N, K, kind):
    """NR_W8=1 on weights w against NR_W8 unset on dequantize(quantize(w)), everything else the same: torch.equal.  For the LayerNorm kinds w is the
    gamma-scaled matrix the kernel reads (the engine quantises that one), ln_c and the folded bias are those of the bf16 fold in both arms."""
    from neurons_amd import _lib, ops
    lib = _lib.load()
    monkeypatch.setenv("NR_SMALLM", "2")      # also the several-slabs-per-workgroup plan the shipped heuristic leaves to the tiled igemm
    g = torch.Generator(device="cuda").manual_seed(M * 7 + N + K)
    a = (torch.randn(M, K, generator=g, device="cuda") * 1.5 + 0.3).to(torch.bfloat16)
    w = torch.randn(N, K, generator=g, device="cuda") * K ** -0.5
    w = w * torch.logspace(-1, 1, N, device="cuda")[torch.randperm(N, generator=g, device="cuda")][:, None]      # every row its own scale
    bias = 0.1 * torch.randn(N, generator=g, device="cuda")
    gamma = 1.0 + 0.2 * torch.randn(K, generator=g, device="cuda")
    beta = 0.1 * torch.randn(K, generator=g, device="cuda")
    ln = kind in ("ln", "lngeglu")
    geglu = kind in ("geglu", "lngeglu")
    nout = N // 2 if geglu else N
    res = torch.randn(M, nout, generator=g, device="cuda").to(torch.bfloat16)
    rv = torch.randn(16, N, generator=g, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    # the matrix the kernel reads, and the LayerNorm fold beside it (ops.ln_gemm's own recipe)
    if ln:
        wk = (w * gamma[None]).to(torch.bfloat16)
        c = wk.float().sum(1)
        b = (w.double() @ beta.double()).float() + bias
        if geglu:
            wk, _ = ops.geglu_permute(wk, None)
            c, b = ops.geglu_permute(c[:, None].contiguous(), b)
        c, b = c.contiguous(), b.contiguous()
    elif geglu:
        wk, b = ops.geglu_permute(w.to(torch.bfloat16), bias)
    else:
        wk, b = w.to(torch.bfloat16), bias
    wk = wk.contiguous()

    def run(wm):
        if ln:
            out = torch.empty(M, nout, dtype=torch.bfloat16, device="cuda")
            r = None if geglu else res
            _lib.check(lib.nr_op_ln_gemm(st, a.data_ptr(), K, wm.data_ptr(), c.data_ptr(), b.data_ptr(), 1e-5, None if r is None else r.data_ptr(), nout,
                                         out.data_ptr(), nout, M, N, K, 1 if geglu else 0, 0))
            return out
        if kind == "geglu":
            return ops.gemm(a, wm, b, None, geglu=True)
        if kind == "rv":
            return ops.gemm_ex(a, wm, b, rowvec=rv, rowvec_div=4, rowvec_mod=16, res=res, act=1, out_scale=0.5)
        if kind == "cat":
            return ops.gemm2(a[:, :640].contiguous(), a[:, 640:].contiguous(), wm, b, res)
        if kind == "res":
            return ops.gemm(a, wm, b, res)
        return ops.gemm(a, wm, None, None)

    monkeypatch.delenv("NR_W8", raising=False)
    wdq = _dq(wk)
    want = run(wdq)
    bf16_on_w = run(wk)
    monkeypatch.setenv("NR_W8", "1")
    got = run(wk)
    diff = (got.float() - want.float()).abs().max().item()
    print(f"[w8 {kind} {M}x{N}x{K}] max |e4m3 - bf16 on dequantised| = {diff:.3e}; rel-L2 to the bf16 weights "
          f"{((got.float() - bf16_on_w.float()).norm() / bf16_on_w.float().norm()).item():.3e}")
    assert torch.isfinite(got.float()).all()
    assert torch.equal(got, want)
    assert not torch.equal(got, bf16_on_w), "the request did not reach an e4m3 kernel"
    for _ in range(3):
        assert torch.equal(got, run(wk))
    if kind == "ln":      # ops.ln_gemm folds the same way: the wrapper reaches the same kernel with the same operands
        assert torch.equal(got, ops.ln_gemm(a, w, gamma, beta, bias, res))
    monkeypatch.delenv("NR_W8")
    assert torch.equal(want, run(wdq))


def test_e4m3_kernel_against_fp32_torch_on_the_dequantised_weights(cuda, monkeypatch):
    from test_ops_gpu import _cmp
    from neurons_amd import ops
    M, N, K = 512, 1280, 1280
    g = torch.Generator(device="cuda").manual_seed(11)
    a = (torch.randn(M, K, generator=g, device="cuda") * 1.5 + 0.3).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g, device="cuda") * K ** -0.5).to(torch.bfloat16)
    bias = 0.1 * torch.randn(N, generator=g, device="cuda")
    res = torch.randn(M, N, generator=g, device="cuda").to(torch.bfloat16)
    ref = F.linear(a.float(), _dq(w).float(), bias) + res.float()
    monkeypatch.setenv("NR_W8", "1")
    out = ops.gemm(a, w, bias, res)
    _cmp("smallm e4m3 res 512x1280x1280", out, ref)


def _leaf_state_dict(seed, dequantised):
    """random weights of the C = 1280 Transformer3DModel leaf; dequantised: every matrix replaced by dequantize(quantize(.)) (bf16 values, so the
    engine's own bf16 conversion keeps them) and every LayerNorm gamma = 1 (the gamma-scaled matrix is then the matrix itself)"""
    from neurons_amd import w8
    from neurons_amd.synth import randn
    from neurons_amd.unet3d import _transformer_keys
    sd = {}
    for k, shape in _transformer_keys("m", 1280, 768).items():
        k = k[2:]
        z = randn(f"w8leaf.{k}", shape, seed)
        if len(shape) == 1:
            z = (1.0 + 0.1 * z) if k.endswith("weight") else 0.05 * z
            if dequantised and k.endswith("weight") and ".norm" in k and k.startswith("transformer_blocks"):
                z = torch.ones_like(z)
        else:
            z = z / (z[0].numel() ** 0.5)
            if dequantised:
                m = z.reshape(shape[0], -1).to(torch.bfloat16)
                z = w8.dequantize(*w8.quantize(m), dtype=torch.float32).reshape(shape)
        sd[k] = z
    return sd


def test_engine_flag_on_a_1280_channel_transformer_leaf(cuda):
    """b = 2, f = 16, 4 x 4: 512 rows.  ABI surface (fails on a tree without the feature), which launches name the e4m3 form, flag on == flag off on
    dequantised weights, export -> import into a fresh handle, and generic weights: finite, repeatable, and really different from bf16."""
    from neurons_amd import _lib
    from neurons_amd.ops import NativeLeaf
    from neurons_amd.synth import randn
    assert "nr_net_set_weight_fp8" in _lib.SYMBOLS and "nr_op_w8_pack" in _lib.SYMBOLS
    assert hasattr(_lib.load(), "nr_net_set_weight_fp8")
    x = randn("w8leaf.x", (2, 1280, 16, 4, 4), 1).cuda()
    ctx = randn("w8leaf.ctx", (2, 77, 768), 2).cuda()

    leaf = NativeLeaf("transformer3d", channels=1280, heads=8, cross_attention_dim=768)
    leaf.load_state_dict(_leaf_state_dict(3, True))
    y_off = leaf(x, ctx).clone()
    assert not any("e4m3" in d for d in leaf.op_descriptions())
    leaf.set_weight_fp8(True)
    y_on = leaf(x, ctx).clone()
    named = [d for d in leaf.op_descriptions() if "w=e4m3" in d]
    print("\n".join(named))
    assert any("M=512 N=1280 K=1280" in d and "res=0" in d for d in named), "proj_in"
    assert any("M=512 N=1280 K=1280" in d and "res=1" in d for d in named), "a to_out"
    assert not any("K=6400" in d for d in named), "the folded net.2 | proj_out operand is a product: it stays bf16"
    assert torch.isfinite(y_on).all()
    assert torch.equal(y_on, y_off)

    manifest, arena = leaf.export_weights()
    assert b" w8:" in manifest
    fresh = NativeLeaf("transformer3d", channels=1280, heads=8, cross_attention_dim=768)
    fresh.set_weight_fp8(True)
    fresh.import_weights(manifest, arena)
    y_imp = fresh(x, ctx)
    assert any("w=e4m3" in d for d in fresh.op_descriptions())
    assert torch.equal(y_imp, y_on)
    leaf.set_weight_fp8(False)
    assert torch.equal(leaf(x, ctx), y_off)
    assert not any("e4m3" in d for d in leaf.op_descriptions())
    del leaf, fresh

    gen = NativeLeaf("transformer3d", channels=1280, heads=8, cross_attention_dim=768)
    gen.load_state_dict(_leaf_state_dict(4, False))
    y_bf16 = gen(x, ctx).clone()
    gen.set_weight_fp8(True)
    y1 = gen(x, ctx).clone()
    y2 = gen(x, ctx).clone()
    assert torch.isfinite(y1).all()
    assert torch.equal(y1, y2)
    assert not torch.equal(y1, y_bf16)
    rel = ((y1 - y_bf16).norm() / y_bf16.norm()).item()
    print(f"[w8 leaf, generic weights] rel-L2 of the e4m3 output to the bf16 output: {rel:.3e}")
