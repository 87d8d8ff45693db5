"""Every row of the tiled igemm's table of instantiations (gemm.hip: TILES) computes a GEMM: one ops.gemm call per row under the NR_IGEMM_FORCE
string that names it (the route reads the variable per call), against the fp32 torch reference with the helper and tolerances of
tests/test_ops_gpu.py::test_gemm_bias_res / ::test_gemm_geglu.  Ring depth 2 for the eleven regular tiles, 3 for the row-wave tile.
M = 300, N = 352, K = 256: a row tail for 64 / 128 / 256-row tiles, a column tail for every bn, four k-tiles; too few rows and the wrong K for the
other four GEMM classes.  The row-wave tile can only be forced for a GEGLU projection: N = 640 there, bias only (the GEGLU epilogue has no residual).
That the forced string arrives at the instantiation it names is tests/test_igemm_table_host.py's subject.  The other forms of the kernel (conv,
two sources, ADMA, deeper rings, LayerNorm-folded, phase, split-K, tile orders) are computed bit-exactly in tests/test_igemm_forms_gpu.py."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_ops_gpu import _bf, _cmp  # noqa: E402

M, N, K = 300, 352, 256
# (bm, bn, waves of TiledPlan: 41 = 4 x 1 row waves)
ROWS = [(256, 160, 4), (256, 128, 4), (256, 128, 8), (128, 160, 41), (128, 160, 4), (128, 128, 8), (128, 128, 4), (128, 64, 8), (128, 64, 4),
        (64, 160, 4), (64, 64, 4), (64, 32, 4)]


@pytest.fixture(scope="module")
def operands(cuda):
    torch.manual_seed(0)
    a, w, bias, res = _bf(M, K), _bf(N, K, scale=K ** -0.5), torch.randn(N, device=cuda), _bf(M, N)
    wg, bg = _bf(640, K, scale=K ** -0.5), torch.randn(640, device=cuda) * 0.1
    h = a.float() @ wg.float().t() + bg
    val, gate = h.chunk(2, dim=-1)
    return dict(a=a, w=w, bias=bias, res=res, ref=a.float() @ w.float().t() + bias + res.float(), wg=wg, bg=bg, ref_geglu=val * F.gelu(gate))


@pytest.mark.parametrize("bm,bn,waves", ROWS)
def test_forced_table_row_matches_torch(operands, monkeypatch, bm, bn, waves):
    from neurons_amd import ops
    o = operands
    monkeypatch.setenv("NR_IGEMM_FORCE", f"{bm},{bn},-1,{3 if waves == 41 else 2},-1,{waves}")
    if waves == 41:
        wp, bp = ops.geglu_permute(o["wg"], o["bg"])
        _cmp(f"geglu row-wave {bm}x{bn}", ops.gemm(o["a"], wp, bp, geglu=True), o["ref_geglu"])
    else:
        _cmp(f"gemm {bm}x{bn} waves {waves}", ops.gemm(o["a"], o["w"], o["bias"], o["res"]), o["ref"])
