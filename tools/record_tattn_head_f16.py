"""Recording of the 16-frame temporal attention head kernel (tattnw.hip) at C = 640 -> tests/golden/tattn_head_f16_c640.npz.

The regression guard of "the 32-frame form changes nothing at 16 frames": run this on the commit BEFORE a change to tattnw.hip (GPU box), commit the
file, and tests/test_tattn_head_f32_gpu.py asserts that the kernel still returns these bits.  Inputs come from the Philox recipe
(``neurons_amd.synth.randn``: the same numbers on every machine), so the file holds the OUTPUT only (bf16 bit patterns as uint16).

Usage (GPU box):  python tools/record_tattn_head_f16.py [output path]
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

C, NBATCH, HW, FRAMES = 640, 2, 8, 16          # 256 rows: two pixel groups, the "head h on XCD h" workgroup mapping


def inputs(device):
    """the seeded operands of the recording (shared with the test)"""
    from neurons_amd.synth import randn
    t = (randn("tah16.t", (NBATCH * FRAMES * HW, C), 101) * 1.1 + 0.1).to(torch.bfloat16).to(device)
    gamma = (1.0 + 0.2 * randn("tah16.gamma", (C,), 102)).to(device)
    beta = (0.1 * randn("tah16.beta", (C,), 103)).to(device)
    wq, wk, wv = ((randn(f"tah16.w{n}", (C, C), 104 + i) * C ** -0.5).to(device) for i, n in enumerate("qkv"))
    return t, gamma, beta, wq * 2.0, wk, wv


def main(path):
    from neurons_amd import ops
    t, gamma, beta, wq, wk, wv = inputs(torch.device("cuda", 0))
    a = ops.tattn_head(t, NBATCH, HW, gamma, beta, wq, wk, wv)
    torch.cuda.synchronize()
    assert torch.isfinite(a.float()).all()
    np.savez_compressed(path, a=a.view(torch.int16).cpu().numpy().view(np.uint16), shape=np.array(a.shape))
    print(path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "tattn_head_f16_c640.npz"))
