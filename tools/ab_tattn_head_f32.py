"""Same-box A/B of the 32-frame temporal attention head kernel (tattnw.hip) at the smallest shapes the planner routes to it: the temporal module
(two Temporal_Self blocks, leaf handle = the launch sequence of the U-Net at that level) with the head kernel (default) against NR_TATTN_HEAD=0
(q|k|v GEMM + attention core).  One child process per arm and repetition (the switch is read once per process), arms interleaved; the time is the
graph replay of the whole module (GroupNorm, proj_in, 2 x attention + to_out, FeedForward + proj_out), so the DIFFERENCE is two temporal attentions.

Usage (GPU box):  python tools/ab_tattn_head_f32.py > profiles/r08_tattn_head_f32_ab.txt
"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# (C, clips, h = w): C = 1280 at its row floor (2048 rows = one 32-frame clip at 8 x 8), C = 640 at the smallest hw the rule takes (8 pixels: 256 rows)
# and at one clip of the 8 x 8 level (2048 rows)
SHAPES = ((1280, 1, 8, 8), (640, 1, 2, 4), (640, 1, 8, 8))
REPS, ITERS = 3, 300


def child(C, b, h, w):
    import torch
    from neurons_amd.ops import NativeLeaf
    from neurons_amd.synth import randn
    from neurons_amd.unet3d import _motion_keys
    from test_leaf_gpu import _fill
    leaf = NativeLeaf("temporal", channels=C, heads=8, num_attention_blocks=2, pe_max_len=32)
    leaf.load_state_dict(_fill({k[2:]: v for k, v in _motion_keys("m", C, 2).items()}, f"tm{C}f32", 81))
    x = randn("ab.x", (b, C, 32, h, w), 5).cuda()
    for _ in range(20):
        leaf(x)
    torch.cuda.synchronize()
    best = 1e9
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(ITERS):
            leaf(x)
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t0) / ITERS * 1e6)
    kinds = sorted(set(d.split(" ")[0] for d in leaf.op_descriptions() if d.startswith(("tattn_head", "attention"))))
    print(f"RESULT {best:.1f} {'+'.join(kinds)}")


def main():
    import torch
    print(f"# box: {torch.cuda.get_device_name(0)}; temporal module at 32 frames, us per graph replay (best of 3 x {ITERS}), {REPS} interleaved repetitions per arm")
    for C, b, h, w in SHAPES:
        res = {"1": [], "0": []}
        for _ in range(REPS):
            for arm in ("1", "0"):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "child", str(C), str(b), str(h), str(w)], env=dict(os.environ, NR_TATTN_HEAD=arm),
                                   capture_output=True, text=True, timeout=300)
                if r.returncode != 0:
                    print(r.stdout[-1000:], r.stderr[-2000:])
                    sys.exit(1)                          # nothing more is started on the GPU after a failed arm
                line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT")][0].split()
                res[arm].append((float(line[1]), line[2]))
        on, off = [t for t, _ in res["1"]], [t for t, _ in res["0"]]
        print(f"C={C} clips={b} hw={h * w} rows={b * 32 * h * w}: head kernel ({res['1'][0][1]}) {' '.join(f'{t:.1f}' for t in on)} | NR_TATTN_HEAD=0 ({res['0'][0][1]}) "
              f"{' '.join(f'{t:.1f}' for t in off)} | median {sorted(on)[REPS // 2]:.1f} vs {sorted(off)[REPS // 2]:.1f} us: "
              f"{(sorted(off)[REPS // 2] - sorted(on)[REPS // 2]) / 2:+.1f} us per temporal attention in favour of the head kernel", flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "child":
        child(*(int(a) for a in sys.argv[2:6]))
    else:
        main()
