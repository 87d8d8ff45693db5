"""CPU-only: the routing rule of the temporal attention head kernel (tattnw.hip) at 32 frames (BASELINE config 5).

``nr_tattnw_eligible(C, heads, frames, hw, rows)`` is the one place the engine asks whether a temporal attention of the C = 640 / 1280 levels runs on
the head kernel; it makes no GPU call, so the rule is checked here on the loaded library.  The launch PLAN at 32 frames (description strings, the
16 -> 32 -> 16 -> ineligible re-plans, the per-frame-count table cache) is dry-run on the CPU in tests/test_tattn_head_f32_planner_host.py, and asserted
again on the GPU in tests/test_tattn_head_f32_gpu.py."""
import ctypes
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

from neurons_amd import _lib  # noqa: E402


def _rule():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    rule = lib.nr_tattnw_eligible
    rule.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_longlong]
    rule.restype = ctypes.c_int
    return rule


def test_head_kernel_rule_accepts_32_frames_under_the_rules_of_16():
    if os.environ.get("NR_TATTN_HEAD", "")[:1] == "0":      # the switch is read once per process: ask a child without it
        env = {k: v for k, v in os.environ.items() if k != "NR_TATTN_HEAD"}
        r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", __file__, "-k", "accepts_32_frames"], env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return
    rule = _rule()
    for frames in (16, 32):
        for b in (1, 2, 8):
            assert rule(640, 8, frames, 64, frames * 64 * b) != 0, (frames, b)        # C = 640: no row floor
        assert rule(640, 8, frames, 8, frames * 8) != 0, frames
        assert rule(640, 8, frames, 256, 2 * frames * 256) != 0, frames
        assert rule(1280, 8, frames, 64, 2048) != 0, frames                          # C = 1280: from 2048 rows of one launch
        assert rule(1280, 8, frames, 64, 2 * frames * 64) != 0, frames
        assert rule(1280, 8, frames, 16, 512) == 0, frames                           # below the floor
        assert rule(1280, 8, frames, 64, 2047) == 0, frames
        assert rule(640, 8, frames, 12, frames * 12) == 0, frames                    # hw not a multiple of 8
        assert rule(640, 8, frames, 60, frames * 60) == 0, frames
        for heads in (1, 4, 5, 10, 16, 20):
            assert rule(640, heads, frames, 64, frames * 64) == 0, (frames, heads)
            assert rule(1280, heads, frames, 64, 4096) == 0, (frames, heads)
        for C in (320, 64, 128, 960, 2560):
            assert rule(C, 8, frames, 64, 8192) == 0, (frames, C)
    for frames in (1, 8, 15, 17, 24, 31, 33, 48, 64):
        assert rule(640, 8, frames, 64, frames * 64 * 2) == 0, frames
        assert rule(1280, 8, frames, 64, 8192) == 0, frames


def test_head_kernel_switch_turns_32_frames_off_too():
    code = ("import ctypes, sys; sys.path.insert(0, %r); from neurons_amd import _lib; lib = ctypes.CDLL(_lib.LIB_PATH); r = lib.nr_tattnw_eligible; "
            "r.argtypes = [ctypes.c_int] * 4 + [ctypes.c_longlong]; r.restype = ctypes.c_int; "
            "print('rule', r(640, 8, 32, 64, 4096), r(1280, 8, 32, 64, 4096), r(640, 8, 16, 64, 2048), r(1280, 8, 16, 64, 2048))" % ROOT)
    for value, want in (("0", "rule 0 0 0 0"), ("1", "rule 1 1 1 1")):
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, NR_TATTN_HEAD=value), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        assert want in r.stdout, (value, r.stdout)
