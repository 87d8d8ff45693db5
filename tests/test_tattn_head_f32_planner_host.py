"""CPU-only: the PLANNER at 32 frames on the C = 640 / 1280 temporal leaves, dry-run under AddressSanitizer + UndefinedBehaviorSanitizer.

The route of tests/test_sanitize_host.py: the engine compiled host-only against tests/sanitize/hip_stub.cpp (device memory is host heap memory, kernel
launches are no-ops), here with the driver tests/sanitize/planner_f32.cpp and a schema of its own (temporal_position_encoding_max_len = 32).  The driver
plans one C = 640 handle at 16 -> 32 -> 16 -> 24 (not eligible) -> 32 frames and asserts per plan the ``tattn_head M=... C=640 F=<frames>`` descriptions,
that the 32-frame plan has no q|k|v GEMM and no attention core, that a re-plan 16 -> 32 adds exactly one two-part epilogue table per block beside the
shared weight stream (the table is cached per frame count), that a reloaded to_q drops both tables; the C = 1280 row floor at 32 frames; and that a re-plan
to an ineligible frame count after nr_net_release_host_weights gives the same status at 32 frames as at 16."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
SAN = os.path.join(HERE, "sanitize")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
SAN_FLAGS = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
SRCS = "gemm gemm8p smallm lin160 rowpanel ffpanel tattn tattnw xattn xattnw norm attention elementwise sampler engine engine_weights engine_layers engine_nets engine_ops".split()    # tests/sanitize/Makefile


def _write_schema(path):
    from neurons_amd import _lib
    from neurons_amd.unet3d import _motion_keys
    from test_sanitize_host import _cfg_words
    with open(path, "w") as f:
        for width in (640, 1280):
            c = _lib.NrNetConfig()
            c.kind = _lib.NR_KIND_LEAF_TEMPORAL
            c.in_channels = c.out_channels = width
            c.num_levels = 1
            c.block_out_channels[0] = width
            c.num_heads, c.cross_attention_dim, c.norm_num_groups, c.norm_eps = 8, 768, 32, 1e-5
            c.use_motion_module, c.motion_num_heads, c.motion_num_attention_blocks, c.motion_pe_max_len = 1, 8, 2, 32
            f.write(f"N leaf_temporal{width}_pe32 " + " ".join(str(w) for w in _cfg_words(c)) + "\n")
            for k, shape in _motion_keys("m", width, 2).items():
                f.write(f"T {k} {len(shape)} " + " ".join(str(int(d)) for d in shape) + "\n")


def test_planner_at_32_frames_head_kernel_plans_tables_and_replans_under_asan_ubsan(tmp_path):
    if not os.path.exists(CLANG):
        pytest.skip("ROCm clang not present")
    out = str(tmp_path / "build")
    r = subprocess.run(["make", "-C", SAN, "-j4", f"OUT={out}"], capture_output=True, text=True, timeout=900)       # the engine's objects + hip_stub.o
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    objs = [os.path.join(out, s + ".o") for s in SRCS]
    drv = os.path.join(out, "planner_f32.o")
    r = subprocess.run([CLANG, "-O1", "-g", "-std=c++20", *SAN_FLAGS, "-I" + os.path.join(ROOT, "include"), "-c", os.path.join(SAN, "planner_f32.cpp"), "-o", drv],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    # the device code objects the host objects refer to do not exist in a host-only build: define their symbols as 0, as the Makefile does
    nm = subprocess.run(["nm", *objs], capture_output=True, text=True, check=True).stdout
    fatbins = sorted({ln.split()[-1] for ln in nm.splitlines() if " U __hip_fatbin_" in ln})
    exe = os.path.join(out, "planner_f32")
    r = subprocess.run([CLANG, *SAN_FLAGS, "-o", exe, *objs, os.path.join(out, "hip_stub.o"), drv, *[f"-Wl,--defsym,{s}=0" for s in fatbins]],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    schema = str(tmp_path / "schema_f32.txt")
    _write_schema(schema)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1",
               LSAN_OPTIONS="suppressions=" + os.path.join(SAN, "lsan.supp"))
    for k in ("NR_DETERMINISTIC_BATCH", "NR_TATTN_HEAD"):
        env.pop(k, None)
    r = subprocess.run([exe, schema], capture_output=True, text=True, timeout=900, env=env)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + "\n" + r.stderr[-6000:]
    assert "planner f32 dry-run OK" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
