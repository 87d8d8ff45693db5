"""A plan launches the GEMM route it was planned with (nr_gemm_route decides once, nr_launch_gemm reads no switch): host-only, on the stand-alone
stub build of tests/sanitize/ (AddressSanitizer + UndefinedBehaviorSanitizer, a stand-in HIP runtime whose trace lists every kernel launch).

The C = 1280 transformer leaf is planned at 1024 rows under gemm8p mode 2, so its long-K Linears (the folded FeedForward.net.2 | proj_out GEMM:
N = 1280, K = 6400) go to the ping-pong kernel and reserve no split-K scratch.  It is replayed with the graph off, then the process-wide switches
change under it -- nr_g8p_set_mode(1), under which the same shape plans the tiled kernel with split-K 4, and NR_IGEMM_FORCE -- and it is replayed
again: both replays must succeed with identical launch lines.  (Before the route existed the second replay re-derived the kernel at launch, wanted
scratch the plan never reserved and failed with launcher status 6.)"""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SAN = os.path.join(HERE, "sanitize")


def test_replay_after_the_switches_changed_launches_what_was_planned(tmp_path):
    clang = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(clang):
        pytest.skip("ROCm clang not present")
    out = str(tmp_path / "build")
    r = subprocess.run(["make", "-C", SAN, "-j4", f"OUT={out}", os.path.join(out, "plan_dump")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    schema, trace = str(tmp_path / "schema.txt"), str(tmp_path / "trace.txt")
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "plan_schema.py"), schema], check=True, timeout=300)
    env = dict(os.environ, NR_STUB_TRACE=trace, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1", LSAN_OPTIONS="suppressions=" + os.path.join(SAN, "lsan.supp"))
    for k in ("NR_DETERMINISTIC_BATCH", "NR_G8P", "NR_IGEMM_FORCE", "NR_SMALLM"):
        env.pop(k, None)
    r = subprocess.run([os.path.join(out, "plan_dump"), "--decide-once", schema], capture_output=True, text=True, timeout=300, env=env)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + "\n" + r.stderr[-6000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
    for which in ("planned", "switched", "control"):
        assert f"replay {which}: status 0" in r.stdout, r.stdout
    launches = {}
    cur = None
    for line in open(trace):
        if line.startswith("# replay "):
            cur = launches.setdefault(line.split()[2], [])
        elif line.startswith("L ") and cur is not None:
            cur.append(line)
    planned, switched, control = launches["planned"], launches["switched"], launches["control"]
    assert len(planned) > 5 and any("g8p_kernel" in ln for ln in planned), "mode 2 must plan the ping-pong kernel"
    assert not any("splitk_reduce_kernel" in ln for ln in planned)
    assert switched == planned, "a replay must launch what its plan decided, whatever the switches say now"
    # the scenario means something: planned afresh under mode 1 the same shape takes the tiled kernel with split-K
    assert any("splitk_reduce_kernel" in ln for ln in control) and not any("g8p_kernel" in ln for ln in control)
