"""GroupNorm, attention and the fused FeedForward launch what was decided when the launch was described (nr_gn_route, nr_attn_route, the wave
count the engine captures): host-only, on the stand-alone stub build of tests/sanitize/ (AddressSanitizer + UndefinedBehaviorSanitizer, a stand-in
HIP runtime whose trace lists every kernel launch).

1. The C = 320 temporal and transformer leaves are planned at 4096 rows under 8 FeedForward waves, so their plans hold ff_fused, tattn_fused /
   xattn_fused, GroupNorm and attention.  Each is replayed with the graph off, nr_ff_set_waves(4) is called under it and it is replayed again: both
   replays must show identical launch lines.  Planned afresh under 4 waves the same leaf shows the 256-thread ff_fused_kernel.  (Before the wave
   count was captured the launcher read the process-wide setting: the second replay ran the 4-wave kernel.)
2. For GroupNorm shapes that reach every form (slab, small image, chunked in 2 and in 3 launches) the route's kernel count is the number of kernels
   its launcher really enqueues, and its scratch size is what the engine has always reserved: nimg * (nchunk + 1) * groups * 2 floats, nchunk from
   the chunking rule of norm.hip, restated below."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SAN = os.path.join(HERE, "sanitize")


@pytest.fixture(scope="module")
def stub_build(tmp_path_factory):
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("ROCm clang not present")
    out = str(tmp_path_factory.mktemp("build"))
    r = subprocess.run(["make", "-C", SAN, "-j4", f"OUT={out}", os.path.join(out, "plan_dump"), os.path.join(out, "gn_route")], capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return out


def _run(cmd, trace):
    env = dict(os.environ, NR_STUB_TRACE=trace, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1", LSAN_OPTIONS="suppressions=" + os.path.join(SAN, "lsan.supp"))
    for k in ("NR_DETERMINISTIC_BATCH", "NR_FF_WAVES", "NR_FF_FUSED", "NR_TATTN_FUSED", "NR_XATTN_FUSED", "NR_GN_SLAB", "NR_GN_T", "NR_GN_SMALL",
              "NR_ATTN_ROWSUM"):
        env.pop(k, None)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + "\n" + r.stderr[-6000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
    return r.stdout


def _sections(trace, prefix):
    """launch lines of the trace behind each '# <prefix> <key...>' note, by key"""
    sections, cur = {}, None
    for line in open(trace):
        if line.startswith("# "):
            cur = sections.setdefault(line[2:].strip()[len(prefix):].strip(), []) if line[2:].startswith(prefix) else None
        elif line.startswith("L ") and cur is not None:
            cur.append(line)
    return sections


def test_replay_after_ff_set_waves_launches_what_was_planned(stub_build, tmp_path):
    schema, trace = str(tmp_path / "schema.txt"), str(tmp_path / "trace.txt")
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "plan_schema.py"), schema], check=True, timeout=300)
    out = _run([os.path.join(stub_build, "plan_dump"), "--ff-waves", schema], trace)
    replays = _sections(trace, "replay")
    for leaf in ("leaf_temporal", "leaf_transformer"):
        for which in ("planned", "switched", "control"):
            assert f"replay {which} {leaf}: status 0" in out, out
        planned, switched, control = (replays[f"{w} {leaf}"] for w in ("planned", "switched", "control"))
        ff = [ln for ln in planned if "ff_fused_kernel" in ln]
        assert len(ff) == 1 and " 512,1,1 " in ff[0], "planned under 8 waves: the 512-thread kernel"
        assert switched == planned, "a replay must launch what its plan decided, whatever nr_ff_set_waves says now"
        # the scenario means something: planned afresh under 4 waves the same leaf takes the 256-thread form
        ff4 = [ln for ln in control if "ff_fused_kernel" in ln]
        assert len(ff4) == 1 and " 256,1,1 " in ff4[0], control
    names = "".join(replays["planned leaf_temporal"] + replays["planned leaf_transformer"])
    for k in ("ff_fused_kernel", "tattn_fused_kernel", "xattn_fused_kernel", "gn_", "attn_fwd"):
        assert k in names, f"the plans must contain {k}"


def _reserved_floats(nimg, hw, groups, plan_nimg):
    """what nr_net::groupnorm has always reserved (the chunking rule of norm.hip, made for one clip's images under deterministic batching)"""
    pn = plan_nimg if 0 < plan_nimg < nimg else nimg
    ppb = min(max((hw + 15) // 16, 8), 128, hw)
    while ppb > 2 and pn * ((hw + ppb - 1) // ppb) < 256:
        ppb = (ppb + 1) // 2
    nchunk = (hw + ppb - 1) // ppb
    return nimg * (nchunk * groups * 2 + groups * 2)


# (nimg, hw, C, plan_nimg), 32 groups: slab | small image | chunked, 2 launches | chunked with finalize, 3 launches | a deeper slab | too many pixels for a
# slab | a wider small image | deterministic batching, 64 images planned as 2: chunked, finer chunks than 64 images need (3 launches against 2) | and a slab
GN_SHAPES = [(2, 256, 320, 0), (2, 64, 320, 0), (32, 128, 64, 0), (1, 1024, 64, 0), (2, 1024, 320, 0), (2, 4096, 320, 0), (1, 64, 2560, 0), (64, 128, 64, 2),
             (64, 128, 64, 0), (64, 256, 320, 2)]


def test_groupnorm_route_agrees_with_its_launcher(stub_build, tmp_path):
    trace = str(tmp_path / "trace.txt")
    out = _run([os.path.join(stub_build, "gn_route")] + [str(v) for s in GN_SHAPES for v in s], trace)
    launched = _sections(trace, "shape")
    forms = set()
    for nimg, hw, C, plan_nimg in GN_SHAPES:
        key = f"{nimg} {hw} {C} {plan_nimg}"
        line = next(ln for ln in out.splitlines() if ln.startswith(f"shape {key}:")).split()
        status, launches, ws_floats = int(line[line.index("status") + 1]), int(line[line.index("launches") + 1]), int(line[line.index("ws_floats") + 1])
        names = [ln.split()[1] for ln in launched[key]]
        print(key, status, launches, ws_floats, names)
        assert status == 0
        assert launches == len(names), f"{key}: the route counts {launches} kernels, the launcher enqueued {names}"
        assert ws_floats == _reserved_floats(nimg, hw, 32, plan_nimg), key
        if any("gn_slab_kernel" in n for n in names):
            forms.add("slab")
        elif any("gn_fused_small_kernel" in n for n in names):
            forms.add("small")
        else:
            assert any("gn_stats_kernel" in n for n in names) and any("gn_apply_kernel" in n for n in names), names
            forms.add("chunked3" if any("gn_finalize_kernel" in n for n in names) else "chunked2")
            assert len(names) == (3 if "gn_finalize_kernel" in "".join(names) else 2)
    assert forms == {"slab", "small", "chunked2", "chunked3"}, forms
    assert len(launched["64 128 64 2"]) == 3 and len(launched["64 128 64 0"]) == 2, "plan_nimg must enter the chunking"
