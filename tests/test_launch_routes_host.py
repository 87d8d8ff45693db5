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


def test_groupnorm_case_table_reaches_every_instantiation(stub_build, tmp_path):
    """The GroupNorm cases of tests/test_norm_gpu.py (tests/norm_cases.py), routed and launched under the stub: each case takes the form its table
    entry names, and together they launch every kernel nr_launch_groupnorm can launch at 512 threads: the slab at 2 .. 32 chunks per thread and
    1 / 2 / 4 / 8 groups per workgroup, in both block orders; the three small-image kernels; the chunked form with and without gn_finalize, with
    several pixel lanes and with one.  (The 1024-thread slab and the NR_GN_* bisect switches are read once per process from the environment: not here.)"""
    import re
    sys.path.insert(0, HERE)
    from norm_cases import GN_CASES
    trace = str(tmp_path / "trace.txt")
    out = _run([os.path.join(stub_build, "gn_route"), "--c1-groups"] + [str(v) for c in GN_CASES for v in (c.nimg, c.hw, c.c0, 0, c.c1, c.groups)], trace)
    launched = _sections(trace, "shape")
    slab_nv, slab_gs, slab_order, small, chunked, lanes = set(), set(), set(), set(), set(), set()
    for c in GN_CASES:
        key = f"{c.nimg} {c.hw} {c.c0} 0 {c.c1} {c.groups}"
        line = next(ln for ln in out.splitlines() if ln.startswith(f"shape {key}:")).split()
        assert int(line[line.index("status") + 1]) == 0, key
        C = c.c0 + c.c1
        ls = [ln.split() for ln in launched[key]][:int(line[line.index("launches") + 1])]      # two cases share a shape: the first launch of each is the same
        names = [f[1] for f in ls]
        grid, block, lds = [int(v) for v in ls[0][2].split(",")], [int(v) for v in ls[0][3].split(",")], int(ls[0][4])
        want = c.form
        print(key, names, grid, block, lds, want)
        if (m := re.search(r"gn_slab_kernelILi(\d+)ELi(\d+)EE", names[0])):
            nv, threads = int(m.group(1)), int(m.group(2))
            assert want["kind"] == "slab" and len(names) == 1 and threads == 512 and block == [512, 1, 1] and grid[1:] == [1, 1], key
            assert (c.nimg * c.groups) % grid[0] == 0, key
            gs = c.nimg * c.groups // grid[0]      # grid = nimg * (groups / GS)
            cpp = gs * (C // c.groups) // 8
            assert (gs * (C // c.groups)) % 8 == 0 and 1 <= cpp <= 64 and -(-c.hw // (512 // cpp)) <= nv, f"{key}: the slab must hold the image"
            assert nv == want.get("nv", nv) and gs == want.get("gs", gs) and grid[0] == want.get("grid", grid[0]), (key, nv, gs, grid)
            slab_nv.add(nv); slab_gs.add(gs); slab_order.add("remapped" if grid[0] % 8 == 0 else "plain")
        elif (m := re.search(r"gn_fused_small_kernelILi(\d+)EE", names[0])):
            maxp = int(m.group(1))
            assert want["kind"] == "small" and len(names) == 1 and grid == [c.groups, c.nimg, 1] and block == [256, 1, 1], key
            assert c.hw * (C // c.groups // 2) <= 256 * maxp and maxp == want.get("maxp", maxp), (key, maxp)
            small.add(maxp)
        else:
            assert "gn_stats_kernel" in names[0] and "gn_apply_kernel" in names[-1] and block == [256, 1, 1], (key, names)
            kind = "chunked3" if len(names) == 3 else "chunked2"
            assert want["kind"] == kind and (len(names) == 2 or "gn_finalize_kernel" in names[1]), (key, names)
            pl = lds // (2 * C * 4)                 # gn_stats_kernel's dynamic LDS: 2 * PL * C floats
            assert lds == 2 * pl * C * 4 and pl == (256 // (C // 8) if C // 8 <= 256 else 1) and (pl == 1) == bool(want.get("pl1")), (key, lds)
            chunked.add(kind); lanes.add("one" if pl == 1 else "many")
    assert slab_nv == {2, 4, 8, 12, 16, 24, 32}, slab_nv
    assert slab_gs == {1, 2, 4, 8}, slab_gs
    assert slab_order == {"remapped", "plain"}, slab_order
    assert small == {8, 16, 48}, small
    assert chunked == {"chunked2", "chunked3"} and lanes == {"one", "many"}, (chunked, lanes)
