"""The tiled igemm's table of instantiations is the truth (gemm.hip: TILES): host-only, on the stand-alone stub build of tests/sanitize/
(AddressSanitizer + UndefinedBehaviorSanitizer, a stand-in HIP runtime whose trace lists every kernel launch).

`plan_dump --force-sweep` calls the op hook of every request kind (Linear, GEGLU Linear, LayerNorm-folded Linear plain and GEGLU, 3x3 conv, two-source
3x3 conv, phase-form upsample conv) under every NR_IGEMM_FORCE string of bm {64, 128, 256} x bn {32, 64, 128, 160} x stages 2 .. 8 x waves
{-1, 4, 8, 41} and notes the route's tiled plan in front of the launch lines.  For every call: the hook succeeds; exactly one igemm_bf16_kernel is
launched (plus the split-K reduce when the plan has slices); the template arguments in the traced kernel name ARE the noted plan (tile, wave grid,
ring depth, adma, lin, LayerNorm-folded, phase), so the launcher rewrites nothing; the plan is a row and a ring of the literal copy of the table
below for the request's form; the LDS bytes are the table's formula.  And the sweep reaches every row and ring of the table.

One exception to "reaches every ring", with its reason: the LayerNorm-folded kernels of the 64 x 32 tile are instantiated (a hand-made NrGemmRoute can
launch them) but nr_gemm_route widens bn = 32 to 64 for the folded form (every n-tile recomputes the row statistics), so no hook call arrives there."""
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SAN = os.path.join(HERE, "sanitize")

# (bm, bn, wgm, wgn): (ring depths of the conv / Linear forms, of the LayerNorm-folded form, phase form at depth 2)
TABLE = {
    (256, 160, 2, 2): ({2, 3}, set(), False),
    (256, 128, 2, 2): ({2, 3}, set(), False),
    (256, 128, 4, 2): ({2, 3}, set(), True),
    (128, 160, 4, 1): ({3, 4}, {3, 4}, False),      # row-wave: TiledPlan::waves == 41
    (128, 160, 2, 2): ({2, 3, 4}, set(), True),
    (128, 128, 2, 4): ({2, 3, 4}, {2}, True),
    (128, 128, 2, 2): ({2, 3, 4}, {2}, False),
    (128, 64, 4, 2): ({2, 3, 4}, {2, 4}, False),
    (128, 64, 2, 2): ({2, 3, 4}, {2, 4}, True),
    (64, 160, 2, 2): ({2, 3, 4}, {2, 3}, False),
    (64, 64, 2, 2): ({2, 3, 4, 6, 8}, {2, 4}, True),
    (64, 32, 2, 2): ({2, 3, 4, 6, 8}, {2, 4}, False),
}
LN_UNROUTED = {((64, 32, 2, 2), 2), ((64, 32, 2, 2), 4)}      # see the module text
LN_KINDS = {"ln_linear", "ln_geglu"}
PHASE_KIND = "conv3x3_ups_phase"
KINDS = {"linear", "geglu", "conv3x3", "conv3x3_2src", PHASE_KIND} | LN_KINDS
CU_LDS = 160 * 1024


def lds_bytes(row, ns, ln):
    bm, bn, _, wgn = row
    return ns * (bm + bn) * 128 + (2 * wgn * bm * 4 if ln else 0)


def test_the_literal_table_fits_a_cu():
    for row, (rings, ln_rings, _) in TABLE.items():
        assert ln_rings <= rings, row
        assert all(lds_bytes(row, ns, False) <= CU_LDS for ns in rings) and all(lds_bytes(row, ns, True) <= CU_LDS for ns in ln_rings), row
    # per ring {builtin DMA, ADMA}, up to 4 deep also {LIN} of each; one kernel per LayerNorm ring; two per phase tile
    assert sum(sum(4 if ns <= 4 else 2 for ns in r) + len(ln) + 2 * ph for r, ln, ph in TABLE.values()) == 160


def test_every_forced_plan_launches_the_instantiation_the_route_names(tmp_path):
    clang = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(clang):
        pytest.skip("ROCm clang not present")
    out = str(tmp_path / "build")
    r = subprocess.run(["make", "-C", SAN, "-j4", f"OUT={out}", os.path.join(out, "plan_dump")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    trace = str(tmp_path / "trace.txt")
    env = dict(os.environ, NR_STUB_TRACE=trace, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1", LSAN_OPTIONS="suppressions=" + os.path.join(SAN, "lsan.supp"))
    for k in list(env):
        if k.startswith(("NR_IGEMM_", "NR_SMALLM", "NR_G8P", "NR_W8", "NR_DETERMINISTIC_BATCH", "NR_LIN160", "NR_ROWPANEL")):
            del env[k]
    r = subprocess.run([os.path.join(out, "plan_dump"), "--force-sweep"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + "\n" + r.stderr[-6000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]

    calls = []          # (note fields, lines that follow)
    for line in open(trace):
        if line.startswith("# route "):
            words = line.split()
            calls.append((dict(w.split("=", 1) for w in words[3:]) | {"kind": words[2]}, []))
        elif calls and (line.startswith("L ") or line.startswith("# status")):
            calls[-1][1].append(line.strip())
    assert len(calls) == 3 * 4 * 7 * 4 * len(KINDS) and {c[0]["kind"] for c in calls} == KINDS
    assert any(int(c[0]["splitk"]) > 1 for c in calls), "the sweep has a split-K plan, so the reduce launch is checked too"

    reached = {"plain": set(), "ln": set(), "phase": set()}
    for note, lines in calls:
        what = f"{note} -> {lines}"
        kind, ln, phase = note["kind"], note["kind"] in LN_KINDS, note["kind"] == PHASE_KIND
        assert note["status"] == "0" and note["class"] == "tiled" and not any(ln_.startswith("# status") for ln_ in lines), what
        plan = {k: int(note[k]) for k in ("bm", "bn", "splitk", "stages", "waves", "adma", "lin")}
        kernels = [ln_.split() for ln_ in lines]
        igemm = [k for k in kernels if "igemm_bf16_kernel" in k[1]]
        reduce_ = [k for k in kernels if "splitk_reduce_kernel" in k[1]]
        assert len(igemm) == 1 and len(reduce_) == (1 if plan["splitk"] > 1 else 0) and len(kernels) == len(igemm) + len(reduce_), what
        m = re.search(r"igemm_bf16_kernelI((?:L[ib]\d+E){9})E", igemm[0][1])
        assert m, what
        bm, bn, ns, wgm, wgn, lnf, adma, lin, ph = (int(v) for v in re.findall(r"L[ib](\d+)E", m.group(1)))
        assert (bm, bn, ns, 41 if wgn == 1 else wgm * wgn, adma, lin) == tuple(plan[k] for k in ("bm", "bn", "stages", "waves", "adma", "lin")), what
        assert (lnf, ph) == (int(ln), int(phase)), what
        row = (bm, bn, wgm, wgn)
        assert row in TABLE, what
        rings, ln_rings, has_phase = TABLE[row]
        assert ns in (ln_rings if ln else rings) and (not phase or (has_phase and ns == 2)), what
        assert int(igemm[0][4]) == lds_bytes(row, ns, ln) and igemm[0][3] == f"{64 * wgm * wgn},1,1", what
        reached["ln" if ln else "phase" if phase else "plain"].add((row, ns))

    assert reached["plain"] == {(row, ns) for row, (rings, _, _) in TABLE.items() for ns in rings}
    assert reached["ln"] == {(row, ns) for row, (_, ln_rings, _) in TABLE.items() for ns in ln_rings} - LN_UNROUTED
    assert reached["phase"] == {(row, 2) for row, (_, _, ph) in TABLE.items() if ph}
