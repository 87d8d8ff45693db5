"""The weight store owns what each fused transformer kernel reads (WeightStore::X_weights): host-only, on the stand-alone stub build of
tests/sanitize/ (AddressSanitizer + UndefinedBehaviorSanitizer, a stand-in HIP runtime, its own main, nothing preloaded).

A kernel's weight stream is packed from converted matrices that only feed it; once the stream exists they are erased again, so they neither stay
resident nor travel in the exported arena (1 - 6.5 MB per block).  The names of those inputs are spelled by the converters that make them; a bundle
that named one differently would erase nothing and fail nothing.  So, on a FRESH handle of each leaf planned first at a shape that takes a fused
kernel, the export manifest must hold that kernel's stream / table and none of the stream's inputs; and after every plan of the sequence that
follows on the same handle (streams cached, inputs made again for the unfused paths, folded matrices rebuilt beside their kept vectors) the sizes of
the manifest's records must add up to the weight bytes the handle reports."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SAN = os.path.join(HERE, "sanitize")

# leaf -> (its first plan in plan_dump.cpp, (name prefix, count) that must be there, substrings of which no converted name may hold all of one tuple)
T0, T1 = "m.temporal_transformer.transformer_blocks.0.attention_blocks.0", "m.temporal_transformer.transformer_blocks.0.attention_blocks.1"
X = "m.transformer_blocks.0"
CASES = {
    "leaf_temporal": ("batch=1 frames=16 h=16 w=16 ctx=0", [("tas:", 2), ("ffs:", 1)],
                      [("lin:" + ab + w,) for ab in (T0, T1) for w in (".to_q.weight", ".to_k.weight", ".to_v.weight", ".to_out.0.weight")] + [("foldw:",), ("geglu:",)]),
    "leaf_transformer": ("batch=1 frames=2 h=48 w=48 ctx=77", [("xas:", 1), ("ffs:", 1)],
                         [("lin:" + X + ".attn2.to_q.weight",), ("lin:" + X + ".attn2.to_out.0.weight",), ("lnw:", X + ".norm2|" + X + ".attn2.to_q.weight"),
                          ("foldw:",), ("geglu:",)]),
    "leaf_temporal640": ("batch=1 frames=16 h=8 w=8 ctx=0", [("taws:", 2), ("tawe:", 2)],
                         [("lnw:", ".norms.0|" + T0 + ".to_q.weight"), ("lnw:", ".norms.1|" + T1 + ".to_q.weight")]),
    "leaf_transformer1280": ("batch=2 frames=1 h=32 w=32 ctx=77", [("xaws:", 1), ("xawt:", 1)], [("lnw:", X + ".norm2|" + X + ".attn2.to_q.weight")]),
}


def parse_plans(dump):
    """[(header, weight_bytes, {converted name: bytes})] of a plan_dump text, in order"""
    plans = []
    for line in dump.splitlines():
        tok = line.split()
        if line.startswith("== "):
            plans.append([line[3:], None, {}])
        elif line.startswith("weight_bytes:"):
            plans[-1][1] = int(tok[1])
        elif line.startswith("D ") and len(tok) == 4:
            plans[-1][2][tok[1]] = int(tok[3])
    return plans


def check_plans(plans):
    first_seen = set()
    for header, weight_bytes, recs in plans:
        net = header.split()[0]
        print(header, "weight_bytes", weight_bytes, "records", len(recs), "sum", sum(recs.values()))
        assert weight_bytes is not None and recs, header
        assert sum(recs.values()) == weight_bytes, f"{header}: the manifest's records hold {sum(recs.values())} bytes, the handle reports {weight_bytes}"
        if net in first_seen:
            continue
        first_seen.add(net)
        shape, present, absent = CASES[net]
        assert shape in header, f"the first plan of {net} must be the fused shape {shape}: {header}"
        for prefix, count in present:
            got = [n for n in recs if n.startswith(prefix)]
            assert len(got) == count, f"{header}: {count} x {prefix} expected, manifest holds {got}"
        for parts in absent:
            left = [n for n in recs if n.startswith(parts[0]) and all(p in n for p in parts[1:])]
            assert not left, f"{header}: an input of a packed weight stream stayed resident: {left}"
    assert first_seen == set(CASES), first_seen


@pytest.fixture(scope="module")
def stub_build(tmp_path_factory):
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("ROCm clang not present")
    out = str(tmp_path_factory.mktemp("build"))
    r = subprocess.run(["make", "-C", SAN, "-j4", f"OUT={out}", os.path.join(out, "plan_dump")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return out


def test_fused_kernels_keep_their_streams_and_drop_the_inputs(stub_build, tmp_path):
    schema = str(tmp_path / "schema.txt")
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "plan_schema.py"), schema], check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1",
               LSAN_OPTIONS="suppressions=" + os.path.join(SAN, "lsan.supp"))
    for k in ("NR_DETERMINISTIC_BATCH", "NR_FF_FUSED", "NR_TATTN_FUSED", "NR_XATTN_FUSED", "NR_TATTN_HEAD", "NR_XATTN_HEAD", "NR_FOLD_PROJ_OUT", "NR_LN_FUSE",
              "NR_STUB_TRACE"):
        env.pop(k, None)
    r = subprocess.run([os.path.join(stub_build, "plan_dump"), schema, ",".join(CASES)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + "\n" + r.stderr[-6000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
    plans = parse_plans(r.stdout)
    assert len(plans) >= 4 * len(CASES) - 2, "every leaf is planned at several shapes on one handle"
    check_plans(plans)
