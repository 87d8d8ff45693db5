#!/usr/bin/env bash
# Is the device code of the working tree the same as that of a git revision?  The acceptance instrument of a device-side refactor: identical
# assembly needs no timing A/B.
#
#   tools/isa_equal.sh <git-rev> [extra compile flags, e.g. -DNR_STAMP]
#
# Exports <git-rev>'s neurons_amd/csrc and include into a temporary directory (git archive: the working tree is not touched), compiles every
# kernel file of the Makefile's SRCS (all but the engine*.hip files, which are host code; FILES=engine.hip compares its two small kernels) of both trees to device-only assembly with each
# tree's own Makefile flags (CXXFLAGS, NOPK, FLAGS_<name>; read from the Makefile, not retyped here) and compares the two texts per file.
# One line per file: "identical", or "DIFFERS" and the first differing lines.  Exit status 1 if any file differs.
# The only normalisation: the per-compile __hip_cuid_<hex> symbol becomes a fixed token (two compiles of the same source differ in exactly that).
# Needs no GPU.  JOBS=<n> compiles in parallel (default 8, at most 16); FILES="a.hip b.hip" compares only those; KEEP=<dir> keeps both sets of
# assembly as <dir>/old and <dir>/new (tools/isa_kernels.py compares a file per kernel when a refactor renames or reorders its kernels).
set -euo pipefail

[ $# -ge 1 ] || { echo "usage: $0 <git-rev> [extra compile flags]" >&2; exit 2; }
rev=$1; shift
extra="$*"
jobs=${JOBS:-8}; [ "$jobs" -le 16 ] || jobs=16
root=$(git -C "$(dirname "$0")" rev-parse --show-toplevel)
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT

mkdir -p "$tmp/old" "$tmp/asm/old" "$tmp/asm/new"
git -C "$root" archive "$rev" neurons_amd/csrc include | tar -x -C "$tmp/old"

# a second makefile on top of the tree's own: prints its variables
cat > "$tmp/vars.mk" <<'EOF'
isa-srcs: ; @echo $(filter-out engine.hip engine_weights.hip engine_layers.hip engine_nets.hip engine_ops.hip,$(SRCS))
isa-flags-%: ; @echo $(CXXFLAGS) $(NOPK) $(FLAGS_$*)
isa-hipcc: ; @echo $(HIPCC)
EOF

# one compile: $1 = old | new, $2 = csrc directory, $3 = file
compile_one() {
  local name=${3%.hip} flags hipcc
  flags=$(make -s -C "$2" -f Makefile -f "$tmp/vars.mk" "isa-flags-$name")
  hipcc=$(make -s -C "$2" -f Makefile -f "$tmp/vars.mk" isa-hipcc)
  # shellcheck disable=SC2086
  (cd "$2" && $hipcc $flags $extra --offload-device-only -S "$3" -o "$tmp/asm/$1/$name.s" 2> "$tmp/asm/$1/$name.log") ||
    { echo "$1 $3: compile failed" >&2; tail -n 20 "$tmp/asm/$1/$name.log" >&2; return 1; }
  sed -E -i 's/__hip_cuid_[0-9a-f]+/__hip_cuid_X/g' "$tmp/asm/$1/$name.s"
}
export -f compile_one
export tmp extra

srcs=${FILES:-$(make -s -C "$root/neurons_amd/csrc" -f Makefile -f "$tmp/vars.mk" isa-srcs)}
for f in $srcs; do
  [ -f "$tmp/old/neurons_amd/csrc/$f" ] && printf '%s\0%s\0%s\0' old "$tmp/old/neurons_amd/csrc" "$f"
  printf '%s\0%s\0%s\0' new "$root/neurons_amd/csrc" "$f"
done | xargs -0 -n 3 -P "$jobs" bash -c 'compile_one "$@"' _

if [ -n "${KEEP:-}" ]; then mkdir -p "$KEEP" && cp -r "$tmp/asm/old" "$tmp/asm/new" "$KEEP/"; fi

echo "# device assembly of the working tree against $rev ($(git -C "$root" rev-parse --short "$rev"))${extra:+, extra flags: $extra}"
status=0
for f in $srcs; do
  name=${f%.hip}
  if [ ! -f "$tmp/asm/old/$name.s" ]; then
    echo "$f: not in $rev"; status=1
  elif cmp -s "$tmp/asm/old/$name.s" "$tmp/asm/new/$name.s"; then
    echo "$f: identical ($(wc -l < "$tmp/asm/new/$name.s") lines)"
  else
    echo "$f: DIFFERS"; status=1
    diff "$tmp/asm/old/$name.s" "$tmp/asm/new/$name.s" | head -n 12 | sed 's/^/    /' || true
  fi
done
exit $status
