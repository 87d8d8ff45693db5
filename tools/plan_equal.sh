#!/usr/bin/env bash
# Does the working tree's engine plan what a git revision's engine plans?  The acceptance instrument of a host-side engine refactor: the same
# op list, workspace, converted weights (names, sizes, bytes) and kernel launches need no GPU A/B.
#
#   tools/plan_equal.sh <git-rev>
#
# Exports <git-rev>'s neurons_amd/csrc and include into a temporary directory (git archive: the working tree is not touched), builds both trees
# host-only and without a sanitizer against the WORKING TREE's stand-in HIP runtime (tests/sanitize/hip_stub.cpp) and plan-dump driver
# (tests/sanitize/plan_dump.cpp), runs both on the schema of tools/plan_schema.py and compares, per run, the driver's dump (op descriptions,
# workspace and weight bytes, export manifest) and the stub's trace (every kernel launch with grid / block / LDS bytes, every device allocation,
# size and hash of every uploaded weight).  Runs: every network at its listed shapes, then the C = 320 leaf modules once per planner switch that a
# process reads once (NR_LN_FUSE=0, NR_FOLD_PROJ_OUT=0, NR_SMALLM=0), then the networks with GEMM-heavy plans once per switch of the GEMM route (NR_G8P=0 / 2,
# NR_ROWPANEL=0, NR_LIN160=0, one NR_IGEMM_FORCE setting), then once per switch of the GroupNorm and attention routes (NR_GN_SLAB=0, NR_GN_SMALL=0,
# NR_GN_T=1024, NR_ATTN_ROWSUM=adds), of the fused FeedForward (NR_FF_WAVES=4, NR_FF_FUSED=0) and of the fused attention blocks (NR_TATTN_FUSED=0,
# NR_XATTN_FUSED=0, NR_TATTN_HEAD=0, NR_XATTN_HEAD=0) on the networks whose plans contain those kernels, then the op hooks (plan_dump --ops: the whole trace) and the
# NR_IGEMM_FORCE sweep of the tiled igemm (plan_dump --force-sweep: the launch lines only; the route notes between them are counted).  One line per run: "identical", or "DIFFERS" and the first differing lines.
# The dump must also contain every kernel class the planner can choose (a shape list that loses one is no evidence).  Exit status 1 on any of it.
# DIFF_LINES=<n> prints the first n lines of every differing run instead of 12.
# The only normalisation: pointer values (0x...) become a fixed token.  Needs no GPU.  JOBS=<n> compiles in parallel (default 8, at most 16).
set -euo pipefail

[ $# -eq 1 ] || { echo "usage: $0 <git-rev>" >&2; exit 2; }
rev=$1
jobs=${JOBS:-8}; [ "$jobs" -le 16 ] || jobs=16
difflines=${DIFF_LINES:-12}      # lines of each differing run that are printed (DIFF_LINES=1000000: the whole diff list)
root=$(git -C "$(dirname "$0")" rev-parse --show-toplevel)
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT

mkdir -p "$tmp/old"
git -C "$root" archive "$rev" neurons_amd/csrc include | tar -x -C "$tmp/old"
python "$root/tools/plan_schema.py" "$tmp/schema.txt"

# one tree: $1 = old | new, $2 = its root
build_one() {
  local srcs
  srcs=$(cd "$2/neurons_amd/csrc" && ls ./*.hip | sed -e 's|^\./||' -e 's|\.hip$||' | tr '\n' ' ')
  make -s -C "$root/tests/sanitize" -j"$jobs" SAN= OUT="$tmp/$1/build" SRC="$2/neurons_amd/csrc" INC="$2/include" SRCS="$srcs" "$tmp/$1/build/plan_dump" \
    > "$tmp/$1.build.log" 2>&1 || { echo "$1: build failed" >&2; tail -n 30 "$tmp/$1.build.log" >&2; exit 1; }
}
build_one old "$tmp/old"
build_one new "$root"

# one run of both trees: $1 = label, $2 = networks ("" = all), rest = environment
run_both() {
  local label=$1 only=$2 t; shift 2
  for t in old new; do
    env -u NR_DETERMINISTIC_BATCH "$@" NR_STUB_TRACE="$tmp/$t.$label.trace" "$tmp/$t/build/plan_dump" "$tmp/schema.txt" $only > "$tmp/$t.$label.dump" ||
      { echo "$t $label: plan_dump failed" >&2; exit 1; }
    sed -E -i 's/0x[0-9a-f]+/PTR/g' "$tmp/$t.$label.dump" "$tmp/$t.$label.trace"
  done
}
run_both default ""
run_both ln_fuse_0 leaf_transformer,leaf_temporal NR_LN_FUSE=0
run_both fold_proj_out_0 leaf_transformer,leaf_temporal NR_FOLD_PROJ_OUT=0
run_both smallm_0 leaf_transformer,leaf_temporal NR_SMALLM=0
# the process-wide switches the GEMM route reads (nr_gemm_route), on the networks whose plans those kernels appear in
gemm_nets=leaf_transformer,leaf_temporal,leaf_transformer640,leaf_temporal640,leaf_transformer1280,tiny_vae_dec
run_both g8p_0 $gemm_nets NR_G8P=0
run_both g8p_2 $gemm_nets NR_G8P=2
run_both rowpanel_0 $gemm_nets NR_ROWPANEL=0
run_both lin160_0 $gemm_nets NR_LIN160=0
run_both igemm_force $gemm_nets NR_IGEMM_FORCE=128,64,2,3,1
# the switches nr_gn_route and nr_attn_route read, the FeedForward wave count and the A/B switches of the five fused transformer kernels
gn_nets=tiny_unet,leaf_transformer,leaf_temporal,tiny_sgm,tiny_vae_dec,tiny_vae_enc
leaves320=leaf_transformer,leaf_temporal
run_both gn_slab_0 $gn_nets NR_GN_SLAB=0
run_both gn_small_0 $gn_nets NR_GN_SMALL=0
run_both gn_t_1024 $gn_nets NR_GN_T=1024
run_both attn_rowsum_adds tiny_unet,leaf_transformer NR_ATTN_ROWSUM=adds
run_both ff_waves_4 $leaves320 NR_FF_WAVES=4
run_both ff_fused_0 $leaves320 NR_FF_FUSED=0
run_both tattn_fused_0 leaf_temporal NR_TATTN_FUSED=0
run_both xattn_fused_0 leaf_transformer NR_XATTN_FUSED=0
run_both tattn_head_0 leaf_temporal640,leaf_temporal1280 NR_TATTN_HEAD=0
run_both xattn_head_0 leaf_transformer640,leaf_transformer1280 NR_XATTN_HEAD=0
# the GEMM / conv op hooks at the shapes of tests/sanitize/op_route_shapes.txt, and the tiled igemm under the NR_IGEMM_FORCE sweep of plan_dump --force-sweep
for t in old new; do
  env -u NR_DETERMINISTIC_BATCH -u NR_IGEMM_FORCE NR_STUB_TRACE="$tmp/$t.ops.trace" "$tmp/$t/build/plan_dump" --ops "$root/tests/sanitize/op_route_shapes.txt" > /dev/null ||
    { echo "$t ops: plan_dump failed" >&2; exit 1; }
  env -u NR_DETERMINISTIC_BATCH NR_STUB_TRACE="$tmp/$t.sweep.trace" "$tmp/$t/build/plan_dump" --force-sweep > /dev/null || { echo "$t sweep: plan_dump failed" >&2; exit 1; }
  sed -E -i 's/0x[0-9a-f]+/PTR/g' "$tmp/$t.ops.trace" "$tmp/$t.sweep.trace"
  grep '^L ' "$tmp/$t.sweep.trace" > "$tmp/$t.sweep.launches"
  grep '^# ' "$tmp/$t.sweep.trace" > "$tmp/$t.sweep.notes"
done

echo "# plans of the working tree against $rev ($(git -C "$root" rev-parse --short "$rev"))"
status=0
for label in default ln_fuse_0 fold_proj_out_0 smallm_0 g8p_0 g8p_2 rowpanel_0 lin160_0 igemm_force gn_slab_0 gn_small_0 gn_t_1024 attn_rowsum_adds \
             ff_waves_4 ff_fused_0 tattn_fused_0 xattn_fused_0 tattn_head_0 xattn_head_0; do
  for what in dump trace; do
    a="$tmp/old.$label.$what"; b="$tmp/new.$label.$what"
    if cmp -s "$a" "$b"; then
      echo "$label $what: identical ($(wc -l < "$b") lines, $(grep -c -E '^(== |L )' "$b") $([ $what = dump ] && echo plans || echo launches))"
    else
      echo "$label $what: DIFFERS"; status=1
      diff "$a" "$b" | head -n "$difflines" | sed 's/^/    /' || true
    fi
  done
done
for what in ops.trace sweep.launches; do
  a="$tmp/old.$what"; b="$tmp/new.$what"
  if cmp -s "$a" "$b"; then
    echo "${what/./ }: identical ($(wc -l < "$b") lines, $(grep -c '^L ' "$b") launches)"
  else
    echo "${what/./ }: DIFFERS"; status=1
    diff "$a" "$b" | head -n "$difflines" | sed 's/^/    /' || true
  fi
done
# the sweep's route notes may differ where $rev's route recorded a plan its launcher then changed: counted, not judged
echo "sweep notes: $(diff "$tmp/old.sweep.notes" "$tmp/new.sweep.notes" | grep -c '^>' || true) of $(wc -l < "$tmp/new.sweep.notes") differ from $rev's"
# coverage: <rev>'s own default dump plans every kernel class
for k in ff_fused xattn_fused xattn_head tattn_fused tattn_head 'lin160 ' 'lin160 panel' igemm groupnorm layernorm attention; do
  n=$(grep -c -E "^op [0-9]+: $k" "$tmp/old.default.dump" || true)
  echo "coverage '$k': $n ops in $rev's dump"
  [ "$n" -gt 0 ] || status=1
done
# ... and its default trace launches every kernel class the GEMM, GroupNorm and attention routes can choose
for k in smallm_kernel lin160_kernel lin128q_kernel rowpanel_kernel g8p_kernel igemm_bf16_kernel splitk_reduce_kernel \
         gn_slab_kernel gn_fused_small_kernel gn_stats_kernel gn_finalize_kernel attn_fwd_kernel attn_fwd_shared_kernel; do
  n=$(grep -c -E "^L [^ ]*$k" "$tmp/old.default.trace" || true)
  echo "coverage '$k': $n launches in $rev's trace"
  [ "$n" -gt 0 ] || status=1
done
# ... and the default dump plans the networks that reach the builders' rarer branches (noisy sample not zeroed, mid-block motion module, one add per residual)
for k in tiny_ctrl_noisy tiny_ctrl_image_noisy tiny_unet_midmotion tiny_unet_lpb3; do
  n=$(grep -c "^== $k plan " "$tmp/old.default.dump" || true)
  echo "coverage '$k': $n plans in $rev's dump"
  [ "$n" -gt 0 ] || status=1
done
exit $status
