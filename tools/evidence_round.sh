#!/bin/bash
# Round evidence on ONE box: default bench (with CPU baseline), kernel stats, HBM traffic, MFMA utilisation, per-op CSVs,
# keyframe / VAE / config-4 / config-5 lines.  Usage: bash tools/evidence_round.sh OUTDIR
# The bench lines, per-op CSVs and logs go under OUTDIR; the profiler scripts (profile_round.sh, profile_mfma.sh,
# profile_keyframe.sh) keep their summaries where they write them.  Copy the summaries to profiles/.
OUT=${1:?usage: bash tools/evidence_round.sh OUTDIR}
R=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$OUT"
OUT=$(cd "$OUT" && pwd)
cd "$R"
python bench.py --full > "$OUT/bench.log" 2>&1
python bench.py --full --workload keyframe > "$OUT/bench_keyframe.log" 2>&1
python bench.py --full --workload keyframe --keyframe-latent 96 --keyframe-steps 38 --no-cpu-baseline > "$OUT/bench_keyframe96.log" 2>&1
python bench.py --full --workload keyframe --batch 8 --steps 1 --warmup 1 --no-cpu-baseline > "$OUT/bench_keyframe_b8.log" 2>&1
python bench.py --full --workload enhance --batch 8 --steps 1 --warmup 1 > "$OUT/bench_enhance_b8.log" 2>&1
python bench.py --full --workload vae > "$OUT/bench_vae.log" 2>&1
python bench.py --full --batch 8 --steps 1 --warmup 1 --no-cpu-baseline --no-psnr > "$OUT/bench_c4_batch8.log" 2>&1
python bench.py --full --frames 32 --latent 64 --batch 4 --steps 1 --warmup 1 > "$OUT/bench_c5_bf16.log" 2>&1
python bench.py --full --frames 32 --latent 64 --batch 4 --steps 1 --warmup 1 --attn-fp8 > "$OUT/bench_c5_fp8.log" 2>&1
python tools/per_op_profile.py "$OUT/per_op_unet.csv" "$OUT/per_op_ctrl.csv" 1 16 32 5 > "$OUT/per_op.log" 2>&1
python tools/per_op_profile.py "$OUT/per_op_c4_unet.csv" "$OUT/per_op_c4_ctrl.csv" 8 16 32 4 > "$OUT/per_op_c4.log" 2>&1
python tools/launch_floor.py > "$OUT/launch_floor.txt" 2>&1
bash tools/profile_round.sh > "$OUT/profile_round.log" 2>&1
bash tools/profile_mfma.sh > "$OUT/profile_mfma.log" 2>&1
bash tools/profile_keyframe.sh > "$OUT/profile_keyframe.log" 2>&1
tail -c 300 "$OUT/bench.log"
