# same-box A/B of the round-6 cross-attention head kernel (xattnw.hip): NR_XATTN_HEAD=0 restores the q GEMM + attention core.  Interleaved (ABAB).
cd $GRAFT_REPO_ROOT
out=${1:-gpurun_out/xattn_head_ab.txt}
: > $out
for rep in 1 2; do
  for arm in 0 1; do
    NR_XATTN_HEAD=$arm python bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-psnr --no-end-to-end 2>/dev/null | tail -1 | python -c "
import json,sys
d=json.loads(sys.stdin.read()); print('headline  NR_XATTN_HEAD=$arm rep $rep:', d['value'], 'frames/s', d['config']['ms_per_ddim_step'], 'ms/DDIM step; class frac', d['roofline']['frac'])" >> $out
  done
done
for arm in 0 1; do
  NR_XATTN_HEAD=$arm python bench.py --full --workload video --batch 8 --steps 1 --warmup 1 --no-cpu-baseline --no-psnr --no-end-to-end 2>/dev/null | tail -1 | python -c "
import json,sys
d=json.loads(sys.stdin.read()); print('config 4 (8 clips)  NR_XATTN_HEAD=$arm:', d['value'], 'frames/s; class frac', d['roofline']['frac'])" >> $out
done
cat $out
