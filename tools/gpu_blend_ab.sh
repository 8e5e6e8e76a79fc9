# eager bench, repeated: blend kernel times are noisy box to box, compare within one box
set -e
cd $GRAFT_REPO_ROOT
OUT=${OUT:-bench_out}
mkdir -p $OUT
for rep in 1 2 3; do
  python bench.py --full --steps 20 --warmup 3 --no-cpu-baseline --graphs off > $OUT/bench_bl.json 2> $OUT/bench_bl.err || { tail -20 $OUT/bench_bl.err; exit 1; }
  python -c "
import json
d=json.loads(open('$OUT/bench_bl.json').read().strip().splitlines()[-1])
print('blend_fwd', d['kernels']['blend_fwd']['ms_per_step'], 'blend_bwd', d['kernels']['blend_bwd']['ms_per_step'])"
done
