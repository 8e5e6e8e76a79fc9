# shade backward: where the specular light-gradient scatter spends its time (GIGS_ABLATE bits: 1 diffuse, 2 all
# specular, 4 specular levels accumulated in LDS, 8 specular levels added with global atomics)
set -e
cd $GRAFT_REPO_ROOT
OUT=${OUT:-bench_out}
mkdir -p $OUT
for ab in 0 2 4 8; do
  GIGS_ABLATE=$ab python bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --graphs off > $OUT/bench_abl.json 2> $OUT/bench_abl.err || { tail -20 $OUT/bench_abl.err; exit 1; }
  python -c "
import json
d=json.loads(open('$OUT/bench_abl.json').read().strip().splitlines()[-1])
print('ablate=$ab shade_bwd', d['kernels']['shade_bwd']['ms_per_step'])"
done
