#!/bin/bash
# Same-box A/B of this tree's C2 bench against another source tree's own bench + library
# (e.g. a previous round's final commit, exported with git archive and built in place).
# Usage: tools/ab_tree.sh TAG OTHER_TREE_DIR [OTHER_FLAGS]   (OTHER_FLAGS: --full by default; '' for a tree
# whose bench.py predates --full and prints the kernel times unasked)
set -o pipefail
cd "${GRAFT_REPO_ROOT:-.}"
TAG=$1; OTHER=$2; OFLAGS=${3---full}
OUT=${OUT:-bench_out}; mkdir -p "$OUT"
HERE=$PWD
for rep in 1 2; do
  timeout -k 10 240 python bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --no-aggregate --no-secondary > $OUT/abt_${TAG}_head_$rep.json 2> $OUT/abt_${TAG}_head_$rep.err || { echo "head failed"; tail -5 $OUT/abt_${TAG}_head_$rep.err; exit 1; }
  (cd "$OTHER" && timeout -k 10 240 python bench.py $OFLAGS --steps 3 --warmup 1 --no-cpu-baseline --no-aggregate --no-secondary) > $OUT/abt_${TAG}_other_$rep.json 2> $OUT/abt_${TAG}_other_$rep.err || { echo "other failed"; tail -5 $OUT/abt_${TAG}_other_$rep.err; exit 1; }
  for w in head other; do
    python -c "import json; d=json.loads(open('$OUT/abt_${TAG}_${w}_$rep.json').read().splitlines()[-1]); print('$w', round(d['value']), {k: round(x,2) for k,x in d['roofline']['kernel_avg_ms'].items()})"
  done
done
