set -o pipefail
O=${OUT_DIR:-out}
mkdir -p $O
for d in 4096 8192 10240 12500 16384; do
  timeout -k 10 200 python -u bench.py --workload trees --docs-per-gpu $d --full --cpu-sample 0 --pmc off --verbose > $O/r6x_trees_$d.log 2>&1 || { echo FAIL $d; tail -5 $O/r6x_trees_$d.log; exit 1; }
  echo "$d $(grep -o '"ms_per_step": [0-9.]*' $O/r6x_trees_$d.log | head -1) $(grep -E 'k_forest_wave' $O/r6x_trees_$d.log | head -1)"
done
