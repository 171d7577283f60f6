set -o pipefail
O=${OUT_DIR:-out}
mkdir -p $O
timeout -k 10 400 python -u bench.py --full --cpu-sample 0 > $O/r4p_flat10m.log 2>&1 || { tail -20 $O/r4p_flat10m.log; exit 1; }
timeout -k 10 400 python -u bench.py --workload incr --full --cpu-sample 0 --steps 2 --warmup 1 > $O/r4p_incr.log 2>&1 || { tail -20 $O/r4p_incr.log; exit 1; }
timeout -k 10 400 python -u bench.py --workload trees --full --cpu-sample 0 --steps 3 --warmup 1 > $O/r4p_trees.log 2>&1 || { tail -20 $O/r4p_trees.log; exit 1; }
echo done
