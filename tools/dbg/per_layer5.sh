# per-layer HBM table of the depthwise / SE passes from kernel traces with the weight-gradient side stream OFF and ON
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
OUT=${OUT:-out}; mkdir -p $OUT      # where this script writes (relative to the repository root)
for v in 0 1; do
  rm -rf $OUT/pl_$v
  MUSCLE_WGRAD_STREAM=$v timeout -k 10 300 rocprofv3 --kernel-trace --output-format csv -d $OUT/pl_$v -- python3 bench.py --full --no-cpu-baseline --no-other-arith --no-configs --steps 3 --warmup 2 > $OUT/pl_$v.log 2>&1 || { echo failed $v; tail -3 $OUT/pl_$v.log; exit 1; }
  python tools/per_layer_hbm.py $(find $OUT/pl_$v -name "*_kernel_trace.csv") > $OUT/r05_per_layer_hbm_side$v.txt 2>&1
  find $OUT/pl_$v -name "*_kernel_trace.csv" -delete
  tail -2 $OUT/r05_per_layer_hbm_side$v.txt
done
