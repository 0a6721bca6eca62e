# launch-geometry table of the headline step (B7 / 448 / batch 32), side stream off (tools/occupancy_table.py)
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
OUT=${OUT:-out}; mkdir -p $OUT      # where this script writes (relative to the repository root)
rm -rf $OUT/occ_b7
MUSCLE_WGRAD_STREAM=0 timeout -k 10 300 rocprofv3 --kernel-trace --output-format csv -d $OUT/occ_b7 -- python3 bench.py --full --no-cpu-baseline --no-other-arith --no-configs --steps 8 --warmup 2 > $OUT/occ_b7.log 2>&1 || { echo b7 failed; tail -5 $OUT/occ_b7.log; exit 1; }
python tools/occupancy_table.py $OUT/occ_b7 10 90 > $OUT/occ_b7.txt
find $OUT/occ_b7 -name "*_kernel_trace.csv" -delete
head -64 $OUT/occ_b7.txt
