cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
OUT=${OUT:-out}; mkdir -p $OUT      # where this script writes (relative to the repository root)
rm -rf $OUT/r5a_stats
MUSCLE_WGRAD_STREAM=0 timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/r5a_stats -- python3 bench.py --full --no-cpu-baseline --no-other-arith --no-configs --steps 5 --warmup 2 > $OUT/r5a_stats.log 2>&1 || { echo stats failed; tail -5 $OUT/r5a_stats.log; exit 1; }
python tools/summarize_prof.py $OUT/r5a_stats $OUT/r05_a_split_noside_kernel_stats.csv 10 > /dev/null
python tools/dbg/trace_neighbours.py $OUT/r5a_stats copyBuffer > $OUT/r5a_copybuffer.txt
python tools/dbg/trace_neighbours.py $OUT/r5a_stats FillFunctor > $OUT/r5a_fill.txt
find $OUT/r5a_stats -name "*_kernel_trace.csv" -size +30M -delete
head -30 $OUT/r5a_copybuffer.txt
