# The round's closing measurements on ONE box: the driver-style line, the per-shape GEMM table, the standalone kernel table
# (side stream off) and the three PMC passes.  usage: final_measure.sh TAG   (outputs under $OUT/TAG_*)
tag=${1:-final}
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
OUT=${OUT:-out}; mkdir -p $OUT      # where this script writes (relative to the repository root)
timeout -k 10 900 python bench.py --full --steps 20 --warmup 5 --gemm-table $OUT/${tag}_gemm_table.txt > $OUT/${tag}_bench.json 2> $OUT/${tag}_bench.err || { echo bench failed; tail -5 $OUT/${tag}_bench.err; exit 1; }
echo "bench done: $(python -c "import json;d=json.loads(open('$OUT/${tag}_bench.json').read().strip().splitlines()[-1]);print(d['value'], d['ms_per_step'])")"
rm -rf $OUT/${tag}_stats
MUSCLE_WGRAD_STREAM=0 timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${tag}_stats -- python3 bench.py --full --no-cpu-baseline --no-other-arith --no-configs --steps 5 --warmup 2 > $OUT/${tag}_stats.log 2>&1 || { echo stats failed; exit 1; }
python tools/summarize_prof.py $OUT/${tag}_stats $OUT/${tag}_split_noside_kernel_stats.csv 10 > /dev/null
echo stats done
for c in FETCH_SIZE WRITE_SIZE SQ_VALU_MFMA_BUSY_CYCLES; do
  rm -rf $OUT/pmc_${tag}_$c
  timeout -k 10 330 rocprofv3 --kernel-trace --pmc $c --output-format csv -d $OUT/pmc_${tag}_$c -- python3 bench.py --full --no-cpu-baseline --no-other-arith --no-configs --steps 2 --warmup 1 > $OUT/pmc_${tag}_$c.log 2>&1 || exit 1
  echo done $c
done
python tools/summarize_pmc.py $OUT/${tag}_pmc_per_kernel.json fetch=$OUT/pmc_${tag}_FETCH_SIZE write=$OUT/pmc_${tag}_WRITE_SIZE mfma=$OUT/pmc_${tag}_SQ_VALU_MFMA_BUSY_CYCLES steps=5 | tail -30
