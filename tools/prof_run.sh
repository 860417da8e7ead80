set -x
TAG=${1:-r1_v4}
cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
OUT=${PROF_OUT:-$R/prof_out}/prof_$TAG     # (tools/prof_summarize.py reads the same folder)
mkdir -p $OUT
cd $R
# 1) kernel-trace stats of the default bench command (steps 4 warmup 2; --full: the line carries the per-kernel figures rocprofv3 is checked against)
timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trace -- python bench.py --full --steps 4 --warmup 2 --no-cpu-baseline --no-sweep --no-extras > $OUT/bench_under_rocprof.json 2> $OUT/trace.log
# 2) PMC passes (own runs, 1 step)
for C in FETCH_SIZE WRITE_SIZE "SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CU_CYCLES GRBM_GUI_ACTIVE"; do
  tag=$(echo $C | tr ' ' '_' | cut -c1-24)
  timeout 900 rocprofv3 --pmc $C --kernel-trace --output-format csv -d $OUT/pmc_$tag -- python bench.py --steps 1 --warmup 1 --no-cpu-baseline --no-sweep --no-extras > $OUT/pmc_$tag.json 2> $OUT/pmc_$tag.log
done
# 3) the bench line itself with the CPU baseline
timeout 900 python bench.py --full > $OUT/bench.json 2> $OUT/bench.log
ls -la $OUT $OUT/*/* | head -40
du -sh $OUT
