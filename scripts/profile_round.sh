#!/bin/bash
# One GPU call that produces everything scripts/summarize_prof.py condenses into profiles/<tag>_*:
#   kernel trace + stats of the bench command, FETCH_SIZE and WRITE_SIZE in their own passes (the pool refuses --pmc
#   together with the trace domains), plus kernel stats over every BASELINE config and the integer kernels.
set -e
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
PRE=${PROF_PREFIX:-prof2_}
OUT=${PROF_OUT:-prof_out}          # where the run leaves its files (scripts/summarize_prof.py, pmc_ops.py read it)
mkdir -p "$OUT"
rm -rf $OUT/${PRE}*
python3 bench.py --full --steps 20 --warmup 3 > $OUT/${PRE}bench.json 2> $OUT/${PRE}bench.err
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${PRE}stats -o runc -- python3 bench.py --full --no-cpu-baseline --steps 20 --warmup 3 > $OUT/${PRE}stats.log 2>&1
rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/${PRE}fetch -o runc -- python3 bench.py --full --no-cpu-baseline --steps 4 --warmup 2 > $OUT/${PRE}fetch.log 2>&1
rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/${PRE}write -o runc -- python3 bench.py --full --no-cpu-baseline --steps 4 --warmup 2 > $OUT/${PRE}write.log 2>&1
python3 scripts/bench_configs.py > $OUT/${PRE}configs.txt 2>&1
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${PRE}cfgstats -o runc -- python3 scripts/bench_configs.py > $OUT/${PRE}cfgstats.log 2>&1
# HBM traffic per OPERATOR (index_buckets, pads, narrow rows ...): scripts/pmc_ops.py, one pass per counter; summarise
# with `python3 scripts/pmc_ops.py summarize <tag>` -> profiles/<tag>_pmc_ops.json
python3 scripts/pmc_ops.py run --time > $OUT/pmcops_time.json 2> $OUT/${PRE}pmcops_time.err
rm -rf $OUT/pmcops_fetch $OUT/pmcops_write
rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/pmcops_fetch -o run -- python3 scripts/pmc_ops.py run > $OUT/${PRE}pmcops_fetch.log 2>&1
rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/pmcops_write -o run -- python3 scripts/pmc_ops.py run > $OUT/${PRE}pmcops_write.log 2>&1
# the per-dispatch CSVs are large: keep the stats, drop the traces
find $OUT/${PRE}stats $OUT/${PRE}cfgstats -name '*kernel_trace.csv' -delete
du -sh $OUT/${PRE}* | tail -20
cat $OUT/${PRE}bench.json
