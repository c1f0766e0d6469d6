#!/bin/bash
# The round's closing GPU call, part 2 (after scripts/profile_round.sh): the sweeps behind profiles/<tag>_*_sweep.txt /
# _odd_widths.txt / _shape_cliffs.txt and the HBM counters of the operator families profile_round.sh does not cover.
set -e
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
PRE=${PROF_PREFIX:-fin_}
OUT=${PROF_OUT:-prof_out}          # where the run leaves its files (scripts/summarize_prof.py, pmc_ops.py read it)
mkdir -p "$OUT"
python3 scripts/backward_sweep.py > $OUT/${PRE}backward_sweep.txt 2>&1
python3 scripts/odd_width_probe.py > $OUT/${PRE}odd_widths.txt 2>&1
python3 scripts/width_sweep.py > $OUT/${PRE}width_sweep.txt 2>&1
python3 scripts/exp/devlens_cliffs.py > $OUT/${PRE}shape_cliffs.txt 2>&1
FAM=${PMC_FAMILIES:-n16,odd,bwd,w8}
python3 scripts/pmc_ops.py run --time --only=$FAM > $OUT/pmcx_time.json 2> $OUT/${PRE}pmcx_time.err
rm -rf $OUT/pmcx_fetch $OUT/pmcx_write
rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/pmcx_fetch -o run -- python3 scripts/pmc_ops.py run --only=$FAM > $OUT/${PRE}pmcx_fetch.log 2>&1
rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/pmcx_write -o run -- python3 scripts/pmc_ops.py run --only=$FAM > $OUT/${PRE}pmcx_write.log 2>&1
tail -n +1 $OUT/${PRE}backward_sweep.txt $OUT/${PRE}odd_widths.txt
