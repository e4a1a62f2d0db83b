#!/bin/bash
# Round-end check on the GPU box, run from the repo root as `bash scripts/final_check.sh <out-dir>`: the GPU test suite, the
# smoke entry, the full bench line (--full), the DBoF bench line, kernel-stat and PMC profiles -> <out-dir> (scripts/prof.sh
# names its own output directories; copy what is to be kept into profiles/).
set -u
O="${1:?usage: bash scripts/final_check.sh <out-dir>}"
mkdir -p "$O"
timeout 2400 python -m pytest tests -x -q -m gpu 2>&1 | tail -4 > "$O/final_gputest.log"
timeout 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" >> "$O/final_gputest.log" 2>&1
timeout 900 python bench.py --full > "$O/final_bench.json" 2> "$O/final_bench.err"
timeout 300 python bench.py --full --config dbof --no_cpu_baseline > "$O/final_bench_dbof.json" 2> /dev/null
if [ "${PROFILES:-1}" = "1" ]; then
  bash scripts/prof.sh final_prof_default --no_cpu_baseline --no_secondary > /dev/null 2>&1
  bash scripts/prof.sh final_prof_nooverlap --no_cpu_baseline --no_secondary --no_overlap > /dev/null 2>&1
  bash scripts/prof.sh final_prof_dbof --config dbof --no_cpu_baseline > /dev/null 2>&1
  bash scripts/pmc_collect.sh "$O/final_pmc" > /dev/null 2>&1
fi
cat "$O/final_gputest.log"
