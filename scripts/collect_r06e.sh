#!/bin/bash
# Round 6, fifth call: the candidate "high" layouts for the 512-step horizon, emulated (scripts/precision_budget.py "R6 ...") on four deterministic draws
# (init seeds 3 = good, 5 = worst, 7, 8); the data-parallel stand-in runs again with the spare-stream schedule of single-tower graphs; cfg 5 single-GPU A/B.
set -u
O=gpurun_out/r06e
mkdir -p $O
timeout 600 python -m pytest tests/test_gpu_dp.py -x -q -k "dbof" > $O/pytest_dbof_dp.txt 2>&1
D=/tmp/evc_draws; mkdir -p $D
for seed in 5 3 7 8; do
  rm -rf $D/s; mkdir -p $D/s
  EVC_LONG_SEED=$seed timeout 600 python scripts/long_horizon.py train $D/s 16 1e-3 512 > /dev/null 2>&1
  echo "== init seed $seed" >> $O/budget_plans.txt
  timeout 1200 python scripts/precision_budget.py --load_sd $D/s/step512.pt --only "R6 " 2>&1 | grep -v amdgpu.ids | cut -c1-230 >> $O/budget_plans.txt
done
rm -rf $D
bash scripts/dp_sim_world.sh $O/dp_sim_world.txt > /dev/null 2>&1
for i in 1 2; do
  for v in 0 1; do
    EVC_OPT_SPARE_STREAM=$v timeout 300 python bench.py --full --mode student --every_n 30 --batch 1024 --no_cpu_baseline --no_secondary --steps 20 2>/dev/null | python3 -c "
import json, sys
d = json.loads(sys.stdin.read().strip().splitlines()[-1]); print('cfg5 single GPU, EVC_OPT_SPARE_STREAM=$v: %.3f ms/step (median %.3f)' % (d['ms_per_step'], d['ms_per_step_median']))" >> $O/cfg5_spare_ab.txt
    EVC_OPT_SPARE_STREAM=$v timeout 300 python bench.py --full --mode teacher --no_cpu_baseline --no_secondary --steps 20 2>/dev/null | python3 -c "
import json, sys
d = json.loads(sys.stdin.read().strip().splitlines()[-1]); print('cfg2 single GPU, EVC_OPT_SPARE_STREAM=$v: %.3f ms/step (median %.3f)' % (d['ms_per_step'], d['ms_per_step_median']))" >> $O/cfg5_spare_ab.txt
  done
done
tail -3 $O/pytest_dbof_dp.txt
cat $O/budget_plans.txt
cat $O/dp_sim_world.txt | cut -c1-250
cat $O/cfg5_spare_ab.txt
