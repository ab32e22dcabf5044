#!/bin/bash
# Env-var tuning sweep on the box: one short MSM bench per setting, e.g.
#   tools/sweep.sh "MBLS_WSEG_LOG=2" "MBLS_WSEG_LOG=3 MBLS_ROW_SEG_LOG=3"
# (--full: the stage times printed below come from its stage profile; output under $SWEEP_OUT)
O=${SWEEP_OUT:-build/sweep}
mkdir -p $O
i=0
for S in "$@"; do
  i=$((i+1))
  env $S timeout -k 10 200 python bench.py --full --no-cpu --no-mix --steps 10 > $O/$i.json 2> $O/$i.err || exit $?
  python3 -c "import json,sys; d=json.load(open(sys.argv[1])); s=d['msm_stage_ms']; print(sys.argv[2], '|', d['value'], '| dig', s['msm.digits'], 'sort', s['msm.sort'], 'acc', s['msm.accumulate'], 'red', s['msm.reduce'], 'fin', s['msm.final'], 'bs', s['msm.bucket_sum'])" $O/$i.json "$S"
done
