#!/bin/bash
# on the GPU box: alternate two A/B libraries several times (headline mode only) to see through run-to-run noise
cd "$(dirname "$0")/.."; O=${AB_OUT:-bbs_sign_amd/build/ab}; mkdir -p $O
a=$1; b=$2; reps=${3:-3}
for r in $(seq 1 $reps); do for v in $a $b; do
  BBS_SIGN_AMD_LIB=${AB_LIBS:?directory tools/ab_build.sh built into}/$v/libbbs_sign_amd.so timeout -k 10 200 python bench.py --full --no-cpu-baseline --no-extras --steps 96 > $O/$v.$r.json 2> $O/$v.err || { echo "$v failed"; exit 1; }
  python -c "import json;d=json.load(open('$O/$v.$r.json'));print('$v', $r, round(d['value']), round(d['single_batch']['stage_ms']['pairing_6lane'],2))"
done; done
