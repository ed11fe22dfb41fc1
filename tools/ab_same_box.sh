#!/bin/bash
# Same-box A/B of two builds of libgnc_hip.so (box-to-box spread on the pool is +-3-5 %, more than most kernel
# changes are worth, so variants are compared inside ONE gpurun call):
#   gpurun -- 'bash tools/ab_same_box.sh build/libgnc_base.so build/libgnc_new.so'
# Runs the c3 forward bench twice per variant (A B A B) and the training bench once each; leaves A installed.
# Every pass keeps its own log ($OUT/ab_<pass>_<variant>.log) and prints the step time and K1's isolated launch time.
set -e
A=$1; B=$2; LIB=graphnet_classifier_amd/libgnc_hip.so
OUT=${OUT:-out}
mkdir -p "$OUT"
pass=0
for v in A B A B; do
  pass=$((pass + 1))
  log="$OUT/ab_${pass}_$v.log"
  cp "${!v}" $LIB
  python bench.py --full --no-cpu-baseline --preheat-ms 300 > "$log" 2>&1
  echo "$v fwd   $(grep -o '"ms_per_step": [0-9.]*' "$log" | head -1) K1 $(grep -o '"avg_launch_ms": [0-9.]*' "$log" | head -1) $(grep -o '"kernel_ms_per_step": {[^}]*}' "$log" | cut -c1-400)"
done
for v in A B; do
  cp "${!v}" $LIB
  python bench.py --full --mode train --steps 5 --warmup 2 --preheat-ms 300 > "$OUT/abt_$v.log" 2>&1
  echo "$v train $(grep -o '"ms_per_step": [0-9.]*' "$OUT/abt_$v.log" | head -1)"
done
cp "$A" $LIB
