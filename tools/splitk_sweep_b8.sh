#!/bin/bash
# sweep of the forward split-K heuristic at the benchmark batch (B = 8): per-shape tables under <outdir>/sk8_*.json
# triples: ACTMI_FWD_SPLITK_TARGET / _MINNK / _MAXTILES.  usage: tools/splitk_sweep_b8.sh <outdir>
O=${1:?usage: tools/splitk_sweep_b8.sh <outdir>}
mkdir -p $O
for cfg in "1536 12 768" "2432 12 1300" "4864 12 1300" "4800 12 2500" "2432 8 1300" "4800 8 2500"; do
  set -- $cfg
  ACTMI_FWD_SPLITK_TARGET=$1 ACTMI_FWD_SPLITK_MINNK=$2 ACTMI_FWD_SPLITK_MAXTILES=$3 \
    python bench.py --full --steps 30 --warmup 5 --no-cpu-baseline --no-extras --sustained-s 0 --shapes \
      2> $O/sk8_$1_$2_$3.err > $O/sk8_$1_$2_$3.json || exit 1
  echo "done $cfg" >> $O/sk8_progress.log
done
