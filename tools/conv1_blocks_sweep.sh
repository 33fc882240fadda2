#!/bin/bash
# conv1 (f16x3) workgroup-count sweep: avg launch time at B = 1, 2, 8 (one bench line per point: <outdir>/c1_<B>_<N>.json)
# usage: tools/conv1_blocks_sweep.sh <outdir>
O=${1:?usage: tools/conv1_blocks_sweep.sh <outdir>}
mkdir -p $O
for B in 1 2 8; do for N in 256 512 1024 2048; do
  ACTMI_CONV1_BLOCKS=$N python bench.py --full --batch $B --steps 50 --warmup 10 --no-cpu-baseline 2>/dev/null > $O/c1_${B}_${N}.json || exit 1
done; done
