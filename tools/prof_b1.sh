set -e
R=$GRAFT_REPO_ROOT
O=$(realpath -m "${1:?usage: tools/prof_b1.sh <outdir>}")
mkdir -p $O
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $O/kt -o kt -- python3 $R/bench.py --full --batch 1 --no-cpu-baseline --steps 200 --warmup 20 > $O/bench_b1_under_rocprof.json 2>/dev/null
echo kt done >&2
