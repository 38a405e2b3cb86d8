#!/bin/sh
# prof_bench.sh TAG [bench args...] — rocprofv3 kernel trace + stats of one bench update
# (into $BENCH_OUT/TAG, default bench_out/TAG under the repository root)
set -e
cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
TAG=$1; shift
O=${BENCH_OUT:-$R/bench_out}
mkdir -p $O
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $O/$TAG -o run --output-format csv -- python3 $R/bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --no-kernel-events "$@" > $O/$TAG.log 2>&1
