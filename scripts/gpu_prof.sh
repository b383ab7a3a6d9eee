#!/bin/bash
# rocprofv3 kernel trace of a short decode bench (plain launches: stream capture under the tracer crashes rocprofv3 7.2)
set -u
cd "${GRAFT_REPO_ROOT:-/root/repo}"
R=$PWD
export TMPDIR=/tmp
D=${OUT_DIR:-out}        # traces and logs, relative to the repository root
mkdir -p $D/prof
cd /tmp
timeout 600 rocprofv3 --kernel-trace --stats -d $R/$D/prof -o ${1:-r1} -- python $R/bench.py --full --steps ${2:-48} --no-cpu --no-ref-order --no-graph > $R/$D/prof_run.log 2>&1
echo "rocprof exit $?"
cd $R
find $D/prof -type f | head -20
f=$(find $D/prof -name "*kernel_stats.csv" | head -1)
[ -n "$f" ] && head -30 "$f"
tail -c 1500 $D/prof_run.log
