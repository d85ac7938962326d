#!/bin/bash
# One GPU-box pass: parity tests, smoke, full bench line (with CPU baseline).
# usage: bash tools/gpu_check.sh <tag>     (logs and the bench line: $OUT_DIR, default bench_out/)
set -o pipefail
TAG=${1:-r01}
R=${GRAFT_REPO_ROOT:-$(pwd)}
cd $R
O=${OUT_DIR:-bench_out}
mkdir -p $O
export TMPDIR=/tmp
timeout -k 10 600 python -u -m pytest tests -m gpu -x -v --timeout 120 --timeout-method thread > $O/pytest_$TAG.log 2>&1 || { echo "pytest failed"; tail -30 $O/pytest_$TAG.log; exit 1; }
tail -3 $O/pytest_$TAG.log
timeout -k 10 180 python -u -c "import __graft_entry__ as g; g.smoke()" > $O/smoke_$TAG.log 2>&1 || { echo "smoke failed"; cat $O/smoke_$TAG.log; exit 1; }
cat $O/smoke_$TAG.log
timeout -k 10 600 python -u bench.py --full > $O/bench_$TAG.json 2> $O/bench_$TAG.err || { echo "bench failed"; tail -20 $O/bench_$TAG.err; exit 1; }
cat $O/bench_$TAG.json
