#!/bin/bash
# One GPU call: the -m gpu suite (or a subset: $1 = pytest -k expression), then a full bench line.
# Usage (from the repo root on the box): bash tools/gpu_run.sh TAG [pytest -k expr] [bench args...]
# Logs and the bench line go to $OUT_DIR (default: bench_out/).
set -o pipefail
tag=${1:-run}; kexpr=${2:-}; shift 2 2>/dev/null
O=${OUT_DIR:-bench_out}
mkdir -p $O
if [ -n "$kexpr" ] && [ "$kexpr" != "-" ]; then
  timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread -k "$kexpr" > $O/pytest_$tag.log 2>&1 || { tail -30 $O/pytest_$tag.log; exit 1; }
elif [ "$kexpr" != "-" ]; then
  timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > $O/pytest_$tag.log 2>&1 || { tail -30 $O/pytest_$tag.log; exit 1; }
fi
tail -3 $O/pytest_$tag.log 2>/dev/null
if [ "$#" -gt 0 ] || [ -z "$NO_BENCH" ]; then
  timeout -k 10 600 python -u bench.py --full "$@" > $O/bench_$tag.json 2> $O/bench_$tag.err || { tail -20 $O/bench_$tag.err; exit 1; }
  tail -c 1500 $O/bench_$tag.json
fi
