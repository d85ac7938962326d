#!/bin/bash
# Kernel-trace the bench's entity-sync leg for libgwaoi variants (GPU box):
#   bash tools/sync_prof.sh base wu4 ...   -> $OUT_DIR/sync_prof_<v>/ (rocprofv3 databases; default bench_out/)
# then (here) python3 tools/sync_prof.py bench_out/sync_prof_* for per-kernel mean durations
R=${GRAFT_REPO_ROOT:-$(pwd)}
O=${OUT_DIR:-$R/bench_out}
mkdir -p $O
cd /tmp && export TMPDIR=/tmp
for v in "$@"; do
    if [ "$v" = base ]; then unset GWAOI_LIB; else export GWAOI_LIB=$R/goworld_amd/lib/variants/$v.so; fi
    timeout -k 10 300 rocprofv3 --kernel-trace -d $O/sync_prof_$v -o p -- python3 $R/bench.py --full --steps 6 --warmup 1 \
        --no-cpu-baseline --cfg4-steps 0 --cfg5-steps 0 --host-tick-steps 0 --host-io-steps 0 --wire-steps 0 \
        --small-flush-reps 0 --claims-steps 0 > $O/sync_prof_$v.json 2> $O/sync_prof_$v.err || { echo "$v failed"; exit 1; }
done
