#!/bin/bash
# per-call-site kernel profile of the bench config: $O/sites.json (O = $ATHD_OUT, default bench_out)
O=${ATHD_OUT:-bench_out}
mkdir -p $O
ATHD_PROF_SITES=1 timeout -k 10 600 python bench.py --full --steps 2 --warmup 2 --no-cpu-baseline --dump-kernels $O/sites.json > $O/bench_sites.log 2>&1
rc=$?; tail -1 $O/bench_sites.log; exit $rc
