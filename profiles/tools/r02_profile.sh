#!/bin/bash
# Round-2 profile of the bench command on the GPU box (run from the repository; output under OUT, default profile_out/):
#   kernel trace + stats, then the two HBM traffic counter passes (separate runs, --kernel-trace only).
R=$(cd "$(dirname "$0")/../.." && pwd)
OUT=$(mkdir -p "${OUT:-$R/profile_out}" && cd "${OUT:-$R/profile_out}" && pwd)
cd /tmp && export TMPDIR=/tmp
rm -rf $OUT/r02_prof $OUT/r02_pmc
rocprofv3 --kernel-trace --stats -d $OUT/r02_prof --output-format csv -- python3 $R/bench.py --full --steps 5 --warmup 2 --no-cpu-baseline > $OUT/r02_prof_bench.json 2> $OUT/r02_prof_bench.err
rocprofv3 --pmc FETCH_SIZE --kernel-trace -d $OUT/r02_pmc/fetch --output-format csv -- python3 $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > /dev/null 2>&1
rocprofv3 --pmc WRITE_SIZE --kernel-trace -d $OUT/r02_pmc/write --output-format csv -- python3 $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > /dev/null 2>&1
cd $R && python3 profiles/make_pmc_traffic.py $OUT/r02_pmc r02 1048576
cp profiles/r02_pmc_hbm_traffic.json $OUT/
ls $OUT/r02_prof/*/ | head
