#!/bin/bash
# Round-3 profile of the bench command on the GPU box (run from the repository; output under OUT, default profile_out/):
#   1. the full bench line (--full: with extra_configs), 2. the same bench under a one-rank RCCL process group
#   (torch.distributed.run --nproc-per-node 1), 3. kernel trace + stats of the full command (all configurations),
#   4. the two HBM traffic counter passes (separate runs, --kernel-trace only) of the C3 leg;
#   0. before them: smoke(), the small-batch latency table and the graphed training step (second session of the round).
R=$(cd "$(dirname "$0")/../.." && pwd)
OUT=$(mkdir -p "${OUT:-$R/profile_out}" && cd "${OUT:-$R/profile_out}" && pwd)
cd $R
python3 -c "import __graft_entry__ as g; g.smoke()" > $OUT/r03_smoke.log 2>&1; echo "smoke rc $?"; tail -1 $OUT/r03_smoke.log
python3 profiles/tools/small_batch_latency.py > $OUT/r03_small_batch_latency.log 2>&1; echo "latency rc $?"
python3 profiles/tools/train_graph_bench.py > $OUT/r03_train_graph_bench.log 2>&1; echo "train graph rc $?"
python3 bench.py --full > $OUT/r03_bench.json 2> $OUT/r03_bench.err; echo "bench rc $?"
python3 -m torch.distributed.run --nnodes=1 --nproc-per-node 1 --master-addr 127.0.0.1 --master-port 29517 \
    bench.py --gpus 1 --steps 5 --warmup 2 --full --no-extra --no-cpu-baseline > $OUT/r03_rccl_one_rank.json 2> $OUT/r03_rccl_one_rank.err; echo "rccl bench rc $?"
cd /tmp && export TMPDIR=/tmp
rm -rf $OUT/r03_prof $OUT/r03_pmc
rocprofv3 --kernel-trace --stats -d $OUT/r03_prof --output-format csv -- python3 $R/bench.py --full --steps 5 --warmup 2 --no-cpu-baseline > $OUT/r03_prof_bench.json 2> $OUT/r03_prof_bench.err; echo "prof rc $?"
rocprofv3 --pmc FETCH_SIZE --kernel-trace -d $OUT/r03_pmc/fetch --output-format csv -- python3 $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-extra > /dev/null 2>&1; echo "fetch rc $?"
rocprofv3 --pmc WRITE_SIZE --kernel-trace -d $OUT/r03_pmc/write --output-format csv -- python3 $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-extra > /dev/null 2>&1; echo "write rc $?"
cd $R && python3 profiles/make_pmc_traffic.py $OUT/r03_pmc r03 1048576
cp profiles/r03_pmc_hbm_traffic.json $OUT/
find $OUT/r03_prof -name "*kernel_stats.csv" | head -3
