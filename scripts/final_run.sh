#!/bin/bash
# End-of-session evidence run on the GPU box (through gpurun): GPU tests, one bench line per BASELINE configuration,
# rocprofv3 kernel stats of the default bench and of the C5 shard, PMC passes of both.  Output: gpurun_out/$TAG/.
TAG=${1:-final}
R=${GRAFT_REPO_ROOT:-$(pwd)}
O=$R/gpurun_out/$TAG
mkdir -p $O
cd $R
timeout -k 10 700 python3 -m pytest tests -m gpu -x -q > $O/pytest.log 2>&1; echo "pytest rc=$?"; tail -2 $O/pytest.log
python3 bench.py --full > $O/bench_default.json 2> $O/bench_default.err; echo "bench rc=$?"
scripts/bench_configs.sh $TAG/configs > $O/configs.txt 2>&1; cat $O/configs.txt
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/kt_c4 -o c4 -- python3 $R/bench.py --full --no-cpu-baseline > $O/kt_c4.log 2>&1
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/kt_c5s -o c5s -- python3 $R/bench.py --full --no-cpu-baseline --data device --repeats 2 --n 250000 --f 12288 --k 500 --steps 10 --warmup 2 > $O/kt_c5s.log 2>&1
cd $R
rm -f $(find $O -name "*kernel_trace.csv") $(find $O -name "*agent_info.csv")
for f in $O/kt_c4/c4_kernel_stats.csv $O/kt_c5s/c5s_kernel_stats.csv; do echo $f; grep klnmf $f | cut -c1-150 | head -8; done
scripts/pmc_profile.sh $TAG/pmc_c4 > $O/pmc_c4.txt 2>&1
scripts/pmc_profile.sh $TAG/pmc_c5s --n 250000 --f 12288 --k 500 --steps 3 --warmup 1 --repeats 1 --data device --full --no-cpu-baseline > $O/pmc_c5s.txt 2>&1
rm -f $(find $O -name "*kernel_trace.csv") $(find $O -name "*agent_info.csv") $(find $O -name "*counter_collection.csv")
tail -3 $O/pmc_c4.txt; tail -3 $O/pmc_c5s.txt
