#!/bin/bash
# usage: tools/profile_round.sh TAG [ROUND]   (on the GPU box, from the repo root; ROUND defaults to r05)
# kernel stats, the two PMC passes, a bench line of the same build (with roofline.traffic from those passes) and the
# same line through the sharded path as a process group of one -> tool_out/<TAG>_*  (copy what is to be judged
# into profiles/ afterwards: tool_out/ is scratch)
set -e
tag=$1
round=${2:-r05}
root=$PWD
mkdir -p $root/tool_out
cd /tmp && export TMPDIR=/tmp
rm -rf $root/tool_out/${tag}_stats $root/tool_out/${tag}_fetch $root/tool_out/${tag}_write
rocprofv3 --kernel-trace --stats --output-format csv -d $root/tool_out/${tag}_stats -o s -- python3 $root/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > $root/tool_out/${tag}_stats.log 2>&1
echo "stats done"
rocprofv3 --kernel-trace --pmc FETCH_SIZE --kernel-include-regex ckl --output-format csv -d $root/tool_out/${tag}_fetch -o f -- python3 $root/bench.py --full --steps 1 --warmup 1 --no-cpu-baseline > $root/tool_out/${tag}_fetch.log 2>&1
echo "fetch done"
rocprofv3 --kernel-trace --pmc WRITE_SIZE --kernel-include-regex ckl --output-format csv -d $root/tool_out/${tag}_write -o w -- python3 $root/bench.py --full --steps 1 --warmup 1 --no-cpu-baseline > $root/tool_out/${tag}_write.log 2>&1
echo "write done"
cd $root
python3 tools/pmc_summary.py tool_out/${tag}_fetch tool_out/${tag}_write "1024x1024x512 uint32 markov 0" tool_out/${tag}_pmc_traffic.json > tool_out/${tag}_pmc.txt
cp tool_out/${tag}_pmc_traffic.json profiles/${round}_pmc_traffic.json   # bench.py below reads roofline.traffic from it (same build: lib_sha16)
# the raw traces are tens of MiB: keep the summaries only
mkdir -p tool_out/${tag}
find tool_out/${tag}_stats -name "*kernel_stats.csv" -exec cp {} tool_out/${tag}/kernel_stats.csv \;
rm -rf tool_out/${tag}_stats tool_out/${tag}_fetch tool_out/${tag}_write
python3 bench.py --full > tool_out/${tag}_bench.json 2> tool_out/${tag}_bench.err
tail -c 600 tool_out/${tag}_bench.json
# the same line through the sharded path as a process group of one over RCCL (what N ranks pay per rank)
CKL_BENCH_REHEARSAL=group1 python3 bench.py --full --no-cpu-baseline > tool_out/${tag}_bench_group1.json 2> tool_out/${tag}_bench_group1.err || echo "group-of-one run failed"
tail -c 300 tool_out/${tag}_bench_group1.json
