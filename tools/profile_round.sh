#!/bin/bash
# Round profile on the GPU box: kernel-trace stats of the default bench command, then the PMC
# passes (FETCH_SIZE and WRITE_SIZE need separate passes: TCC has 4 slots, they cost 3 + 2; the SQ /
# GRBM counters for MFMA-busy ride in a third).  Counters are collected with --kernel-trace only.
# The counter passes run eager steps (--no-graph); the twin-operand x.Wx launch (gemm_xwx_glds_kernel)
# exists only in steps 2 .. G of a captured replay, so FETCH_SIZE / WRITE_SIZE get a graph-mode pass
# of their own next to the eager one (pmc_<counter>/graph: pmc_traffic.py averages over both).
# Every GPU step runs under its own time limit and the chain stops at the first failure.
# usage: tools/profile_round.sh <tag> [bench args...]      (outputs under gpurun_out/prof_<tag>/)
tag=$1; shift
root=$(cd "$(dirname "$0")/.." && pwd)
out=$root/gpurun_out/prof_$tag
mkdir -p $out
export TMPDIR=/tmp
cd /tmp
lean="--no-cpu-baseline --no-roofline --no-extras"
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $out/trace -o trace -- python3 $root/bench.py --steps 50 --warmup 5 --full --no-cpu-baseline --no-extras "$@" > $out/trace.log 2>&1 &&
timeout -k 10 200 rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $out/pmc_FETCH_SIZE -o pmc -- python3 $root/bench.py --steps 10 --warmup 2 $lean --no-graph "$@" > $out/pmc_FETCH_SIZE.log 2>&1 &&
timeout -k 10 200 rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $out/pmc_WRITE_SIZE -o pmc -- python3 $root/bench.py --steps 10 --warmup 2 $lean --no-graph "$@" > $out/pmc_WRITE_SIZE.log 2>&1 &&
timeout -k 10 200 rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $out/pmc_FETCH_SIZE/graph -o pmc -- python3 $root/bench.py --steps 10 --warmup 2 $lean "$@" > $out/pmc_FETCH_SIZE_graph.log 2>&1 &&
timeout -k 10 200 rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $out/pmc_WRITE_SIZE/graph -o pmc -- python3 $root/bench.py --steps 10 --warmup 2 $lean "$@" > $out/pmc_WRITE_SIZE_graph.log 2>&1 &&
timeout -k 10 200 rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES GRBM_GUI_ACTIVE --kernel-trace --output-format csv -d $out/pmc_MFMA -o pmc -- python3 $root/bench.py --steps 10 --warmup 2 $lean --no-graph "$@" > $out/pmc_MFMA.log 2>&1
rc=$?
find $out -type f | head -80 > $out/files.txt
if [ $rc -ne 0 ]; then echo "profile_round: a GPU step failed (rc $rc); see the logs under $out" >&2; exit $rc; fi
python3 $root/tools/rocprof_summary.py $(find $out/trace -name '*.db' | head -1) > $out/kernel_stats.txt 2>&1
python3 $root/tools/pmc_traffic.py $out > $out/pmc_traffic.txt 2>&1
python3 $root/tools/profile_merge.py $out > $out/kernel_profile.txt 2>&1
# keep only the small summaries (gpurun_out merges <= 64 MiB)
find $out -name '*.db' -size +20M -delete
