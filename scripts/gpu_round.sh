#!/bin/bash
# One GPU-box pass: parity tests, the default bench line, and the rocprofv3 kernel trace of the same bench command.
# Usage (from the repo root, on the GPU box): bash scripts/gpu_round.sh <tag>
set -e -o pipefail
R=$(pwd)
tag=${1:-r01}
out=gpurun_out/$tag
mkdir -p $out
timeout -k 10 900 python -m pytest tests -m gpu -x -q > $out/pytest_gpu.log 2>&1 || { tail -30 $out/pytest_gpu.log; exit 1; }
tail -2 $out/pytest_gpu.log
timeout -k 10 600 python bench.py --full > $out/bench.json 2> $out/bench.err
cat $out/bench.json
cd /tmp && export TMPDIR=/tmp
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $R/$out/prof -o run -- python3 $R/bench.py --steps 3 --warmup 1 --full --no-cpu-baseline > $R/$out/bench_prof.json 2> $R/$out/prof.log
cd $R
cat $out/bench_prof.json
python scripts/trace_summary.py $out/prof/run_results.db > $out/kernels.md
head -12 $out/kernels.md
