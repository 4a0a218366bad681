#!/bin/bash
# On a GPU machine: GPU test suite, smoke, the headline bench with everything it measures besides the figure
# (--full) at 8 frames per GPU, the plain bench at 1 / 4, and a rocprofv3 kernel trace of one bench step;
# everything lands in DIR (first argument, default validate_out/ in the repository root).  Every GPU step runs
# under a time limit, and the first one that fails, faults or times out ends the script.
set -e -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
O=$(mkdir -p "${1:-$R/validate_out}" && cd "${1:-$R/validate_out}" && pwd)
cd "$R"
timeout -k 10 1800 python -m pytest tests -m gpu -x -q > $O/pytest_gpu.log 2>&1 || { tail -30 $O/pytest_gpu.log; exit 1; }
tail -2 $O/pytest_gpu.log
timeout -k 10 300 python __graft_entry__.py --smoke > $O/smoke.log 2>&1 || { tail -30 $O/smoke.log; exit 1; }
tail -1 $O/smoke.log
timeout -k 10 600 python bench.py --full > $O/bench_full.json 2> $O/bench_full.err || { tail -30 $O/bench_full.err; exit 1; }
cat $O/bench_full.json
timeout -k 10 300 python bench.py --frames-per-gpu 1 > $O/bench_f1.json 2> $O/bench_f1.err || { tail -30 $O/bench_f1.err; exit 1; }
cut -c1-160 $O/bench_f1.json
timeout -k 10 300 python bench.py --frames-per-gpu 4 > $O/bench_f4.json 2> $O/bench_f4.err || { tail -30 $O/bench_f4.err; exit 1; }
cut -c1-160 $O/bench_f4.json
cd /tmp && export TMPDIR=/tmp
rm -rf $O/prof_final
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_final -- python3 $R/bench.py --steps 1 --warmup 0 --prime 1 > $O/prof_final.json 2> $O/prof_final.err || { tail -5 $O/prof_final.err; exit 1; }
cut -c1-160 $O/prof_final.json
echo done
