#!/bin/bash
# Round GPU check: the whole -m gpu suite (one process), smoke, then the
# driver-shaped bench.  Every GPU step has its own time limit; the first
# failure ends the call.
set -o pipefail
mkdir -p bench_out
export TMPDIR=/tmp
timeout -k 10 1500 python -u -m pytest tests -m gpu -x -v -p no:cacheprovider --timeout 900 --timeout-method thread "$@" > bench_out/gpu_tests.log 2>&1 || { echo "TESTS FAILED"; tail -60 bench_out/gpu_tests.log; exit 1; }
tail -3 bench_out/gpu_tests.log
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > bench_out/smoke.log 2>&1 || { echo SMOKE FAILED; cat bench_out/smoke.log; exit 1; }
cat bench_out/smoke.log
timeout -k 10 600 python bench.py --full --steps 20 --warmup 5 > bench_out/bench.json 2> bench_out/bench.err || { echo BENCH FAILED; tail -20 bench_out/bench.err; exit 1; }
python3 tools/bench_summary.py bench_out/bench.json
