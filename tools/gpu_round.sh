#!/bin/bash
# One GPU session: tests, bench, kernel-trace profile (+ HIP API trace), each step under its own limit.
# usage: tools/gpu_round.sh <tag> [skip_tests]      (logs under ${OUT_DIR:-build/gpu_runs}/<tag>)
cd "$(dirname "$0")/.." || exit 2
export TMPDIR=/tmp
tag=${1:-run}
out=${OUT_DIR:-build/gpu_runs}/$tag
mkdir -p "$out"
if [ "$2" != "skip_tests" ]; then
  timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread \
    > "$out/pytest.log" 2>&1
  rc=$?; echo "pytest rc=$rc"; tail -15 "$out/pytest.log"
  if [ $rc -ge 2 ]; then exit $rc; fi
fi
timeout -k 10 300 python -u bench.py --full --steps 10 --warmup 3 > "$out/bench.log" 2>&1
rc=$?; echo "bench rc=$rc"; tail -c 3000 "$out/bench.log"
if [ $rc -ne 0 ]; then exit $rc; fi
timeout -k 10 300 rocprofv3 --kernel-trace --hip-trace --stats -d "$out/prof" -o run --output-format csv \
  -- python bench.py --steps 3 --warmup 1 > "$out/prof.log" 2>&1
rc=$?; echo "prof rc=$rc"; tail -3 "$out/prof.log"
exit $rc
