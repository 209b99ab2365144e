#!/bin/bash
# GPU-box validation recipe: GPU test suite, smoke(), the full bench line, rocprofv3 kernel stats.
# Usage (GPU box, from the repo root): bash tools/validate.sh TAG
# Output under $OUT_DIR/TAG (default bench_out/TAG).
set -u
TAG=${1:-val}
export TMPDIR=/tmp
O=${OUT_DIR:-bench_out}/$TAG
mkdir -p $O
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > $O/pytest_gpu.log 2>&1 &&
timeout -k 10 200 python -u -c "import __graft_entry__ as g; g.smoke()" > $O/smoke.log 2>&1 &&
timeout -k 10 300 python -u bench.py --full > $O/bench.log 2>&1 &&
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $O/prof -o run --output-format csv -- python3 bench.py --full --no-cpu-baseline > $O/prof.log 2>&1
rc=$?
echo "validate rc=$rc"
tail -3 $O/pytest_gpu.log
tail -1 $O/bench.log
exit $rc
