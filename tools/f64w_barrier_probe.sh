# Timing-only probe (round 3): f64w without the barrier before digit 1's pass A (results invalid); the
# probe build lives in the test library (bench.py --test-lib --knob probe=4).
# Logs under $OUT_DIR/r03fp (default bench_out/r03fp).
set -u
O=${OUT_DIR:-bench_out}/r03fp
mkdir -p $O
for r in 1 2; do
  timeout -k 10 200 python3 bench.py --full --params STD192 --no-cpu-baseline --no-dropin --no-host-array --steps 2 > $O/base_$r.log 2>&1 || exit 1
  python3 -c "import json; d=json.loads([l for l in open('$O/base_$r.log') if l.startswith('{')][-1]); print('base rep $r', d['roofline']['kernel_ms'])" | tee -a $O/summary.txt
  timeout -k 10 200 python3 bench.py --full --test-lib --knob probe=4 --params STD192 --no-cpu-baseline --no-dropin --no-host-array --steps 2 > $O/nobar_$r.log 2>&1 || exit 1
  python3 -c "import json; d=json.loads([l for l in open('$O/nobar_$r.log') if l.startswith('{')][-1]); print('no-barrier rep $r', d['roofline']['kernel_ms'])" | tee -a $O/summary.txt
done
