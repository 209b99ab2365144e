#!/bin/bash
# L1/L2 behaviour of the blind-rotation kernel (one --pmc pass, no tracing domains).
# Usage: tools/pmc_cache.sh TAG [bench args]   (TFHE_FAST_VARIANT selects the kernel variant)
# Output under $OUT_DIR (default bench_out/).
set -u
TAG=${1:-cache}
shift || true
export TMPDIR=/tmp
O=${OUT_DIR:-bench_out}
mkdir -p $O
timeout -k 10 300 rocprofv3 --pmc TCP_TOTAL_CACHE_ACCESSES_sum TCP_TCC_READ_REQ_sum TCC_HIT_sum TCC_MISS_sum -d $O/${TAG} -o run --output-format csv -- python3 bench.py --full --no-cpu-baseline --steps 1 --warmup 0 "$@" > $O/${TAG}.log 2>&1
rc=$?
python3 - "$O/$TAG" <<'PY'
import csv, glob, os, sys, collections
d = sys.argv[1]
tag = os.path.basename(d)
agg = collections.defaultdict(list)
for f in glob.glob(f"{d}/**/*counter_collection.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        if "blind_rotate" in r["Kernel_Name"]:
            agg[r["Counter_Name"]].append(float(r["Counter_Value"]))
for k, v in sorted(agg.items()):
    print(f"{tag} {k:28s} per-launch {sum(v)/len(v):.4g} (n={len(v)})")
PY
exit $rc
