#!/bin/bash
# VGPR / spill summary per kernel of one object of the build, compiled with the flags tfhe-gpu_amd/Makefile gives it:
#   tools/regs.sh blind_rotate_f64 [name filter]          (build/blind_rotate_f64.o)
#   tools/regs.sh blind_rotate_sf_probes sfduo            (the test library's -DTFHE_TEST_PROBES object)
set -eu
cd "$(dirname "$0")/../tfhe-gpu_amd"
CMD=$(make -n -B "build/$1.o" | grep -- ' -c csrc/' | sed -e "s# -o build/$1\.o# -o /tmp/regs_$1.o#")
[ -n "$CMD" ] || { echo "no rule for build/$1.o" >&2; exit 1; }
eval "$CMD -Rpass-analysis=kernel-resource-usage" 2>&1 | python3 -c "
import sys, re
cur = None
for line in sys.stdin:
    if 'error' in line: print(line, end='')
    m = re.search(r'Function Name: (\S+)', line)
    if m: cur = m.group(1); print(); print(cur[:100], end=' ')
    for k in ('VGPRs:', 'AGPRs:', 'VGPRs Spill:', 'ScratchSize \[bytes/lane\]:', 'Occupancy \[waves/SIMD\]:'):
        m = re.search(k + r' (\d+)', line)
        if m: print(k.replace('\\\\', ''), m.group(1), end=' ')
print()
" | grep -E "${2:-.}"
