#!/bin/bash
# Build a test-library variant with extra defines for ONE source file (A/B of its compile-time knobs):
#   tools/alt_build.sh SRC TAG "-DNAME=VALUE ..."   ->   altlib/TAG/libtfhe_hip_test.so
# SRC: blind_rotate_sf | ks_tiled | ... (csrc/SRC.hip); the other objects are the tree's test-library ones.
set -eu
SRC=$1; TAG=$2; DEFS=$3
cd "$(dirname "$0")/../tfhe-gpu_amd"
make -s -j8 lib/libtfhe_hip_test.so
mkdir -p ../altlib/$TAG
CXX="/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -Wno-inline-asm -Wno-unused-value -Wno-unused-result -I../include -Icsrc"
EXTRA="-DTFHE_TEST_PROBES"
[ "$SRC" = blind_rotate_sf ] && EXTRA="$EXTRA -mllvm -pragma-unroll-threshold=100000"
$CXX $EXTRA $DEFS -c csrc/$SRC.hip -o ../altlib/$TAG/alt.o
# the test library's objects, with SRC's replaced (sources with a _probes object contribute that one)
OBJS=""
for o in build/*.o; do
  b=$(basename $o .o)
  [ -e build/${b}_probes.o ] && continue                              # product-only objects (the Makefile's PROBED)
  case $b in
    ${SRC}|${SRC}_probes) continue ;;                                 # replaced
  esac
  OBJS="$OBJS $o"
done
/opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 -pthread -o ../altlib/$TAG/libtfhe_hip_test.so $OBJS ../altlib/$TAG/alt.o
rm ../altlib/$TAG/alt.o
echo "built altlib/$TAG/libtfhe_hip_test.so ($SRC: $DEFS)"
