// arith_probes.hpp -- TEST LIBRARY ONLY (-DTFHE_TEST_PROBES, lib/libtfhe_hip_test.so): entry points that run the
// kernels' own arithmetic __device__ functions on operands the test supplies and return their raw results
// (tests/test_gpu_arith_units.py).  Not part of include/tfhe_hip.h; the product library has none of this.
//
// One entry point per family, each owned by the source whose functions it calls:
//   dm    device_math.hpp                 (arith_probes.hip)
//   kg    the keygen helpers              (keygen_kernels.hip)
//   g3    Harvey butterflies, gen3 cores  (blind_rotate_generic.hip)
//   sf    the special-form leaves         (blind_rotate_sf.hip)
//   f64   the exact-FP64 leaves           (blind_rotate_f64.hip)
//   fast4 signed Montgomery leaves        (blind_rotate_fast4.hip)
// Arguments, all families: op = the function (the family's table, next to its probe kernel) | width << 4 (1: the
// u32 instance, dm and g3) | (r + 1) << 8 to branch lanes with lane % 3 == r around the call (they store nothing:
// the function then runs under a partial exec mask); Q = the modulus the launcher's constants are built for;
// in = cases x ni words, out = cases x no words, tab = the twiddle table of the radix cores (two halves of
// tab_words / 2 for (W0, W1) / (w, companion) pairs), all device buffers.  Signed and double values travel as
// their 64-bit patterns (int32 sign-extended).  A case whose table index would leave the table stores nothing.
// Returns 0, -1 for an argument the entry point rejects (op, word counts), or the hipError_t of the launch.
#pragma once
#ifdef TFHE_TEST_PROBES

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

extern "C" {
#define TFHE_ARITH_PROBE(family)                                                                                  \
    int tfhe_test_arith_##family(int op, uint64_t Q, size_t cases, const uint64_t* in, size_t in_words,           \
                                 const uint64_t* tab, size_t tab_words, uint64_t* out, size_t out_words)
TFHE_ARITH_PROBE(dm);
TFHE_ARITH_PROBE(kg);
TFHE_ARITH_PROBE(g3);
TFHE_ARITH_PROBE(sf);
TFHE_ARITH_PROBE(f64);
TFHE_ARITH_PROBE(fast4);
}

namespace tfhe {

constexpr int kProbeThreads = 256;  // four wavefronts: carry and no-carry cases share wavefronts

// this lane runs case i (op's lane-mask field branches every third lane out)
__device__ __forceinline__ bool probe_lane_runs(int op, size_t i, size_t cases) {
    const int skip = (op >> 8) & 3;
    return i < cases && !(skip && (int)((threadIdx.x & 63) % 3) == skip - 1);
}

// checks the word counts, launches kern<<<ceil(cases / 256), 256>>>(op, cases, in, tab, tab_words, out, extra...)
// on the null stream and waits for it
template <class Kern, class... Extra>
int probe_launch(Kern kern, int ni, int no, int op, size_t cases, const uint64_t* in, size_t in_words,
                 const uint64_t* tab, size_t tab_words, uint64_t* out, size_t out_words, Extra... extra) {
    if (ni <= 0 || no <= 0 || cases == 0 || !in || !out || in_words != cases * (size_t)ni ||
        out_words != cases * (size_t)no || (tab_words != 0 && !tab))
        return -1;
    hipLaunchKernelGGL(kern, dim3((unsigned)((cases + kProbeThreads - 1) / kProbeThreads)), dim3(kProbeThreads), 0, 0, op,
                       cases, in, tab, tab_words, out, extra...);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return (int)e;
    return (int)hipDeviceSynchronize();
}

}  // namespace tfhe
#endif  // TFHE_TEST_PROBES
