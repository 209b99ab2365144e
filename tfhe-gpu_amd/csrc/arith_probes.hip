// arith_probes.hip -- TEST LIBRARY ONLY (lib/libtfhe_hip_test.so; the product library does not link this file):
// the arithmetic probe of device_math.hpp's functions (arith_probes.hpp, tests/test_gpu_arith_units.py).
// op (| 16: the u32 instance): 0 shoup_lazy(a, w, wp)  1 shoup(a, w, wp)  2 reduce_full(x, r1)  3 addm(a, b)
//     4 subm(a, b)  5 csub(a)  6 round_qQ(v, q, Q) (q and Q travel with the case; u64 only)
// 3 words in, 1 out per case; no table.  (sf_mul and fmodmul_f64 are probed with their families.)
#define TFHE_TEST_PROBES 1
#include "arith_probes.hpp"
#include "device_math.hpp"

namespace tfhe {
namespace {
constexpr int DMP_NI = 3, DMP_NO = 1;
template <typename W>
__global__ void k_arith_dm(int op, size_t cases, const uint64_t* __restrict__ in, const uint64_t* __restrict__, size_t,
                           uint64_t* __restrict__ out, uint64_t Q64) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (!probe_lane_runs(op, i, cases)) return;
    const uint64_t* x = in + i * DMP_NI;
    const W Q = (W)Q64;
    uint64_t r = 0;
    switch (op & 15) {
        case 0: r = shoup_lazy<W>((W)x[0], (W)x[1], (W)x[2], Q); break;
        case 1: r = shoup<W>((W)x[0], (W)x[1], (W)x[2], Q); break;
        case 2: r = reduce_full<W>((W)x[0], (W)x[1], Q); break;
        case 3: r = addm<W>((W)x[0], (W)x[1], Q); break;
        case 4: r = subm<W>((W)x[0], (W)x[1], Q); break;
        case 5: r = csub<W>((W)x[0], Q); break;
        default: r = round_qQ(x[0], x[1], x[2]); break;
    }
    out[i * DMP_NO] = r;
}
}  // namespace
}  // namespace tfhe

extern "C" TFHE_ARITH_PROBE(dm) {
    using namespace tfhe;
    const bool u32 = (op >> 4) & 1;
    if ((op & 15) > 6 || ((op & 15) == 6 && u32) || Q < 2 || (u32 && Q >= (1ull << 32))) return -1;
    if (u32)
        return probe_launch(k_arith_dm<uint32_t>, DMP_NI, DMP_NO, op, cases, in, in_words, tab, tab_words, out, out_words, Q);
    return probe_launch(k_arith_dm<uint64_t>, DMP_NI, DMP_NO, op, cases, in, in_words, tab, tab_words, out, out_words, Q);
}
