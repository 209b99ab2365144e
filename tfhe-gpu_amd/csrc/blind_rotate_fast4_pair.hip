// blind_rotate_fast4_pair.hip -- the pair instance of the four-wavefront kernel at the STD128 shape: two
// ciphertexts per wavefront (every key row loaded feeds both), three workgroups per CU (MINW = 3: 168 VGPRs),
// key ring two groups deep, no pass-4 table area in LDS (50.1 KiB per workgroup).  A translation unit of its
// own because of the scheduler: under max-ilp it allocates 168 VGPRs with no scratch access in the round loop,
// under blind_rotate_fast4.hip's iterative-ilp it spills 6 to 12 registers there (Makefile).
// Two builds: the radix-4 passes as fused groups (PAIR_FU; kernel variant 71) and as plain butterflies (70).
#define TFHE_FAST4_KERNEL_ONLY
#include "blind_rotate_fast4.hip"

namespace tfhe {

// The fused passes that met the register gate (168 VGPRs, no scratch access in the round loop): all but
// the forward pass 4, whose two more per-lane products cost 4 scratch loads per round.
#ifndef TFHE_PAIR_FU
#define TFHE_PAIR_FU (f4::FU_ALL & ~f4::FU_F4)
#endif
constexpr int PAIR_FU = TFHE_PAIR_FU;

hipError_t launch_blind_rotate_fast4_pair(const f4::FastConst& K, uint32_t n, uint32_t loga, const int32_t* tabs4,
                                          const int32_t* bsk, const uint64_t* a, uint64_t* acc, size_t B, hipStream_t s,
                                          bool fused) {
    auto kern = fused ? f4::k_blind_rotate_fast4<3, 2, 0, 7, 1, 1, 4, 7, 0, true, false, false, 2, PAIR_FU>
                      : f4::k_blind_rotate_fast4<3, 2, 0, 7, 1, 1, 4, 7, 0, true, false, false, 2>;
    const size_t lb = f4::lds_bytes(4, 1, 1, false);
    (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lb);
    hipLaunchKernelGGL(kern, dim3((unsigned)((B + 1) / 2)), dim3(f4::TPC), lb, s, K, n, loga, tabs4, bsk, a, acc,
                       (uint32_t)B, nullptr);
    return hipGetLastError();
}

}  // namespace tfhe
