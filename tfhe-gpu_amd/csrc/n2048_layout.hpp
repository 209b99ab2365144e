// n2048_layout.hpp -- the N = 2048 thread / LDS layout that gen3 (blind_rotate_generic.hip) and the special-form
// kernels (blind_rotate_sf.hip) share: 512 threads, 4 slots of both polynomials per thread, radix-8 register
// passes over an XOR-swizzled buffer (the FP64 kernel's layout, blind_rotate_f64.hip ad_A/ad_B/ad_C; the swizzle
// and the index algebra are checked by tools/lds_layouts_f64.py and tools/lds_layouts_wl.py).
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace tfhe {

constexpr uint32_t G3_N = 2048, G3_TH = 512, G3_CN = 4;

__device__ __forceinline__ uint32_t g3_swz(uint32_t x) {
    const uint32_t c = (x >> 5) & 7;
    return x ^ (c << 2) ^ (c & 3);
}
__device__ __forceinline__ uint32_t g3_swzf(uint32_t c) { return (c << 2) ^ (c & 3); }

// element addresses of the passes
__device__ __forceinline__ void g3_ad(int pass, uint32_t tau, uint32_t (&ad)[8]) {
    if (pass == 0) {
        const uint32_t a0 = g3_swz(tau);
#pragma unroll
        for (uint32_t k = 0; k < 8; ++k) ad[k] = a0 + 256 * k;
    } else if (pass == 1) {
        const uint32_t b0 = ((tau >> 5) << 8) + (tau & 31);
#pragma unroll
        for (uint32_t k = 0; k < 8; ++k) ad[k] = (b0 ^ g3_swzf(k)) + 32 * k;
    } else {
        const uint32_t c0 = g3_swz(((tau >> 2) << 5) + (tau & 3));
#pragma unroll
        for (uint32_t k = 0; k < 8; ++k) ad[k] = c0 ^ (4 * k);
    }
}

__device__ __forceinline__ uint32_t g3_tau() {
    uint32_t tau = threadIdx.x & 255;
    asm volatile("" : "+v"(tau));  // keep the passes' addresses out of the round loop
    return tau;
}

// The epilogue of the N = 2048 kernels: buf holds the accumulator (acc0 at [0, N), acc1 at [N, 2N), canonical
// values); acc0 leaves transposed (X -> X^-1, poly.cpp:762-770), acc1 as it is.  The caller has synchronised.
template <typename W>
__device__ __forceinline__ void g3_store_acc(const W* buf, uint64_t* g, uint32_t t, W Q) {
    for (uint32_t k = t; k < G3_N; k += G3_TH) {
        const uint64_t v = buf[k == 0 ? 0 : G3_N - k];
        g[k] = k == 0 ? v : (v == 0 ? 0 : (uint64_t)Q - v);
        g[G3_N + k] = buf[G3_N + k];
    }
}

}  // namespace tfhe
