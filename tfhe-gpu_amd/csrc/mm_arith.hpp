// mm_arith.hpp -- the arithmetic classes shared by the matrix-product kernels (mul_matrix.hip, conv2d.hip;
// DESIGN 3.9): which class a modulus takes, the tile and accumulator types of each, and the modular add.
#pragma once
#include <cstddef>
#include <cstdint>
#include <type_traits>

#include <hip/hip_runtime.h>

namespace tfhe {

using u128 = unsigned __int128;

enum MmMode { MM_M32 = 0, MM_M64 = 1, MM_GEN = 2, MM_GEN_TERM = 3 };

// the class of a sum of K products at `modulus` (> 0): a power of two wraps in 32 or 64 bits, any other modulus
// sums in u128 while K (m-1)^2 < 2^128 and reduces every term past that
inline int mm_mode_for(uint64_t modulus, size_t K) {
    if ((modulus & (modulus - 1)) == 0) return modulus <= (1ull << 32) ? MM_M32 : MM_M64;
    const u128 sq = (u128)(modulus - 1) * (modulus - 1);
    return (sq != 0 && sq > ~(u128)0 / K) ? MM_GEN_TERM : MM_GEN;
}

// (a + b) mod m for a, b < m <= 2^64 - 1 (the sum may carry out of 64 bits)
__device__ __forceinline__ uint64_t mm_addm(uint64_t a, uint64_t b, uint64_t m) {
    const uint64_t s = a + b;
    return (s < a || s >= m) ? s - m : s;
}

template <int MODE>
struct MmTypes {
    using Tile = std::conditional_t<MODE == MM_M32, uint32_t, uint64_t>;
    using Acc = std::conditional_t<MODE == MM_M32, uint32_t, std::conditional_t<MODE == MM_GEN, u128, uint64_t>>;
};

}  // namespace tfhe
