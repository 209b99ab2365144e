// mul_matrix.hip -- the tiled CiphertextMulMatrix:
//     out[i][c][w] = (bias[c] [w == n] + sum_k matrix[k][c] ct[i][k][w]) mod m,   i < instances, c < cols, w <= n
// with ct [instances][K][n+1] u64, the matrix [K][cols] int64 shared by every instance and bias [cols] u64 (or
// null) added to the b word only, as EvalAddConstEq.  No input is written.
//
// The reference computes the product as an FP64 DGEMM and fmod (lwe-operation.cu:106-111), exact only while
// |sums| < 2^53 and non-negative; here every sum is exact at every modulus.
//
// Layout.  A workgroup of MM_THREADS threads owns MM_THREADS consecutive words w of one instance and a tile of
// MM_CT output columns; every thread keeps MM_CT accumulators in registers.  The matrix tile [MM_KT][MM_CT] sits
// in LDS and every lane of a wave reads the same word of it (a broadcast: no bank conflict); a ciphertext word
// is loaded once per k, coalesced across w, and used MM_CT times -- the first-draft kernel (one workgroup per
// column) read it once per column.  Column tiles are the grid's x, so that workgroups dispatched together share
// one [K][MM_THREADS] slab of the ciphertexts in L2.
//
// A pre-pass (k_mm_reduce_matrix) writes the residues of the signed entries into a scratch of K cols words.
// Three arithmetic instances, chosen on the host from the modulus:
//   M32  m = 2^k, k <= 32       32-bit wrapping multiply-add on the low words, masked at the end
//   M64  m = 2^k, 33 <= k <= 63 low-64-bit wrapping multiply-add, masked at the end
//   GEN  any other modulus      operands in [0, m) (ciphertext words reduced on load); unreduced u128 sum
//                               while K (m-1)^2 < 2^128 (GEN), else a modular add per term (GEN_TERM)
// M32 / M64 are exact because 2^k divides 2^32 / 2^64 and a signed entry's two's-complement word is congruent
// to it mod 2^64.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.hpp"
#include "mm_arith.hpp"

namespace tfhe {

namespace {

// signed entries -> residues: a power-of-two modulus masks the two's-complement word, any other takes the
// mathematical residue through __int128
__global__ void k_mm_reduce_matrix(const int64_t* __restrict__ mat, size_t count, uint64_t modulus, int pow2,
                                   uint64_t* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const int64_t v = mat[i];
    if (pow2) {
        out[i] = (uint64_t)v & (modulus - 1);
    } else {
        __int128 r = (__int128)v % (__int128)modulus;
        if (r < 0) r += modulus;
        out[i] = (uint64_t)r;
    }
}

// grid: x = column tile, y = block of MM_THREADS words, z = instance
template <int MODE>
__global__ __launch_bounds__(MM_THREADS) void k_mm_tile(uint32_t width, size_t K, const uint64_t* __restrict__ ct,
                                                        size_t cols, const uint64_t* __restrict__ mat,
                                                        const uint64_t* __restrict__ bias, uint64_t modulus,
                                                        uint64_t* __restrict__ out) {
    using Tile = typename MmTypes<MODE>::Tile;
    using Acc = typename MmTypes<MODE>::Acc;
    // k steps in flight: two keep the power-of-two instances at 7 to 8 waves per SIMD; the u128 accumulators of
    // GEN leave room for one
    constexpr int UNROLL_K = MODE <= MM_M64 ? 2 : 1;
    __shared__ Tile tile[MM_KT][MM_CT];
    const uint32_t w = blockIdx.y * MM_THREADS + threadIdx.x;
    const size_t c0 = (size_t)blockIdx.x * MM_CT;
    const size_t inst = blockIdx.z;
    const bool live = w < width;
    const uint64_t* ctp = ct + inst * K * width + w;  // dereferenced only when live
    Acc acc[MM_CT];
#pragma unroll
    for (int cc = 0; cc < MM_CT; ++cc) acc[cc] = 0;

    for (size_t k0 = 0; k0 < K; k0 += MM_KT) {
        const int kn = (int)std::min<size_t>(MM_KT, K - k0);
        __syncthreads();  // the previous tile has been consumed
        for (int i = threadIdx.x; i < MM_KT * MM_CT; i += MM_THREADS) {
            const int kk = i / MM_CT, cc = i % MM_CT;
            const size_t k = k0 + kk, c = c0 + cc;
            tile[kk][cc] = (k < K && c < cols) ? (Tile)mat[k * cols + c] : (Tile)0;  // tails in K and cols: zeros
        }
        __syncthreads();
        if (live) {
#pragma unroll UNROLL_K
            for (int kk = 0; kk < kn; ++kk) {
                uint64_t v = ctp[(k0 + kk) * width];
                if (MODE == MM_GEN || MODE == MM_GEN_TERM) {
                    if (v >= modulus) v %= modulus;  // reduced on load; inputs are usually reduced already
                }
#pragma unroll
                for (int cc = 0; cc < MM_CT; ++cc) {
                    const Tile t = tile[kk][cc];
                    if (MODE == MM_M32) acc[cc] += (Acc)((uint32_t)t * (uint32_t)v);
                    else if (MODE == MM_M64) acc[cc] += (Acc)((uint64_t)t * v);
                    else if (MODE == MM_GEN) acc[cc] += (Acc)((u128)t * v);
                    else acc[cc] = (Acc)mm_addm((uint64_t)acc[cc], (uint64_t)(((u128)t * v) % modulus), modulus);
                }
            }
        }
    }
    if (!live) return;
    const bool isb = bias != nullptr && w == width - 1;
#pragma unroll
    for (int cc = 0; cc < MM_CT; ++cc) {
        const size_t c = c0 + cc;
        if (c >= cols) break;
        uint64_t r;
        if (MODE == MM_M32 || MODE == MM_M64) {
            Acc a = acc[cc];
            if (isb) a += (Acc)bias[c];
            r = (uint64_t)a & (modulus - 1);
        } else {
            r = MODE == MM_GEN ? (uint64_t)(acc[cc] % modulus) : (uint64_t)acc[cc];
            if (isb) r = mm_addm(r, bias[c] % modulus, modulus);
        }
        out[(inst * cols + c) * width + w] = r;
    }
}

template <int MODE>
void mm_launch(dim3 grid, uint32_t width, size_t K, const uint64_t* ct, size_t cols, const uint64_t* mat,
               const uint64_t* bias, uint64_t modulus, uint64_t* out, hipStream_t s) {
    hipLaunchKernelGGL(k_mm_tile<MODE>, grid, dim3(MM_THREADS), 0, s, width, K, ct, cols, mat, bias, modulus, out);
}

}  // namespace

hipError_t launch_mul_matrix(uint32_t width, size_t instances, size_t K, const uint64_t* ct, size_t cols,
                             const int64_t* matrix, const uint64_t* bias, uint64_t modulus, uint64_t* mat_scratch,
                             uint64_t* out, hipStream_t s) {
    if (instances == 0 || K == 0 || cols == 0 || width == 0) return hipSuccess;
    if (modulus == 0) return hipErrorInvalidValue;
    const size_t col_tiles = (cols + MM_CT - 1) / MM_CT, w_blocks = ((size_t)width + MM_THREADS - 1) / MM_THREADS;
    if (col_tiles > 0x7fffffffull || w_blocks > 65535) return hipErrorInvalidValue;
    const bool pow2 = (modulus & (modulus - 1)) == 0;
    const int mode = mm_mode_for(modulus, K);
    const size_t nm = K * cols;
    hipLaunchKernelGGL(k_mm_reduce_matrix, dim3((unsigned)((nm + 255) / 256)), dim3(256), 0, s, matrix, nm, modulus,
                       (int)pow2, mat_scratch);
    const size_t zmax = 65535;  // the grid's z limit: more instances take several launches
    for (size_t first = 0; first < instances; first += zmax) {
        const size_t cnt = std::min(zmax, instances - first);
        const dim3 grid((unsigned)col_tiles, (unsigned)w_blocks, (unsigned)cnt);
        const uint64_t* cti = ct + first * K * width;
        uint64_t* outi = out + first * cols * width;
        switch (mode) {
            case MM_M32: mm_launch<MM_M32>(grid, width, K, cti, cols, mat_scratch, bias, modulus, outi, s); break;
            case MM_M64: mm_launch<MM_M64>(grid, width, K, cti, cols, mat_scratch, bias, modulus, outi, s); break;
            case MM_GEN: mm_launch<MM_GEN>(grid, width, K, cti, cols, mat_scratch, bias, modulus, outi, s); break;
            default: mm_launch<MM_GEN_TERM>(grid, width, K, cti, cols, mat_scratch, bias, modulus, outi, s); break;
        }
    }
    return hipGetLastError();
}

}  // namespace tfhe
