// ct_matmul.hip -- the two streaming kernels around the EvalFunc batch of a product of two encrypted tensors
// (tfhe_ct_matmul).  A slice holds whole outputs o = (i rows + r) cols + c, [first_out, first_out +
// count / inner); item `it` of the slice is product (o, k), k innermost:
//     k_ctmm_pairs    z[it] = x[i][r][k] + y[i][k][c] mod q,  z[count + it] = x[i][r][k] - y[i][k][c] mod q
//                     the flat EvalFunc input: the sums take the call's first table, the differences its second
//     k_ctmm_reduce   out[o] = sum_k f[o' inner + k] - f[count + o' inner + k] mod q,  o' = o - first_out
// q is a power of two: the modular step is a mask, and since q divides 2^64 the sum may wrap in a u64 register and be
// masked once.  No input word is written.
//
// Layout, as pool2d.hip.  A workgroup of CM_THREADS threads takes CM_ITEMS items at a time, one per wave, and strides
// over the rest by the grid: the item and its rows are wave-uniform, decoded once per item (three divisions), never
// per word; y_transposed and y_shared only change the row's address.  The 64 lanes sweep the row's n+1 words with
// 8-byte accesses, 512 contiguous bytes per wave-instruction; rows are only 8-byte aligned (n+1 words each), so
// nothing wider is used.  The reduction keeps one word's sum per lane in a register and walks k: every step reads
// two rows, each contiguous.  No LDS, no atomics.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.hpp"

namespace tfhe {

namespace {

constexpr unsigned CM_MAX_GRID = 2048;  // memory-bound: a few workgroups per CU, the rest by grid stride

__global__ __launch_bounds__(CM_THREADS) void k_ctmm_pairs(CtmmArgs p, uint64_t* __restrict__ z) {
    const uint32_t lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (size_t it = (size_t)blockIdx.x * CM_ITEMS + wave; it < p.count; it += (size_t)gridDim.x * CM_ITEMS) {
        const size_t ol = it / p.inner, k = it - ol * p.inner, o = p.first_out + ol;
        const size_t ir = o / p.cols, c = o - ir * p.cols, i = ir / p.rows;
        const uint64_t* xr = p.x + (ir * p.inner + k) * p.width;
        const size_t yi = (p.y_shared ? 0 : i * p.inner * p.cols) + (p.y_transposed ? c * p.inner + k : k * p.cols + c);
        const uint64_t* yr = p.y + yi * p.width;
        uint64_t *zs = z + it * p.width, *zd = z + (p.count + it) * p.width;
#pragma unroll 4
        for (uint32_t j = lane; j < p.width; j += 64) {
            const uint64_t a = xr[j], b = yr[j];
            zs[j] = (a + b) & p.mask;
            zd[j] = (a - b) & p.mask;
        }
    }
}

__global__ __launch_bounds__(CM_THREADS) void k_ctmm_reduce(CtmmArgs p, const uint64_t* __restrict__ f,
                                                            uint64_t* __restrict__ out) {
    const uint32_t lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const size_t nout = p.count / p.inner;
    for (size_t ol = (size_t)blockIdx.x * CM_ITEMS + wave; ol < nout; ol += (size_t)gridDim.x * CM_ITEMS) {
        const uint64_t *fs = f + ol * p.inner * p.width, *fd = fs + p.count * p.width;
        uint64_t* dst = out + (p.first_out + ol) * p.width;
        for (uint32_t j = lane; j < p.width; j += 64) {
            uint64_t acc = 0;
#pragma unroll 4
            for (size_t k = 0; k < p.inner; ++k) acc += fs[k * p.width + j] - fd[k * p.width + j];
            dst[j] = acc & p.mask;
        }
    }
}

unsigned ctmm_grid(size_t items) { return (unsigned)std::min<size_t>((items + CM_ITEMS - 1) / CM_ITEMS, CM_MAX_GRID); }

bool ctmm_ok(const CtmmArgs& p) {
    return p.rows && p.inner && p.cols && p.count % p.inner == 0 && p.y_transposed <= 1 && p.y_shared <= 1;
}

}  // namespace

hipError_t launch_ctmm_pairs(const CtmmArgs& p, uint64_t* z, hipStream_t s) {
    if (p.count == 0 || p.width == 0) return hipSuccess;
    if (!ctmm_ok(p)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_ctmm_pairs, dim3(ctmm_grid(p.count)), dim3(CM_THREADS), 0, s, p, z);
    return hipGetLastError();
}

hipError_t launch_ctmm_reduce(const CtmmArgs& p, const uint64_t* f, uint64_t* out, hipStream_t s) {
    if (p.count == 0 || p.width == 0) return hipSuccess;
    if (!ctmm_ok(p)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_ctmm_reduce, dim3(ctmm_grid(p.count / p.inner)), dim3(CM_THREADS), 0, s, p, f, out);
    return hipGetLastError();
}

}  // namespace tfhe
