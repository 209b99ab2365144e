// pool2d.hip -- the two streaming kernels around each round of a windowed pairwise reduction (tfhe_pool2d; DESIGN
// 3.11).  A round's pairs over every instance and plane are one flat batch, item = (instance c + plane) nrec + r
// with r the record of the plane's plan (pool.hpp):
//     k_pool_diff   z[item] = a - b mod q          the flat EvalFunc input
//     k_pool_add    dst     = f[item] + b mod q    scattered to the slot store or to the output position
//     k_pool_add<COPY>  dst = b                    positions with one valid tap (a 1 x 1 window: a strided copy)
// q is a power of two: the modular step is a mask.  No input word is written.
//
// Layout.  A workgroup of PL_THREADS threads takes PL_ITEMS items at a time, one per wave, and strides over the
// rest by the grid: the item, its plane and its record are wave-uniform, decoded once per item (one division, three
// scalar loads), never per word.  The 64 lanes sweep the row's n+1 words with 8-byte accesses, 512 contiguous bytes
// per wave-instruction; rows are only 8-byte aligned (n+1 words each), so nothing wider is used.  No LDS, no
// atomics.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.hpp"

namespace tfhe {

namespace {

constexpr unsigned PL_MAX_GRID = 2048;  // memory-bound: a few workgroups per CU, the rest by grid stride

// the row a record names inside plane ip: >= 0 a row of `plane` (input taps / output positions), < 0 slot ~r
__device__ __forceinline__ uint64_t* pool_row(int64_t r, size_t ip, uint64_t* plane, size_t plane_words,
                                              uint64_t* slots, size_t slot_words, uint32_t width) {
    return r >= 0 ? plane + ip * plane_words + (size_t)r * width : slots + ip * slot_words + (size_t)~r * width;
}

__global__ __launch_bounds__(PL_THREADS) void k_pool_diff(PoolArgs p, uint64_t* __restrict__ z) {
    const uint32_t lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (size_t it = (size_t)blockIdx.x * PL_ITEMS + wave; it < p.count; it += (size_t)gridDim.x * PL_ITEMS) {
        const size_t item = p.first + it, ip = item / p.nrec;
        const PoolRec rec = p.recs[item - ip * p.nrec];
        uint64_t* in = const_cast<uint64_t*>(p.in);  // read only
        const uint64_t* a = pool_row(rec.a, ip, in, p.in_plane, p.slots, p.slot_plane, p.width);
        const uint64_t* b = pool_row(rec.b, ip, in, p.in_plane, p.slots, p.slot_plane, p.width);
        uint64_t* zr = z + it * p.width;
#pragma unroll 4
        for (uint32_t j = lane; j < p.width; j += 64) zr[j] = (a[j] - b[j]) & p.mask;
    }
}

template <bool COPY>
__global__ __launch_bounds__(PL_THREADS) void k_pool_add(PoolArgs p, const uint64_t* __restrict__ f) {
    const uint32_t lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (size_t it = (size_t)blockIdx.x * PL_ITEMS + wave; it < p.count; it += (size_t)gridDim.x * PL_ITEMS) {
        const size_t item = p.first + it, ip = item / p.nrec;
        const PoolRec rec = p.recs[item - ip * p.nrec];
        const uint64_t* b = pool_row(rec.b, ip, const_cast<uint64_t*>(p.in), p.in_plane, p.slots, p.slot_plane, p.width);
        uint64_t* dst = pool_row(rec.dst, ip, p.out, p.out_plane, p.slots, p.slot_plane, p.width);
        const uint64_t* fr = COPY ? nullptr : f + it * p.width;
#pragma unroll 4
        for (uint32_t j = lane; j < p.width; j += 64) dst[j] = COPY ? b[j] : (fr[j] + b[j]) & p.mask;
    }
}

unsigned pool_grid(size_t count) { return (unsigned)std::min<size_t>((count + PL_ITEMS - 1) / PL_ITEMS, PL_MAX_GRID); }

}  // namespace

hipError_t launch_pool_diff(const PoolArgs& p, uint64_t* z, hipStream_t s) {
    if (p.count == 0 || p.width == 0) return hipSuccess;
    if (p.nrec == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pool_diff, dim3(pool_grid(p.count)), dim3(PL_THREADS), 0, s, p, z);
    return hipGetLastError();
}

hipError_t launch_pool_add(const PoolArgs& p, const uint64_t* f, hipStream_t s) {
    if (p.count == 0 || p.width == 0) return hipSuccess;
    if (p.nrec == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pool_add<false>, dim3(pool_grid(p.count)), dim3(PL_THREADS), 0, s, p, f);
    return hipGetLastError();
}

hipError_t launch_pool_copy(const PoolArgs& p, hipStream_t s) {
    if (p.count == 0 || p.width == 0) return hipSuccess;
    if (p.nrec == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pool_add<true>, dim3(pool_grid(p.count)), dim3(PL_THREADS), 0, s, p, (const uint64_t*)nullptr);
    return hipGetLastError();
}

}  // namespace tfhe
