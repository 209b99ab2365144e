// conv2d.hip -- Conv2d on ciphertexts: the tiled matrix product of mul_matrix.hip with the im2col gather inside
// the kernel.  With Cg = c_in / groups, Og = c_out / groups and o = g Og + c:
//     out[i][o][oy][ox][w] = (bias[o] [w == n] + sum_{ic < Cg, ky < kh, kx < kw}
//                             weight[o][ic][ky][kx] ct[i][g Cg + ic][oy sh - ph + ky][ox sw - pw + kx][w]) mod m
// ct [instances][c_in][h][w][n+1] u64, weight [c_out][Cg][kh][kw] int64 (OIHW) shared by every instance, bias
// [c_out] u64 (or null) added to the b word only, out [instances][c_out][oh][ow][n+1].  A tap outside the plane is
// zero padding and contributes nothing.  No input is written, and no im2col buffer exists.
//
// Layout.  A workgroup of CV_THREADS threads owns CV_THREADS consecutive words w of one instance, a tile of CV_CT
// output planes of ONE group (a tile never crosses a group: each group's last tile has its own tail) and CV_P
// consecutive output positions; every thread keeps CV_P CV_CT accumulators in registers.  Per K-tile of CV_KT
// taps (k = (ic kh + ky) kw + kx, K = Cg kh kw) the weights [CV_KT][CV_CT] and a table src[CV_P][CV_KT] of the
// taps' source offsets sit in LDS: src is the word offset of the tap's ciphertext inside the instance, or -1 where
// the tap falls in the padding.  Both are the same for every lane, so the inner loop reads them as broadcasts,
// moves the offset to scalar registers and branches on it: a padded tap costs no load, and no lane divides.  A
// ciphertext word is loaded once per tap and position, coalesced across w, and used CV_CT times.
//
// Grid.  One dimension, decoded as (instance, word block, position tile, plane tile) with the plane tile
// fastest, after a remap that hands each XCD a contiguous run of those ids: workgroups that read the same
// [c_in][h][w][CV_THREADS] slab of one instance then share one L2.  The remap is a speed choice only.
//
// The pre-pass (k_conv_reduce_weights) writes the residues of the signed weights into a scratch of c_out K words in
// the order the tile load reads, [group][K][Og].  The arithmetic classes are mul_matrix.hip's (mm_arith.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.hpp"
#include "mm_arith.hpp"

namespace tfhe {

namespace {

// what the kernels need of the geometry, computed once on the host
struct ConvDims {
    ConvGeom g;
    uint32_t Cg, Og;
    uint32_t khw;            // kh kw
    uint32_t group_tiles;    // plane tiles per group
    uint32_t plane_tiles;    // groups group_tiles
    uint32_t w_blocks;
    size_t K, npos, pos_tiles;
};

// OIHW signed weights -> residues in [group][K][Og]: a power-of-two modulus masks the two's-complement word, any
// other takes the mathematical residue through __int128 (as k_mm_reduce_matrix)
__global__ void k_conv_reduce_weights(const int64_t* __restrict__ weight, size_t count, size_t K, uint32_t Og,
                                      uint64_t modulus, int pow2, uint64_t* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;  // destination index (g K + k) Og + c
    if (i >= count) return;
    const size_t gk = i / Og, c = i % Og, g = gk / K, k = gk % K;
    const int64_t v = weight[(g * Og + c) * K + k];
    if (pow2) {
        out[i] = (uint64_t)v & (modulus - 1);
    } else {
        __int128 r = (__int128)v % (__int128)modulus;
        if (r < 0) r += modulus;
        out[i] = (uint64_t)r;
    }
}

// the run of logical ids of one XCD is contiguous: blocks with the same id % 8 share an XCD (bijective for
// every nwg)
__device__ __forceinline__ uint32_t conv_xcd_remap(uint32_t bid, uint32_t nwg) {
    const uint32_t xcd = bid % 8, q = nwg / 8, r = nwg % 8;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + bid / 8;
}

// grid: x = workgroup id of this launch; base = the logical id of its first workgroup
template <int MODE>
__global__ __launch_bounds__(CV_THREADS) void k_conv2d_tile(ConvDims d, uint32_t width, const uint64_t* __restrict__ ct,
                                                            const uint64_t* __restrict__ mat,
                                                            const uint64_t* __restrict__ bias, uint64_t modulus,
                                                            uint64_t* __restrict__ out, size_t base) {
    using Tile = typename MmTypes<MODE>::Tile;
    using Acc = typename MmTypes<MODE>::Acc;
    __shared__ Tile tile[CV_KT][CV_CT];
    __shared__ long long src[CV_P][CV_KT];

    size_t id = base + conv_xcd_remap(blockIdx.x, gridDim.x);
    const uint32_t ptile = (uint32_t)(id % d.plane_tiles);
    id /= d.plane_tiles;
    const size_t pos0 = (id % d.pos_tiles) * CV_P;
    id /= d.pos_tiles;
    const uint32_t w = (uint32_t)(id % d.w_blocks) * CV_THREADS + threadIdx.x;
    const size_t inst = id / d.w_blocks;
    const uint32_t grp = ptile / d.group_tiles, c0 = (ptile % d.group_tiles) * CV_CT;  // c0: plane inside the group
    const size_t K = d.K;
    const bool live = w < width;
    const uint64_t* ctp = ct + inst * d.g.c_in * d.g.h * d.g.w * width + w;  // dereferenced only when live
    const uint64_t* matg = mat + (size_t)grp * K * d.Og;

    Acc acc[CV_P][CV_CT];
#pragma unroll
    for (int p = 0; p < CV_P; ++p)
#pragma unroll
        for (int cc = 0; cc < CV_CT; ++cc) acc[p][cc] = 0;

    for (size_t k0 = 0; k0 < K; k0 += CV_KT) {
        const int kn = (int)std::min<size_t>(CV_KT, K - k0);
        __syncthreads();  // the previous tile has been consumed
        for (int i = threadIdx.x; i < CV_KT * CV_CT; i += CV_THREADS) {
            const int kk = i / CV_CT, cc = i % CV_CT;
            const size_t k = k0 + kk;
            const uint32_t c = c0 + cc;
            tile[kk][cc] = (k < K && c < d.Og) ? (Tile)matg[k * d.Og + c] : (Tile)0;  // tails in K and the group
        }
        // the taps' sources, once per K-tile: the divisions are here, not in the inner loop
        for (int i = threadIdx.x; i < CV_P * CV_KT; i += CV_THREADS) {
            const int p = i / CV_KT, kk = i % CV_KT;
            const size_t k = k0 + kk, pos = pos0 + p;
            long long off = -1;
            if (k < K && pos < d.npos) {
                const size_t ic = k / d.khw;
                const uint32_t r = (uint32_t)(k % d.khw), ky = r / d.g.kw, kx = r % d.g.kw;
                const long long oy = (long long)(pos / d.g.ow), ox = (long long)(pos % d.g.ow);
                const long long iy = oy * d.g.sh - d.g.ph + ky, ix = ox * d.g.sw - d.g.pw + kx;
                if (iy >= 0 && iy < (long long)d.g.h && ix >= 0 && ix < (long long)d.g.w)
                    off = (long long)(((((size_t)grp * d.Cg + ic) * d.g.h + (size_t)iy) * d.g.w + (size_t)ix) * width);
            }
            src[p][kk] = off;
        }
        __syncthreads();
        if (live) {
            for (int kk = 0; kk < kn; ++kk) {
#pragma unroll
                for (int p = 0; p < CV_P; ++p) {
                    // the same word for every lane: keep it scalar, so that the skip is a scalar branch
                    const long long o = src[p][kk];
                    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)o);
                    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)((unsigned long long)o >> 32));
                    const long long off = (long long)(((unsigned long long)hi << 32) | lo);
                    if (off < 0) continue;  // zero padding (or a position past the end): nothing is loaded
                    uint64_t v = ctp[off];
                    if (MODE == MM_GEN || MODE == MM_GEN_TERM) {
                        if (v >= modulus) v %= modulus;  // reduced on load; inputs are usually reduced already
                    }
#pragma unroll
                    for (int cc = 0; cc < CV_CT; ++cc) {
                        const Tile t = tile[kk][cc];
                        if (MODE == MM_M32) acc[p][cc] += (Acc)((uint32_t)t * (uint32_t)v);
                        else if (MODE == MM_M64) acc[p][cc] += (Acc)((uint64_t)t * v);
                        else if (MODE == MM_GEN) acc[p][cc] += (Acc)((u128)t * v);
                        else acc[p][cc] = (Acc)mm_addm((uint64_t)acc[p][cc], (uint64_t)(((u128)t * v) % modulus), modulus);
                    }
                }
            }
        }
    }
    if (!live) return;
    const bool isb = bias != nullptr && w == width - 1;
#pragma unroll
    for (int p = 0; p < CV_P; ++p) {
        const size_t pos = pos0 + p;
        if (pos >= d.npos) break;
#pragma unroll
        for (int cc = 0; cc < CV_CT; ++cc) {
            if (c0 + cc >= d.Og) break;
            const size_t o = (size_t)grp * d.Og + c0 + cc;
            uint64_t r;
            if (MODE == MM_M32 || MODE == MM_M64) {
                Acc a = acc[p][cc];
                if (isb) a += (Acc)bias[o];
                r = (uint64_t)a & (modulus - 1);
            } else {
                r = MODE == MM_GEN ? (uint64_t)(acc[p][cc] % modulus) : (uint64_t)acc[p][cc];
                if (isb) r = mm_addm(r, bias[o] % modulus, modulus);
            }
            out[((inst * d.g.c_out + o) * d.npos + pos) * width + w] = r;
        }
    }
}

template <int MODE>
void conv_launch(unsigned nwg, const ConvDims& d, uint32_t width, const uint64_t* ct, const uint64_t* mat,
                 const uint64_t* bias, uint64_t modulus, uint64_t* out, size_t base, hipStream_t s) {
    hipLaunchKernelGGL(k_conv2d_tile<MODE>, dim3(nwg), dim3(CV_THREADS), 0, s, d, width, ct, mat, bias, modulus, out,
                       base);
}

}  // namespace

hipError_t launch_conv2d(uint32_t width, const ConvGeom& g, size_t instances, const uint64_t* ct,
                         const int64_t* weight, const uint64_t* bias, uint64_t modulus, uint64_t* mat_scratch,
                         uint64_t* out, hipStream_t s) {
    if (instances == 0 || width == 0) return hipSuccess;
    if (modulus == 0 || g.groups == 0 || g.kh == 0 || g.kw == 0 || g.oh == 0 || g.ow == 0) return hipErrorInvalidValue;
    ConvDims d;
    d.g = g;
    d.Cg = g.c_in / g.groups, d.Og = g.c_out / g.groups;
    if (d.Cg == 0 || d.Og == 0) return hipErrorInvalidValue;
    d.khw = g.kh * g.kw;
    d.K = (size_t)d.Cg * g.kh * g.kw;
    d.npos = (size_t)g.oh * g.ow;
    d.pos_tiles = (d.npos + CV_P - 1) / CV_P;
    d.group_tiles = (d.Og + CV_CT - 1) / CV_CT;
    d.plane_tiles = d.group_tiles * g.groups;
    d.w_blocks = (width + CV_THREADS - 1) / CV_THREADS;
    const size_t per_instance = (size_t)d.plane_tiles * d.pos_tiles * d.w_blocks;
    if ((uint64_t)g.kh * g.kw > 0xffffffffull || (uint64_t)d.group_tiles * g.groups > 0xffffffffull ||
        per_instance / d.plane_tiles / d.w_blocks != d.pos_tiles || instances > SIZE_MAX / per_instance)
        return hipErrorInvalidValue;
    const size_t total = per_instance * instances;
    const bool pow2 = (modulus & (modulus - 1)) == 0;
    const int mode = mm_mode_for(modulus, d.K);
    const size_t nm = d.K * g.c_out;
    if ((nm + 255) / 256 > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_conv_reduce_weights, dim3((unsigned)((nm + 255) / 256)), dim3(256), 0, s, weight, nm, d.K,
                       d.Og, modulus, (int)pow2, mat_scratch);
    const size_t chunk = (size_t)1 << 30;  // workgroups per launch: instances oh ow may exceed one grid
    for (size_t base = 0; base < total; base += chunk) {
        const unsigned nwg = (unsigned)std::min(chunk, total - base);
        switch (mode) {
            case MM_M32: conv_launch<MM_M32>(nwg, d, width, ct, mat_scratch, bias, modulus, out, base, s); break;
            case MM_M64: conv_launch<MM_M64>(nwg, d, width, ct, mat_scratch, bias, modulus, out, base, s); break;
            case MM_GEN: conv_launch<MM_GEN>(nwg, d, width, ct, mat_scratch, bias, modulus, out, base, s); break;
            default: conv_launch<MM_GEN_TERM>(nwg, d, width, ct, mat_scratch, bias, modulus, out, base, s); break;
        }
    }
    return hipGetLastError();
}

}  // namespace tfhe
