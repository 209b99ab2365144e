// func_tables.hip -- the kernels of EvalFunc with one table per channel (engine.hip dev_func_tables).
// Ciphertext i of a flat batch uses table t(i) = (i / inner) mod T of luts[T][q].
//   * k_build_testvector_tab: k_build_testvector (lwe_kernels.hip) for the table modes (TV_LUT, TV_LUT1, TV_LUT2),
//     value for value, with the table chosen per ciphertext: by the index rule when the rows are the batch's own
//     (ids null), or from ids[] when they are a class's gathered sub-batch.  It writes 16 N bytes per ciphertext,
//     so each thread stores 16-byte pairs; the table's address depends on blockIdx alone.
//   * k_tab_move: the gather and the scatter of a slice that holds more than one class.  Item s of the slice,
//     i = first + s in the whole batch, of class c, is row base[c] + (number of class-c items in [first, i)) of the
//     gathered array.  The count below index i is closed-form: with period = inner T, i = p period + r,
//     t = r / inner, it is p inner ntab[c] + inner pre_c[t] + (r mod inner if class[t] = c), pre_c[t] the number of
//     class-c tables below t (meta[t] = {class, pre_0, pre_1, pre_2}).
// q, 2q and 2N are powers of two (the launchers check).
#include "device_math.hpp"
#include "kernels.hpp"

namespace tfhe {

__global__ void __launch_bounds__(256)
k_build_testvector_tab(TvParams P, TabSel S, const uint64_t* __restrict__ ct, uint64_t* __restrict__ acc,
                       uint64_t* __restrict__ a_out) {
    const size_t s = blockIdx.x;
    const uint32_t N = P.N, n = P.n;
    const uint64_t t = S.ids ? (uint64_t)S.ids[s] : ((S.first + s) / S.inner) % S.T;
    const uint64_t* L = P.lut + t * P.lut_len;
    const uint64_t* c = ct + s * (n + 1);
    const uint64_t q = P.ctmod, F = P.fmod, half = q >> 1, len1 = P.lut_len - 1;
    const uint64_t b = c[n] & (q - 1);
    const uint32_t lf = (uint32_t)__builtin_ctzll(2ull * N) - (uint32_t)__builtin_ctzll(q);  // log2 of 2N / q
    const uint64_t scale = P.Q / F;
    const uint32_t mode = P.mode;
    auto tv = [&](uint32_t k) -> uint64_t {  // acc1[k]
        if (k & ((1u << lf) - 1)) return 0;
        const uint64_t j = k >> lf;
        if (j >= half) return 0;
        const uint64_t x = (b - j) & (q - 1);
        uint64_t f;
        if (mode == TV_LUT) f = L[x];
        else f = x < half ? L[x & len1] : F - L[(x - half) & len1];  // TV_LUT1 (q = len), TV_LUT2 (q = 2 len)
        return scale * f;
    };
    ulonglong2* a0 = reinterpret_cast<ulonglong2*>(acc + s * 2 * N);
    ulonglong2* a1 = a0 + N / 2;
    for (uint32_t p = threadIdx.x; p < N / 2; p += blockDim.x) {
        a0[p] = make_ulonglong2(0, 0);
        a1[p] = make_ulonglong2(tv(2 * p), tv(2 * p + 1));
    }
    for (uint32_t k = threadIdx.x; k < n; k += blockDim.x) a_out[s * n + k] = c[k];
}

hipError_t launch_build_testvector_tab(const TvParams& P, const TabSel& S, const uint64_t* ct, uint64_t* acc,
                                       uint64_t* a_out, size_t B, hipStream_t s) {
    if (B == 0) return hipSuccess;
    const uint64_t q = P.ctmod, len = P.lut_len;
    if (P.N < 2 || (P.N & (P.N - 1)) || q < 2 || (q & (q - 1)) || q > 2ull * P.N || len == 0 || (len & (len - 1)) ||
        (P.mode != TV_LUT && P.mode != TV_LUT1 && P.mode != TV_LUT2) || (q != len && q != 2 * len) || S.inner == 0 ||
        S.T == 0)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_build_testvector_tab, dim3((unsigned)B), dim3(256), 0, s, P, S, ct, acc, a_out);
    return hipGetLastError();
}

// SCATTER false: rows[pos] = flat[s], ids[pos] = t;  true: flat[s] = rows[pos]
template <bool SCATTER>
__global__ void __launch_bounds__(256)
k_tab_move(TabMove M, const uint64_t* __restrict__ src, uint64_t* __restrict__ dst, uint32_t* __restrict__ ids) {
    const size_t s = blockIdx.x;
    const uint64_t i = M.first + s, period = M.inner * M.T;
    const uint64_t p = i / period, r = i - p * period, t = r / M.inner, within = r - t * M.inner;
    const uint4 m = M.meta[t];
    const uint32_t c = m.x;
    if (c > 2) return;  // never by the rule
    const uint64_t pre = c == 0 ? m.y : c == 1 ? m.z : m.w;
    const uint64_t pos = M.base[c] + (p * M.inner * M.ntab[c] + M.inner * pre + within - M.lo[c]);
    if (pos >= M.count) return;  // never by the rule; no row outside the slice is touched
    const uint32_t w = M.width;
    const uint64_t* from = src + (SCATTER ? pos : s) * w;
    uint64_t* to = dst + (SCATTER ? s : pos) * w;
    for (uint32_t k = threadIdx.x; k < w; k += blockDim.x) to[k] = from[k];
    if (!SCATTER && threadIdx.x == 0) ids[pos] = (uint32_t)t;
}

hipError_t launch_tab_gather(const TabMove& M, const uint64_t* flat, uint64_t* rows, uint32_t* ids, hipStream_t s) {
    if (M.count == 0) return hipSuccess;
    if (!M.meta || M.inner == 0 || M.T == 0 || M.width == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_tab_move<false>, dim3((unsigned)M.count), dim3(256), 0, s, M, flat, rows, ids);
    return hipGetLastError();
}

hipError_t launch_tab_scatter(const TabMove& M, const uint64_t* rows, uint64_t* flat, hipStream_t s) {
    if (M.count == 0) return hipSuccess;
    if (!M.meta || M.inner == 0 || M.T == 0 || M.width == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_tab_move<true>, dim3((unsigned)M.count), dim3(256), 0, s, M, rows, flat, (uint32_t*)nullptr);
    return hipGetLastError();
}

}  // namespace tfhe
