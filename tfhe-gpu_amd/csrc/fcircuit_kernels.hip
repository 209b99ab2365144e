// fcircuit_kernels.hip -- the two kernels of the function-circuit path (engine.hip dev_fcircuit) around the
// shared blind rotation / extraction / key switch:
//   * k_fcircuit_prep: one launch per level.  One workgroup per (record, instance) reads its 32-byte plan
//     record, gathers the rows of its folded linear form from the input array or the wire store, forms
//     v = sum coef * row + k mod q, applies its stage of EvalFunc (dev_func, engine.hip: b += 128; a second
//     stage first subtracts its first stage's slot and then also takes m / 4 off b, m the record's
//     ciphertext modulus q or 2q), and writes the mask and the accumulator (acc0 = 0, acc1 = the sparse test
//     vector of the record's own mode, moduli and table, scaled by Q / fmod as k_build_testvector does).
//     It replaces launch_lwe_op (x2 to x4) + launch_build_testvector of dev_func: the prepared ciphertext is
//     never stored.  Every mask word is written scaled to modulus 2N, a (2N / m), so that one blind
//     rotation with amod = 2N serves records of both moduli: the rotation exponent (m - a) (2N / m) is the
//     same number as (2N - a (2N / m)).
//   * k_fcircuit_out: evaluates the folded forms of the output wires into the caller's array.
// k_fcircuit_prep writes 16 N bytes of accumulator per bootstrap and reads (terms + 1) (n+1) words: it is
// store-bound, so each thread writes 16-byte pairs; the record's and the terms' addresses depend on blockIdx
// alone, so they are scalar loads.  q, 2q and 2N are powers of two: sums wrap in 64 bits and are masked.
#include "fcircuit.hpp"
#include "device_math.hpp"
#include "kernels.hpp"

namespace tfhe {

static_assert((uint32_t)FM_HALF == (uint32_t)TV_HALF && (uint32_t)FM_LUT == (uint32_t)TV_LUT &&
                  (uint32_t)FM_LUT1 == (uint32_t)TV_LUT1 && (uint32_t)FM_LUT2 == (uint32_t)TV_LUT2,
              "FuncRec names its mode by TvMode's values");

namespace {

// word k of the folded form (without its constant), mod 2^64
__device__ __forceinline__ uint64_t fcircuit_form(const FuncTerm* __restrict__ terms, uint32_t nterms, size_t inst,
                                                  const FuncPrep& P, const uint64_t* __restrict__ in,
                                                  const uint64_t* __restrict__ store, uint32_t k) {
    uint64_t v = 0;
    for (uint32_t t = 0; t < nterms; ++t) {
        const FuncTerm T = terms[t];
        const uint64_t* base = T.kind == CK_SLOT ? store : in;
        v += T.coef * base[((size_t)T.idx * P.instances + inst) * (P.n + 1) + k];
    }
    return v;
}

}  // namespace

__global__ void __launch_bounds__(256)
k_fcircuit_prep(FuncPrep P, const FuncRec* __restrict__ recs, const FuncTerm* __restrict__ terms,
                const uint64_t* __restrict__ luts, const uint64_t* __restrict__ in, const uint64_t* __restrict__ store,
                uint64_t* __restrict__ acc, uint64_t* __restrict__ a_out) {
    // bootstrap `flat` of the level: record flat / instances, instance flat % instances
    const size_t flat = P.first + blockIdx.x;
    const size_t g = flat / P.instances, inst = flat - g * P.instances;
    const FuncRec r = recs[g];
    const uint32_t mode = r.ctl & 7, N = P.N, n = P.n;
    const bool second = r.ctl & FR_SECOND;
    const uint64_t q = P.q, m = r.ctl & FR_CT2Q ? q << 1 : q, F = r.ctl & FR_OUT2Q ? q << 1 : q;
    const uint32_t lf = P.log2N + 1 - (uint32_t)__builtin_ctzll(m);  // log2 of factor = 2N / m
    const FuncTerm* T = terms + r.term0;
    const uint64_t* s1 = store + ((size_t)r.stage1 * P.instances + inst) * (n + 1);  // read by a second stage only

    uint64_t* ao = a_out + (size_t)blockIdx.x * n;
    for (uint32_t k = threadIdx.x; k < n; k += blockDim.x) {
        uint64_t v = fcircuit_form(T, r.nterms, inst, P, in, store, k) & (q - 1);
        if (second) v = (v - s1[k]) & (m - 1);
        ao[k] = v << lf;
    }

    uint64_t b = (fcircuit_form(T, r.nterms, inst, P, in, store, n) + r.k) & (q - 1);
    if (second) b = b - s1[n] - (m >> 2);
    b = (b + 128) & (m - 1);

    const uint64_t* L = luts + (size_t)r.lut * q;
    const uint64_t scale = P.Q / F, half = m >> 1;
    auto tv = [&](uint32_t k) -> uint64_t {  // acc1[k]: k_build_testvector's value for this record
        if (k & ((1u << lf) - 1)) return 0;
        const uint64_t j = k >> lf;
        if (j >= half) return 0;
        const uint64_t x = (b - j) & (m - 1);
        uint64_t f;
        if (mode == TV_HALF) f = x < half ? F - (m >> 2) : m >> 2;
        else if (mode == TV_LUT) f = L[x];
        else f = x < half ? L[x & (q - 1)] : F - L[(x - half) & (q - 1)];  // TV_LUT1 (m = q), TV_LUT2 (m = 2q)
        return scale * f;
    };
    ulonglong2* a0 = reinterpret_cast<ulonglong2*>(acc + (size_t)blockIdx.x * 2 * N);
    ulonglong2* a1 = a0 + N / 2;
    for (uint32_t p = threadIdx.x; p < N / 2; p += blockDim.x) {
        a0[p] = make_ulonglong2(0, 0);
        a1[p] = make_ulonglong2(tv(2 * p), tv(2 * p + 1));
    }
}

hipError_t launch_fcircuit_prep(const FuncPrep& P, const FuncRec* recs, const FuncTerm* terms, const uint64_t* luts,
                                const uint64_t* in, const uint64_t* store, uint64_t* acc, uint64_t* a_out, size_t B,
                                hipStream_t s) {
    if (B == 0) return hipSuccess;
    // q a power of two with 2q <= 2N unless no record runs at 2q (the caller checks that); N = 2^log2N
    if (P.N < 2 || P.N != 1u << P.log2N || P.q < 8 || (P.q & (P.q - 1)) || P.q > 2ull * P.N || P.instances == 0)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_fcircuit_prep, dim3((unsigned)B), dim3(256), 0, s, P, recs, terms, luts, in, store, acc, a_out);
    return hipGetLastError();
}

__global__ void __launch_bounds__(256)
k_fcircuit_out(FuncPrep P, const FuncOut* __restrict__ outs, const FuncTerm* __restrict__ terms,
               const uint64_t* __restrict__ in, const uint64_t* __restrict__ store, uint64_t* __restrict__ out) {
    const size_t flat = P.first + blockIdx.x;  // output flat / instances, instance flat % instances
    const size_t o = flat / P.instances, inst = flat - o * P.instances;
    const FuncOut r = outs[o];
    const uint32_t n = P.n;
    uint64_t* dst = out + flat * (n + 1);
    for (uint32_t k = threadIdx.x; k <= n; k += blockDim.x)
        dst[k] = (fcircuit_form(terms + r.term0, r.nterms, inst, P, in, store, k) + (k == n ? r.k : 0)) & (P.q - 1);
}

hipError_t launch_fcircuit_out(const FuncPrep& P, const FuncOut* outs, const FuncTerm* terms, const uint64_t* in,
                               const uint64_t* store, uint64_t* out, size_t B, hipStream_t s) {
    if (B == 0) return hipSuccess;
    if (P.q == 0 || (P.q & (P.q - 1)) || P.instances == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_fcircuit_out, dim3((unsigned)B), dim3(256), 0, s, P, outs, terms, in, store, out);
    return hipGetLastError();
}

}  // namespace tfhe
