// blind_rotate_generic.hip -- LDS-resident CGGI blind rotation for any supported
// (N, Q, dG2): one 256-thread workgroup per ciphertext, polynomials in LDS,
// radix-2 transforms with workgroup barriers.  This is the path for the >32-bit
// moduli (STD192, STD128Q, logQ/arbFunc contexts) and the cross-check for the
// specialised STD128 kernel (blind_rotate_fast.hip).
//
// Math per round i (rgsw-acc-cggi.cpp:246-307, restated in the oracle):
//   dct   = SignedDigitDecompose(acc)                 rgsw-acc.cpp:57-111
//   A_kj  = sum_l NTT(dct_l) * BSK[i][k][l][j]        (BSK pre-scaled by N^-1)
//   S_j   = A_0j * NTT(X^a' - 1) + A_1j * NTT(X^-a' - 1),  NTT(X^m - 1)[x] = psi^(e_x m) - 1
//   acc_j += INTT(S_j)
// acc stays in coefficient form, so the kernel input/output is the reference's
// EvalAcc_CUDA coefficient form (acc0 transposed on exit, bootstrapping.cu:675-686).
#include <cstdlib>

#include "device_math.hpp"
#include "kernels.hpp"
#include "n2048_layout.hpp"

namespace tfhe {

constexpr int GEN_THREADS = 256;

template <typename W>
__device__ __forceinline__ void lds_ntt_fwd(W* buf, uint32_t polys, uint32_t N, uint32_t logN, W Q,
                                            const W* __restrict__ psi, const W* __restrict__ psi_sh) {
    const uint32_t half = N >> 1, total = polys * half;
    uint32_t len = N, loglen = logN;
    for (uint32_t m = 1; m < N; m <<= 1) {
        len >>= 1;
        --loglen;
        for (uint32_t b = threadIdx.x; b < total; b += blockDim.x) {
            const uint32_t poly = b >> (logN - 1), bb = b & (half - 1);
            const uint32_t i = bb >> loglen;
            const uint32_t j = (i << (loglen + 1)) | (bb & (len - 1));
            W* a = buf + (size_t)poly * N;
            const W U = a[j];
            const W V = shoup<W>(a[j + len], psi[m + i], psi_sh[m + i], Q);
            a[j] = addm<W>(U, V, Q);
            a[j + len] = subm<W>(U, V, Q);
        }
        __syncthreads();
    }
}

// Gentleman-Sande inverse without the N^-1 scaling (folded into the BSK)
template <typename W>
__device__ __forceinline__ void lds_ntt_inv(W* buf, uint32_t polys, uint32_t N, uint32_t logN, W Q,
                                            const W* __restrict__ ipsi, const W* __restrict__ ipsi_sh) {
    const uint32_t half = N >> 1, total = polys * half;
    uint32_t len = 1, loglen = 0;
    for (uint32_t m = N; m > 1; m >>= 1) {
        const uint32_t h = m >> 1;
        for (uint32_t b = threadIdx.x; b < total; b += blockDim.x) {
            const uint32_t poly = b >> (logN - 1), bb = b & (half - 1);
            const uint32_t i = bb >> loglen;
            const uint32_t j = (i << (loglen + 1)) | (bb & (len - 1));
            W* a = buf + (size_t)poly * N;
            const W U = a[j], V = a[j + len];
            a[j] = addm<W>(U, V, Q);
            a[j + len] = shoup<W>(subm<W>(U, V, Q), ipsi[h + i], ipsi_sh[h + i], Q);
        }
        __syncthreads();
        len <<= 1;
        ++loglen;
    }
}

template <typename W>
__global__ void __launch_bounds__(GEN_THREADS)
k_blind_rotate_generic(BRParams P, const W* __restrict__ psi, const W* __restrict__ psi_sh,
                       const W* __restrict__ ipsi, const W* __restrict__ ipsi_sh, const W* __restrict__ mono,
                       const W* __restrict__ mono_sh, const uint32_t* __restrict__ eidx, const W* __restrict__ bsk,
                       const W* __restrict__ bsk_sh, const uint64_t* __restrict__ a, uint64_t amod,
                       uint64_t* __restrict__ acc_io) {
    extern __shared__ __align__(16) unsigned char smem[];
    const uint32_t N = P.N, twoN = 2 * N, tid = threadIdx.x, T = blockDim.x;
    W* acc = reinterpret_cast<W*>(smem);  // [2][N] coefficient form
    W* buf = acc + twoN;                  // [dG2][N]
    const W Q = (W)P.Q, r1 = (W)P.r1;
    const uint64_t Qhalf = P.Q >> 1;
    const int64_t Qs = (int64_t)P.Q;
    const uint32_t sh = 64 - P.logG;
    uint64_t* g = acc_io + (size_t)blockIdx.x * twoN;
    const uint64_t* ap = a + (size_t)blockIdx.x * P.n;
    uint32_t* ex = reinterpret_cast<uint32_t*>(smem + (size_t)(2 + P.dG2) * N * sizeof(W));  // rotation exponents [n]
    stage_rot_exponents<GEN_THREADS>(ex, ap, P.n, amod, twoN);
    __syncthreads();
    const size_t round_words = (size_t)4 * P.dG2 * N;

    for (uint32_t k = tid; k < twoN; k += T) acc[k] = (W)g[k];
    __syncthreads();

    for (uint32_t i = 0; i < P.n; ++i) {
        const uint32_t ai = ex[i];  // a'_i = ((amod - a_i) mod amod) * (2N / amod), staged (rgsw-acc-cggi.cpp:153)

        // signed digit decomposition, row = poly + 2*digit (rgsw-acc.cpp:80-110)
        for (uint32_t k = tid; k < twoN; k += T) {
            const uint32_t p = k >= N, x = k - p * N;
            const uint64_t t = (uint64_t)acc[k];
            int64_t d = t < Qhalf ? (int64_t)t : (int64_t)t - Qs;
            for (uint32_t z = 0; z < P.thr; ++z) {
                const int64_t r = (int64_t)((uint64_t)d << sh) >> sh;
                d = (d - r) >> P.logG;
            }
            for (uint32_t l = 0; l < P.digits; ++l) {
                int64_t r = (int64_t)((uint64_t)d << sh) >> sh;
                d = (d - r) >> P.logG;
                if (r < 0) r += Qs;
                buf[(size_t)(p + 2 * l) * N + x] = (W)r;
            }
        }
        __syncthreads();
        lds_ntt_fwd<W>(buf, P.dG2, N, P.logN, Q, psi, psi_sh);

        // external product with the two ternary keys, times the NTT-domain monomials
        const W* ek = bsk + (size_t)i * round_words;
        const W* eks = bsk_sh + (size_t)i * round_words;
        for (uint32_t x = tid; x < N; x += T) {
            W A00 = 0, A01 = 0, A10 = 0, A11 = 0;  // A_kj, lazily reduced (< 2*dG2*Q)
            for (uint32_t l = 0; l < P.dG2; ++l) {
                const W d = buf[(size_t)l * N + x];
                const size_t o00 = ((size_t)(0 * P.dG2 + l) * 2 + 0) * N + x;
                const size_t o10 = ((size_t)(1 * P.dG2 + l) * 2 + 0) * N + x;
                A00 += shoup_lazy<W>(d, ek[o00], eks[o00], Q);
                A01 += shoup_lazy<W>(d, ek[o00 + N], eks[o00 + N], Q);
                A10 += shoup_lazy<W>(d, ek[o10], eks[o10], Q);
                A11 += shoup_lazy<W>(d, ek[o10 + N], eks[o10 + N], Q);
            }
            A00 = reduce_full<W>(A00, r1, Q);
            A01 = reduce_full<W>(A01, r1, Q);
            A10 = reduce_full<W>(A10, r1, Q);
            A11 = reduce_full<W>(A11, r1, Q);
            const uint32_t ip = (eidx[x] * ai) & (twoN - 1);
            const uint32_t in = (twoN - ip) & (twoN - 1);
            const W mp = mono[ip], mps = mono_sh[ip], mn = mono[in], mns = mono_sh[in];
            // this thread has consumed every buf[l][x]; rows 0/1 at x now hold S_0/S_1
            buf[x] = addm<W>(shoup<W>(A00, mp, mps, Q), shoup<W>(A10, mn, mns, Q), Q);
            buf[N + x] = addm<W>(shoup<W>(A01, mp, mps, Q), shoup<W>(A11, mn, mns, Q), Q);
        }
        __syncthreads();
        lds_ntt_inv<W>(buf, 2, N, P.logN, Q, ipsi, ipsi_sh);
        for (uint32_t k = tid; k < twoN; k += T) acc[k] = addm<W>(acc[k], buf[k], Q);
        __syncthreads();
    }
    // acc0 -> transpose (automorphism X -> X^-1, poly.cpp:762-770), reduced values
    for (uint32_t k = tid; k < N; k += T) {
        const W v = acc[k == 0 ? 0 : N - k];
        g[k] = (uint64_t)(k == 0 ? v : (v == 0 ? (W)0 : (W)(Q - v)));
        g[N + k] = (uint64_t)acc[N + k];
    }
}


// ---------------------------------------------------------------------------
// Register-resident variant (k_blind_rotate_gen2): N = TH CN, TH = 256 threads for N in {1024, 2048},
// 1024 threads for N in {4096, 8192} (round 3: the reference dispatches N up to 8192,
// bootstrapping.cu:772-871; v1 needs (2 + dG2) N words of LDS and stops at N = 4096 with dG2 = 2).
// The accumulator and the external-product sums live in registers: thread t owns
// coefficients / NTT slots x = t + TH k (k < CN), so the decomposition, the
// MAC (coalesced BSK reads) and the accumulator update need no LDS.  Only the current
// digit's two polynomials pass through LDS for the transforms (2N words), so a workgroup
// needs 16-32 KiB instead of (2 + dG2) N words: several workgroups share a CU.  Digits
// come from the centred accumulator in closed form (see blind_rotate_fast.hip):
//   d_l = (c + (B/2)(B^l - 1)/(B - 1)) >> (l logG),  digit_l = sext_logG(d_l)
// which equals SignedDigitDecompose (rgsw-acc.cpp:83-109) digit by digit, thrown
// digits included.  Transforms are radix-4 LDS stages (one barrier per two stages).
// ---------------------------------------------------------------------------

// Lazy (Harvey) butterflies: forward values stay in [0, 4Q), inverse values in [0, 2Q)
// (4Q < 2^W: Q < 2^30 for u32 words, Q < 2^58 for u64), one conditional subtraction each.
template <typename W>
__device__ __forceinline__ void ct_lazy(W& x, W& y, W w, W ws, W Q2, W Q) {
    const W u = csub<W>(x, Q2), v = shoup_lazy<W>(y, w, ws, Q);
    x = u + v;
    y = u + Q2 - v;
}
template <typename W>
__device__ __forceinline__ void gs_lazy(W& x, W& y, W w, W ws, W Q2, W Q) {
    const W u = x, v = y;
    x = csub<W>(u + v, Q2);
    y = shoup_lazy<W>(u + Q2 - v, w, ws, Q);
}

// CT stages m and 2m fused: a0=x[j], a1=x[j+h], a2=x[j+2h], a3=x[j+3h], h = len/2
template <typename W>
__device__ __forceinline__ void lds_ntt_fwd_r4(W* buf, uint32_t N, uint32_t logN, W Q, const W* __restrict__ psi,
                                               const W* __restrict__ psi_sh) {
    const W Q2 = 2 * Q;
    uint32_t m = 1, loglen = logN - 1;  // stage with m blocks has half-length len = 2^loglen
    while (m < N) {
        if (m * 2 < N) {  // radix-4 unit: stages m (len) and 2m (len/2)
            const uint32_t lh = loglen - 1, h = 1u << lh, units = N >> 2;
            for (uint32_t u = threadIdx.x; u < 2 * units; u += blockDim.x) {
                const uint32_t poly = u >= units, uu = u - poly * units;
                const uint32_t i = uu >> lh, jj = uu & (h - 1);       // block of stage m, offset in quarter
                W* a = buf + (size_t)poly * N + ((size_t)i << (loglen + 1)) + jj;
                const W w = psi[m + i], ws = psi_sh[m + i];
                const W w1 = psi[2 * m + 2 * i], w1s = psi_sh[2 * m + 2 * i];
                const W w2 = psi[2 * m + 2 * i + 1], w2s = psi_sh[2 * m + 2 * i + 1];
                W a0 = a[0], a1 = a[h], a2 = a[2 * h], a3 = a[3 * h];
                ct_lazy<W>(a0, a2, w, ws, Q2, Q);
                ct_lazy<W>(a1, a3, w, ws, Q2, Q);
                ct_lazy<W>(a0, a1, w1, w1s, Q2, Q);
                ct_lazy<W>(a2, a3, w2, w2s, Q2, Q);
                a[0] = a0, a[h] = a1, a[2 * h] = a2, a[3 * h] = a3;
            }
            m <<= 2;
            loglen -= 2;
        } else {  // last single stage
            const uint32_t half = N >> 1;
            for (uint32_t b = threadIdx.x; b < 2 * half; b += blockDim.x) {
                const uint32_t poly = b >= half, bb = b - poly * half;
                W* a = buf + (size_t)poly * N + 2 * bb;
                W a0 = a[0], a1 = a[1];
                ct_lazy<W>(a0, a1, psi[m + bb], psi_sh[m + bb], Q2, Q);
                a[0] = a0, a[1] = a1;
            }
            m <<= 1;
        }
        __syncthreads();
    }
}

// GS inverse (no N^-1), stages fused in pairs from the small blocks up; inputs and
// outputs in [0, 2Q)
template <typename W>
__device__ __forceinline__ void lds_ntt_inv_r4(W* buf, uint32_t N, uint32_t logN, W Q, const W* __restrict__ ipsi,
                                               const W* __restrict__ ipsi_sh) {
    const W Q2 = 2 * Q;
    uint32_t m = N >> 1, loglen = 0;  // stage with m blocks, half-length 2^loglen
    if (logN & 1) {  // odd number of stages: the single stage first
        const uint32_t half = N >> 1;
        for (uint32_t b = threadIdx.x; b < 2 * half; b += blockDim.x) {
            const uint32_t poly = b >= half, bb = b - poly * half;
            W* a = buf + (size_t)poly * N + 2 * bb;
            W a0 = a[0], a1 = a[1];
            gs_lazy<W>(a0, a1, ipsi[m + bb], ipsi_sh[m + bb], Q2, Q);
            a[0] = a0, a[1] = a1;
        }
        __syncthreads();
        m >>= 1;
        loglen = 1;
    }
    while (m > 1) {  // stages m (half-length h) then m/2 (half-length 2h)
        const uint32_t lh = loglen, h = 1u << lh, units = N >> 2;
        for (uint32_t u = threadIdx.x; u < 2 * units; u += blockDim.x) {
            const uint32_t poly = u >= units, uu = u - poly * units;
            const uint32_t i = uu >> lh, jj = uu & (h - 1);  // block of stage m/2
            W* a = buf + (size_t)poly * N + ((size_t)i << (lh + 2)) + jj;
            const W w1 = ipsi[m + 2 * i], w1s = ipsi_sh[m + 2 * i];
            const W w2 = ipsi[m + 2 * i + 1], w2s = ipsi_sh[m + 2 * i + 1];
            const W w = ipsi[(m >> 1) + i], ws = ipsi_sh[(m >> 1) + i];
            W a0 = a[0], a1 = a[h], a2 = a[2 * h], a3 = a[3 * h];
            gs_lazy<W>(a0, a1, w1, w1s, Q2, Q);
            gs_lazy<W>(a2, a3, w2, w2s, Q2, Q);
            gs_lazy<W>(a0, a2, w, ws, Q2, Q);
            gs_lazy<W>(a1, a3, w, ws, Q2, Q);
            a[0] = a0, a[h] = a1, a[2 * h] = a2, a[3 * h] = a3;
        }
        __syncthreads();
        m >>= 2;
        loglen += 2;
    }
}

template <typename W, int CN, int TH = GEN_THREADS>
__global__ void __launch_bounds__(TH, TH == GEN_THREADS ? 2 : 1)
k_blind_rotate_gen2(BRParams P, const W* __restrict__ psi, const W* __restrict__ psi_sh, const W* __restrict__ ipsi,
                    const W* __restrict__ ipsi_sh, const W* __restrict__ mono, const W* __restrict__ mono_sh,
                    const uint32_t* __restrict__ eidx, const W* __restrict__ bsk, const W* __restrict__ bsk_sh,
                    const uint64_t* __restrict__ a, uint64_t amod, uint64_t* __restrict__ acc_io) {
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr uint32_t N = TH * CN;
    W* buf = reinterpret_cast<W*>(smem);  // [2][N]: the current digit of both polynomials
    const uint32_t t = threadIdx.x, twoN = 2 * N, logG = P.logG;
    const W Q = (W)P.Q, r1 = (W)P.r1;
    const uint64_t Qhalf = P.Q >> 1;
    const int64_t Qs = (int64_t)P.Q, Bh = (int64_t)1 << (logG - 1);
    const uint32_t sh = 64 - logG;
    uint64_t* g = acc_io + (size_t)blockIdx.x * twoN;
    const uint64_t* ap = a + (size_t)blockIdx.x * P.n;
    uint32_t* ex = reinterpret_cast<uint32_t*>(smem + (size_t)2 * N * sizeof(W));  // rotation exponents [n]
    stage_rot_exponents<TH>(ex, ap, P.n, amod, twoN);
    __syncthreads();
    const size_t round_words = (size_t)4 * P.dG2 * N;

    W acc[2][CN];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int k = 0; k < CN; ++k) acc[p][k] = (W)g[p * N + t + TH * k];

    for (uint32_t i = 0; i < P.n; ++i) {
        const uint32_t ai = ex[i];  // a'_i, staged at kernel start (rgsw-acc-cggi.cpp:153)
        W A[2][2][CN];  // A_kj per owned slot, lazily reduced (< 2 dG2 Q)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int k = 0; k < CN; ++k) A[kk][j][k] = 0;
        const W* ek = bsk + (size_t)i * round_words;
        const W* eks = bsk_sh + (size_t)i * round_words;
        for (uint32_t l = 0; l < P.digits; ++l) {
            const uint32_t lt = l + P.thr;  // digit index including the thrown ones
            const uint32_t shift = lt * logG;
            // (B/2)(B^lt - 1)/(B - 1) = (B/2)(1 + B + ... + B^(lt-1))
            int64_t K = 0;
            for (uint32_t z = 0; z < lt; ++z) K = (K << logG) + Bh;
#pragma unroll
            for (int p = 0; p < 2; ++p)
#pragma unroll
                for (int k = 0; k < CN; ++k) {
                    const uint64_t v = (uint64_t)acc[p][k];
                    const int64_t c = v < Qhalf ? (int64_t)v : (int64_t)v - Qs;
                    const int64_t d = (c + K) >> shift;
                    int64_t r = (int64_t)((uint64_t)d << sh) >> sh;
                    if (r < 0) r += Qs;
                    buf[p * N + t + TH * k] = (W)r;
                }
            __syncthreads();
            lds_ntt_fwd_r4<W>(buf, N, P.logN, Q, psi, psi_sh);
            // rows 2l (poly 0) and 2l+1 (poly 1), both keys, both output polynomials
#pragma unroll
            for (int k = 0; k < CN; ++k) {
                const uint32_t x = t + TH * k;
                const W d0 = buf[x], d1 = buf[N + x];
#pragma unroll
                for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        const size_t o0 = ((size_t)(kk * P.dG2 + 2 * l) * 2 + j) * N + x;
                        const size_t o1 = ((size_t)(kk * P.dG2 + 2 * l + 1) * 2 + j) * N + x;
                        A[kk][j][k] += shoup_lazy<W>(d0, ek[o0], eks[o0], Q) + shoup_lazy<W>(d1, ek[o1], eks[o1], Q);
                    }
            }
            __syncthreads();  // buf is rewritten by the next digit
        }
        // S_j = A_0j * NTT(X^a' - 1) + A_1j * NTT(X^-a' - 1) into buf, then INTT
#pragma unroll
        for (int k = 0; k < CN; ++k) {
            const uint32_t x = t + TH * k;
            const uint32_t ip = (eidx[x] * ai) & (twoN - 1), in = (twoN - ip) & (twoN - 1);
            const W mp = mono[ip], mps = mono_sh[ip], mn = mono[in], mns = mono_sh[in];
            const W A00 = reduce_full<W>(A[0][0][k], r1, Q), A01 = reduce_full<W>(A[0][1][k], r1, Q);
            const W A10 = reduce_full<W>(A[1][0][k], r1, Q), A11 = reduce_full<W>(A[1][1][k], r1, Q);
            buf[x] = addm<W>(shoup<W>(A00, mp, mps, Q), shoup<W>(A10, mn, mns, Q), Q);
            buf[N + x] = addm<W>(shoup<W>(A01, mp, mps, Q), shoup<W>(A11, mn, mns, Q), Q);
        }
        __syncthreads();
        lds_ntt_inv_r4<W>(buf, N, P.logN, Q, ipsi, ipsi_sh);
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int k = 0; k < CN; ++k)  // inverse outputs are in [0, 2Q)
                acc[p][k] = csub<W>(csub<W>(acc[p][k] + buf[p * N + t + TH * k], 2 * Q), Q);
        __syncthreads();  // buf is rewritten by the next round
    }
    // acc0 -> transpose (X -> X^-1, poly.cpp:762-770) through LDS, reduced values
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int k = 0; k < CN; ++k) buf[p * N + t + TH * k] = acc[p][k];
    __syncthreads();
    for (uint32_t k = t; k < N; k += TH) {
        const W v = buf[k == 0 ? 0 : N - k];
        g[k] = (uint64_t)(k == 0 ? v : (v == 0 ? (W)0 : (W)(Q - v)));
        g[N + k] = (uint64_t)buf[N + k];
    }
}

// ---------------------------------------------------------------------------
// gen3: u64 words, N = 2048 (the Q > 2^50 contexts: logQ/arbFunc C3, C5b).  The layout of the
// FP64 kernel (blind_rotate_f64.hip): 512 threads, 4 slots of both polynomials per thread
// (t + 512k) for the products, the accumulator in the transforms' pass-A layout (thread t:
// polynomial t >> 8, coefficients (t & 255) + 256q), radix-8 register passes over an
// XOR-swizzled LDS buffer (four barriers per transform; the swizzle and the index algebra are
// checked by tools/lds_layouts_f64.py; n2048_layout.hpp).  Thread state is half of gen2's (220 VGPRs, 2 waves per
// SIMD), so the kernel runs 4 waves per SIMD.  Harvey lazy butterflies as in gen2: forward
// values in [0, 4Q), inverse values in [0, 2Q).
namespace {

template <typename W>
struct G3Tw {
    const W* __restrict__ w;
    const W* __restrict__ s;
};

template <typename W>
__device__ __forceinline__ void g3_ct(W& x, W& y, const G3Tw<W>& T, uint32_t i, W Q2, W Q) {
    ct_lazy<W>(x, y, T.w[i], T.s[i], Q2, Q);
}
template <typename W>
__device__ __forceinline__ void g3_gs(W& x, W& y, const G3Tw<W>& T, uint32_t i, W Q2, W Q) {
    gs_lazy<W>(x, y, T.w[i], T.s[i], Q2, Q);
}

// forward CT stages s0 .. s0+2 (m0 = 2^s0) on 8 elements; g = block
template <typename W>
__device__ __forceinline__ void g3_fwd_core(W (&v)[8], uint32_t m0, uint32_t g, const G3Tw<W>& T, W Q2,
                                            W Q) {
#pragma unroll
    for (int k = 0; k < 4; ++k) g3_ct(v[k], v[k + 4], T, m0 + g, Q2, Q);
    g3_ct(v[0], v[2], T, 2 * m0 + 2 * g, Q2, Q), g3_ct(v[1], v[3], T, 2 * m0 + 2 * g, Q2, Q);
    g3_ct(v[4], v[6], T, 2 * m0 + 2 * g + 1, Q2, Q), g3_ct(v[5], v[7], T, 2 * m0 + 2 * g + 1, Q2, Q);
#pragma unroll
    for (int j = 0; j < 4; ++j) g3_ct(v[2 * j], v[2 * j + 1], T, 4 * m0 + 4 * g + j, Q2, Q);
}
// inverse GS stages h0, 2h0, 4h0 on 8 elements; g = block, m = N / (2 h0)
template <typename W>
__device__ __forceinline__ void g3_inv_core(W (&v)[8], uint32_t m, uint32_t g, const G3Tw<W>& T, W Q2,
                                            W Q) {
#pragma unroll
    for (int j = 0; j < 4; ++j) g3_gs(v[2 * j], v[2 * j + 1], T, m + 4 * g + j, Q2, Q);
    g3_gs(v[0], v[2], T, (m >> 1) + 2 * g, Q2, Q), g3_gs(v[1], v[3], T, (m >> 1) + 2 * g, Q2, Q);
    g3_gs(v[4], v[6], T, (m >> 1) + 2 * g + 1, Q2, Q), g3_gs(v[5], v[7], T, (m >> 1) + 2 * g + 1, Q2, Q);
#pragma unroll
    for (int k = 0; k < 4; ++k) g3_gs(v[k], v[k + 4], T, (m >> 2) + g, Q2, Q);
}

template <typename W>
__device__ __forceinline__ void g3_pass_fwd(W* p, int pass, uint32_t tau, uint32_t m0, uint32_t g, const G3Tw<W>& T,
                                            W Q2, W Q) {
    uint32_t ad[8];
    g3_ad(pass, tau, ad);
    W v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = p[ad[k]];
    g3_fwd_core(v, m0, g, T, Q2, Q);
#pragma unroll
    for (int k = 0; k < 8; ++k) p[ad[k]] = v[k];
}
template <typename W>
__device__ __forceinline__ void g3_pass_inv(W* p, int pass, uint32_t tau, uint32_t m, uint32_t g, const G3Tw<W>& T,
                                            W Q2, W Q) {
    uint32_t ad[8];
    g3_ad(pass, tau, ad);
    W v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = p[ad[k]];
    g3_inv_core(v, m, g, T, Q2, Q);
#pragma unroll
    for (int k = 0; k < 8; ++k) p[ad[k]] = v[k];
}

// forward transform of polynomial t >> 8; v = its pass-A elements (registers), outputs in LDS
template <typename W>
__device__ __forceinline__ void g3_ntt_fwd(W* buf, W (&v)[8], const G3Tw<W>& T, W Q2, W Q) {
    constexpr uint32_t N = G3_N;
    const uint32_t tau = g3_tau();
    W* p = buf + (threadIdx.x >> 8) * N;
    {
        uint32_t ad[8];
        g3_ad(0, tau, ad);
        g3_fwd_core(v, 1, 0, T, Q2, Q);
#pragma unroll
        for (int k = 0; k < 8; ++k) p[ad[k]] = v[k];
    }
    __syncthreads();
    g3_pass_fwd(p, 1, tau, 8, tau >> 5, T, Q2, Q);
    __syncthreads();
    g3_pass_fwd(p, 2, tau, 64, tau >> 2, T, Q2, Q);
    __syncthreads();
#pragma unroll
    for (uint32_t r = 0; r < 2; ++r) {  // stages 9 (h = 2) and 10 (h = 1) on units 4u .. 4u+3
        const uint32_t u = tau + 256 * r, u0 = g3_swz(4 * u);
        W v0 = p[u0], v1 = p[u0 ^ 1], v2 = p[u0 ^ 2], v3 = p[u0 ^ 3];
        g3_ct(v0, v2, T, N / 4 + u, Q2, Q), g3_ct(v1, v3, T, N / 4 + u, Q2, Q);
        g3_ct(v0, v1, T, N / 2 + 2 * u, Q2, Q), g3_ct(v2, v3, T, N / 2 + 2 * u + 1, Q2, Q);
        p[u0] = v0, p[u0 ^ 1] = v1, p[u0 ^ 2] = v2, p[u0 ^ 3] = v3;
    }
    __syncthreads();
}

// inverse transform of polynomial t >> 8 from LDS; v = its pass-A outputs, left in registers
// (no trailing barrier: the last pass only read this thread's own entries)
template <typename W>
__device__ __forceinline__ void g3_ntt_inv(W* buf, W (&v)[8], const G3Tw<W>& T, W Q2, W Q) {
    constexpr uint32_t N = G3_N;
    const uint32_t tau = g3_tau();
    W* p = buf + (threadIdx.x >> 8) * N;
#pragma unroll
    for (uint32_t r = 0; r < 2; ++r) {  // h = 1 then h = 2 on units 4u .. 4u+3
        const uint32_t u = tau + 256 * r, u0 = g3_swz(4 * u);
        W v0 = p[u0], v1 = p[u0 ^ 1], v2 = p[u0 ^ 2], v3 = p[u0 ^ 3];
        g3_gs(v0, v1, T, N / 2 + 2 * u, Q2, Q), g3_gs(v2, v3, T, N / 2 + 2 * u + 1, Q2, Q);
        g3_gs(v0, v2, T, N / 4 + u, Q2, Q), g3_gs(v1, v3, T, N / 4 + u, Q2, Q);
        p[u0] = v0, p[u0 ^ 1] = v1, p[u0 ^ 2] = v2, p[u0 ^ 3] = v3;
    }
    __syncthreads();
    g3_pass_inv(p, 2, tau, 256, tau >> 2, T, Q2, Q);
    __syncthreads();
    g3_pass_inv(p, 1, tau, 32, tau >> 5, T, Q2, Q);
    __syncthreads();
    uint32_t ad[8];
    g3_ad(0, tau, ad);
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = p[ad[k]];
    g3_inv_core(v, 4, 0, T, Q2, Q);
}

template <typename W>
__global__ void __launch_bounds__(G3_TH, 4)
k_blind_rotate_gen3(BRParams P, const W* __restrict__ psi, const W* __restrict__ psi_sh,
                    const W* __restrict__ ipsi, const W* __restrict__ ipsi_sh,
                    const W* __restrict__ mono, const W* __restrict__ mono_sh,
                    const uint32_t* __restrict__ eidx, const W* __restrict__ bsk,
                    const W* __restrict__ bsk_sh, const uint64_t* __restrict__ a, uint64_t amod,
                    uint64_t* __restrict__ acc_io) {
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr uint32_t N = G3_N, TH = G3_TH, CN = G3_CN;
    W* buf = reinterpret_cast<W*>(smem);  // [2][N], swizzled
    const uint32_t t = threadIdx.x, twoN = 2 * N, logG = P.logG;
    const uint32_t ts = g3_swz(t);  // slot t + 512k lives at swz(t) + 512k
    const W Q = (W)P.Q, Q2 = 2 * Q, r1 = (W)P.r1;
    const uint64_t Qhalf = P.Q >> 1;
    const int64_t Qs = (int64_t)P.Q, Bh = (int64_t)1 << (logG - 1);
    const uint32_t sh = 64 - logG;
    // forward twiddles (word + Shoup companion) live in LDS after the two polynomials: 64 KiB
    // per workgroup, two workgroups per CU
    W* psi_l = buf + 2 * N;
    W* psis_l = psi_l + N;
    for (uint32_t k = t; k < N; k += TH) psi_l[k] = psi[k], psis_l[k] = psi_sh[k];
    const G3Tw<W> TF{psi_l, psis_l}, TI{ipsi, ipsi_sh};
    uint64_t* g = acc_io + (size_t)blockIdx.x * twoN;
    const uint64_t* ap = a + (size_t)blockIdx.x * P.n;
    uint32_t* ex = reinterpret_cast<uint32_t*>(smem + (size_t)4 * G3_N * sizeof(W));  // rotation exponents [n]
    stage_rot_exponents<G3_TH>(ex, ap, P.n, amod, twoN);
    __syncthreads();
    const size_t round_words = (size_t)4 * P.dG2 * N;
    // accumulator entry [p][k]: polynomial t >> 8, coefficient (t & 255) + 256 (p CN + k)
    auto lpos = [t](int p, int k) -> uint32_t { return (t >> 8) * N + (t & 255) + 256 * (p * CN + k); };

    W acc[2][CN];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int k = 0; k < CN; ++k) acc[p][k] = (W)g[lpos(p, k)];
    __syncthreads();  // forward twiddles in LDS

    for (uint32_t i = 0; i < P.n; ++i) {
        const uint32_t ai = ex[i];  // a'_i, staged at kernel start (rgsw-acc-cggi.cpp:153)
        W A[2][2][CN];  // A_kj per owned slot, lazily reduced (< 2 dG2 Q)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int k = 0; k < CN; ++k) A[kk][j][k] = 0;
        const W* ek = bsk + (size_t)i * round_words;
        const W* eks = bsk_sh + (size_t)i * round_words;
        for (uint32_t l = 0; l < P.digits; ++l) {
            const uint32_t lt = l + P.thr, shift = lt * logG;
            int64_t Kd = 0;
            for (uint32_t z = 0; z < lt; ++z) Kd = (Kd << logG) + Bh;
            W v[8];
#pragma unroll
            for (int p = 0; p < 2; ++p)
#pragma unroll
                for (int k = 0; k < CN; ++k) {
                    const uint64_t x = (uint64_t)acc[p][k];
                    const int64_t c = x < Qhalf ? (int64_t)x : (int64_t)x - Qs;
                    const int64_t d = (c + Kd) >> shift;
                    int64_t r = (int64_t)((uint64_t)d << sh) >> sh;
                    if (r < 0) r += Qs;
                    v[p * CN + k] = (W)r;
                }
            g3_ntt_fwd(buf, v, TF, Q2, Q);  // pass A writes this thread's own entries: no barrier before
            // rows 2l (poly 0) and 2l+1 (poly 1), both keys, both output polynomials;
            // software-pipelined as in blind_rotate_f64.hip: group g = (slot k, key kk) holds 4 key
            // words + 4 Shoup companions, the next group's loads are issued before this group's
            // arithmetic (double-buffered, sched_barrier fences)
            constexpr int NG = CN * 2;
            auto kload = [&](int g, W (&kv)[8]) {
                const uint32_t x = t + TH * (g >> 1), kk = g & 1;
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 2; ++r) {
                        const size_t o = ((size_t)(kk * P.dG2 + 2 * l + r) * 2 + j) * N + x;
                        kv[(j * 2 + r) * 2] = ek[o];
                        kv[(j * 2 + r) * 2 + 1] = eks[o];
                    }
            };
            W kv[2][8];
            kload(0, kv[0]);
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                if (g + 1 < NG) kload(g + 1, kv[(g + 1) & 1]);
                __builtin_amdgcn_sched_barrier(0);
                const int k = g >> 1, kk = g & 1;
                const W d0 = buf[ts + TH * k], d1 = buf[N + ts + TH * k];
                const W(&c)[8] = kv[g & 1];
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    A[kk][j][k] += shoup_lazy<W>(d0, c[(j * 2) * 2], c[(j * 2) * 2 + 1], Q) +
                                   shoup_lazy<W>(d1, c[(j * 2 + 1) * 2], c[(j * 2 + 1) * 2 + 1], Q);
                __builtin_amdgcn_sched_barrier(0);
            }
            __syncthreads();  // the next pass A rewrites entries other threads' products read
        }
#pragma unroll
        for (int k = 0; k < CN; ++k) {
            const uint32_t x = t + TH * k;
            const uint32_t ip = (eidx[x] * ai) & (twoN - 1), in = (twoN - ip) & (twoN - 1);
            const W mp = mono[ip], mps = mono_sh[ip], mn = mono[in], mns = mono_sh[in];
            const W A00 = reduce_full<W>(A[0][0][k], r1, Q), A01 = reduce_full<W>(A[0][1][k], r1, Q);
            const W A10 = reduce_full<W>(A[1][0][k], r1, Q), A11 = reduce_full<W>(A[1][1][k], r1, Q);
            buf[ts + TH * k] = addm<W>(shoup<W>(A00, mp, mps, Q), shoup<W>(A10, mn, mns, Q), Q);
            buf[N + ts + TH * k] = addm<W>(shoup<W>(A01, mp, mps, Q), shoup<W>(A11, mn, mns, Q), Q);
        }
        __syncthreads();
        W v[8];
        g3_ntt_inv(buf, v, TI, Q2, Q);  // outputs in [0, 2Q)
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int k = 0; k < CN; ++k) acc[p][k] = csub<W>(csub<W>(acc[p][k] + v[p * CN + k], Q2), Q);
    }
    __syncthreads();  // every last inverse pass has read its entries
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int k = 0; k < CN; ++k) buf[lpos(p, k)] = acc[p][k];
    __syncthreads();
    g3_store_acc<W>(buf, g, t, Q);
}

}  // namespace

hipError_t launch_blind_rotate_generic(int word_bits, const BRParams& P, const DevTables& T, const void* bsk,
                                       const void* bsk_sh, const uint64_t* a, uint64_t amod, uint64_t* acc, size_t B,
                                       hipStream_t s, const Knobs& kn) {
    if (B == 0) return hipSuccess;
    const size_t wb = word_bits == 32 ? 4 : 8;
    const bool v1 = kn.generic == 1;       // all digits in LDS (cross-check)
    const bool no_gen3 = kn.generic == 2;  // v2 also at N = 2048 (cross-check)
    if (!v1 && !no_gen3 && P.N == G3_N) {
        const size_t lds = (size_t)4 * G3_N * wb + rot_exponent_bytes(P.n);  // two polynomials, forward twiddles, a'_i
        auto go3 = [&](auto tag) {
            using W = decltype(tag);
            auto kern = k_blind_rotate_gen3<W>;
            hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            hipLaunchKernelGGL(kern, dim3((unsigned)B), dim3(G3_TH), lds, s, P, (const W*)T.psi, (const W*)T.psi_sh,
                               (const W*)T.ipsi, (const W*)T.ipsi_sh, (const W*)T.mono, (const W*)T.mono_sh, T.eidx,
                               (const W*)bsk, (const W*)bsk_sh, a, amod, acc);
        };
        if (word_bits == 32) go3(uint32_t{});
        else go3(uint64_t{});
        return hipGetLastError();
    }
    if (!v1 && (P.N == 1024 || P.N == 2048 || P.N == 4096 || P.N == 8192)) {
        const size_t lds2 = (size_t)2 * P.N * wb + rot_exponent_bytes(P.n);
        if (lds2 > 160 * 1024) return hipErrorNotSupported;
        dim3 grid((unsigned)B), block(P.N >= 4096 ? 1024 : GEN_THREADS);
        auto go = [&](auto kern, auto tag) {
            using W = decltype(tag);
            hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds2);
            hipLaunchKernelGGL(kern, grid, block, lds2, s, P, (const W*)T.psi, (const W*)T.psi_sh, (const W*)T.ipsi,
                               (const W*)T.ipsi_sh, (const W*)T.mono, (const W*)T.mono_sh, T.eidx, (const W*)bsk,
                               (const W*)bsk_sh, a, amod, acc);
        };
        auto pick = [&](auto tag) {
            using W = decltype(tag);
            switch (P.N) {
                case 1024: go(k_blind_rotate_gen2<W, 4>, tag); break;
                case 2048: go(k_blind_rotate_gen2<W, 8>, tag); break;
                case 4096: go(k_blind_rotate_gen2<W, 4, 1024>, tag); break;
                default: go(k_blind_rotate_gen2<W, 8, 1024>, tag); break;  // 8192
            }
        };
        if (word_bits == 32) pick(uint32_t{});
        else pick(uint64_t{});
        return hipGetLastError();
    }
    const size_t lds = (size_t)(2 + P.dG2) * P.N * wb + rot_exponent_bytes(P.n);
    if (lds > 160 * 1024) return hipErrorNotSupported;
    dim3 grid((unsigned)B), block(GEN_THREADS);
    if (word_bits == 32) {
        auto k = k_blind_rotate_generic<uint32_t>;
        hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(k, grid, block, lds, s, P, (const uint32_t*)T.psi, (const uint32_t*)T.psi_sh,
                           (const uint32_t*)T.ipsi, (const uint32_t*)T.ipsi_sh, (const uint32_t*)T.mono,
                           (const uint32_t*)T.mono_sh, T.eidx, (const uint32_t*)bsk, (const uint32_t*)bsk_sh, a, amod,
                           acc);
    } else {
        auto k = k_blind_rotate_generic<uint64_t>;
        hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(k, grid, block, lds, s, P, (const uint64_t*)T.psi, (const uint64_t*)T.psi_sh,
                           (const uint64_t*)T.ipsi, (const uint64_t*)T.ipsi_sh, (const uint64_t*)T.mono,
                           (const uint64_t*)T.mono_sh, T.eidx, (const uint64_t*)bsk, (const uint64_t*)bsk_sh, a, amod,
                           acc);
    }
    return hipGetLastError();
}

}  // namespace tfhe

#ifdef TFHE_TEST_PROBES
// ---- arithmetic probes (test library only; arith_probes.hpp, tests/test_gpu_arith_units.py) ----
// op (| 16: the u32 instance): 0 ct_lazy(x, y, w, ws)  1 gs_lazy(x, y, w, ws)  2 g3_fwd_core(v[8], m0, g)
//     3 g3_inv_core(v[8], m, g)
// 10 words in, 8 out per case; tab = w[T] then the Shoup companions s[T] (u64 words, truncated for u32)
#include "arith_probes.hpp"

namespace tfhe {
namespace {
constexpr int G3P_NI = 10, G3P_NO = 8, G3P_TAB = 1 << 16;  // (most table pairs an entry takes)
template <typename W>
__global__ void k_arith_g3(int op, size_t cases, const uint64_t* __restrict__ in, const uint64_t* __restrict__ tab,
                           size_t tab_words, uint64_t* __restrict__ out, uint64_t Q64, const W* __restrict__ tw) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (!probe_lane_runs(op, i, cases)) return;
    const uint64_t* x = in + i * G3P_NI;
    uint64_t* o = out + i * G3P_NO;
    const W Q = (W)Q64, Q2 = 2 * Q;
    const size_t T = tab_words / 2;
    const G3Tw<W> G{tw, tw + T};
    const int f = op & 15;
    if (f == 0 || f == 1) {
        W a = (W)x[0], b = (W)x[1];
        if (f == 0) ct_lazy<W>(a, b, (W)x[2], (W)x[3], Q2, Q);
        else gs_lazy<W>(a, b, (W)x[2], (W)x[3], Q2, Q);
        o[0] = a, o[1] = b;
    } else {
        W v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = (W)x[k];
        const uint64_t m = x[8], g = x[9];
        if (m >= T || g >= T) return;
        if (f == 2) {
            if (4 * m + 4 * g + 3 >= T) return;
            g3_fwd_core<W>(v, (uint32_t)m, (uint32_t)g, G, Q2, Q);
        } else {
            if (m + 4 * g + 3 >= T) return;
            g3_inv_core<W>(v, (uint32_t)m, (uint32_t)g, G, Q2, Q);
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = v[k];
    }
}
// the u32 instance reads a u32 table: the u64 table narrowed on the device
__global__ void k_arith_g3_narrow(const uint64_t* __restrict__ src, size_t words, uint32_t* __restrict__ dst) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < words) dst[i] = (uint32_t)src[i];
}
}  // namespace
}  // namespace tfhe

extern "C" TFHE_ARITH_PROBE(g3) {
    using namespace tfhe;
    const bool u32 = (op >> 4) & 1;
    if ((op & 15) > 3 || Q < 3 || (tab_words & 1) || tab_words > 2 * (size_t)G3P_TAB) return -1;
    if (u32 ? Q >= (1ull << 30) : Q >= (1ull << 58)) return -1;  // 4Q fits the word
    if (!u32)
        return probe_launch(k_arith_g3<uint64_t>, G3P_NI, G3P_NO, op, cases, in, in_words, tab, tab_words, out, out_words, Q,
                            tab);
    uint32_t* narrow = nullptr;
    if (hipError_t e = hipMalloc(&narrow, (tab_words + 1) * sizeof(uint32_t)); e != hipSuccess) return (int)e;
    if (tab_words)
        hipLaunchKernelGGL(k_arith_g3_narrow, dim3((unsigned)((tab_words + 255) / 256)), dim3(256), 0, 0, tab, tab_words, narrow);
    const int rc = probe_launch(k_arith_g3<uint32_t>, G3P_NI, G3P_NO, op, cases, in, in_words, tab, tab_words, out, out_words,
                                Q, (const uint32_t*)narrow);
    (void)hipFree(narrow);
    return rc;
}
#endif  // TFHE_TEST_PROBES
