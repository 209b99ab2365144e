// keygen_kernels.hip -- key generation, LWE encryption and decryption on the device.
//
// Every random word is one fixed position of ONE counter-based splitmix64 stream (include/tfhe_hip.h
// "The stream"): draw k of a stream whose state is s is mix(s + (k + 1) gamma).  A lane therefore computes
// the draws of its own columns directly -- no lane, row or kernel depends on another one's generator state --
// and the keys equal or_keygen's (oracle/tfhe_oracle.c) word for word.
//
//   * k_keygen_ksk   one wavefront per eight key-switching rows (N baseKS dKS rows of n + 1 words): lanes stride
//                    the n uniform columns, the inner product <A, s> is reduced across the wave, the stores are
//                    8 bytes per lane and contiguous.  Writes either the caller's u64 layout (B at index n) or
//                    the arena's packed A / B arrays (pack_ksk's layout, engine.hip) at their u16 / u32 / u64
//                    width, pad columns included.
//   * k_keygen_bsk   one workgroup per RLWE row (n 2 dG2 rows of two polynomials): a and e are generated in
//                    LDS and a sN is formed through the exact negacyclic NTT of host_ntt_fwd / host_ntt_inv
//                    (host_math.cpp) over the Shoup tables of the context, in the context's word class.  The
//                    arena form writes NTT(row) N^-1 and its Shoup companions directly (two forward transforms,
//                    no inverse); the coefficient form adds the inverse transform.
//   * k_lwe_encrypt / k_lwe_decrypt   one wavefront per ciphertext, the same reduction.
//
// The secret vectors s (n words) and sN (N words) and NTT(sN) are n + N draws: the host forms them and the
// launchers take them as small device arrays (engine.hip keygen_prepare).
#include "device_math.hpp"
#include "kernels.hpp"

namespace tfhe {

namespace {

constexpr uint64_t KG_GAMMA = 0x9E3779B97F4A7C15ull;
constexpr int KG_WAVES = 4;     // wavefronts per workgroup of the wave-per-row kernels
constexpr int KG_ROWS = 8;      // KSK rows per wavefront (k_keygen_ksk)
constexpr int KG_THREADS = 256; // k_keygen_bsk

// draw k (0-based) of the stream whose state is `state` (or_splitmix64 after k earlier draws)
__device__ __forceinline__ uint64_t draw_at(uint64_t state, uint64_t k) {
    uint64_t z = state + (k + 1) * KG_GAMMA;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// rng_gauss: draws k and k + 1.  Every product and sum is one explicitly rounded IEEE operation (no
// contraction), as the oracle is compiled; log and cos are the device library's.
__device__ __forceinline__ int64_t gauss_at(uint64_t state, uint64_t k) {
    const uint64_t d0 = draw_at(state, k), d1 = draw_at(state, k + 1);
    const double u1 = __dmul_rn(__dadd_rn((double)(d0 >> 11), 1.0), 1.0 / 9007199254740993.0);
    const double u2 = __dmul_rn((double)(d1 >> 11), 1.0 / 9007199254740992.0);
    const double r = __dsqrt_rn(__dmul_rn(-2.0, log(u1)));
    const double z = __dmul_rn(r, cos(__dmul_rn(6.283185307179586, u2)));
    return (int64_t)llround(__dmul_rn(3.19, z));
}

// modulus with its power-of-two mask (0: not a power of two, take the division)
struct Mod {
    uint64_t m, mask;
};
__device__ __forceinline__ Mod make_mod(uint64_t m) { return Mod{m, (m & (m - 1)) == 0 ? m - 1 : 0}; }
__device__ __forceinline__ uint64_t umod(uint64_t x, const Mod& M) { return M.mask ? (x & M.mask) : x % M.m; }
// safe for every m < 2^64, a, b < m
__device__ __forceinline__ uint64_t addm64(uint64_t a, uint64_t b, uint64_t m) {
    const uint64_t r = a + b;
    return (r < a || r >= m) ? r - m : r;
}
__device__ __forceinline__ uint64_t subm64(uint64_t a, uint64_t b, uint64_t m) { return a >= b ? a - b : a + (m - b); }
// the oracle's to_mod: v % (int64) m, made non-negative
__device__ __forceinline__ uint64_t to_mod(int64_t v, uint64_t m) {
    const int64_t r = v % (int64_t)m;
    return (uint64_t)(r < 0 ? r + (int64_t)m : r);
}
// a b mod m for a, b < m, any m (double and add: the few products that have no table constant)
__device__ uint64_t mulmod_any(uint64_t a, uint64_t b, uint64_t m) {
    uint64_t r = 0;
    for (; b; b >>= 1) {
        if (b & 1) r = addm64(r, a, m);
        a = addm64(a, a, m);
    }
    return r;
}
// the low 64 bits of floor((hi 2^64 + lo) / d), restoring division
__device__ uint64_t div128(uint64_t hi, uint64_t lo, uint64_t d) {
    uint64_t rem = hi % d, q = 0;
    for (int i = 63; i >= 0; --i) {
        const bool top = rem >> 63;
        rem = (rem << 1) | ((lo >> i) & 1);
        if (top || rem >= d) {
            rem -= d;
            q |= 1ull << i;
        }
    }
    return q;
}
__device__ __forceinline__ uint64_t wave_sum_mod(uint64_t v, uint64_t m) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = addm64(v, __shfl_xor(v, off), m);
    return v;
}
// acc += a c mod m for the centred key word c (ternary keys take no product)
__device__ __forceinline__ uint64_t add_key_term(uint64_t acc, uint64_t a, int64_t c, uint64_t m) {
    if (c == 0) return acc;
    if (c == 1) return addm64(acc, a, m);
    if (c == -1) return subm64(acc, a, m);
    return addm64(acc, mulmod_any(a, to_mod(c, m), m), m);
}
// sk_to_mod's centred value of a key word stored mod qKS
__device__ __forceinline__ int64_t centred(uint64_t v, uint64_t qKS) {
    return v > qKS / 2 ? (int64_t)v - (int64_t)qKS : (int64_t)v;
}

// ---------------------------------------------------------------------------
// KSK rows.  KW: the stored word; ARENA: A [rows][n_pad] + B [rows] (else KW = u64, [rows][n + 1]).
// A wavefront takes KG_ROWS consecutive rows: their Gaussians and message terms -- one lane's work per row,
// a log and a cos each -- are computed side by side on lanes 0 .. KG_ROWS - 1 instead of on one lane per row;
// the uniform columns then go row by row.  A lane owns COLS consecutive columns per step (8 bytes), so a wave
// stores 512 contiguous bytes.
// ---------------------------------------------------------------------------
template <typename KW, bool ARENA>
__global__ void __launch_bounds__(64 * KG_WAVES)
k_keygen_ksk(KeygenParams P, KeygenTables T, void* __restrict__ out_a, void* __restrict__ out_b) {
    constexpr uint32_t COLS = ARENA ? 8 / sizeof(KW) : 1;
    const uint32_t lane = threadIdx.x & 63, n = P.n;
    const size_t row0 = ((size_t)blockIdx.x * KG_WAVES + (threadIdx.x >> 6)) * KG_ROWS;
    if (row0 >= P.ksk_rows) return;  // whole wavefront; no workgroup barrier in this kernel
    const uint32_t nrows = (uint32_t)(P.ksk_rows - row0 < KG_ROWS ? P.ksk_rows - row0 : KG_ROWS);
    const Mod M = make_mod(P.qKS);
    const uint64_t row_step = (uint64_t)(n + 2) * KG_GAMMA;
    const uint32_t width = ARENA ? P.n_pad : n;  // n_pad is a multiple of 2 COLS
    uint64_t b = 0;  // lane l < nrows: B of row row0 + l
    if (lane < nrows) {
        const size_t row = row0 + lane;
        const uint32_t k = (uint32_t)(row % P.dKS), j = (uint32_t)((row / P.dKS) % P.baseKS);
        const size_t i = row / P.dKS / P.baseKS;
        b = to_mod(gauss_at(P.ksk_state + (uint64_t)row * row_step, 0), M.m);
        const uint64_t t = mulmod_any(T.pw[k], j % M.m, M.m);  // j baseKS^k
        b = add_key_term(b, t, T.sN[i], M.m);
    }
    for (uint32_t r = 0; r < nrows; ++r) {
        const size_t row = row0 + r;
        const uint64_t state = P.ksk_state + (uint64_t)row * row_step;
        uint64_t acc = 0;
        for (uint32_t c0 = lane * COLS; c0 < width; c0 += 64 * COLS) {
            uint64_t packed = 0;
#pragma unroll
            for (uint32_t v = 0; v < COLS; ++v) {
                const uint32_t c = c0 + v;
                if (c < n) {
                    const uint64_t a = umod(draw_at(state, 2 + c), M);
                    acc = add_key_term(acc, a, T.s[c], M.m);
                    packed |= a << (8 * sizeof(KW) * v % 64);
                }
            }
            if constexpr (ARENA) *reinterpret_cast<uint64_t*>(static_cast<KW*>(out_a) + row * P.n_pad + c0) = packed;
            else static_cast<uint64_t*>(out_a)[row * (size_t)(n + 1) + c0] = packed;
        }
        acc = wave_sum_mod(acc, M.m);  // every lane holds <A, s>
        if (lane == r) b = addm64(b, acc, M.m);
    }
    if (lane < nrows) {
        if constexpr (ARENA) static_cast<KW*>(out_b)[row0 + lane] = (KW)b;
        else static_cast<uint64_t*>(out_a)[(row0 + lane) * (size_t)(n + 1) + n] = b;
    }
}

// ---------------------------------------------------------------------------
// The negacyclic NTT of host_ntt_fwd / host_ntt_inv on NP polynomials held in LDS (buf[p N + x]), one
// stage per barrier, fully reduced values.  Called by the whole workgroup.
// ---------------------------------------------------------------------------
template <typename W, int NP>
__device__ void ntt_fwd_lds(W* buf, uint32_t N, const W* __restrict__ psi, const W* __restrict__ psi_sh, W Q) {
    uint32_t loglen = 31 - __builtin_clz(N);
    for (uint32_t m = 1; m < N; m <<= 1) {
        --loglen;
        const uint32_t len = 1u << loglen;
        __syncthreads();
        for (uint32_t t = threadIdx.x; t < N / 2; t += KG_THREADS) {
            const uint32_t i = t >> loglen, j = ((i << loglen) << 1) + (t & (len - 1));
            const W S = psi[m + i], Sp = psi_sh[m + i];
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                W* a = buf + (size_t)p * N;
                const W U = a[j], V = shoup<W>(a[j + len], S, Sp, Q);
                a[j] = addm<W>(U, V, Q);
                a[j + len] = subm<W>(U, V, Q);
            }
        }
    }
    __syncthreads();
}
template <typename W>
__device__ void ntt_inv_lds(W* a, uint32_t N, const W* __restrict__ ipsi, const W* __restrict__ ipsi_sh, W Q) {
    uint32_t loglen = 0;
    for (uint32_t m = N; m > 1; m >>= 1, ++loglen) {
        const uint32_t h = m >> 1, len = 1u << loglen;
        __syncthreads();
        for (uint32_t t = threadIdx.x; t < N / 2; t += KG_THREADS) {
            const uint32_t i = t >> loglen, j = ((i << loglen) << 1) + (t & (len - 1));
            const W S = ipsi[h + i], Sp = ipsi_sh[h + i];
            const W U = a[j], V = a[j + len];
            a[j] = addm<W>(U, V, Q);
            a[j + len] = shoup<W>(subm<W>(U, V, Q), S, Sp, Q);
        }
    }
    __syncthreads();
}

// fill_companions' word: floor(v 2^bits / Q)
__device__ __forceinline__ uint32_t companion(uint32_t v, uint32_t Q) { return (uint32_t)(((uint64_t)v << 32) / Q); }
__device__ __forceinline__ uint64_t companion(uint64_t v, uint64_t Q) { return div128(v, 0, Q); }

// ---------------------------------------------------------------------------
// BSK rows.  W: the context's word class (storage of the tables and of the arena).
// ARENA: out / out_sh are the arena's bsk / bsk_sh ([rows][2][N] of W): NTT(row) N^-1 and companions.
// else:  out is the caller's coefficient array ([rows][2][N] of u64).
// ---------------------------------------------------------------------------
template <typename W, bool ARENA>
__global__ void __launch_bounds__(KG_THREADS)
k_keygen_bsk(KeygenParams P, KeygenTables T, void* __restrict__ out, void* __restrict__ out_sh) {
    extern __shared__ __align__(16) unsigned char kg_smem[];
    W* buf = reinterpret_cast<W*>(kg_smem);  // ARENA: a | e; else a
    const uint32_t N = P.N;
    const size_t row = blockIdx.x;
    const uint32_t rw = (uint32_t)(row % P.dG2), key = (uint32_t)((row / P.dG2) % 2);
    const int8_t si = T.s[row / P.dG2 / 2];
    const bool msg = key == 0 ? si == 1 : si == -1;
    const uint64_t state = P.bsk_state + (uint64_t)row * 3 * N * KG_GAMMA;
    const W Q = (W)P.Q;
    const W* psi = static_cast<const W*>(T.psi);
    const W* psi_sh = static_cast<const W*>(T.psi_sh);
    const W* snt = static_cast<const W*>(T.snt);
    const W* snt_sh = static_cast<const W*>(T.snt_sh);

    if constexpr (ARENA) {
        for (uint32_t x = threadIdx.x; x < N; x += KG_THREADS) {
            buf[x] = (W)(draw_at(state, x) % P.Q);
            buf[N + x] = (W)to_mod(gauss_at(state, (uint64_t)N + 2 * x), P.Q);
        }
        ntt_fwd_lds<W, 2>(buf, N, psi, psi_sh, Q);
        // the message term g goes to coefficient 0 of a (even row) or b (odd row): + g in every NTT slot;
        // everything scaled by N^-1 (g N^-1: T.gN)
        const W g = msg ? (W)T.gN[rw >> 1] : 0, ga = (rw & 1) ? 0 : g, gb = (rw & 1) ? g : 0;
        const W ninv = (W)P.Ninv, ninv_sh = (W)P.Ninv_sh;
        W* oa = static_cast<W*>(out) + row * 2 * N;
        W* osh = static_cast<W*>(out_sh) + row * 2 * N;
        for (uint32_t x = threadIdx.x; x < N; x += KG_THREADS) {
            const W ah = buf[x];
            const W va = addm<W>(shoup<W>(ah, ninv, ninv_sh, Q), ga, Q);
            W vb = addm<W>(shoup<W>(ah, snt[x], snt_sh[x], Q), shoup<W>(buf[N + x], ninv, ninv_sh, Q), Q);
            vb = addm<W>(vb, gb, Q);
            oa[x] = va;
            oa[N + x] = vb;
            osh[x] = companion(va, Q);
            osh[N + x] = companion(vb, Q);
        }
    } else {
        uint64_t* pa = static_cast<uint64_t*>(out) + row * 2 * N;
        uint64_t* pb = pa + N;
        const uint64_t g = msg ? T.g[rw >> 1] : 0;
        for (uint32_t x = threadIdx.x; x < N; x += KG_THREADS) {
            const uint64_t a = draw_at(state, x) % P.Q;
            buf[x] = (W)a;
            pa[x] = (x == 0 && !(rw & 1)) ? addm64(a, g, P.Q) : a;
        }
        ntt_fwd_lds<W, 1>(buf, N, psi, psi_sh, Q);
        for (uint32_t x = threadIdx.x; x < N; x += KG_THREADS) buf[x] = shoup<W>(buf[x], snt[x], snt_sh[x], Q);
        ntt_inv_lds<W>(buf, N, static_cast<const W*>(T.ipsi), static_cast<const W*>(T.ipsi_sh), Q);
        for (uint32_t x = threadIdx.x; x < N; x += KG_THREADS) {
            uint64_t b = addm64((uint64_t)buf[x], to_mod(gauss_at(state, (uint64_t)N + 2 * x), P.Q), P.Q);
            if (x == 0 && (rw & 1)) b = addm64(b, g, P.Q);
            pb[x] = b;
        }
    }
}

// ---------------------------------------------------------------------------
// or_encrypt / or_decrypt, one wavefront per ciphertext
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(64 * KG_WAVES)
k_lwe_encrypt(uint32_t n, uint64_t qKS, const uint64_t* __restrict__ sk, size_t B, const int64_t* __restrict__ msg,
              uint64_t ptxt_mod, uint64_t mod, uint64_t seed, uint64_t* __restrict__ ct) {
    const uint32_t lane = threadIdx.x & 63;
    const size_t b = (size_t)blockIdx.x * KG_WAVES + (threadIdx.x >> 6);
    if (b >= B) return;  // whole wavefront
    const Mod M = make_mod(mod);
    const uint64_t state = seed + (uint64_t)b * (n + 2) * KG_GAMMA;
    uint64_t* o = ct + b * (size_t)(n + 1);
    uint64_t acc = 0;
    for (uint32_t c = lane; c < n; c += 64) {
        const uint64_t a = umod(draw_at(state, 2 + c), M);
        acc = add_key_term(acc, a, centred(sk[c], qKS), mod);
        o[c] = a;
    }
    acc = wave_sum_mod(acc, mod);
    if (lane == 0) {
        const uint64_t mm = to_mod(msg[b] % (int64_t)ptxt_mod, ptxt_mod);
        uint64_t v = mulmod_any((mod / ptxt_mod) % mod, mm % mod, mod);
        v = addm64(v, to_mod(gauss_at(state, 0), mod), mod);
        o[n] = addm64(v, acc, mod);
    }
}

__global__ void __launch_bounds__(64 * KG_WAVES)
k_lwe_decrypt(uint32_t n, uint64_t qKS, const uint64_t* __restrict__ sk, size_t B, const uint64_t* __restrict__ ct,
              uint64_t ptxt_mod, uint64_t mod, int64_t* __restrict__ msg) {
    const uint32_t lane = threadIdx.x & 63;
    const size_t b = (size_t)blockIdx.x * KG_WAVES + (threadIdx.x >> 6);
    if (b >= B) return;  // whole wavefront
    const Mod M = make_mod(mod);
    const uint64_t* x = ct + b * (size_t)(n + 1);
    uint64_t acc = 0;
    for (uint32_t c = lane; c < n; c += 64) acc = add_key_term(acc, umod(x[c], M), centred(sk[c], qKS), mod);
    acc = wave_sum_mod(acc, mod);
    if (lane == 0) {
        uint64_t r = subm64(x[n], acc, mod);
        r = addm64(r, mod / (ptxt_mod * 2), mod);
        msg[b] = (int64_t)div128(__umul64hi(ptxt_mod, r), ptxt_mod * r, mod);
    }
}

unsigned wave_grid(size_t items) { return (unsigned)((items + KG_WAVES - 1) / KG_WAVES); }

}  // namespace

hipError_t launch_keygen_ksk(const KeygenParams& P, const KeygenTables& T, int ksk_bits, void* out_a, void* out_b,
                             hipStream_t s) {
    if (P.ksk_rows == 0) return hipSuccess;
    const dim3 grid(wave_grid((P.ksk_rows + KG_ROWS - 1) / KG_ROWS)), block(64 * KG_WAVES);
    if (ksk_bits == 0) hipLaunchKernelGGL((k_keygen_ksk<uint64_t, false>), grid, block, 0, s, P, T, out_a, out_b);
    else if (ksk_bits == 16) hipLaunchKernelGGL((k_keygen_ksk<uint16_t, true>), grid, block, 0, s, P, T, out_a, out_b);
    else if (ksk_bits == 32) hipLaunchKernelGGL((k_keygen_ksk<uint32_t, true>), grid, block, 0, s, P, T, out_a, out_b);
    else if (ksk_bits == 64) hipLaunchKernelGGL((k_keygen_ksk<uint64_t, true>), grid, block, 0, s, P, T, out_a, out_b);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

size_t keygen_bsk_lds_bytes(uint32_t N, int word_bits, bool arena) { return (size_t)(arena ? 2 : 1) * N * (word_bits / 8); }

hipError_t launch_keygen_bsk(const KeygenParams& P, const KeygenTables& T, int word_bits, bool arena, void* out,
                             void* out_sh, hipStream_t s) {
    if (P.bsk_rows == 0) return hipSuccess;
    const size_t lds = keygen_bsk_lds_bytes(P.N, word_bits, arena);
    if (lds > kKeygenMaxLds || (word_bits != 32 && word_bits != 64)) return hipErrorNotSupported;
    auto launch = [&](auto kern) {
        hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kern, dim3((unsigned)P.bsk_rows), dim3(KG_THREADS), lds, s, P, T, out, out_sh);
        return hipGetLastError();
    };
    if (word_bits == 32) return arena ? launch(k_keygen_bsk<uint32_t, true>) : launch(k_keygen_bsk<uint32_t, false>);
    return arena ? launch(k_keygen_bsk<uint64_t, true>) : launch(k_keygen_bsk<uint64_t, false>);
}

hipError_t launch_lwe_encrypt(uint32_t n, uint64_t qKS, const uint64_t* sk, size_t B, const int64_t* msg,
                              uint64_t ptxt_mod, uint64_t mod, uint64_t seed, uint64_t* ct, hipStream_t s) {
    hipLaunchKernelGGL(k_lwe_encrypt, dim3(wave_grid(B)), dim3(64 * KG_WAVES), 0, s, n, qKS, sk, B, msg, ptxt_mod, mod,
                       seed, ct);
    return hipGetLastError();
}

hipError_t launch_lwe_decrypt(uint32_t n, uint64_t qKS, const uint64_t* sk, size_t B, const uint64_t* ct,
                              uint64_t ptxt_mod, uint64_t mod, int64_t* msg, hipStream_t s) {
    hipLaunchKernelGGL(k_lwe_decrypt, dim3(wave_grid(B)), dim3(64 * KG_WAVES), 0, s, n, qKS, sk, B, ct, ptxt_mod, mod,
                       msg);
    return hipGetLastError();
}

}  // namespace tfhe

#ifdef TFHE_TEST_PROBES
// ---- arithmetic probes (test library only; arith_probes.hpp, tests/test_gpu_arith_units.py) ----
// op: 0 addm64(a, b, m)  1 subm64(a, b, m)  2 to_mod(v, m)  3 centred(v, m)  4 mulmod_any(a, b, m)
//     5 div128(hi, lo, d)  6 companion(v, Q) u64  7 companion(v, Q) u32  8 draw_at(state, k)
// 3 words in, 1 out per case (the modulus travels with the case; Q is unused); no table
#include "arith_probes.hpp"

namespace tfhe {
namespace {
constexpr int KGP_NI = 3, KGP_NO = 1;
__global__ void k_arith_kg(int op, size_t cases, const uint64_t* __restrict__ in, const uint64_t* __restrict__, size_t,
                           uint64_t* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (!probe_lane_runs(op, i, cases)) return;
    const uint64_t* x = in + i * KGP_NI;
    uint64_t r = 0;
    switch (op & 15) {
        case 0: r = addm64(x[0], x[1], x[2]); break;
        case 1: r = subm64(x[0], x[1], x[2]); break;
        case 2: r = to_mod((int64_t)x[0], x[1]); break;
        case 3: r = (uint64_t)centred(x[0], x[1]); break;
        case 4: r = mulmod_any(x[0], x[1], x[2]); break;
        case 5: r = div128(x[0], x[1], x[2]); break;
        case 6: r = companion(x[0], x[1]); break;
        case 7: r = companion((uint32_t)x[0], (uint32_t)x[1]); break;
        default: r = draw_at(x[0], x[1]); break;
    }
    out[i * KGP_NO] = r;
}
}  // namespace
}  // namespace tfhe

extern "C" TFHE_ARITH_PROBE(kg) {
    (void)Q;
    if ((op & 15) > 8) return -1;
    return tfhe::probe_launch(tfhe::k_arith_kg, tfhe::KGP_NI, tfhe::KGP_NO, op, cases, in, in_words, tab, tab_words, out,
                              out_words);
}
#endif  // TFHE_TEST_PROBES
