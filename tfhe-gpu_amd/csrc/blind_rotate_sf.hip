// blind_rotate_sf.hip -- the special-form u64 blind rotations for N = 2048 and Q = 2^54 - c, c < 2^20 (the
// logQ / arbFunc contexts, Q = 2^54 - 77823: C3, C5b and their small-batch shards): gen3sf (gen3's schedule,
// blind_rotate_generic.hip, in sf arithmetic), sf2 (wave-local passes), sf2p (two ciphertexts per workgroup)
// and the two-workgroup forms sf2duo and sfduo (duo.hpp).  The round loop is written out in each kernel (one
// function for sf2's and sf2p's round took 83 spilled VGPRs at the 128-register budget); the steps they share
// are the sf_* leaves below and g3_store_acc (n2048_layout.hpp).
#include <cstdlib>

#include "device_math.hpp"
#include "duo.hpp"
#include "kernels.hpp"
#include "n2048_layout.hpp"

namespace tfhe {
namespace {

// ---------------------------------------------------------------------------
// gen3sf: gen3 for Q = 2^54 - c, c < 2^20 (the logQ / arbFunc contexts, Q = 2^54 - 77823: C3,
// C5b).  Every constant w (twiddle, key, monomial) is held as W0 = w and W1 = w 2^32 mod Q (the
// same 16 bytes as a word and its Shoup companion), and a product of any a < 2^64 with w is
//     a w = a0 W0 + a1 W1 (mod Q),  a0 = a mod 2^32, a1 = a >> 32:   S < 2^87
//     r = (S mod 2^55) + (S >> 55) 2c  < 2^55 + 2^33 c
// -- five v_mad_u64_u32 and no quotient estimate, against ten multiplies for the u64 Shoup
// product (round 4: nine VALU, device_math.hpp sf_mul).  Values stay unsigned and lazy: the
// forward transform needs no reduction and no offset (its inputs carry 28Q, so y' = x - v stays
// non-negative through 11 stages; outputs < 54 Q -- round 5: one VALU per butterfly less than
// x + (3Q - v)), the inverse
// folds its pure sums once per pass (x -> (x mod 2^54) + (x >> 54) c, one mad), the accumulator
// update folds once and subtracts Q at most once.  tools/bounds_sf.py checks every bound of
// this schedule.
// (SF_K and sf_mul live in device_math.hpp, shared with the VALU microbenchmark)

struct SfC {
    uint64_t Q, Q3, Qf, Q10;  // Q, 3Q (sf2p's forward offset), 28Q (what the other forward transforms'
                              // inputs carry), 10Q (inverse and monomial offsets; tools/bounds_sf.py)
    uint32_t c2;          // 2c: sf_mul folds at 2^55
    uint32_t c;
};
__device__ __forceinline__ uint64_t sf_fold(uint64_t x, uint32_t c) {
    return (x & ((1ull << SF_K) - 1)) + (uint64_t)(uint32_t)(x >> SF_K) * c;
}

struct SfTw {
    const uint64_t* __restrict__ w0;
    const uint64_t* __restrict__ w1;
};
// the same table pair in memory through buffer resources: a lane's twiddle address is a 32-bit
// offset from a uniform base, so no 64-bit per-lane addresses stay live across the round loop
// (sf2's two-digit build kept six of them in scratch)
struct SfTwB {
    __amdgpu_buffer_rsrc_t r0, r1;
};
__device__ __forceinline__ uint64_t tw0(const SfTw& T, uint32_t i) { return T.w0[i]; }
__device__ __forceinline__ uint64_t tw1(const SfTw& T, uint32_t i) { return T.w1[i]; }
__device__ __forceinline__ uint64_t tw0(const SfTwB& T, uint32_t i) {
    return __builtin_bit_cast(uint64_t, __builtin_amdgcn_raw_buffer_load_b64(T.r0, (int)(i * 8), 0, 0));
}
__device__ __forceinline__ uint64_t tw1(const SfTwB& T, uint32_t i) {
    return __builtin_bit_cast(uint64_t, __builtin_amdgcn_raw_buffer_load_b64(T.r1, (int)(i * 8), 0, 0));
}

// Monomial factors from two 64-entry LDS tables instead of gathers from the 2N-entry table in
// memory (those missed the cache and stalled every round, profiles/r02z): T[j] = psi^(64 j),
// T[64 + j] = psi^j as (W0, W1) pairs, built from mono = psi^k - 1 at kernel start, and
//     A0 (psi^e0 - 1) + A1 (psi^e1 - 1) = sf(sf(A0, T[e0 >> 6]), T[64 + (e0 & 63)]) + (the same for A1)
//                                       + (10Q - fold(A0 + A1))
// The low table's row is swizzled: a wave's exponents share their low four bits (sf_mrow below), so
// unswizzled its lanes hit 2-4 rows in one 16-byte bank group; bits 4-5 XOR-ed into 0-1 spread them.
constexpr uint32_t SF_MT = 256;  // u64 words of the two tables
__device__ __forceinline__ uint32_t sf_lrow(uint32_t x) { return 64 + (x ^ ((x >> 4) & 3)); }
__device__ __forceinline__ void sf_mono_tables(uint64_t* T, const uint64_t* __restrict__ mono,
                                               const uint64_t* __restrict__ mono1, uint64_t Q) {
    for (uint32_t k = threadIdx.x; k < 128; k += blockDim.x) {
        const uint32_t e = k < 64 ? 64 * k : k - 64, row = k < 64 ? k : sf_lrow(e);
        const uint64_t w0 = mono[e] + 1, w1 = mono1[e] + (1ull << 32);  // psi^e, psi^e 2^32
        T[2 * row] = w0 >= Q ? w0 - Q : w0;
        T[2 * row + 1] = w1 >= Q ? w1 - Q : w1;
    }
}
// both keys' factors of one column: A0 (psi^e0 - 1) + A1 (psi^e1 - 1), the two offsets merged into one
// subtraction of fold(A0 + A1), the sum folded (< 1.01 Q)
__device__ __forceinline__ uint64_t sf_mono_pair(uint64_t A0, uint32_t e0, uint64_t A1, uint32_t e1, const uint64_t* T,
                                                 const SfC& K) {
    const uint64_t* h0 = T + 2 * (e0 >> 6);
    const uint64_t* l0 = T + 2 * sf_lrow(e0 & 63);
    const uint64_t* h1 = T + 2 * (e1 >> 6);
    const uint64_t* l1 = T + 2 * sf_lrow(e1 & 63);
    const uint64_t p0 = sf_mul(sf_mul(A0, h0[0], h0[1], K.c2), l0[0], l0[1], K.c2);
    const uint64_t p1 = sf_mul(sf_mul(A1, h1[0], h1[1], K.c2), l1[0], l1[1], K.c2);
    return sf_fold(p0 + p1 + (K.Q10 - sf_fold(A0 + A1, K.c)), K.c);
}

// The whole 2N-row factor table in LDS (sf2p and the duo forms, whose workgroups have a CU's LDS to themselves):
// row e = (psi^e - 1, its W1), so A (X^(+-a') - 1) is ONE product per factor instead of sf_mono_pair's two and
// the offset (sf_factor_full).  Row of factor e: a wave's 64 lanes look up e = (2 br(slot) + 1) a' mod 2N with
// slots 4 lane + s: br(slot) keeps its low three bits (the wave's), so every lane's e has the same
// low four bits -- one 16-byte bank group, a 64-way conflict with rows stored in order (25 % of the
// kernel's cycles, profiles/r04p).  XOR-ing bits 4-7 and 8-11 into the low four spreads them.
__device__ __forceinline__ uint32_t sf_mrow(uint32_t e) { return e ^ (((e >> 4) ^ (e >> 8)) & 15); }
// both keys' factors of one slot: A0 (psi^e - 1) + A1 (psi^-e - 1), folded
__device__ __forceinline__ uint64_t sf_factor_full(uint64_t A0, uint64_t A1, uint32_t e, const uint64_t* mt, const SfC& K) {
    const uint64_t* fp = mt + 2 * sf_mrow(e);
    const uint64_t* fm = mt + 2 * sf_mrow((2 * G3_N - e) & (2 * G3_N - 1));
    return sf_fold(sf_mul(A0, fp[0], fp[1], K.c2) + sf_mul(A1, fm[0], fm[1], K.c2), K.c);
}

// ---- the round steps that sf2, sf2p, sf2duo and sfduo share ----
// A few steps stay written out in the kernels although they read the same: through a helper each changed the
// device code of a product kernel (scalar scheduling or operand order in the prologue, once the factor lookup's
// address arithmetic in sfduo's round; tools/asm_compare.py), and the kernels are held to the code measured.
// They are the Kd offset loop (every kernel), the factor table's staging `mt[2 sf_mrow(k)] = ...`, sf2p's own
// rotation exponents, sfduo's slot exponents and factor lookup, and the duo members' write-back.
// One key group: the 4 slots u4 .. u4+3 of one key row as (W0, W1) pairs, kw[s] = W0, kw[4 + s] = W1, through
// buffer resources (o: the round's and the row's uniform byte offset; a 32-bit lane offset)
typedef uint32_t v4u __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void sf_key_group(__amdgpu_buffer_rsrc_t rk0, __amdgpu_buffer_rsrc_t rk1, uint32_t u4,
                                             uint32_t o, uint64_t (&kw)[8]) {
    const v4u a0 = __builtin_bit_cast(v4u, __builtin_amdgcn_raw_buffer_load_b128(rk0, (int)(u4 * 8), (int)o, 0));
    const v4u a1 = __builtin_bit_cast(v4u, __builtin_amdgcn_raw_buffer_load_b128(rk0, (int)(u4 * 8 + 16), (int)o, 0));
    const v4u b0 = __builtin_bit_cast(v4u, __builtin_amdgcn_raw_buffer_load_b128(rk1, (int)(u4 * 8), (int)o, 0));
    const v4u b1 = __builtin_bit_cast(v4u, __builtin_amdgcn_raw_buffer_load_b128(rk1, (int)(u4 * 8 + 16), (int)o, 0));
    kw[0] = a0.x | ((uint64_t)a0.y << 32), kw[1] = a0.z | ((uint64_t)a0.w << 32);
    kw[2] = a1.x | ((uint64_t)a1.y << 32), kw[3] = a1.z | ((uint64_t)a1.w << 32);
    kw[4] = b0.x | ((uint64_t)b0.y << 32), kw[5] = b0.z | ((uint64_t)b0.w << 32);
    kw[6] = b1.x | ((uint64_t)b1.y << 32), kw[7] = b1.z | ((uint64_t)b1.w << 32);
}
// Slot x evaluates at psi^(2 bitrev(x) + 1): the rotation's exponents (2 bitrev(x) + 1) a' mod 2N at the lane's
// slots u4 .. u4+3.  The opaque copy keeps the compiler from hoisting them out of the round loop.
__device__ __forceinline__ void sf_slot_exponents(uint32_t u4, uint32_t ai, uint32_t (&ip)[4]) {
    uint32_t uo = u4;
    asm volatile("" : "+v"(uo));
#pragma unroll
    for (int s = 0; s < 4; ++s) ip[s] = ((2 * (__builtin_bitreverse32(uo + s) >> 21) + 1) * ai) & (2 * G3_N - 1);
}
// The closed-form decomposition (blind_rotate_fast.hip): digit lt of x (thrown digits counted) is that of
// c + Kd, c = x or x - Q (centred), Kd = (B/2)(B^lt - 1)/(B - 1) -- i.e. of x + (x < Q/2 ? Klo : Khi) with
// Klo = Kd, Khi = Kd - Q: the low logG bits, signed, of that sum >> (lt logG) (shift; sh = 64 - logG).  The
// digit r in [-B/2, B/2) enters the forward transform as r + 28Q or r + Q (congruent, no sign test; the offset
// the transform's differences consume, tools/bounds_sf.py).
__device__ __forceinline__ int64_t sf_digit(uint64_t x, uint64_t Qhalf, int64_t Klo, int64_t Khi, uint32_t shift,
                                            uint32_t sh) {
    const int64_t d = ((int64_t)x + (x < Qhalf ? Klo : Khi)) >> shift;
    return (int64_t)((uint64_t)d << sh) >> sh;
}
// the accumulator: canonical [0, Q) on entry and after every round's update (inc lazy: the sum folded, < 2Q)
__device__ __forceinline__ uint64_t sf_load_acc(uint64_t v, uint64_t Q) { return v >= Q ? v % Q : v; }
__device__ __forceinline__ uint64_t sf_add_acc(uint64_t a, uint64_t inc, const SfC& K) {
    const uint64_t x = sf_fold(a + inc, K.c);
    return x >= K.Q ? x - K.Q : x;
}

// OFS: the round-4 form, the offset in the difference (inputs r + Q, outputs < 35 Q), kept for sf2p and
// sf2duo: the offset-free form (89 / 46 fewer VALU per round there) measured 0.5 % / 0.9 % slower -- their
// rounds wait at barriers or on the partner, and in sf2p the allocator added three scratch loads to the
// loop (profiles/r05j, r05k).  sf2 and gen3sf use the offset-free form (C3 -1.3 %).
template <bool OFS = false, class TW>
__device__ __forceinline__ void sf_ct(uint64_t& x, uint64_t& y, const TW& T, uint32_t i, const SfC& K) {
    const uint64_t v = sf_mul(y, tw0(T, i), tw1(T, i), K.c2);
    if constexpr (OFS) y = x + (K.Q3 - v);
    else y = x - v;  // x >= 28Q - 11 x 2.3Q: no offset (tools/bounds_sf.py)
    x = x + v;
}
template <bool FOLD = false, class TW>
__device__ __forceinline__ void sf_gs(uint64_t& x, uint64_t& y, const TW& T, uint32_t i, const SfC& K) {
    const uint64_t d = x + (K.Q10 - y), s = x + y;
    x = FOLD ? sf_fold(s, K.c) : s;
    y = sf_mul(d, tw0(T, i), tw1(T, i), K.c2);
}

template <bool OFS = false, class TW>
__device__ __forceinline__ void sf_fwd_core(uint64_t (&v)[8], uint32_t m0, uint32_t g, const TW& T, const SfC& K) {
#pragma unroll
    for (int k = 0; k < 4; ++k) sf_ct<OFS>(v[k], v[k + 4], T, m0 + g, K);
    sf_ct<OFS>(v[0], v[2], T, 2 * m0 + 2 * g, K), sf_ct<OFS>(v[1], v[3], T, 2 * m0 + 2 * g, K);
    sf_ct<OFS>(v[4], v[6], T, 2 * m0 + 2 * g + 1, K), sf_ct<OFS>(v[5], v[7], T, 2 * m0 + 2 * g + 1, K);
#pragma unroll
    for (int j = 0; j < 4; ++j) sf_ct<OFS>(v[2 * j], v[2 * j + 1], T, 4 * m0 + 4 * g + j, K);
}
// FOLD: fold the last stage's sums (inverse passes C and B; bounds_sf.py INV_FOLD_PASS)
template <bool FOLD, class TW>
__device__ __forceinline__ void sf_inv_core(uint64_t (&v)[8], uint32_t m, uint32_t g, const TW& T, const SfC& K) {
#pragma unroll
    for (int j = 0; j < 4; ++j) sf_gs(v[2 * j], v[2 * j + 1], T, m + 4 * g + j, K);
    sf_gs(v[0], v[2], T, (m >> 1) + 2 * g, K), sf_gs(v[1], v[3], T, (m >> 1) + 2 * g, K);
    sf_gs(v[4], v[6], T, (m >> 1) + 2 * g + 1, K), sf_gs(v[5], v[7], T, (m >> 1) + 2 * g + 1, K);
#pragma unroll
    for (int k = 0; k < 4; ++k) sf_gs<FOLD>(v[k], v[k + 4], T, (m >> 2) + g, K);
}

__device__ __forceinline__ void sf_ntt_fwd(uint64_t* buf, uint64_t (&v)[8], const SfTw& T, const SfC& K) {
    constexpr uint32_t N = G3_N;
    const uint32_t tau = g3_tau();
    uint64_t* p = buf + (threadIdx.x >> 8) * N;
    {
        uint32_t ad[8];
        g3_ad(0, tau, ad);
        sf_fwd_core(v, 1, 0, T, K);
#pragma unroll
        for (int k = 0; k < 8; ++k) p[ad[k]] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int pass = 1; pass <= 2; ++pass) {
        uint32_t ad[8];
        g3_ad(pass, tau, ad);
        uint64_t w[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) w[k] = p[ad[k]];
        if (pass == 1) sf_fwd_core(w, 8, tau >> 5, T, K);
        else sf_fwd_core(w, 64, tau >> 2, T, K);
#pragma unroll
        for (int k = 0; k < 8; ++k) p[ad[k]] = w[k];
        __syncthreads();
    }
#pragma unroll
    for (uint32_t r = 0; r < 2; ++r) {  // stages 9 (h = 2) and 10 (h = 1) on units 4u .. 4u+3
        const uint32_t u = tau + 256 * r, u0 = g3_swz(4 * u);
        uint64_t v0 = p[u0], v1 = p[u0 ^ 1], v2 = p[u0 ^ 2], v3 = p[u0 ^ 3];
        sf_ct(v0, v2, T, N / 4 + u, K), sf_ct(v1, v3, T, N / 4 + u, K);
        sf_ct(v0, v1, T, N / 2 + 2 * u, K), sf_ct(v2, v3, T, N / 2 + 2 * u + 1, K);
        p[u0] = v0, p[u0 ^ 1] = v1, p[u0 ^ 2] = v2, p[u0 ^ 3] = v3;
    }
    __syncthreads();
}

__device__ __forceinline__ void sf_ntt_inv(uint64_t* buf, uint64_t (&v)[8], const SfTw& T, const SfC& K) {
    constexpr uint32_t N = G3_N;
    const uint32_t tau = g3_tau();
    uint64_t* p = buf + (threadIdx.x >> 8) * N;
#pragma unroll
    for (uint32_t r = 0; r < 2; ++r) {  // h = 1 then h = 2 on units 4u .. 4u+3; the second stage's sums folded
        const uint32_t u = tau + 256 * r, u0 = g3_swz(4 * u);
        uint64_t v0 = p[u0], v1 = p[u0 ^ 1], v2 = p[u0 ^ 2], v3 = p[u0 ^ 3];
        sf_gs(v0, v1, T, N / 2 + 2 * u, K), sf_gs(v2, v3, T, N / 2 + 2 * u + 1, K);
        sf_gs<true>(v0, v2, T, N / 4 + u, K), sf_gs<true>(v1, v3, T, N / 4 + u, K);
        p[u0] = v0, p[u0 ^ 1] = v1, p[u0 ^ 2] = v2, p[u0 ^ 3] = v3;
    }
    __syncthreads();
#pragma unroll
    for (int pass = 2; pass >= 1; --pass) {
        uint32_t ad[8];
        g3_ad(pass, tau, ad);
        uint64_t w[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) w[k] = p[ad[k]];
        if (pass == 2) sf_inv_core<true>(w, 256, tau >> 2, T, K);
        else sf_inv_core<true>(w, 32, tau >> 5, T, K);
#pragma unroll
        for (int k = 0; k < 8; ++k) p[ad[k]] = w[k];
        __syncthreads();
    }
    uint32_t ad[8];
    g3_ad(0, tau, ad);
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = p[ad[k]];
    sf_inv_core<false>(v, 4, 0, T, K);  // outputs < 18.1 Q: the accumulator update folds
}

// keys / monomials / inverse twiddles: W0 = the generic arena's words, W1 from sf1 (the same
// layout); forward twiddles (W0, W1) in LDS
__global__ void __launch_bounds__(G3_TH, 4)
k_blind_rotate_gen3sf(BRParams P, SfC K, const uint64_t* __restrict__ psi, const uint64_t* __restrict__ psi1,
                      const uint64_t* __restrict__ ipsi, const uint64_t* __restrict__ ipsi1,
                      const uint64_t* __restrict__ mono, const uint64_t* __restrict__ mono1,
                      const uint32_t* __restrict__ eidx, const uint64_t* __restrict__ bsk,
                      const uint64_t* __restrict__ bsk1, const uint64_t* __restrict__ a, uint64_t amod,
                      uint64_t* __restrict__ acc_io) {
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr uint32_t N = G3_N, TH = G3_TH, CN = G3_CN;
    uint64_t* buf = reinterpret_cast<uint64_t*>(smem);  // [2][N], swizzled
    const uint32_t t = threadIdx.x, twoN = 2 * N, logG = P.logG;
    const uint32_t ts = g3_swz(t);
    const uint64_t Q = K.Q, Qhalf = P.Q >> 1;
    const int64_t Qs = (int64_t)P.Q, Bh = (int64_t)1 << (logG - 1);
    const uint32_t sh = 64 - logG;
    uint64_t* psi_l = buf + 2 * N;
    uint64_t* psi1_l = psi_l + N;
    for (uint32_t k = t; k < N; k += TH) psi_l[k] = psi[k], psi1_l[k] = psi1[k];
    uint64_t* mt = psi1_l + N;  // monomial tables
    sf_mono_tables(mt, mono, mono1, Q);
    const SfTw TF{psi_l, psi1_l}, TI{ipsi, ipsi1};
    uint64_t* g = acc_io + (size_t)blockIdx.x * twoN;
    const uint64_t* ap = a + (size_t)blockIdx.x * P.n;
    uint32_t* ex = reinterpret_cast<uint32_t*>(smem + ((size_t)4 * G3_N + SF_MT) * 8);  // rotation exponents [n]
    stage_rot_exponents<G3_TH>(ex, ap, P.n, amod, twoN);
    __syncthreads();
    const size_t round_words = (size_t)4 * P.dG2 * N;
    auto lpos = [t](int p, int k) -> uint32_t { return (t >> 8) * N + (t & 255) + 256 * (p * CN + k); };

    uint64_t acc[2][CN];  // canonical [0, Q)
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int k = 0; k < CN; ++k) {
            acc[p][k] = sf_load_acc(g[lpos(p, k)], Q);
        }
    __syncthreads();  // forward twiddles in LDS

    for (uint32_t i = 0; i < P.n; ++i) {
        const uint32_t ai = ex[i];  // a'_i, staged at kernel start (rgsw-acc-cggi.cpp:153)
        uint64_t A[2][2][CN];  // A_kj per owned slot (< 2.3 Q per digit)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int k = 0; k < CN; ++k) A[kk][j][k] = 0;
        const uint64_t* ek = bsk + (size_t)i * round_words;
        const uint64_t* ek1 = bsk1 + (size_t)i * round_words;
        for (uint32_t l = 0; l < P.digits; ++l) {
            const uint32_t lt = l + P.thr, shift = lt * logG;
            int64_t Kd = 0;
            for (uint32_t z = 0; z < lt; ++z) Kd = (Kd << logG) + Bh;
            uint64_t v[8];
#pragma unroll
            for (int p = 0; p < 2; ++p)
#pragma unroll
                for (int k = 0; k < CN; ++k) {
                    const uint64_t x = acc[p][k];
                    const int64_t c = x < Qhalf ? (int64_t)x : (int64_t)x - Qs;
                    const int64_t d = (c + Kd) >> shift;
                    const int64_t r = (int64_t)((uint64_t)d << sh) >> sh;
                    v[p * CN + k] = (uint64_t)r + (r < 0 ? K.Qf + Q : K.Qf);  // r mod Q + 28Q
                }
            sf_ntt_fwd(buf, v, TF, K);  // pass A writes this thread's own entries: no barrier before
            // rows 2l (poly 0) and 2l+1 (poly 1), both keys, both columns; group g = (slot k, key kk)
            // holds 4 (W0, W1) key pairs, the next group's are loaded before this group's arithmetic
            constexpr int NG = CN * 2;
            auto kload = [&](int g, uint64_t (&kv)[8]) {
                const uint32_t x = t + TH * (g >> 1), kk = g & 1;
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 2; ++r) {
                        const size_t o = ((size_t)(kk * P.dG2 + 2 * l + r) * 2 + j) * N + x;
                        kv[(j * 2 + r) * 2] = ek[o];
                        kv[(j * 2 + r) * 2 + 1] = ek1[o];
                    }
            };
            uint64_t kv[2][8];
            kload(0, kv[0]);
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                if (g + 1 < NG) kload(g + 1, kv[(g + 1) & 1]);
                __builtin_amdgcn_sched_barrier(0);
                const int k = g >> 1, kk = g & 1;
                const uint64_t d0 = buf[ts + TH * k], d1 = buf[N + ts + TH * k];
                const uint64_t(&c)[8] = kv[g & 1];
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    A[kk][j][k] += sf_mul(d0, c[(j * 2) * 2], c[(j * 2) * 2 + 1], K.c2) +
                                   sf_mul(d1, c[(j * 2 + 1) * 2], c[(j * 2 + 1) * 2 + 1], K.c2);
                __builtin_amdgcn_sched_barrier(0);
            }
            __syncthreads();  // the next pass A rewrites entries other threads' products read
        }
#pragma unroll
        for (int k = 0; k < CN; ++k) {
            const uint32_t x = t + TH * k;
            const uint32_t ip = (eidx[x] * ai) & (twoN - 1), in = (twoN - ip) & (twoN - 1);
            buf[ts + TH * k] = sf_mono_pair(A[0][0][k], ip, A[1][0][k], in, mt, K);
            buf[N + ts + TH * k] = sf_mono_pair(A[0][1][k], ip, A[1][1][k], in, mt, K);
        }
        __syncthreads();
        uint64_t v[8];
        sf_ntt_inv(buf, v, TI, K);  // outputs < 18.1 Q
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int k = 0; k < CN; ++k) {
                acc[p][k] = sf_add_acc(acc[p][k], v[p * CN + k], K);
            }
    }
    __syncthreads();  // every last inverse pass has read its entries
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int k = 0; k < CN; ++k) buf[lpos(p, k)] = acc[p][k];
    __syncthreads();
    g3_store_acc(buf, g, t, Q);
}

// ---------------------------------------------------------------------------
// sf2: gen3sf with wave-local passes.  Wave w (of 8) owns the 256-element block w of BOTH
// polynomials after the forward transform's first pass: pass A (stages 0-2, elements
// tau + 256k) is the only exchange across wavefronts; passes B (3-5) and C (6-8) and the units
// (9-10) of block w run in wave w (lane l: polynomial l >> 5, sub-block index 32w + (l & 31);
// units u = 64w + l of both polynomials), with no workgroup barrier in between.  The units leave
// slots 4u .. 4u+3 of both polynomials in registers, so the products, the monomial factors and
// the inverse units run in registers (the key rows are 32 contiguous bytes per lane), and the
// inverse mirrors it: units, passes C and B in wave w, one barrier, pass A.  Barriers per round:
// one per forward transform, one more before each further digit's pass A (other waves may still
// read their blocks), one per inverse -- 2 for C3 and 4 for C5b instead of 9 and 14.
// tools/lds_layouts_wl.py checks the index algebra, the wave-locality and the banks.
__device__ __forceinline__ void wl_sync() {  // order this wave's LDS accesses (in-order LDS unit)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// forward: pass A from registers (polynomial t >> 8), barrier, B and C wave-local; then the units
// of u = 64w + l for both polynomials into d[p][j] = slot 4u + j
// TO_LDS: the units' outputs stay in the buffer (read back by this wave's products)
// PAIR: two ciphertexts per 1024-thread workgroup (k_blind_rotate_sf2p): the thread's index within its
// ciphertext's 512 threads
template <bool TO_LDS = false, class TW = SfTw, bool PAIR = false, bool OFS = PAIR>
__device__ __forceinline__ void sf2_ntt_fwd(uint64_t* buf, uint64_t (&v)[8], uint64_t (&d)[2][4], const TW& T,
                                            const SfC& K) {
    constexpr uint32_t N = G3_N;
    const uint32_t t = PAIR ? threadIdx.x & 511 : threadIdx.x, l = t & 63, w = t >> 6;
    {
        const uint32_t tau = g3_tau();
        uint64_t* p = buf + (t >> 8) * N;
        uint32_t ad[8];
        g3_ad(0, tau, ad);
        sf_fwd_core<OFS>(v, 1, 0, T, K);
#pragma unroll
        for (int k = 0; k < 8; ++k) p[ad[k]] = v[k];
    }
    __syncthreads();
    uint32_t tw = (w << 5) | (l & 31);
    asm volatile("" : "+v"(tw));
    uint64_t* p = buf + (l >> 5) * N;
#pragma unroll
    for (int pass = 1; pass <= 2; ++pass) {
        uint32_t ad[8];
        g3_ad(pass, tw, ad);
        uint64_t x[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] = p[ad[k]];
        if (pass == 1) sf_fwd_core<OFS>(x, 8, tw >> 5, T, K);
        else sf_fwd_core<OFS>(x, 64, tw >> 2, T, K);
#pragma unroll
        for (int k = 0; k < 8; ++k) p[ad[k]] = x[k];
        wl_sync();
    }
    const uint32_t u = (w << 6) | l, u0 = g3_swz(4 * u);
#pragma unroll
    for (int q = 0; q < 2; ++q) {  // stages 9 (h = 2) and 10 (h = 1) on slots 4u .. 4u+3
        const uint64_t* pq = buf + q * N;
        uint64_t v0 = pq[u0], v1 = pq[u0 ^ 1], v2 = pq[u0 ^ 2], v3 = pq[u0 ^ 3];
        sf_ct<OFS>(v0, v2, T, N / 4 + u, K), sf_ct<OFS>(v1, v3, T, N / 4 + u, K);
        sf_ct<OFS>(v0, v1, T, N / 2 + 2 * u, K), sf_ct<OFS>(v2, v3, T, N / 2 + 2 * u + 1, K);
        if constexpr (TO_LDS) {
            uint64_t* pw = buf + q * N;
            pw[u0] = v0, pw[u0 ^ 1] = v1, pw[u0 ^ 2] = v2, pw[u0 ^ 3] = v3;
        } else {
            d[q][0] = v0, d[q][1] = v1, d[q][2] = v2, d[q][3] = v3;
        }
    }
    if constexpr (TO_LDS) wl_sync();
}

// inverse: units of slots 4u .. 4u+3 from registers (second stage's sums folded), C and B
// wave-local (last stage's sums folded), barrier, pass A into v (polynomial t >> 8, < 18.1 Q)
// the units of polynomial q (this lane's own slots of the buffer)
template <class TW, bool PAIR = false>
__device__ __forceinline__ void sf2_inv_unit(uint64_t* buf, int q, const uint64_t (&sq)[4], const TW& T,
                                             const SfC& K) {
    constexpr uint32_t N = G3_N;
    const uint32_t t = PAIR ? threadIdx.x & 511 : threadIdx.x, l = t & 63, w = t >> 6;
    const uint32_t u = (w << 6) | l, u0 = g3_swz(4 * u);
    uint64_t* pq = buf + q * N;
    uint64_t v0 = sq[0], v1 = sq[1], v2 = sq[2], v3 = sq[3];
    sf_gs(v0, v1, T, N / 2 + 2 * u, K), sf_gs(v2, v3, T, N / 2 + 2 * u + 1, K);
    sf_gs<true>(v0, v2, T, N / 4 + u, K), sf_gs<true>(v1, v3, T, N / 4 + u, K);
    pq[u0] = v0, pq[u0 ^ 1] = v1, pq[u0 ^ 2] = v2, pq[u0 ^ 3] = v3;
}
// UNITS = false: the caller has already run both polynomials' units (sf2_inv_unit)
template <bool UNITS = true, class TW, bool PAIR = false>
__device__ __forceinline__ void sf2_ntt_inv(uint64_t* buf, uint64_t (&s)[2][4], uint64_t (&v)[8], const TW& T,
                                            const SfC& K) {
    constexpr uint32_t N = G3_N;
    const uint32_t t = PAIR ? threadIdx.x & 511 : threadIdx.x, l = t & 63, w = t >> 6;
    if constexpr (UNITS) {
#pragma unroll
        for (int q = 0; q < 2; ++q) sf2_inv_unit<TW, PAIR>(buf, q, s[q], T, K);
    }
    wl_sync();
    uint32_t tw = (w << 5) | (l & 31);
    asm volatile("" : "+v"(tw));
    uint64_t* p = buf + (l >> 5) * N;
#pragma unroll
    for (int pass = 2; pass >= 1; --pass) {
        uint32_t ad[8];
        g3_ad(pass, tw, ad);
        uint64_t x[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] = p[ad[k]];
        if (pass == 2) sf_inv_core<true>(x, 256, tw >> 2, T, K);
        else sf_inv_core<true>(x, 32, tw >> 5, T, K);
#pragma unroll
        for (int k = 0; k < 8; ++k) p[ad[k]] = x[k];
        if (pass == 2) wl_sync();
    }
    __syncthreads();
    const uint32_t tau = g3_tau();
    const uint64_t* pa = buf + (t >> 8) * N;
    uint32_t ad[8];
    g3_ad(0, tau, ad);
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = pa[ad[k]];
    sf_inv_core<false>(v, 4, 0, T, K);
}

// RESCUE (two digits; launched behind every sf2duo launch): only the ciphertexts whose duo pair timed
// out (failed word of the pair set) run, from the pair's saved input (rescue_src); the others exit at once
template <int DIG, bool RESCUE = false>
__global__ void __launch_bounds__(G3_TH, 4)
k_blind_rotate_sf2(BRParams P, SfC K, const uint64_t* __restrict__ psi, const uint64_t* __restrict__ psi1,
                   const uint64_t* __restrict__ ipsi, const uint64_t* __restrict__ ipsi1,
                   const uint64_t* __restrict__ mono, const uint64_t* __restrict__ mono1,
                   const uint64_t* __restrict__ bsk, const uint64_t* __restrict__ bsk1,
                   const uint64_t* __restrict__ a, uint64_t amod, uint64_t* __restrict__ acc_io,
                   const uint32_t* __restrict__ rescue_failed = nullptr, const uint64_t* __restrict__ rescue_src = nullptr) {
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr uint32_t N = G3_N, TH = G3_TH, CN = G3_CN;
    if constexpr (RESCUE) {
        if (__hip_atomic_load(const_cast<uint32_t*>(rescue_failed + (size_t)blockIdx.x * 64 + 1), __ATOMIC_RELAXED,
                              __HIP_MEMORY_SCOPE_AGENT) == 0)
            return;  // uniform: the pair finished
    }
    uint64_t* buf = reinterpret_cast<uint64_t*>(smem);  // [2][N], swizzled
    const uint32_t t = threadIdx.x, twoN = 2 * N, logG = P.logG;
    const uint64_t Q = K.Q, Qhalf = P.Q >> 1;
    const int64_t Qs = (int64_t)P.Q, Bh = (int64_t)1 << (logG - 1);
    const uint32_t sh = 64 - logG;
    uint64_t* psi_l = buf + 2 * N;
    uint64_t* psi1_l = psi_l + N;
    for (uint32_t k = t; k < N; k += TH) psi_l[k] = psi[k], psi1_l[k] = psi1[k];
    uint64_t* mt = psi1_l + N;  // monomial tables
    sf_mono_tables(mt, mono, mono1, Q);
    const SfTw TF{psi_l, psi1_l};
    const SfTwB TI{__builtin_amdgcn_make_buffer_rsrc(const_cast<uint64_t*>(ipsi), 0, (int)(N * 8), 0x00020000),
                   __builtin_amdgcn_make_buffer_rsrc(const_cast<uint64_t*>(ipsi1), 0, (int)(N * 8), 0x00020000)};
    uint64_t* g = acc_io + (size_t)blockIdx.x * twoN;
    const uint64_t* ap = a + (size_t)blockIdx.x * P.n;
    uint32_t* ex = reinterpret_cast<uint32_t*>(smem + ((size_t)4 * G3_N + SF_MT) * 8);  // rotation exponents [n]
    stage_rot_exponents<G3_TH>(ex, ap, P.n, amod, twoN);
    __syncthreads();
    const size_t round_words = (size_t)4 * P.dG2 * N;
    const uint32_t u4 = 4 * (((t >> 6) << 6) | (t & 63));  // this lane's slots u4 .. u4+3
    auto lpos = [t](int p, int k) -> uint32_t { return (t >> 8) * N + (t & 255) + 256 * (p * CN + k); };

    const uint64_t* gin = RESCUE ? rescue_src + (size_t)blockIdx.x * twoN : g;
    uint64_t acc[2][CN];  // canonical [0, Q), pass A's layout
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int k = 0; k < CN; ++k) {
            acc[p][k] = sf_load_acc(gin[lpos(p, k)], Q);
        }
    __syncthreads();  // forward twiddles in LDS

    const __amdgpu_buffer_rsrc_t rk0 = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint64_t*>(bsk), 0, -1, 0x00020000);
    const __amdgpu_buffer_rsrc_t rk1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint64_t*>(bsk1), 0, -1, 0x00020000);
    // the decomposition's offsets: digit l of x is that of c + Kd_l, c = x or x - Q (centred), i.e. of
    // x + (x < Q/2 ? Kd_l : Kd_l - Q); the digit r in [-B/2, B/2) enters the transform as r + 28Q
    // (congruent, no sign test; the offset the transform's differences consume, tools/bounds_sf.py)
    int64_t Kdl[DIG];
#pragma unroll
    for (int l = 0; l < DIG; ++l) {
        int64_t Kd = 0;
        for (uint32_t z = 0; z < l + P.thr; ++z) Kd = (Kd << logG) + Bh;
        Kdl[l] = Kd;
    }
    for (uint32_t i = 0; i < P.n; ++i) {
        // a_i mod amod (rgsw-acc-cggi.cpp:153) by a division, not a mask: with the mask, the
        // consumer of this round's scalar load moved past the forward transform and results came
        // out wrong intermittently on the STD128Q sets (profiles/r02ax: bisected to this line)
        const uint32_t ai = ex[i];  // a'_i, staged at kernel start (rgsw-acc-cggi.cpp:153)
        const uint32_t round_off = i * (uint32_t)round_words * 8;  // bytes (< 2^32: checked at launch)
        // forward outputs in registers; with an odd digit count the last digit's stay in LDS (one
        // digit: frees 16 VGPRs; three: the register budget of two)
        constexpr bool LAST_LDS = (DIG & 1) != 0;
        uint64_t D[DIG][2][4];
#pragma unroll
        for (int l = 0; l < DIG; ++l) {
            const uint32_t shift = (l + P.thr) * logG;
            const int64_t Klo = Kdl[l], Khi = Kdl[l] - Qs;
            uint64_t v[8];
#pragma unroll
            for (int p = 0; p < 2; ++p)
#pragma unroll
                for (int k = 0; k < CN; ++k) {
                    v[p * CN + k] = (uint64_t)sf_digit(acc[p][k], Qhalf, Klo, Khi, shift, sh) + K.Qf;
                }
            if (l > 0) __syncthreads();  // other waves may still read their blocks of digit l - 1
            // one digit: its outputs stay in LDS (frees 16 VGPRs; C3 18.8K -> 20.0K); two digits:
            // registers (LDS for the second measured 11.4K -> 10.0K on C5b, profiles/r02ah)
            if (LAST_LDS && l == DIG - 1) sf2_ntt_fwd<true>(buf, v, D[l], TF, K);
            else sf2_ntt_fwd(buf, v, D[l], TF, K);
        }
        // products: group g = (column j, key kk, row r = 2l + polynomial), 4 slots x (W0, W1) of key
        // words each, the next group's loaded before this group's arithmetic; A_kj of slots u4 + s
        // (< 2.3 Q per digit); once both keys of column j are summed, its monomial factors from the
        // two-level LDS tables (sf_mono_pair).  (Round 4 measured [2N][N] factor rows read from memory
        // instead, one product per factor: 24 % fewer VALU, but 17x the L2 fetches and slower on C3;
        // DESIGN.md 3.2c.)
        constexpr int RW = 2 * DIG, NG = 4 * RW;
        // key words through buffer resources: uniform round + row offset, 32-bit lane offset
        auto kload = [&](int g, uint64_t (&kw)[8]) {
            const uint32_t j = g / (2 * RW), kk = (g / RW) & 1, r = g % RW;
            const uint32_t o = round_off + ((kk * P.dG2 + r) * 2 + j) * N * 8;
            sf_key_group(rk0, rk1, u4, o, kw);
        };
        // the exponents of the lane's 4 slots, computed once per round (one digit) or at each column's
        // factors (more digits: 4 fewer live VGPRs through the products, 45 -> 16 scratch operations per
        // round for two)
        constexpr bool IP_ONCE = DIG == 1;
        uint32_t ip[4];
        if constexpr (IP_ONCE) sf_slot_exponents(u4, ai, ip);
        uint64_t S[2][4], A[2][4];
        uint64_t kw[2][8];
        kload(0, kw[0]);
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            if (g + 1 < NG) kload(g + 1, kw[(g + 1) & 1]);
            __builtin_amdgcn_sched_barrier(0);
            const int j = g / (2 * RW), kk = (g / RW) & 1, r = g % RW;
            const uint64_t(&c)[8] = kw[g & 1];
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const uint64_t dv = (LAST_LDS && r >= RW - 2) ? buf[(r & 1) * N + (g3_swz(u4) ^ s)] : D[r >> 1][r & 1][s];
                const uint64_t prod = sf_mul(dv, c[s], c[4 + s], K.c2);
                A[kk][s] = r == 0 ? prod : A[kk][s] + prod;
            }
            if (kk == 1 && r == RW - 1) {
                if constexpr (!IP_ONCE) sf_slot_exponents(u4, ai, ip);
#pragma unroll
                for (int s = 0; s < 4; ++s) S[j][s] = sf_mono_pair(A[0][s], ip[s], A[1][s], (twoN - ip[s]) & (twoN - 1), mt, K);
                // two digits: the buffer is dead after the last forward units (its outputs are in
                // registers), so column j's inverse units run now and S[j] dies here (fewer live
                // registers through column 1's products).  One or three digits: the buffer still holds
                // the last digit's outputs for column 1.
                if constexpr (!LAST_LDS) sf2_inv_unit(buf, j, S[j], TI, K);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        uint64_t v[8];
        sf2_ntt_inv<LAST_LDS>(buf, S, v, TI, K);  // outputs < 18.1 Q
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int k = 0; k < CN; ++k) {
                acc[p][k] = sf_add_acc(acc[p][k], v[p * CN + k], K);
            }
    }
    __syncthreads();  // every last inverse pass has read its entries
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int k = 0; k < CN; ++k) buf[lpos(p, k)] = acc[p][k];
    __syncthreads();
    g3_store_acc(buf, g, t, Q);
}

// ---------------------------------------------------------------------------
// sf2p: sf2 with TWO ciphertexts per 1024-thread workgroup (one per CU, 4 waves per SIMD as before),
// so the LDS the two share can hold the whole 2N-entry monomial factor table -- row e = (psi^e - 1,
// its W1), 64 KiB -- and A (X^(+-a') - 1) is ONE product per factor instead of two table products
// and an offset (sf_mono_pair).  The forward twiddles move from LDS to memory (buffer loads, like the
// inverse ones) to make room: per workgroup 2 x (32 KiB polynomial buffer + the exponents) + 64 KiB.
// Threads 512 h .. 512 h + 511 run ciphertext 2 b + h with sf2's code (the transform helpers take the
// thread's index within its ciphertext); every barrier is reached by both halves in the same order.
// PROBE 1 (test library only, timing only, results invalid): wave-uniform factor-table rows (every lane reads
// row a'), the bound on what the table's bank conflicts cost
template <int DIG, int PROBE = 0>
__global__ void __launch_bounds__(2 * G3_TH, 4)
k_blind_rotate_sf2p(BRParams P, SfC K, const uint64_t* __restrict__ psi, const uint64_t* __restrict__ psi1,
                    const uint64_t* __restrict__ ipsi, const uint64_t* __restrict__ ipsi1,
                    const uint64_t* __restrict__ mono, const uint64_t* __restrict__ mono1,
                    const uint64_t* __restrict__ bsk, const uint64_t* __restrict__ bsk1,
                    const uint64_t* __restrict__ a, uint64_t amod, uint64_t* __restrict__ acc_io, uint32_t B) {
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr uint32_t N = G3_N, TH = G3_TH, CN = G3_CN;
    const uint32_t half = __builtin_amdgcn_readfirstlane(threadIdx.x >> 9);
    const uint32_t t = threadIdx.x & 511, twoN = 2 * N, logG = P.logG;
    const uint32_t ct = min(2 * blockIdx.x + half, B - 1);  // an odd batch: the last half repeats its neighbour
    const bool owner = 2 * blockIdx.x + half < B;
    uint64_t* buf = reinterpret_cast<uint64_t*>(smem) + (size_t)half * 2 * N;  // [2][N] of this ciphertext
    uint64_t* mtab = reinterpret_cast<uint64_t*>(smem) + (size_t)4 * N;        // [2N] (W0, W1), shared
    uint32_t* ex = reinterpret_cast<uint32_t*>(smem + ((size_t)4 * N + 4 * N) * 8 + half * rot_exponent_bytes(P.n));
    const uint64_t Q = K.Q, Qhalf = P.Q >> 1;
    const int64_t Qs = (int64_t)P.Q, Bh = (int64_t)1 << (logG - 1);
    const uint32_t sh = 64 - logG;
    for (uint32_t k = threadIdx.x; k < twoN; k += 2 * TH) {
        mtab[2 * sf_mrow(k)] = mono[k] % Q;  // psi^k - 1
        mtab[2 * sf_mrow(k) + 1] = mono1[k];
    }
    const SfTwB TF{__builtin_amdgcn_make_buffer_rsrc(const_cast<uint64_t*>(psi), 0, (int)(N * 8), 0x00020000),
                   __builtin_amdgcn_make_buffer_rsrc(const_cast<uint64_t*>(psi1), 0, (int)(N * 8), 0x00020000)};
    const SfTwB TI{__builtin_amdgcn_make_buffer_rsrc(const_cast<uint64_t*>(ipsi), 0, (int)(N * 8), 0x00020000),
                   __builtin_amdgcn_make_buffer_rsrc(const_cast<uint64_t*>(ipsi1), 0, (int)(N * 8), 0x00020000)};
    uint64_t* g = acc_io + (size_t)ct * twoN;
    const uint64_t* ap = a + (size_t)ct * P.n;
    {
        const uint64_t scale = (uint64_t)twoN / amod;  // stage_rot_exponents for this half's 512 threads
        for (uint32_t k = t; k < P.n; k += TH) {
            const uint64_t ar = ap[k] % amod;
            ex[k] = (uint32_t)((ar == 0 ? 0 : amod - ar) * scale);
        }
    }
    __syncthreads();
    const size_t round_words = (size_t)4 * P.dG2 * N;
    const uint32_t u4 = 4 * (((t >> 6) << 6) | (t & 63));  // this lane's slots u4 .. u4+3
    auto lpos = [t](int p, int k) -> uint32_t { return (t >> 8) * N + (t & 255) + 256 * (p * CN + k); };

    uint64_t acc[2][CN];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int k = 0; k < CN; ++k) {
            acc[p][k] = sf_load_acc(g[lpos(p, k)], Q);
        }

    const __amdgpu_buffer_rsrc_t rk0 = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint64_t*>(bsk), 0, -1, 0x00020000);
    const __amdgpu_buffer_rsrc_t rk1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint64_t*>(bsk1), 0, -1, 0x00020000);
    int64_t Kdl[DIG];
#pragma unroll
    for (int l = 0; l < DIG; ++l) {
        int64_t Kd = 0;
        for (uint32_t z = 0; z < l + P.thr; ++z) Kd = (Kd << logG) + Bh;
        Kdl[l] = Kd;
    }
    for (uint32_t i = 0; i < P.n; ++i) {
        const uint32_t ai = ex[i];
        const uint32_t round_off = i * (uint32_t)round_words * 8;
        constexpr bool LAST_LDS = (DIG & 1) != 0;
        uint64_t D[DIG][2][4];
#pragma unroll
        for (int l = 0; l < DIG; ++l) {
            const uint32_t shift = (l + P.thr) * logG;
            const int64_t Klo = Kdl[l], Khi = Kdl[l] - Qs;
            uint64_t v[8];
#pragma unroll
            for (int p = 0; p < 2; ++p)
#pragma unroll
                for (int k = 0; k < CN; ++k) {
                    // sf_ct<true>: inputs r + Q
                    v[p * CN + k] = (uint64_t)(sf_digit(acc[p][k], Qhalf, Klo, Khi, shift, sh) + Qs);
                }
            if (l > 0) __syncthreads();
            if (LAST_LDS && l == DIG - 1) sf2_ntt_fwd<true, SfTwB, true>(buf, v, D[l], TF, K);
            else sf2_ntt_fwd<false, SfTwB, true>(buf, v, D[l], TF, K);
        }
        constexpr int RW = 2 * DIG, NG = 4 * RW;
        auto kload = [&](int gi, uint64_t (&kw)[8]) {
            const uint32_t j = gi / (2 * RW), kk = (gi / RW) & 1, r = gi % RW;
            const uint32_t o = round_off + ((kk * P.dG2 + r) * 2 + j) * N * 8;
            sf_key_group(rk0, rk1, u4, o, kw);
        };
        constexpr bool IP_ONCE = DIG == 1;
        uint32_t ip[4];
        if constexpr (IP_ONCE) sf_slot_exponents(u4, ai, ip);
        uint64_t S[2][4], A[2][4];
        uint64_t kw[2][8];
        kload(0, kw[0]);
#pragma unroll
        for (int gi = 0; gi < NG; ++gi) {
            if (gi + 1 < NG) kload(gi + 1, kw[(gi + 1) & 1]);
            __builtin_amdgcn_sched_barrier(0);
            const int j = gi / (2 * RW), kk = (gi / RW) & 1, r = gi % RW;
            const uint64_t(&c)[8] = kw[gi & 1];
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const uint64_t dv = (LAST_LDS && r >= RW - 2) ? buf[(r & 1) * N + (g3_swz(u4) ^ s)] : D[r >> 1][r & 1][s];
                const uint64_t prod = sf_mul(dv, c[s], c[4 + s], K.c2);
                A[kk][s] = r == 0 ? prod : A[kk][s] + prod;
            }
            if (kk == 1 && r == RW - 1) {
                if constexpr (!IP_ONCE) sf_slot_exponents(u4, ai, ip);
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    if constexpr (PROBE == 1) ip[s] = ai & (twoN - 1);
                    S[j][s] = sf_factor_full(A[0][s], A[1][s], ip[s], mtab, K);
                }
                if constexpr (!LAST_LDS) sf2_inv_unit<SfTwB, true>(buf, j, S[j], TI, K);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        uint64_t v[8];
        sf2_ntt_inv<LAST_LDS, SfTwB, true>(buf, S, v, TI, K);
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int k = 0; k < CN; ++k) {
                acc[p][k] = sf_add_acc(acc[p][k], v[p * CN + k], K);
            }
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int k = 0; k < CN; ++k) buf[lpos(p, k)] = acc[p][k];
    __syncthreads();
    if (owner) g3_store_acc(buf, g, t, Q);
}

// ---------------------------------------------------------------------------
// sf2duo: the two-digit sf2 round split over TWO workgroups per ciphertext, for batches too small
// to fill the chip (round 4: C5b's 128-ciphertext shard of an 8-GPU node ran one workgroup per CU
// on half the CUs).  Since round 6 the test library's A/B form only (probe 13): sfduo<2> below, split by NTT
// half, measured 1.5-3 % faster and is the default.  Workgroup x of a pair owns accumulator polynomial x: it decomposes acc_x into
// its two digits (threads 0-255 digit 0, 256-511 digit 1: the forward transform of sf2 with the
// digits in place of the polynomials), multiplies them by key rows 2l + x of both keys and both
// columns, applies the monomial factors to its partial sums of both columns and inverts both
// (sf2's inverse).  INTT is linear, so acc_x += INTT(S_x) = its own column-x output plus the
// partner's; each round the workgroup publishes its column-(1-x) output (16 KiB) to the partner and takes
// the partner's (the hand-off, its ordering assumptions and the 10 ms bound on every wait: duo.hpp).  Per
// workgroup and round: half the forward transforms and half the products of sf2<2>, the same monomial and
// inverse work.  A pair that times out is recomputed by k_blind_rotate_sf2<2, true>, queued right behind.
// PROBE 1 (test library only, TFHE_TEST_PROBES; tests/test_gpu_duo.py): member 1 of pair 0 stops publishing
// at round 2, as a partner that never arrives would, and the wait is a 64th of the 10 ms bound
#ifndef SF2D_KPRE
#define SF2D_KPRE 2
#endif
// one workgroup per CU leaves the LDS for sf2p's whole 2N-row factor table (64 KiB): one table product per
// monomial factor instead of two and the offset term (sf_mono_pair)
constexpr size_t SF2D_MT = 4 * G3_N;  // u64 words of the factor table
// one workgroup per CU at the batches it serves (<= kDuoMaxPairs pairs, default 128): two waves per SIMD, so
// the register budget is 256 -- room for the key groups in flight (SF2D_KPRE)
template <int PROBE = 0>
__global__ void __launch_bounds__(G3_TH, SF2D_KPRE >= 2 ? 2 : 4)
k_blind_rotate_sf2duo(BRParams P, SfC K, const uint64_t* __restrict__ psi, const uint64_t* __restrict__ psi1,
                      const uint64_t* __restrict__ ipsi, const uint64_t* __restrict__ ipsi1,
                      const uint64_t* __restrict__ mono, const uint64_t* __restrict__ mono1,
                      const uint64_t* __restrict__ bsk, const uint64_t* __restrict__ bsk1,
                      const uint64_t* __restrict__ a, uint64_t amod, uint64_t* __restrict__ acc_io, DuoBuf X,
                      uint32_t pairs) {
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr uint32_t N = G3_N, TH = G3_TH;
    const uint32_t b = blockIdx.x, pair = (b >> 4) * 8 + (b & 7), x = (b >> 3) & 1;
    if (pair >= pairs) return;  // both members of a pair take this branch together
    __shared__ uint32_t duo_ok;
    uint64_t* buf = reinterpret_cast<uint64_t*>(smem);  // [2][N], swizzled
    const uint32_t t = threadIdx.x, twoN = 2 * N, logG = P.logG;
    const uint32_t half = __builtin_amdgcn_readfirstlane(t >> 8);  // digit (forward), column (inverse)
    const uint64_t Q = K.Q, Qhalf = P.Q >> 1;
    const int64_t Qs = (int64_t)P.Q, Bh = (int64_t)1 << (logG - 1);
    const uint32_t sh = 64 - logG;
    uint64_t* psi_l = buf + 2 * N;
    uint64_t* psi1_l = psi_l + N;
    for (uint32_t k = t; k < N; k += TH) psi_l[k] = psi[k], psi1_l[k] = psi1[k];
    uint64_t* mt = psi1_l + N;  // the whole 2N-row factor table, sf2p's layout
    for (uint32_t k = t; k < twoN; k += TH) {
        mt[2 * sf_mrow(k)] = mono[k] % Q;  // psi^k - 1
        mt[2 * sf_mrow(k) + 1] = mono1[k];
    }
    const SfTw TF{psi_l, psi1_l};
    const SfTwB TI{__builtin_amdgcn_make_buffer_rsrc(const_cast<uint64_t*>(ipsi), 0, (int)(N * 8), 0x00020000),
                   __builtin_amdgcn_make_buffer_rsrc(const_cast<uint64_t*>(ipsi1), 0, (int)(N * 8), 0x00020000)};
    uint64_t* g = acc_io + (size_t)pair * twoN;
    const uint64_t* ap = a + (size_t)pair * P.n;
    uint32_t* ex = reinterpret_cast<uint32_t*>(smem + ((size_t)4 * G3_N + SF2D_MT) * 8);  // rotation exponents [n]
    stage_rot_exponents<G3_TH>(ex, ap, P.n, amod, twoN);
    const size_t round_words = (size_t)4 * P.dG2 * N;
    const uint32_t u4 = 4 * (((t >> 6) << 6) | (t & 63));  // this lane's slots u4 .. u4+3
    const uint32_t c0 = t & 255;                            // coefficients c0 + 256 k of acc_x

    uint64_t acc[8];  // acc_x, canonical [0, Q); both halves hold the same values
    uint64_t* sv = X.save + (size_t)pair * twoN + x * N;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint64_t v = g[x * N + c0 + 256 * k];
        if (half == 0) sv[c0 + 256 * k] = v;  // the rescue kernel's input if the pair times out
        acc[k] = sf_load_acc(v, Q);
    }
    __syncthreads();  // forward twiddles, exponents in LDS

    const __amdgpu_buffer_rsrc_t rk0 = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint64_t*>(bsk), 0, -1, 0x00020000);
    const __amdgpu_buffer_rsrc_t rk1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint64_t*>(bsk1), 0, -1, 0x00020000);
    int64_t Kd = 0;  // digit `half` of acc_x (sf2's closed-form offsets)
    for (uint32_t z = 0; z < half + P.thr; ++z) Kd = (Kd << logG) + Bh;
    const int64_t Klo = Kd, Khi = Kd - Qs;
    const uint32_t shift = (half + P.thr) * logG;
    uint32_t* myflag = X.flags + (pair * 2 + x) * 32;
    const uint32_t* peerflag = X.flags + (pair * 2 + (1 - x)) * 32;
    for (uint32_t i = 0; i < P.n; ++i) {
        const uint32_t ai = ex[i];
        const uint32_t round_off = i * (uint32_t)round_words * 8;  // bytes (< 2^32: checked at launch)
        uint64_t v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            v[k] = (uint64_t)(sf_digit(acc[k], Qhalf, Klo, Khi, shift, sh) + Qs);  // sf_ct<true>: inputs r + Q
        }
        // products: group g = (column j, key kk, digit l: key row 2l + x), then column j's factors
        constexpr int RW = 2, NG = 4 * RW;
        auto kload = [&](int gi, uint64_t (&kw)[8]) {
            const uint32_t j = gi / (2 * RW), kk = (gi / RW) & 1, l = gi % RW;
            const uint32_t o = round_off + ((kk * P.dG2 + 2 * l + x) * 2 + j) * N * 8;
            sf_key_group(rk0, rk1, u4, o, kw);
        };
        // SF2D_KPRE: the round's first key group is requested before the forward transform (its L2 latency
        // overlaps the transform; two waves per SIMD hide little -- as f64wduo, blind_rotate_f64.hip)
        // (SF2D_KPRE = d groups in flight, a ring of d + 1 groups; 0: group 0 requested at the products)
        constexpr int KD = SF2D_KPRE > 0 ? SF2D_KPRE : 1, KR = KD + 1 < 8 ? KD + 1 : 8;
        uint64_t kw[KR][8];
#pragma unroll
        for (int g = 0; g < (SF2D_KPRE > 0 ? KD : 0); ++g) kload(g, kw[g]);
        uint64_t D[2][4];  // D[l][s]: digit l of acc_x at slots u4 + s
        if (i > 0) __syncthreads();  // every thread has read the previous round's exchange from the buffer
        sf2_ntt_fwd<false, SfTw, false, true>(buf, v, D, TF, K);
        uint32_t ip[4];
        sf_slot_exponents(u4, ai, ip);
        uint64_t S[2][4], A[2][4];
        if constexpr (SF2D_KPRE == 0) kload(0, kw[0]);
#pragma unroll
        for (int gi = 0; gi < NG; ++gi) {
            if (gi + KD < NG) kload(gi + KD, kw[(gi + KD) % KR]);
            __builtin_amdgcn_sched_barrier(0);
            const int j = gi / (2 * RW), kk = (gi / RW) & 1, l = gi % RW;
            const uint64_t(&c)[8] = kw[gi % KR];
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const uint64_t prod = sf_mul(D[l][s], c[s], c[4 + s], K.c2);
                A[kk][s] = l == 0 ? prod : A[kk][s] + prod;
            }
            if (kk == 1 && l == RW - 1) {
#pragma unroll
                for (int s = 0; s < 4; ++s) S[j][s] = sf_factor_full(A[0][s], A[1][s], ip[s], mt, K);
                sf2_inv_unit(buf, j, S[j], TI, K);  // the buffer is dead after the forward units
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        sf2_ntt_inv<false>(buf, S, v, TI, K);  // v: this workgroup's INTT(S_half) at c0 + 256 k, < 18.1 Q
        // exchange: column 1 - x goes to the partner, column x stays (through the buffer)
        uint64_t* mine = X.xbuf + (((size_t)pair * 2 + x) * 2 + (i & 1)) * N;
        const uint64_t* theirs = X.xbuf + (((size_t)pair * 2 + (1 - x)) * 2 + (i & 1)) * N;
        if (half != x) {
#pragma unroll
            for (int k = 0; k < 8; ++k) duo_store(mine + c0 + 256 * k, v[k]);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();  // every wave's stores drained; every read of the inverse's pass A done
        if (half == x) {
#pragma unroll
            for (int k = 0; k < 8; ++k) buf[c0 + 256 * k] = v[k];
        }
        if (t == 0) {  // the hand-off protocol: duo.hpp
            const bool gone = PROBE == 1 && pair == 0 && x == 1 && i >= 2;
            const bool ok = duo_publish_and_wait<PROBE != 0>(myflag, peerflag, i, X.wait_ticks, gone);
            duo_ok = ok;
            if (!ok) duo_fail_pair(X, pair);
        }
        __syncthreads();
        if (!duo_ok) break;  // uniform: the partner never arrived (the rescue launch recomputes the pair)
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            acc[k] = sf_add_acc(acc[k], buf[c0 + 256 * k] + duo_load(theirs + c0 + 256 * k), K);  // the sum < 37.2 Q
        }
    }
    __syncthreads();  // every thread has read the last exchange
    if (half == 0) {
#pragma unroll
        for (int k = 0; k < 8; ++k) buf[c0 + 256 * k] = acc[k];
    }
    __syncthreads();
    for (uint32_t k = t; k < N; k += TH) {
        if (x == 0) {  // acc0 transposed (poly.cpp:762-770)
            const uint64_t v = buf[k == 0 ? 0 : N - k];
            g[k] = k == 0 ? v : (v == 0 ? 0 : Q - v);
        } else {
            g[N + k] = buf[k];
        }
    }
}

// ---------------------------------------------------------------------------
// sfduo: the special-form round on TWO workgroups per ciphertext, split by NTT half -- f64wduo's design
// (blind_rotate_f64.hip) in sf arithmetic.  sf2duo splits by accumulator polynomial, which needs two digits
// per polynomial to keep its 512 threads busy; the one-digit contexts (C3's arbFunc logQ 12 class: sf2<1>)
// ran one workgroup per ciphertext at every batch (verdict r5 "missing" 2).  The negacyclic transform's
// stage 0 pairs x and x + N/2; after it the two halves of the slots are independent rings until the
// inverse's stage 0.  Member h of a pair (blocks b and b + 8, as sf2duo) holds the whole accumulator (both
// polynomials, pass-A layout: thread t has coefficients tau + 256k of polynomial t >> 8) and per round:
//   * extracts every coefficient's digits (sf2's closed form, inputs r + 28Q: the offset-free forward);
//   * forward of each digit polynomial: stage 0 for its half's outputs only, stages 1-2 on the thread's 4
//     values (one barrier), stages 3-10 wave-local (wave w: 256-block w & 3 of half h of polynomial w >> 2,
//     radix-4 passes (3,4) (5,6) (7,8) (9,10)), so the lane ends with 4 slots of one polynomial;
//   * products for column w >> 2 of its half's slots: its own polynomial's digits from registers, the other
//     polynomial's through LDS (one barrier), 2 keys x 2 DIG rows; one table product per monomial factor
//     (the whole 2N-row factor table in LDS, sf2p's layout);
//   * inverse stages 10-3 wave-local, stages 2-1 across waves (one barrier), with sf2's folds (the sums of
//     stages 9, 6 and 3), then hands its 4 stage-1 values per thread (16 KiB) to the partner and takes the
//     partner's (the sf2duo hand-off, bounded wait), and both finish stage 0 and the accumulator update for
//     all coefficients.
// Every element goes through sf2's butterflies in sf2's order with the same folds, so sf2's bounds hold
// unchanged (tools/bounds_sf.py); the buffers use f64wduo's swizzle (dswz, 8-byte words as there).  Per lane
// and round: 24 forward products per digit against sf2's 44, 8 x DIG key products against 16 x DIG, 8 factor
// products against 16, 24 inverse against 44.  A member that times out sets the pair's failed word and the
// rescue launch (k_blind_rotate_sf2<DIG, true>) recomputes the ciphertext from its saved input.
// LDS: twiddles 32 KiB (both directions' compact half tables, twi), forward / inverse buffers 2 x 16 KiB, two
// digits a third buffer, factor table 64 KiB, exponents: 132 / 148 KiB, one workgroup per CU.
// Twiddle index of stage s (full table: 2^s + j) in the member's compact half table -- a member of an
// NTT-half pair uses only the entries of its half at every stage s >= 1 (j in [h 2^(s-1), (h + 1) 2^(s-1))),
// so entry 2^s + j moves to 2^(s-1) + (j - h 2^(s-1)), and stage 0's entry 1 to 0: N / 2 entries per table,
// which lets both directions' twiddles sit in LDS
__device__ __forceinline__ uint32_t twi(uint32_t idx, int s, uint32_t h) {
    return s == 0 ? 0u : idx - (1u << (s - 1)) * (1 + h);
}
template <class TW>
__device__ __forceinline__ void sfd_fwd(uint64_t* bf, const uint64_t (&v)[8], uint64_t (&d)[4], uint32_t h,
                                        const TW& T, const SfC& K) {
    constexpr uint32_t H = G3_N / 2;
    const uint32_t t = threadIdx.x, l = t & 63, w = t >> 6;
    {
        const uint32_t tau = g3_tau();
        uint64_t* p = bf + (t >> 8) * H + dswz(tau);
        const uint64_t w0 = tw0(T, twi(1, 0, h)), w1 = tw1(T, twi(1, 0, h));
        uint64_t o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {  // stage 0, this half's outputs (x - v >= 0: inputs carry 28Q)
            const uint64_t x = sf_mul(v[k + 4], w0, w1, K.c2);
            o[k] = h ? v[k] - x : v[k] + x;
        }
        sf_ct(o[0], o[2], T, twi(2 + h, 1, h), K), sf_ct(o[1], o[3], T, twi(2 + h, 1, h), K);
        sf_ct(o[0], o[1], T, twi(4 + 2 * h, 2, h), K), sf_ct(o[2], o[3], T, twi(5 + 2 * h, 2, h), K);
#pragma unroll
        for (int k = 0; k < 4; ++k) p[256 * k] = o[k];
    }
    __syncthreads();
    const uint32_t B = 4 * h + (w & 3);  // 256-block of the whole polynomial
    uint64_t* q = bf + (w >> 2) * H + 256 * (w & 3);
    uint64_t x[4];
    {  // stages 3, 4
        uint32_t y = l;
        asm volatile("" : "+v"(y));
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = q[dswz(y + 64 * k)];
        sf_ct(x[0], x[2], T, twi(8 + B, 3, h), K), sf_ct(x[1], x[3], T, twi(8 + B, 3, h), K);
        sf_ct(x[0], x[1], T, twi(16 + 2 * B, 4, h), K), sf_ct(x[2], x[3], T, twi(17 + 2 * B, 4, h), K);
#pragma unroll
        for (int k = 0; k < 4; ++k) q[dswz(y + 64 * k)] = x[k];
    }
    wl_sync();
    {  // stages 5, 6
        const uint32_t c = l >> 4, y = 64 * c + (l & 15);
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = q[dswz(y + 16 * k)];
        sf_ct(x[0], x[2], T, twi(32 + 4 * B + c, 5, h), K), sf_ct(x[1], x[3], T, twi(32 + 4 * B + c, 5, h), K);
        sf_ct(x[0], x[1], T, twi(64 + 8 * B + 2 * c, 6, h), K), sf_ct(x[2], x[3], T, twi(65 + 8 * B + 2 * c, 6, h), K);
#pragma unroll
        for (int k = 0; k < 4; ++k) q[dswz(y + 16 * k)] = x[k];
    }
    wl_sync();
    {  // stages 7, 8
        const uint32_t c = l >> 2, y = 16 * c + (l & 3);
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = q[dswz(y + 4 * k)];
        sf_ct(x[0], x[2], T, twi(128 + 16 * B + c, 7, h), K), sf_ct(x[1], x[3], T, twi(128 + 16 * B + c, 7, h), K);
        sf_ct(x[0], x[1], T, twi(256 + 32 * B + 2 * c, 8, h), K), sf_ct(x[2], x[3], T, twi(257 + 32 * B + 2 * c, 8, h), K);
#pragma unroll
        for (int k = 0; k < 4; ++k) q[dswz(y + 4 * k)] = x[k];
    }
    wl_sync();
    {  // stages 9, 10: slots 4u .. 4u+3, u = 64 B + l (sf2's units)
        const uint32_t y = 4 * l;
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = q[dswz(y + k)];
        sf_ct(x[0], x[2], T, twi(512 + 64 * B + l, 9, h), K), sf_ct(x[1], x[3], T, twi(512 + 64 * B + l, 9, h), K);
        sf_ct(x[0], x[1], T, twi(1024 + 128 * B + 2 * l, 10, h), K), sf_ct(x[2], x[3], T, twi(1025 + 128 * B + 2 * l, 10, h), K);
#pragma unroll
        for (int k = 0; k < 4; ++k) d[k] = x[k];
    }
}

// inverse: s = column w >> 2's NTT-domain increment at the lane's slots -> after stages 10..1 o = elements
// tau + 256k' (k' < 4) of half h of column t >> 8 (stage-1 outputs; stage 0 follows the hand-off)
template <class TW>
__device__ __forceinline__ void sfd_inv(uint64_t* bi, const uint64_t (&s)[4], uint64_t (&o)[4], uint32_t h,
                                        const TW& T, const SfC& K) {
    constexpr uint32_t H = G3_N / 2;
    const uint32_t t = threadIdx.x, l = t & 63, w = t >> 6;
    const uint32_t B = 4 * h + (w & 3);
    uint64_t* q = bi + (w >> 2) * H + 256 * (w & 3);
    uint64_t x[4] = {s[0], s[1], s[2], s[3]};
    {  // stages 10, 9 (stage 9's sums folded, as sf2's units)
        const uint32_t y = 4 * l;
        sf_gs(x[0], x[1], T, twi(1024 + 128 * B + 2 * l, 10, h), K), sf_gs(x[2], x[3], T, twi(1025 + 128 * B + 2 * l, 10, h), K);
        sf_gs<true>(x[0], x[2], T, twi(512 + 64 * B + l, 9, h), K), sf_gs<true>(x[1], x[3], T, twi(512 + 64 * B + l, 9, h), K);
#pragma unroll
        for (int k = 0; k < 4; ++k) q[dswz(y + k)] = x[k];
    }
    wl_sync();
    {  // stages 8, 7
        const uint32_t c = l >> 2, y = 16 * c + (l & 3);
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = q[dswz(y + 4 * k)];
        sf_gs(x[0], x[1], T, twi(256 + 32 * B + 2 * c, 8, h), K), sf_gs(x[2], x[3], T, twi(257 + 32 * B + 2 * c, 8, h), K);
        sf_gs(x[0], x[2], T, twi(128 + 16 * B + c, 7, h), K), sf_gs(x[1], x[3], T, twi(128 + 16 * B + c, 7, h), K);
#pragma unroll
        for (int k = 0; k < 4; ++k) q[dswz(y + 4 * k)] = x[k];
    }
    wl_sync();
    {  // stages 6, 5 (stage 6's sums folded, as the end of sf2's pass C)
        const uint32_t c = l >> 4, y = 64 * c + (l & 15);
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = q[dswz(y + 16 * k)];
        sf_gs<true>(x[0], x[1], T, twi(64 + 8 * B + 2 * c, 6, h), K), sf_gs<true>(x[2], x[3], T, twi(65 + 8 * B + 2 * c, 6, h), K);
        sf_gs(x[0], x[2], T, twi(32 + 4 * B + c, 5, h), K), sf_gs(x[1], x[3], T, twi(32 + 4 * B + c, 5, h), K);
#pragma unroll
        for (int k = 0; k < 4; ++k) q[dswz(y + 16 * k)] = x[k];
    }
    wl_sync();
    {  // stages 4, 3 (stage 3's sums folded, as the end of sf2's pass B)
        uint32_t y = l;
        asm volatile("" : "+v"(y));
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = q[dswz(y + 64 * k)];
        sf_gs(x[0], x[1], T, twi(16 + 2 * B, 4, h), K), sf_gs(x[2], x[3], T, twi(17 + 2 * B, 4, h), K);
        sf_gs<true>(x[0], x[2], T, twi(8 + B, 3, h), K), sf_gs<true>(x[1], x[3], T, twi(8 + B, 3, h), K);
#pragma unroll
        for (int k = 0; k < 4; ++k) q[dswz(y + 64 * k)] = x[k];
    }
    __syncthreads();
    {  // stages 2, 1 of half h (no fold, as sf2's pass A)
        const uint32_t tau = g3_tau();
        const uint64_t* p = bi + (t >> 8) * H + dswz(tau);
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = p[256 * k];
        sf_gs(o[0], o[1], T, twi(4 + 2 * h, 2, h), K), sf_gs(o[2], o[3], T, twi(5 + 2 * h, 2, h), K);
        sf_gs(o[0], o[2], T, twi(2 + h, 1, h), K), sf_gs(o[1], o[3], T, twi(2 + h, 1, h), K);
    }
}

#ifndef SFD_KPRE
#define SFD_KPRE 2
#endif

// PROBE 1 (test library only, TFHE_TEST_PROBES): member 1 of pair 0 stops publishing at round 2, as a partner
// that never arrives would, and the wait is a 64th of the 10 ms bound.  PROBE 2 (timing only, results invalid):
// no hand-off -- each member takes its own stage-1 values for its partner's.
// The hand-off and its hardware assumptions: duo.hpp.
template <int DIG, int PROBE = 0>
__global__ void __launch_bounds__(G3_TH, 2)
k_blind_rotate_sfduo(BRParams P, SfC K, const uint64_t* __restrict__ psi, const uint64_t* __restrict__ psi1,
                     const uint64_t* __restrict__ ipsi, const uint64_t* __restrict__ ipsi1,
                     const uint64_t* __restrict__ mono, const uint64_t* __restrict__ mono1,
                     const uint64_t* __restrict__ bsk, const uint64_t* __restrict__ bsk1,
                     const uint64_t* __restrict__ a, uint64_t amod, uint64_t* __restrict__ acc_io, DuoBuf X,
                     uint32_t pairs) {
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr uint32_t N = G3_N, H = N / 2, TH = G3_TH;
    const uint32_t b = blockIdx.x, pair = (b >> 4) * 8 + (b & 7), h = (b >> 3) & 1;
    if (pair >= pairs) return;  // both members of a pair take this branch together
    __shared__ uint32_t duo_ok, duo_fail;
    uint64_t* tf0 = reinterpret_cast<uint64_t*>(smem);  // forward and inverse W0, W1 [4][H] (the compact half tables)
    uint64_t* tf1 = tf0 + H;
    uint64_t* ti0 = tf1 + H;
    uint64_t* ti1 = ti0 + H;
    uint64_t* bf = tf0 + 2 * N;              // forward buffer [2][H]
    uint64_t* bi = bf + N;                   // inverse buffer [2][H]
    uint64_t* dx = bi + N;                   // DIG = 2: digit 0's values for the other column's waves [2][H]
    uint64_t* mt = dx + (DIG > 1 ? N : 0);   // factor table: row e = (psi^e - 1, its W1) [2N][2]
    uint32_t* ex = reinterpret_cast<uint32_t*>(mt + 4 * N);  // rotation exponents [n]
    const uint32_t t = threadIdx.x, l = t & 63, w = t >> 6, twoN = 2 * N, logG = P.logG;
    const uint32_t j = __builtin_amdgcn_readfirstlane(w >> 2);  // this wave's polynomial / column
    const uint32_t u4 = 4 * (256 * h + 64 * (w & 3) + l);       // this lane's slots u4 .. u4+3 (whole ring)
    const uint32_t sp = j * H + 256 * (w & 3);                  // their buffer block
    const uint64_t Q = K.Q, Qhalf = P.Q >> 1;
    const int64_t Qs = (int64_t)P.Q, Bh = (int64_t)1 << (logG - 1);
    const uint32_t sh = 64 - logG;
    for (uint32_t k = t; k < H; k += TH) {  // compact entry k of half h: full index k + 2^(s-1) (1 + h)
        const uint32_t e = k == 0 ? 1 : k + (1u << (31 - __builtin_clz(k))) * (1 + h);
        tf0[k] = psi[e], tf1[k] = psi1[e], ti0[k] = ipsi[e], ti1[k] = ipsi1[e];
    }
    for (uint32_t k = t; k < twoN; k += TH) {
        mt[2 * sf_mrow(k)] = mono[k] % Q;  // psi^k - 1
        mt[2 * sf_mrow(k) + 1] = mono1[k];
    }
    const SfTw TF{tf0, tf1}, TI{ti0, ti1};
    uint64_t* g = acc_io + (size_t)pair * twoN;
    const uint64_t* ap = a + (size_t)pair * P.n;
    stage_rot_exponents<TH>(ex, ap, P.n, amod, twoN);
    const size_t round_words = (size_t)4 * P.dG2 * N;
    const uint32_t tau = t & 255, pp = t >> 8;  // pass-A role: coefficients tau + 256k of polynomial pp

    if (t == 0) duo_fail = 0;
    uint64_t acc[8];  // canonical [0, Q), all N coefficients of polynomial pp (both members)
    uint64_t* sv = X.save + (size_t)pair * twoN;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint64_t v = g[pp * N + tau + 256 * k];
        if (pp == h) sv[pp * N + tau + 256 * k] = v;  // the rescue's input if the pair times out
        acc[k] = sf_load_acc(v, Q);
    }
    __syncthreads();  // twiddles, factor table, exponents in LDS
    // the inverse's stage-0 twiddle, once (its load sat behind the hand-off of every round)
    const uint64_t iw0 = ti0[0], iw1 = ti1[0];

    const __amdgpu_buffer_rsrc_t rk0 = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint64_t*>(bsk), 0, -1, 0x00020000);
    const __amdgpu_buffer_rsrc_t rk1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint64_t*>(bsk1), 0, -1, 0x00020000);
    int64_t Kdl[DIG];  // sf2's closed-form digit offsets
#pragma unroll
    for (int d = 0; d < DIG; ++d) {
        int64_t Kd = 0;
        for (uint32_t z = 0; z < d + P.thr; ++z) Kd = (Kd << logG) + Bh;
        Kdl[d] = Kd;
    }
    uint32_t* myflag = X.flags + (pair * 2 + h) * 32;
    const uint32_t* peerflag = X.flags + (pair * 2 + (1 - h)) * 32;
    for (uint32_t i = 0; i < P.n; ++i) {
        const uint32_t ai = ex[i];
        const uint32_t round_off = i * (uint32_t)round_words * 8;  // bytes (< 2^32: checked at launch)
        // products of column j: group gi = (key kk, row rr): rr = 2d (own polynomial's digit d), 2d + 1 (the
        // other polynomial's); key row 2d + polynomial
        constexpr int RW = 2 * DIG, NG = 2 * RW;
        auto krow = [j](uint32_t rr) -> uint32_t { return (rr & ~1u) + ((rr & 1) ? 1 - j : j); };
        auto kload = [&](int gi, uint64_t (&kw)[8]) {
            const uint32_t kk = gi / RW, r = krow(gi % RW);
            const uint32_t o = round_off + ((kk * P.dG2 + r) * 2 + j) * N * 8;
            sf_key_group(rk0, rk1, u4, o, kw);
        };
        // SFD_KPRE key groups requested before the forward transform (a ring of SFD_KPRE + 1), as sf2duo
        constexpr int KD = SFD_KPRE > 0 ? SFD_KPRE : 1, KR = KD + 1 < NG ? KD + 1 : NG;
        uint64_t kw[KR][8];
#pragma unroll
        for (int gq = 0; gq < (SFD_KPRE > 0 ? KD : 0); ++gq) kload(gq, kw[gq]);
        uint64_t D[DIG][4];
#pragma unroll
        for (int d = 0; d < DIG; ++d) {
            const uint32_t shift = (d + P.thr) * logG;
            const int64_t Klo = Kdl[d], Khi = Kdl[d] - Qs;
            uint64_t v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                v[k] = (uint64_t)sf_digit(acc[k], Qhalf, Klo, Khi, shift, sh) + K.Qf;  // the offset-free forward's inputs
            }
            if (d > 0) __syncthreads();  // other waves may still read their blocks of digit d - 1
            sfd_fwd(bf, v, D[d], h, TF, K);
        }
        // this lane's digits for the other column's waves (each wave writes only its own block: bf the last
        // digit, dx digit 0 when DIG = 2)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            bf[sp + dswz(4 * l + s)] = D[DIG - 1][s];
            if constexpr (DIG > 1) dx[sp + dswz(4 * l + s)] = D[0][s];
        }
        __syncthreads();
        uint64_t Do[DIG][4];  // the other polynomial's digits at the same slots
        const uint32_t so = (1 - j) * H + 256 * (w & 3);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            Do[DIG - 1][s] = bf[so + dswz(4 * l + s)];
            if constexpr (DIG > 1) Do[0][s] = dx[so + dswz(4 * l + s)];
        }
        uint64_t A[2][4];
        if constexpr (SFD_KPRE == 0) kload(0, kw[0]);
#pragma unroll
        for (int gi = 0; gi < NG; ++gi) {
            if (gi + KD < NG) kload(gi + KD, kw[(gi + KD) % KR]);
            __builtin_amdgcn_sched_barrier(0);
            const int kk = gi / RW, rr = gi % RW;
            const uint64_t(&c)[8] = kw[gi % KR];
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const uint64_t dv = (rr & 1) ? Do[rr >> 1][s] : D[rr >> 1][s];
                const uint64_t prod = sf_mul(dv, c[s], c[4 + s], K.c2);
                A[kk][s] = rr == 0 ? prod : A[kk][s] + prod;
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        uint32_t uo = u4;
        asm volatile("" : "+v"(uo));
        uint64_t S[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {  // one table product per factor (row e holds psi^e - 1), as sf2p
            const uint32_t ip = ((2 * (__builtin_bitreverse32(uo + s) >> 21) + 1) * ai) & (twoN - 1);
            const uint64_t* fp = mt + 2 * sf_mrow(ip);
            const uint64_t* fm = mt + 2 * sf_mrow((twoN - ip) & (twoN - 1));
            S[s] = sf_fold(sf_mul(A[0][s], fp[0], fp[1], K.c2) + sf_mul(A[1][s], fm[0], fm[1], K.c2), K.c);
        }
        uint64_t o[4];
        sfd_inv(bi, S, o, h, TI, K);
        // hand-off: this half's stage-1 values of both columns to the partner (thread t's 4 at k' 512 + t)
        uint64_t* mine = X.xbuf + (((size_t)pair * 2 + h) * 2 + (i & 1)) * N;
        const uint64_t* theirs = X.xbuf + (((size_t)pair * 2 + (1 - h)) * 2 + (i & 1)) * N;
        // (measured against a data-tagged form -- the round's tag in each word's bits 58-63, per-thread polls, no flag
        // or barrier: a tie at 128 in C3's and C5b's contexts, profiles/r06o; the hand-off costs 1.8 us of a 7.6-us
        // round either way)
        uint64_t pv[4];
        {
            if constexpr (PROBE != 2) {
#pragma unroll
                for (int k = 0; k < 4; ++k) duo_store(mine + 512 * k + t, o[k]);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();  // every wave's stores drained; every read of the buffers done
            if (PROBE != 2 && t == 0) {  // the hand-off protocol: duo.hpp
                const bool gone = PROBE == 1 && pair == 0 && h == 1 && i >= 2;
                const bool ok = duo_publish_and_wait<PROBE != 0>(myflag, peerflag, i, X.wait_ticks, gone);
                duo_ok = ok;
                if (!ok) duo_fail = 1;
            }
            if constexpr (PROBE != 2) {
                __syncthreads();
                if (!duo_ok) break;  // uniform: the partner never arrived (the rescue launch recomputes the pair)
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) pv[k] = PROBE == 2 ? o[k] : duo_load(theirs + 512 * k + t);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {  // stage 0 for all coefficients (sf2's pass A end), then sf2's update
            const uint64_t lo = h ? pv[k] : o[k], hi = h ? o[k] : pv[k];
            const uint64_t r[2] = {lo + hi, sf_mul(lo + (K.Q10 - hi), iw0, iw1, K.c2)};  // < 18.1 Q
#pragma unroll
            for (int z = 0; z < 2; ++z) {
                acc[k + 4 * z] = sf_add_acc(acc[k + 4 * z], r[z], K);
            }
        }
    }
    __syncthreads();
    if (duo_fail && t == 0) duo_fail_pair(X, pair);  // this member timed out (the rescue launch recomputes the pair)
    // member h writes polynomial h (acc0 transposed, poly.cpp:762-770) through the forward buffer (N words)
    if (pp == h) {
#pragma unroll
        for (int k = 0; k < 8; ++k) bf[tau + 256 * k] = acc[k];
    }
    __syncthreads();
    for (uint32_t k = t; k < N; k += TH) {
        if (h == 0) {
            const uint64_t v = bf[k == 0 ? 0 : N - k];
            g[k] = k == 0 ? v : (v == 0 ? 0 : Q - v);
        } else {
            g[N + k] = bf[k];
        }
    }
}

// W1 = w 2^32 mod Q for w < Q: w 2^32 = (w >> 22) 2^54 + (w mod 2^22) 2^32  (< 2^54 + 2^32 c < 2Q)
__global__ void k_pack_sf(uint64_t Q, uint32_t c, const uint64_t* __restrict__ in, size_t words,
                          uint64_t* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= words) return;
    const uint64_t w = in[i] % Q;
    const uint64_t x = ((w & ((1ull << (SF_K - 32)) - 1)) << 32) + (w >> (SF_K - 32)) * c;
    out[i] = x >= Q ? x - Q : x;
}

}  // namespace

bool sf_path_supported(const BRParams& P, int word_bits) {
    return word_bits == 64 && P.N == G3_N && P.Q < (1ull << SF_K) && P.Q > (1ull << SF_K) - (1ull << 20) &&
           P.logG < 64 && P.n > 0;
}

// W1 arrays behind the arena's W0 ones: psi [N], ipsi [N], mono [2N], bsk [n][2][dG2][2][N]
size_t sf_bytes(const BRParams& P) { return ((size_t)4 * P.N + (size_t)P.n * 4 * P.dG2 * P.N) * 8; }

hipError_t launch_pack_sf(const BRParams& P, const DevTables& T, const void* bsk, void* out, hipStream_t s) {
    if (!sf_path_supported(P, 64)) return hipErrorNotSupported;
    const uint32_t c = (uint32_t)((1ull << SF_K) - P.Q);
    uint64_t* o = (uint64_t*)out;
    const size_t words = (size_t)P.n * 4 * P.dG2 * P.N;
    struct Part { const void* src; size_t n; size_t off; } parts[] = {
        {T.psi, P.N, 0}, {T.ipsi, P.N, P.N}, {T.mono, 2ull * P.N, 2ull * P.N}, {bsk, words, 4ull * P.N}};
    for (const Part& q : parts)
        hipLaunchKernelGGL(k_pack_sf, dim3((unsigned)((q.n + 255) / 256)), dim3(256), 0, s, (uint64_t)P.Q, c,
                           (const uint64_t*)q.src, q.n, o + q.off);
    return hipGetLastError();
}

static_assert(G3_N == kDuoN, "the duo buffer holds N = 2048 polynomials");

namespace {
// the kernels' constants for Q = 2^54 - c (the launcher's and the test library's arithmetic probes')
SfC make_sf_const(uint64_t Q) {
    SfC K;
    K.Q = Q, K.Q3 = 3 * Q, K.Qf = 28 * Q, K.Q10 = 10 * Q;
    K.c = (uint32_t)((1ull << SF_K) - Q);
    K.c2 = 2 * K.c;
    return K;
}
}  // namespace

hipError_t launch_blind_rotate_sf(const BRParams& P, const DevTables& T, const void* bsk, const void* sf,
                                  const uint64_t* a, uint64_t amod, uint64_t* acc, size_t B, hipStream_t s,
                                  const Knobs& kn, DuoDev* duo) {
    if (B == 0) return hipSuccess;
    if (!sf_path_supported(P, 64)) return hipErrorNotSupported;
    const SfC K = make_sf_const(P.Q);
    const uint64_t* w1 = (const uint64_t*)sf;
    const size_t lds = ((size_t)4 * G3_N + SF_MT) * 8 + rot_exponent_bytes(P.n);  // two polynomials, forward twiddles, monomial tables, a'_i
    const bool no_sf2 = !kn.sf2;  // gen3sf (cross-check)
    // sf2 addresses the keys with 32-bit byte offsets (buffer resources)
    const bool fits32 = (uint64_t)P.n * 4 * P.dG2 * P.N * 8 < (1ull << 32);
    if (!no_sf2 && fits32 && P.digits >= 1 && P.digits <= 3) {
        auto go = [&](auto kern) {
            (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            hipLaunchKernelGGL(kern, dim3((unsigned)B), dim3(G3_TH), lds, s, P, K, (const uint64_t*)T.psi, w1,
                               (const uint64_t*)T.ipsi, w1 + P.N, (const uint64_t*)T.mono, w1 + 2 * P.N,
                               (const uint64_t*)bsk, w1 + 4 * P.N, a, amod, acc, (const uint32_t*)nullptr,
                               (const uint64_t*)nullptr);
        };
        if ((P.digits == 1 || P.digits == 2) && duo && B <= (size_t)kn.duo && B <= duo->resident_pairs &&
            B <= kDuoMaxPairs) {
            const DuoBuf X = duo_layout(*duo);
            // sfduo<DIG> (split by NTT half).  Two digits: sf2duo (split by accumulator polynomial, rounds 4-5) measured
            // 1.5-2.4 % slower at C5b's 128 (profiles/r06m, two alternations on one box), kept as the test
            // library's A/B form (probe 13)
            auto dk = P.digits == 1 ? k_blind_rotate_sfduo<1> : k_blind_rotate_sfduo<2>;
            size_t ldsd = (size_t)(P.digits == 1 ? 8 : 9) * G3_N * 8 + rot_exponent_bytes(P.n);
#ifdef TFHE_TEST_PROBES
            if (kn.probe == 5) dk = P.digits == 1 ? k_blind_rotate_sfduo<1, 1> : k_blind_rotate_sfduo<2, 1>;  // a partner that never arrives
            if (kn.probe == 7) dk = P.digits == 1 ? k_blind_rotate_sfduo<1, 2> : k_blind_rotate_sfduo<2, 2>;  // timing only: no hand-off
            if (kn.probe == 13 && P.digits == 2) {  // the polynomial split (A/B)
                dk = k_blind_rotate_sf2duo<0>;
                ldsd = ((size_t)4 * G3_N + SF2D_MT) * 8 + rot_exponent_bytes(P.n);
            }
#endif
            (void)hipFuncSetAttribute((const void*)dk, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsd);
            // the rescue: one-workgroup sf2 for the ciphertexts of timed-out pairs, from their saved inputs
            // (every other workgroup reads one word and exits: a few microseconds per launch)
            auto rk = P.digits == 1 ? k_blind_rotate_sf2<1, true> : k_blind_rotate_sf2<2, true>;
            (void)hipFuncSetAttribute((const void*)rk, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            return duo_serialised(*duo, s, [&]() -> hipError_t {
                if (hipError_t e = hipMemsetAsync(X.flags, 0, (size_t)B * 2 * 128, s); e != hipSuccess) return e;
                hipLaunchKernelGGL(dk, dim3((unsigned)(16 * ((B + 7) / 8))), dim3(G3_TH), ldsd, s, P, K,
                                   (const uint64_t*)T.psi, w1, (const uint64_t*)T.ipsi, w1 + P.N, (const uint64_t*)T.mono,
                                   w1 + 2 * P.N, (const uint64_t*)bsk, w1 + 4 * P.N, a, amod, acc, X, (uint32_t)B);
                if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
                hipLaunchKernelGGL(rk, dim3((unsigned)B), dim3(G3_TH), lds, s, P, K, (const uint64_t*)T.psi, w1,
                                   (const uint64_t*)T.ipsi, w1 + P.N, (const uint64_t*)T.mono, w1 + 2 * P.N,
                                   (const uint64_t*)bsk, w1 + 4 * P.N, a, amod, acc, (const uint32_t*)X.flags,
                                   (const uint64_t*)X.save);
                return hipGetLastError();
            });
        }
        // two ciphertexts per workgroup, the monomial table in LDS: two digits only (same box, three reps,
        // profiles/r04m: C5b 70.8 -> 67.7 ms per launch; one digit went the other way, 172.3 -> 178.0 ms,
        // the forward twiddles now read from memory costing more than the table saves)
        // (from 512 ciphertexts: 256 pair workgroups fill the 256 CUs; below, sf2's one-ciphertext
        // workgroups spread over twice the CUs)
        if (P.digits == 2 && kn.sf2p && B >= 512) {
            const size_t ldsp = (size_t)8 * G3_N * 8 + 2 * rot_exponent_bytes(P.n);
            if (ldsp <= 160 * 1024) {
                auto kern = k_blind_rotate_sf2p<2>;
#ifdef TFHE_TEST_PROBES
                if (kn.probe == 12) kern = k_blind_rotate_sf2p<2, 1>;  // timing only: broadcast factor rows
#endif
                (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsp);
                hipLaunchKernelGGL(kern, dim3((unsigned)((B + 1) / 2)), dim3(2 * G3_TH), ldsp, s, P, K,
                                   (const uint64_t*)T.psi, w1, (const uint64_t*)T.ipsi, w1 + P.N,
                                   (const uint64_t*)T.mono, w1 + 2 * P.N, (const uint64_t*)bsk, w1 + 4 * P.N, a, amod,
                                   acc, (uint32_t)B);
                return hipGetLastError();
            }
        }
        if (P.digits == 3) go(k_blind_rotate_sf2<3>);  // (CHES-experiments.cpp's EvalFunc context, baseG 2^18)
        else if (P.digits == 2) go(k_blind_rotate_sf2<2>);
        else go(k_blind_rotate_sf2<1>);
        return hipGetLastError();
    }
    (void)hipFuncSetAttribute((const void*)k_blind_rotate_gen3sf, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(k_blind_rotate_gen3sf, dim3((unsigned)B), dim3(G3_TH), lds, s, P, K, (const uint64_t*)T.psi, w1,
                       (const uint64_t*)T.ipsi, w1 + P.N, (const uint64_t*)T.mono, w1 + 2 * P.N, T.eidx,
                       (const uint64_t*)bsk, w1 + 4 * P.N, a, amod, acc);
    return hipGetLastError();
}

}  // namespace tfhe

#ifdef TFHE_TEST_PROBES
// ---- arithmetic probes (test library only; arith_probes.hpp, tests/test_gpu_arith_units.py) ----
// op: 0 sf_mul(a, w0, w1)  1 sf_fold(x)  2 / 3 sf_ct<OFS = 0 / 1>(x, y, tab[i])  4 / 5 sf_gs<FOLD = 0 / 1>(x, y, tab[i])
//     6 sf_add_acc(a, inc)  7 sf_digit(x, Qhalf, Klo, Khi, shift, sh)  8 sf_load_acc(v)
//     9 / 10 sf_fwd_core<OFS = 0 / 1>(v[8], m0, g)  11 / 12 sf_inv_core<FOLD = 0 / 1>(v[8], m, g)
// 10 words in, 8 out per case; tab = W0[T] then W1[T]
#include "arith_probes.hpp"

namespace tfhe {
namespace {
constexpr int SFP_NI = 10, SFP_NO = 8;
__global__ void k_arith_sf(int op, size_t cases, const uint64_t* __restrict__ in, const uint64_t* __restrict__ tab,
                           size_t tab_words, uint64_t* __restrict__ out, SfC K) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (!probe_lane_runs(op, i, cases)) return;
    const uint64_t* x = in + i * SFP_NI;
    uint64_t* o = out + i * SFP_NO;
    const size_t T = tab_words / 2;
    const SfTw W{tab, tab + T};
    const int f = op & 15;
    if (f == 0) o[0] = sf_mul(x[0], x[1], x[2], K.c2);
    else if (f == 1) o[0] = sf_fold(x[0], K.c);
    else if (f >= 2 && f <= 5) {
        if (x[2] >= T) return;
        uint64_t a = x[0], b = x[1];
        const uint32_t j = (uint32_t)x[2];
        if (f == 2) sf_ct<false>(a, b, W, j, K);
        else if (f == 3) sf_ct<true>(a, b, W, j, K);
        else if (f == 4) sf_gs<false>(a, b, W, j, K);
        else sf_gs<true>(a, b, W, j, K);
        o[0] = a, o[1] = b;
    } else if (f == 6) o[0] = sf_add_acc(x[0], x[1], K);
    else if (f == 7) o[0] = (uint64_t)sf_digit(x[0], x[1], (int64_t)x[2], (int64_t)x[3], (uint32_t)x[4], (uint32_t)x[5]);
    else if (f == 8) o[0] = sf_load_acc(x[0], K.Q);
    else if (f >= 9 && f <= 12) {
        uint64_t v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = x[k];
        const uint64_t m = x[8], g = x[9];
        if (m >= T || g >= T) return;
        if (f <= 10) {
            if (4 * m + 4 * g + 3 >= T) return;
            if (f == 9) sf_fwd_core<false>(v, (uint32_t)m, (uint32_t)g, W, K);
            else sf_fwd_core<true>(v, (uint32_t)m, (uint32_t)g, W, K);
        } else {
            if (m + 4 * g + 3 >= T) return;
            if (f == 11) sf_inv_core<false>(v, (uint32_t)m, (uint32_t)g, W, K);
            else sf_inv_core<true>(v, (uint32_t)m, (uint32_t)g, W, K);
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = v[k];
    }
}
}  // namespace
}  // namespace tfhe

extern "C" TFHE_ARITH_PROBE(sf) {
    if ((op & 15) > 12 || Q >= (1ull << tfhe::SF_K) || Q <= (1ull << tfhe::SF_K) - (1ull << 20)) return -1;
    return tfhe::probe_launch(tfhe::k_arith_sf, tfhe::SFP_NI, tfhe::SFP_NO, op, cases, in, in_words, tab, tab_words, out,
                              out_words, tfhe::make_sf_const(Q));
}
#endif  // TFHE_TEST_PROBES
