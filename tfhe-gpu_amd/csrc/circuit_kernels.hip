// circuit_kernels.hip -- the two kernels of the circuit path (engine.hip dev_circuit) around the
// shared blind rotation / extraction / key switch:
//   * k_circuit_prep: one launch per level.  One workgroup per (gate, instance) reads the gate's
//     16-byte plan record, gathers both operands by wire index from the input array or the wire
//     store (negate flag: EvalNOT, binfhe-base-scheme.cpp:147-159; constant: NoiselessEmbedding,
//     lwe-pke.cpp:326-338), forms in0 + in1 -- 2 (in0 - in1) for the FAST gates
//     (binfhe-base-scheme.cpp:642-655) -- and writes the mask to a_out and the accumulator
//     (acc0 = 0, acc1 = the gate's own test vector, binfhe-base-scheme.cpp:1110-1138) to acc.  It
//     replaces launch_lwe_op + launch_build_testvector of dev_gate: the prepared ciphertext is
//     never stored.
//   * k_circuit_out: gathers the output wires into the caller's array.
// k_circuit_prep writes 16 N bytes of accumulator per bootstrap and reads 2 (n+1) words: it is
// store-bound, so each thread writes 16-byte pairs; the record's address depends on blockIdx alone, so
// it is one scalar load per wavefront.
#include "circuit.hpp"
#include "device_math.hpp"
#include "kernels.hpp"

namespace tfhe {

namespace {

// word k (k == n: b) of an operand row under its kind / negate flag, mod q
__device__ __forceinline__ uint64_t circuit_word(uint32_t kind, bool neg, uint32_t cval, const uint64_t* __restrict__ row,
                                                 uint32_t k, bool isb, uint64_t q) {
    if (kind == CK_CONST) return isb ? cval * (q >> 2) : 0;
    const uint64_t v = row[k];
    if (!neg) return v;
    return isb ? subm<uint64_t>(q >> 2, v, q) : (v == 0 ? 0 : q - v);
}

__device__ __forceinline__ const uint64_t* circuit_row(uint32_t kind, uint32_t idx, size_t inst, const CircuitPrep& P,
                                                       const uint64_t* __restrict__ in, const uint64_t* __restrict__ store) {
    const uint64_t* base = kind == CK_SLOT ? store : in;  // CK_CONST: never dereferenced
    return base + ((size_t)idx * P.instances + inst) * (P.n + 1);
}

__device__ __forceinline__ uint64_t circuit_combine(bool fast, uint64_t x, uint64_t y, uint64_t q) {
    if (!fast) return addm<uint64_t>(x, y, q);
    const uint64_t d = subm<uint64_t>(x, y, q);
    return addm<uint64_t>(d, d, q);
}

}  // namespace

__global__ void __launch_bounds__(256)
k_circuit_prep(CircuitPrep P, const CircuitRec* __restrict__ recs, const uint64_t* __restrict__ in,
               const uint64_t* __restrict__ store, uint64_t* __restrict__ acc, uint64_t* __restrict__ a_out) {
    // bootstrap `flat` of the level: gate flat / instances, instance flat % instances
    const size_t flat = P.first + blockIdx.x;
    const size_t g = flat / P.instances, inst = flat - g * P.instances;
    const CircuitRec r = recs[g];
    const uint32_t op = r.ctl & 7, k0 = r.ctl >> 4 & 3, k1 = r.ctl >> 8 & 3;
    const bool n0 = r.ctl >> 6 & 1, n1 = r.ctl >> 10 & 1;
    const bool fast = op == TFHE_XOR_FAST || op == TFHE_XNOR_FAST;
    const uint32_t N = P.N, n = P.n;
    const uint64_t q = P.q;
    const uint64_t* x = circuit_row(k0, r.i0, inst, P, in, store);
    const uint64_t* y = circuit_row(k1, r.i1, inst, P, in, store);

    uint64_t* ao = a_out + (size_t)blockIdx.x * n;
    for (uint32_t k = threadIdx.x; k < n; k += blockDim.x)
        ao[k] = circuit_combine(fast, circuit_word(k0, n0, r.i0, x, k, false, q), circuit_word(k1, n1, r.i1, y, k, false, q), q);

    // the gate's range [q1, q2) (rgsw-cryptoparameters.h:130-137; engine.hip gate_const)
    const uint64_t b = circuit_combine(fast, circuit_word(k0, n0, r.i0, x, n, true, q), circuit_word(k1, n1, r.i1, y, n, true, q), q) % q;
    const uint32_t mult = op == TFHE_OR || op == TFHE_XOR_FAST ? 5 : op == TFHE_AND ? 7 : op == TFHE_NAND ? 3 : 1;
    const uint64_t q1 = mult * (q >> 3), q2 = addm<uint64_t>(q1, q >> 1, q);
    const uint64_t in_v = q1 < q2 ? P.Q - P.Q8 : P.Q8, out_v = q1 < q2 ? P.Q8 : P.Q - P.Q8;
    const uint64_t lo = q1 < q2 ? q1 : q2, hi = q1 < q2 ? q2 : q1;
    const uint32_t factor = (uint32_t)(2ull * N / q);
    auto tv = [&](uint32_t k) -> uint64_t {  // acc1[k]: k_build_testvector's TV_GATE value
        if (k % factor) return 0;
        const uint64_t j = k / factor;
        if (j >= (q >> 1)) return 0;
        const uint64_t v = b >= j ? b - j : b + (q - j);
        return v >= lo && v < hi ? in_v : out_v;
    };
    ulonglong2* a0 = reinterpret_cast<ulonglong2*>(acc + (size_t)blockIdx.x * 2 * N);
    ulonglong2* a1 = a0 + N / 2;
    for (uint32_t p = threadIdx.x; p < N / 2; p += blockDim.x) {
        a0[p] = make_ulonglong2(0, 0);
        a1[p] = make_ulonglong2(tv(2 * p), tv(2 * p + 1));
    }
}

hipError_t launch_circuit_prep(const CircuitPrep& P, const CircuitRec* recs, const uint64_t* in, const uint64_t* store,
                               uint64_t* acc, uint64_t* a_out, size_t B, hipStream_t s) {
    if (B == 0) return hipSuccess;
    if (P.N < 2 || (P.N & 1) || P.q == 0 || (2ull * P.N) % P.q || P.instances == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_circuit_prep, dim3((unsigned)B), dim3(256), 0, s, P, recs, in, store, acc, a_out);
    return hipGetLastError();
}

__global__ void __launch_bounds__(256)
k_circuit_out(CircuitPrep P, const CircuitOut* __restrict__ outs, const uint64_t* __restrict__ in,
              const uint64_t* __restrict__ store, uint64_t* __restrict__ out) {
    const size_t flat = P.first + blockIdx.x;  // output flat / instances, instance flat % instances
    const size_t o = flat / P.instances, inst = flat - o * P.instances;
    const CircuitOut r = outs[o];
    const uint32_t kind = r.ctl & 3, n = P.n;
    const bool neg = r.ctl >> 2 & 1;
    const uint64_t* x = circuit_row(kind, r.idx, inst, P, in, store);
    uint64_t* dst = out + flat * (n + 1);
    for (uint32_t k = threadIdx.x; k <= n; k += blockDim.x) dst[k] = circuit_word(kind, neg, r.idx, x, k, k == n, P.q);
}

hipError_t launch_circuit_out(const CircuitPrep& P, const CircuitOut* outs, const uint64_t* in, const uint64_t* store,
                              uint64_t* out, size_t B, hipStream_t s) {
    if (B == 0) return hipSuccess;
    if (P.q == 0 || P.instances == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_circuit_out, dim3((unsigned)B), dim3(256), 0, s, P, outs, in, store, out);
    return hipGetLastError();
}

}  // namespace tfhe
