/*
 * tfhe_hip.h -- C-ABI of the MI355X-native batched CGGI/GINX bootstrapping engine.
 *
 * This is the drop-in boundary.  The reference (eric070021/TFHE-GPU) exposes its
 * GPU path as seven C++ static members that OpenFHE's unchanged BinFHE code calls
 * (SURVEY.md 8(b)).  Each of those maps onto one entry point here; the OpenFHE
 * side binding (the shim that defines those seven C++ symbols over this ABI, translating
 * NativeVector / NativePoly <-> u64 rows) is tfhe-gpu_amd/shim/bootstrapping_hip.cpp;
 * INTEGRATION.md describes how a maintainer links it into src/binfhe.
 *
 *   reference symbol                                        entry point
 *   GPUFFTBootstrap::GPUSetup       bootstrapping.cuh:111   tfhe_setup_eval (OpenFHE EVALUATION-format BSK) or tfhe_setup
 *   GPUFFTBootstrap::GPUClean       bootstrapping.cuh:116   tfhe_clean
 *   GPUFFTBootstrap::EvalAcc_CUDA   bootstrapping.cuh:126   tfhe_eval_acc
 *   GPUFFTBootstrap::MKMSwitch_CUDA bootstrapping.cuh:135   tfhe_mkm_switch
 *   GPULWEOperation::CiphertextMulMatrix_CUDA lwe-operation.cuh:49  tfhe_ciphertext_mul_matrix
 *   GPULWEOperation::GPUSetup       lwe-operation.cuh:57    tfhe_lwe_gpu_setup
 *   GPULWEOperation::GPUClean       lwe-operation.cuh:62    tfhe_lwe_gpu_clean
 *
 * Above those, the vector BinFHEContext surface (binfhecontext.cpp:316-347 ->
 * binfhe-base-scheme.cpp:598-1085) is offered as fused entry points that keep
 * every chained bootstrap on the device: tfhe_eval_bin_gate, tfhe_eval_func,
 * tfhe_eval_floor, tfhe_eval_sign, tfhe_eval_decomp.
 *
 * Conventions
 *  - All integers are u64, little-endian, flat row-major arrays in HOST memory
 *    unless the name ends in _device (then device pointers, ordered on the given
 *    hipStream_t passed as void*; the call runs on the context's device that
 *    holds the output buffer, found with hipPointerGetAttributes).
 *  - LWE ciphertext: [n+1] words, a[0..n-1] then b.
 *  - RLWE accumulator: [2][N] words, coefficient form.
 *  - BSK (coefficient form): [n][2][dG2][2][N]: LWE index i, ternary key
 *    (0: s_i=+1, 1: s_i=-1; rgsw-acc-cggi.cpp:53-77), gadget row (poly + 2*digit,
 *    rgsw-acc-cggi.cpp:229-238), RLWE poly, coefficient.  The reference keeps the
 *    RingGSWACCKey in EVALUATION form for OpenFHE's own NTT; the shim converts
 *    it with SetFormat(COEFFICIENT) exactly as the reference's KeyCopy_FFT does
 *    (bootstrapping.cu:1112-1137).
 *  - KSK: [N][baseKS][dKS][n+1], B stored at index n (the reference's device
 *    layout, bootstrapping.cu:961-975).
 *  - Errors: every call returns tfhe_status; tfhe_last_error() gives a message.
 *    The reference exit()s on device faults (bootstrapping.cu:28-37); here the
 *    caller decides (the shim converts to OPENFHE_THROW).
 *  - Not re-entrant per context (like the reference's static state); separate
 *    contexts are independent.
 */
#ifndef TFHE_HIP_H
#define TFHE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TFHE_HIP_ABI_VERSION 8  /* 2: tfhe_info.br_kernel; 3: tfhe_info.replicate_*, tfhe_eval_acc_tv, sharding;
                                   4: row-pointer host arrays (tfhe_eval_acc_tv_rows, tfhe_mkm_switch_rows);
                                   5: device-resident EvalFunc / EvalFloor / EvalSign; tfhe_knobs;
                                   6: tfhe_knobs.duo / .sf2p, tfhe_info.duo_timeouts (two-workgroup and
                                      two-ciphertext sf2 forms);
                                   7: tfhe_knobs.split4 (two-group STD128 form); the duo forms cover
                                      STD128Q (f64wduo) and timed-out pairs are recomputed;
                                   8: tfhe_knobs.ks40 (split-word key-switch records for 8-byte keys);
                                      tfhe_rccl_selftest; the duo form covers the STD192 classes */

typedef enum tfhe_status {
    TFHE_OK = 0,
    TFHE_ERR_INVALID_ARGUMENT = 1,
    TFHE_ERR_UNSUPPORTED = 2,
    TFHE_ERR_NOT_SET_UP = 3,
    TFHE_ERR_DEVICE = 4,
    TFHE_ERR_OUT_OF_MEMORY = 5,
    TFHE_ERR_INTERNAL = 6
} tfhe_status;

/* BINFHE_PARAMSET (binfhe-constants.h:46-90) */
typedef enum tfhe_paramset {
    TFHE_TOY = 0, TFHE_MEDIUM, TFHE_STD128_AP, TFHE_STD128_APOPT, TFHE_STD128, TFHE_STD128_OPT, TFHE_STD192,
    TFHE_STD192_OPT, TFHE_STD256, TFHE_STD256_OPT, TFHE_STD128Q, TFHE_STD128Q_OPT, TFHE_STD192Q,
    TFHE_STD192Q_OPT, TFHE_STD256Q, TFHE_STD256Q_OPT, TFHE_SIGNED_MOD_TEST
} tfhe_paramset;

/* BINGATE (binfhe-constants.h:101) */
typedef enum tfhe_gate {
    TFHE_OR = 0, TFHE_AND, TFHE_NOR, TFHE_NAND, TFHE_XOR_FAST, TFHE_XNOR_FAST, TFHE_XOR, TFHE_XNOR
} tfhe_gate;

/* Flat parameter record (the reference's params_CUDA[10], bootstrapping.cu:917-929,
 * plus the gadget base).  digitsG, dKS and dG2 are derived by tfhe_params_finish. */
typedef struct tfhe_params {
    uint32_t n;                /* LWE dimension */
    uint32_t N;                /* ring dimension (power of two) */
    uint64_t q;                /* LWE modulus */
    uint64_t Q;                /* RLWE modulus, prime, Q = 1 mod 2N */
    uint64_t qKS;              /* key-switching modulus */
    uint32_t baseKS;           /* key-switching base */
    uint32_t baseG;            /* gadget base, power of two */
    uint32_t numDigitsToThrow; /* approximate gadget decomposition */
    uint32_t digitsG;          /* ceil(log Q / log baseG)           (derived) */
    uint32_t dKS;              /* ceil(log qKS / log baseKS)        (derived) */
    uint32_t dG2;              /* 2*(digitsG - numDigitsToThrow)    (derived) */
} tfhe_params;

typedef struct tfhe_info {
    int num_devices;           /* devices the context shards over */
    int word_bits;             /* 32: Q fits the u32 Shoup path; 64 otherwise */
    uint64_t bsk_device_bytes; /* per device */
    uint64_t ksk_device_bytes; /* per device */
    uint64_t bootstraps;       /* blind rotations executed since setup */
    uint64_t key_image_bytes;  /* size of the exportable device key image */
    int br_kernel;             /* blind rotation for power-of-two a-moduli: TFHE_BR_* */
    int replicate_method;      /* how setup replicated the key image to devices 1..: TFHE_REPLICATE_* */
    double replicate_ms;       /* wall time of that replication (0 for one device) */
    uint32_t duo_timeouts;     /* workgroups of the two-workgroup forms (sfduo: one- and two-digit special-form
                                  contexts; f64wduo: STD128Q and STD192 classes) that timed out waiting for their partner
                                  (10 ms of wall clock in one round) since setup, summed over devices
                                  (synchronises them); the ciphertexts of such a pair are recomputed from
                                  their saved inputs by the one-workgroup kernel (sf2 / f64w) queued behind
                                  the same launch, so outputs stay exact */
} tfhe_info;

/* tfhe_info.replicate_method */
#define TFHE_REPLICATE_NONE 0  /* one device */
#define TFHE_REPLICATE_RCCL 1  /* one RCCL broadcast from device 0 over xGMI (librccl, loaded at setup) */
#define TFHE_REPLICATE_PEER 2  /* concurrent peer copies from device 0 (no RCCL, or TFHE_REPLICATE=peer) */

/* tfhe_info.br_kernel */
#define TFHE_BR_GENERIC 0      /* generic v2 (or v1) Shoup kernel, blind_rotate_generic.hip */
#define TFHE_BR_FAST 1         /* specialised STD128 kernel, blind_rotate_fast4.hip */
#define TFHE_BR_F64 2          /* exact-FP64 kernel, blind_rotate_f64.hip */
#define TFHE_BR_F64_FOLD 3     /* exact-FP64 kernel, top digit's transforms eliminated */
#define TFHE_BR_RNS 4          /* (retired in round 3: the four-prime RNS kernel; never returned) */
#define TFHE_BR_SF 5           /* special-form u64 kernel (Q = 2^54 - c), blind_rotate_sf.hip sf2 / gen3sf */

typedef struct tfhe_ctx tfhe_ctx;

/* ---- parameters (binfhecontext.cpp:42-181) ---- */
tfhe_status tfhe_params_from_set(int paramset, tfhe_params* out);
tfhe_status tfhe_params_from_logq(int paramset, int arb_func, uint32_t logQ, int64_t N, uint32_t baseG,
                                  uint32_t num_digits_to_throw, tfhe_params* out);
tfhe_status tfhe_params_finish(tfhe_params* p);

/* ---- reference boundary ----
 * num_gpus as GPUSetup(numGPUs) (bootstrapping.cu:736-739): <= 0 or more than visible = every visible
 * device; batches are cut into one contiguous shard per device. */
tfhe_status tfhe_setup(tfhe_ctx** out, const tfhe_params* p, const uint64_t* bsk_coeff, const uint64_t* ksk,
                       int num_gpus);
/* Same, with the BSK exactly as OpenFHE holds it after KeyGen / BTKeyLoad: EVALUATION
 * format, (*BSkey)[0][key][i][l][m].GetValues() in [n][2][dG2][2][N] order (rgsw-acc-cggi.cpp:231-236).
 * Replaces the host INTT the reference runs in GPUSetup_core (bootstrapping.cu:874-1083)
 * and the shim's SetFormat(COEFFICIENT): the library's NTT uses OpenFHE's root
 * (RootOfUnity(2N, Q), rgsw-cryptoparameters.h:80, nbtheory.cpp:284-343) and transform
 * (transformnat-impl.h:196-236, 684-706), so the values are taken as they are.  Entries
 * must be < Q (TFHE_ERR_INVALID_ARGUMENT otherwise). */
tfhe_status tfhe_setup_eval(tfhe_ctx** out, const tfhe_params* p, const uint64_t* bsk_eval, const uint64_t* ksk,
                            int num_gpus);
tfhe_status tfhe_clean(tfhe_ctx* ctx);
/* a[B][n] mod a_mod; acc[B][2][N] coefficient in/out; acc0 returned transposed
 * (the callers rely on it: binfhe-base-scheme.cpp:665-671, 1203-1204). */
tfhe_status tfhe_eval_acc(tfhe_ctx* ctx, size_t B, const uint64_t* a, uint64_t a_mod, uint64_t* acc);
/* EvalAcc_CUDA for the accumulators the vector callers build (BootstrapGateCore / BootstrapFuncCore,
 * binfhe-base-scheme.cpp:1110-1138, 1163-1185): acc0 = 0 and acc1 zero except at multiples of
 * N / tv_len, whose values are tv[B][tv_len] (tv_len = a_mod / 2 there).  Same output as tfhe_eval_acc
 * on the expanded accumulators, with tv_len instead of 2N words per ciphertext sent to the device
 * (the drop-in shim detects the shape, tfhe-gpu_amd/shim/bootstrapping_hip.cpp). */
tfhe_status tfhe_eval_acc_tv(tfhe_ctx* ctx, size_t B, const uint64_t* a, uint64_t a_mod, const uint64_t* tv,
                             uint32_t tv_len, uint64_t* acc);
/* ct_ext[B][N+1] mod Q -> out[B][n+1] mod fmod: ModSwitch(qKS), KeySwitch, ModSwitch(fmod) */
tfhe_status tfhe_mkm_switch(tfhe_ctx* ctx, size_t B, const uint64_t* ct_ext, uint64_t fmod, uint64_t* out);
/* Row-pointer forms of the two calls above, for callers whose ciphertexts live in separate
 * allocations (OpenFHE: one NativeVector per polynomial and per LWE "a", which the drop-in shim
 * passes as pointers to their u64 storage): the pinned PCIe staging reads and writes the rows where
 * they are, so no flat copy of the arrays exists on either side.  Same results as the flat calls.
 *   tfhe_eval_acc_tv_rows: a_rows[s] -> n words; tv[B][tv_len] flat; acc_rows[2s + j] -> polynomial
 *                          j (N words) of accumulator s (written, acc0 transposed)
 *   tfhe_mkm_switch_rows:  ext_a_rows[s] -> N words, ext_b[s]; out_a_rows[s] -> n words, out_b[s] */
tfhe_status tfhe_eval_acc_tv_rows(tfhe_ctx* ctx, size_t B, const uint64_t* const* a_rows, uint64_t a_mod,
                                  const uint64_t* tv, uint32_t tv_len, uint64_t* const* acc_rows);
tfhe_status tfhe_mkm_switch_rows(tfhe_ctx* ctx, size_t B, const uint64_t* const* ext_a_rows, const uint64_t* ext_b,
                                 uint64_t fmod, uint64_t* const* out_a_rows, uint64_t* out_b);
/* out[c] = sum_k matrix[k][c] * ct[k] mod modulus, c < cols: ct[K][n+1], matrix[K][cols], out[cols][n+1]
 * (host arrays, device 0; tfhe_ciphertext_mul_matrix_device below with instances = 1) */
tfhe_status tfhe_ciphertext_mul_matrix(tfhe_ctx* ctx, size_t K, const uint64_t* ct, size_t cols, const int64_t* matrix,
                                       uint64_t modulus, uint64_t* out);
tfhe_status tfhe_lwe_gpu_setup(int num_gpus);
tfhe_status tfhe_lwe_gpu_clean(void);

/* ---- vector BinFHEContext surface, bootstraps chained on device ---- */
tfhe_status tfhe_eval_bin_gate(tfhe_ctx* ctx, int gate, size_t B, const uint64_t* ct1, const uint64_t* ct2, uint64_t q,
                               uint64_t* out);
/* lut: [q] shared (per_ct_lut = 0) or [B][q] (per_ct_lut = 1); out mod q */
tfhe_status tfhe_eval_func(tfhe_ctx* ctx, size_t B, const uint64_t* ct, uint64_t q, const uint64_t* lut, int per_ct_lut,
                           uint64_t* out);
tfhe_status tfhe_eval_floor(tfhe_ctx* ctx, size_t B, const uint64_t* ct, uint64_t mod, uint32_t roundbits,
                            uint64_t* out);
/* ct mod `mod`; out mod q (the LWE modulus) */
tfhe_status tfhe_eval_sign(tfhe_ctx* ctx, size_t B, const uint64_t* ct, uint64_t mod, uint64_t* out);
/* out[B][max_digits][n+1]; moduli[max_digits]; *num_digits set */
tfhe_status tfhe_eval_decomp(tfhe_ctx* ctx, size_t B, const uint64_t* ct, uint64_t mod, uint32_t max_digits,
                             uint64_t* out, uint64_t* moduli, uint32_t* num_digits);

/* ---- device-resident variants (inputs/outputs already in HBM) ----
 * The device is the one holding d_out / d_acc (a multi-device context runs the
 * call on that device's key arena; the stream must belong to it).  A buffer on
 * a device the context does not use is TFHE_ERR_INVALID_ARGUMENT. */
tfhe_status tfhe_eval_bin_gate_device(tfhe_ctx* ctx, int gate, size_t B, const uint64_t* d_ct1,
                                      const uint64_t* d_ct2, uint64_t q, uint64_t* d_out, void* stream);
tfhe_status tfhe_eval_acc_device(tfhe_ctx* ctx, size_t B, const uint64_t* d_a, uint64_t a_mod, uint64_t* d_acc,
                                 void* stream);
tfhe_status tfhe_mkm_switch_device(tfhe_ctx* ctx, size_t B, const uint64_t* d_ct_ext, uint64_t fmod, uint64_t* d_out,
                                   void* stream);
/* The chained vector ops of binfhe-base-scheme.cpp:679-1037 with every intermediate in HBM (the
 * same pipelines as tfhe_eval_func / _floor / _sign).  d_lut: [q] or [B][q] in device memory; its
 * first q words are read back once per call to classify the batch (binfhe-base-scheme.cpp:697-698). */
tfhe_status tfhe_eval_func_device(tfhe_ctx* ctx, size_t B, const uint64_t* d_ct, uint64_t q, const uint64_t* d_lut,
                                  int per_ct_lut, uint64_t* d_out, void* stream);
tfhe_status tfhe_eval_floor_device(tfhe_ctx* ctx, size_t B, const uint64_t* d_ct, uint64_t mod, uint32_t roundbits,
                                   uint64_t* d_out, void* stream);
tfhe_status tfhe_eval_sign_device(tfhe_ctx* ctx, size_t B, const uint64_t* d_ct, uint64_t mod, uint64_t* d_out,
                                  void* stream);

/* ---- levelled Boolean circuits (no reference counterpart; added without an ABI version change: new
 * symbols only) ----
 * A netlist of mixed gates is compiled once and evaluated on `instances` independent input sets in one
 * call: every level runs as ONE batch of width * instances bootstraps, whatever gate types it mixes
 * (all gates share the blind rotation; they differ in the linear combination of their operands and in
 * two test-vector constants, which the level's preparation kernel reads per gate).
 *
 * Netlist: wires 0 .. num_inputs-1 are the inputs; gate g defines wire num_inputs + g and may read only
 * lower-numbered wires.  op is a tfhe_gate value or a tfhe_circuit_op; in1 is ignored for NOT, both
 * operands for the constants.  An output may name any wire.  Anything else (unknown op, forward or
 * out-of-range wire, no outputs, a null pointer) is TFHE_ERR_INVALID_ARGUMENT, the message naming the gate.
 *
 * Lowering (results equal the vector gate API called gate by gate, bit for bit): XOR / XNOR become the three
 * bootstraps the vector gate runs for them (binfhe-base-scheme.cpp:619-640), NOT becomes a negate flag
 * on whatever reads it (EvalNOT, binfhe-base-scheme.cpp:147-159), constants become operand kinds
 * (NoiselessEmbedding, lwe-pke.cpp:326-338); nothing else is simplified, so
 * bootstraps = #(OR, AND, NOR, NAND, XOR_FAST, XNOR_FAST) + 3 #(XOR, XNOR).  Inputs and constants are
 * level 0, NOT is transparent, a bootstrapped gate sits at 1 + the larger of its operands' levels.
 *
 * A run keeps every bootstrap's result in a per-device wire store of bootstraps * instances * (n+1) words,
 * owned by the context and grown on demand (slots are not reused by liveness). */
typedef enum tfhe_circuit_op {        /* 0..7 are tfhe_gate's values */
    TFHE_C_NOT = 8, TFHE_C_CONST0 = 9, TFHE_C_CONST1 = 10
} tfhe_circuit_op;
typedef struct tfhe_circuit_gate { uint32_t op, in0, in1; } tfhe_circuit_gate;
typedef struct tfhe_circuit_info {
    uint32_t num_inputs, num_outputs, num_gates;
    uint32_t bootstraps;     /* per instance, after lowering */
    uint32_t levels, widest_level;
} tfhe_circuit_info;
typedef struct tfhe_circuit tfhe_circuit;

tfhe_status tfhe_circuit_compile(tfhe_circuit** out, uint32_t num_inputs, const tfhe_circuit_gate* gates,
                                 size_t num_gates, const uint32_t* outputs, size_t num_outputs);
/* also releases the plan copies on every device that ran the circuit; no call may be using it */
tfhe_status tfhe_circuit_free(tfhe_circuit* c);
tfhe_status tfhe_circuit_get_info(const tfhe_circuit* c, tfhe_circuit_info* out);
/* widths[l] = bootstraps of level l + 1, l < info.levels <= cap */
tfhe_status tfhe_circuit_level_widths(const tfhe_circuit* c, uint32_t* widths, size_t cap);
/* the lowered plan on clear bits: in[num_inputs][instances], out[num_outputs][instances] (no GPU) */
tfhe_status tfhe_circuit_eval_plain(const tfhe_circuit* c, size_t instances, const uint8_t* in, uint8_t* out);
/* d_in[num_inputs][instances][n+1] mod q -> d_out[num_outputs][instances][n+1]; q must divide 2N.  Runs on
 * the context's device that holds d_out, on `stream`; a level wider than 65,536 bootstraps runs in slices. */
tfhe_status tfhe_eval_circuit_device(tfhe_ctx* ctx, const tfhe_circuit* c, size_t instances, const uint64_t* d_in,
                                     uint64_t q, uint64_t* d_out, void* stream);
/* the same on host arrays, staged through the context's first device (levels depend on each other, so a
 * circuit is not sharded over devices) */
tfhe_status tfhe_eval_circuit(tfhe_ctx* ctx, const tfhe_circuit* c, size_t instances, const uint64_t* in, uint64_t q,
                              uint64_t* out);

/* ---- function circuits (no reference counterpart): a netlist over Z_q ciphertext wires whose nodes are linear
 * forms (free) or programmable bootstraps, each with its own table; compiled once on the host, evaluated on
 * `instances` independent input sets per call.  Every level runs as ONE mixed batch -- one preparation launch,
 * one blind rotation, one extraction, one key switch per output modulus -- whatever table classes it mixes.
 * Results equal tfhe_eval_func (shared table) composed node by node, bit for bit.
 *
 * Netlist: wires 0 .. num_inputs-1 are the inputs; node g defines wire num_inputs + g and may read only
 * lower-numbered wires.  Every node forms v = c0 w[in0] + c1 w[in1] + k mod q: a negative coefficient means
 * multiplication by q - |c|; c1 == 0 means in1 is ignored; k (< q) is added to b only (EvalAddConstEq).
 *   TFHE_F_LIN: the wire is v (no bootstrap);
 *   TFHE_F_LUT: the wire is EvalFunc(v, luts[lut]) (binfhe-base-scheme.cpp:679-924).
 * luts is [num_luts][q], every entry < q.  A table's class is decided once, at compile time, by the reference's
 * checkInputFunction (binfhe-base-scheme.cpp:162-186): negacyclic -- one bootstrap; periodic -- two; arbitrary --
 * two at modulus 2q followed by SetModulus(q).  An output may name any wire.  An unknown op, a forward or
 * out-of-range wire, a LUT index out of range, a table entry >= q, k >= q, q not a power of two or below 8, no
 * outputs or a null pointer is TFHE_ERR_INVALID_ARGUMENT, the message naming the node or the table.
 *
 * Counts (tfhe_fcircuit_info): bootstraps = #(LUT nodes on negacyclic tables) + 2 #(LUT nodes on the others);
 * nothing is simplified or removed.  Levels: inputs are level 0 and LIN is transparent (the larger of its
 * operands' levels; an operand with c1 == 0 does not count).  A one-bootstrap LUT node sits at 1 + its form's
 * level; a two-bootstrap node has its first stage there and its second stage -- whose level is the node's -- one
 * level later.  Linear forms are folded at compile time into the bootstraps and outputs that read them, so LIN
 * nodes take no slot of the wire store, which holds bootstraps * instances * (n+1) words as for tfhe_circuit. */
typedef enum tfhe_fcircuit_op { TFHE_F_LIN = 0, TFHE_F_LUT = 1 } tfhe_fcircuit_op;
typedef struct tfhe_fcircuit_node {
    uint32_t op, in0, in1;
    int32_t c0, c1;
    uint32_t lut;            /* TFHE_F_LUT: index into luts; ignored for TFHE_F_LIN */
    uint64_t k;
} tfhe_fcircuit_node;
typedef struct tfhe_fcircuit_info {
    uint32_t num_inputs, num_outputs, num_nodes;
    uint32_t bootstraps;     /* per instance, after lowering */
    uint32_t levels, widest_level;
    uint32_t num_luts, negacyclic, periodic, arbitrary; /* tables, and tables in each class */
    uint64_t q;
} tfhe_fcircuit_info;
typedef struct tfhe_fcircuit tfhe_fcircuit;

tfhe_status tfhe_fcircuit_compile(tfhe_fcircuit** out, uint32_t num_inputs, const tfhe_fcircuit_node* nodes,
                                  size_t num_nodes, uint64_t q, const uint64_t* luts, size_t num_luts,
                                  const uint32_t* outputs, size_t num_outputs);
/* also releases the plan copies on every device that ran the circuit; no call may be using it.  Live handles are
 * kept in a registry: a freed (or never compiled) handle is TFHE_ERR_INVALID_ARGUMENT in every tfhe_fcircuit_* /
 * tfhe_eval_fcircuit* call, a second free included, until a later compile happens to reuse its address. */
tfhe_status tfhe_fcircuit_free(tfhe_fcircuit* c);
tfhe_status tfhe_fcircuit_get_info(const tfhe_fcircuit* c, tfhe_fcircuit_info* out);
/* widths[l] = bootstraps of level l + 1, l < info.levels <= cap */
tfhe_status tfhe_fcircuit_level_widths(const tfhe_fcircuit* c, uint32_t* widths, size_t cap);
/* the lowered plan on clear values mod q: in[num_inputs][instances], out[num_outputs][instances] (no GPU);
 * LIN -> (c0 x + c1 y + k) mod q, LUT -> table[v] */
tfhe_status tfhe_fcircuit_eval_plain(const tfhe_fcircuit* c, size_t instances, const uint64_t* in, uint64_t* out);
/* d_in[num_inputs][instances][n+1] mod q -> d_out[num_outputs][instances][n+1], q the circuit's: it must divide
 * 2N, and a circuit with an arbitrary-class table needs q <= N (TFHE_ERR_UNSUPPORTED otherwise, nothing is
 * launched).  Device selection, stream ordering and slicing as tfhe_eval_circuit_device; tfhe_info.bootstraps
 * grows by info.bootstraps * instances. */
tfhe_status tfhe_eval_fcircuit_device(tfhe_ctx* ctx, const tfhe_fcircuit* c, size_t instances, const uint64_t* d_in,
                                      uint64_t* d_out, void* stream);
/* the same on host arrays, staged through the context's first device */
tfhe_status tfhe_eval_fcircuit(tfhe_ctx* ctx, const tfhe_fcircuit* c, size_t instances, const uint64_t* in,
                               uint64_t* out);

/* ---- dense layers (no reference counterpart beyond CiphertextMulMatrix; new symbols only, the ABI version stays) ----
 * The matrix product on device-resident buffers, for `instances` independent input sets that share one matrix, and
 * the layer y = f(W^T x + b) on top of it: the product at modulus q, then EvalFunc with one shared table over the
 * instances * cols results, every intermediate in HBM.
 * Argument errors -- a null pointer other than d_bias / bias, instances, K or cols = 0, modulus = 0, a size product
 * that overflows size_t; for tfhe_eval_dense*: q < 8, q not a power of two or q not dividing 2N -- are
 * TFHE_ERR_INVALID_ARGUMENT, reported before any device call; a buffer on a device the context does not use is
 * TFHE_ERR_INVALID_ARGUMENT as for the other _device calls. */
/* d_ct[instances][K][n+1], d_matrix[K][cols] (shared), d_bias[cols] or NULL -> d_out[instances][cols][n+1]:
 * out[i][c] = sum_k matrix[k][c] ct[i][k] mod modulus, bias[c] added to the b word only; exact at every modulus
 * (signed entries by their residue; unreduced ciphertext words and bias entries are reduced).
 * inputs are not written; device = the one holding d_out; ordered on `stream` */
tfhe_status tfhe_ciphertext_mul_matrix_device(tfhe_ctx* ctx, size_t instances, size_t K, const uint64_t* d_ct,
                                              size_t cols, const int64_t* d_matrix, const uint64_t* d_bias,
                                              uint64_t modulus, uint64_t* d_out, void* stream);
/* out[i][c] = EvalFunc(sum_k matrix[k][c] ct[i][k] + bias[c] mod q, lut): bit for bit what
 * tfhe_ciphertext_mul_matrix (modulus q), an add of bias[c] to b, and tfhe_eval_func (shared table) give.
 * d_lut: [q]; its first q words are read back once per call to classify it, as tfhe_eval_func_device; an
 * arbitrary-class table with q > N is TFHE_ERR_UNSUPPORTED before anything is launched.  More than 65,536
 * results run EvalFunc in slices, as a circuit level; tfhe_info.bootstraps grows by what tfhe_eval_func on
 * instances * cols ciphertexts adds.  The pre-activation buffer and the matrix residues live in grow-only
 * stores of the context: a call no larger than an earlier one allocates nothing. */
tfhe_status tfhe_eval_dense_device(tfhe_ctx* ctx, size_t instances, size_t K, const uint64_t* d_ct, size_t cols,
                                   const int64_t* d_matrix, const uint64_t* d_bias, uint64_t q,
                                   const uint64_t* d_lut, uint64_t* d_out, void* stream);
/* the same on host arrays, staged through the context's first device (pinned staging, as tfhe_eval_circuit) */
tfhe_status tfhe_eval_dense(tfhe_ctx* ctx, size_t instances, size_t K, const uint64_t* ct, size_t cols,
                            const int64_t* matrix, const uint64_t* bias, uint64_t q, const uint64_t* lut,
                            uint64_t* out);
/* the matrix-product kernel's tile sizes, for tests and tools: K-tile, column tile, threads per workgroup
 * (any pointer may be NULL) */
void tfhe_mm_tiles(int* kt, int* ct, int* threads);

/* ---- convolution layers (no reference counterpart; new symbols only, the ABI version stays) ----
 * Conv2d on ciphertexts with the im2col gather inside the matrix-product kernel (no im2col buffer exists), and the
 * layer y = f(conv(x) + b) on top of it.  With Cg = c_in / groups, Og = c_out / groups and o = g Og + c:
 *   out[i][o][oy][ox] = bias[o] (b word only) + sum_{ic < Cg, ky < kh, kx < kw}
 *                       weight[o][ic][ky][kx] ct[i][g Cg + ic][oy stride_h - pad_h + ky][ox stride_w - pad_w + kx]
 * mod modulus; a tap outside [0, h) x [0, w) is zero padding and contributes nothing.
 * ct[instances][c_in][h][w][n+1], weight[c_out][c_in/groups][kh][kw] int64 (OIHW, shared by all instances),
 * bias[c_out] or NULL -> out[instances][c_out][oh][ow][n+1], oh = (h + 2 pad_h - kh) / stride_h + 1 and ow likewise
 * (integer division).  The output layout is the input layout, so convolutions chain, and it is what
 * tfhe_eval_dense_device reads as [instances][c_out oh ow][n+1].  Exact at every modulus, by the rules of
 * tfhe_ciphertext_mul_matrix_device with K = Cg kh kw terms per sum.  No input is written.
 * Argument errors -- a null pointer other than the bias, instances = 0, a zero among c_in, h, w, c_out, kh, kw,
 * stride_*, groups, groups not dividing c_in or c_out, pad_h >= kh, pad_w >= kw, kh > h + 2 pad_h, kw > w + 2 pad_w,
 * modulus = 0, a size product that overflows size_t; for tfhe_eval_conv2d*: q < 8, q not a power of two or q not
 * dividing 2N -- are TFHE_ERR_INVALID_ARGUMENT, reported before any device call, the message naming the field; a
 * buffer on a device the context does not use is TFHE_ERR_INVALID_ARGUMENT as for the other _device calls. */
typedef struct tfhe_conv2d {
    uint32_t c_in, h, w;          /* input planes and their size */
    uint32_t c_out, kh, kw;       /* output planes, window */
    uint32_t stride_h, stride_w;  /* >= 1 */
    uint32_t pad_h, pad_w;        /* zero rows / columns on each side: pad_h < kh, pad_w < kw */
    uint32_t groups;              /* divides c_in and c_out; 1: full; c_in: depthwise */
} tfhe_conv2d;

/* host only, no GPU: validates the descriptor; oh, ow, K = (c_in / groups) kh kw (any pointer may be NULL) */
tfhe_status tfhe_conv2d_shape(const tfhe_conv2d* d, uint32_t* oh, uint32_t* ow, size_t* K);
/* the gathered product alone, at any modulus; device = the one holding d_out; ordered on `stream` */
tfhe_status tfhe_ciphertext_conv2d_device(tfhe_ctx* ctx, const tfhe_conv2d* d, size_t instances, const uint64_t* d_ct,
                                          const int64_t* d_weight, const uint64_t* d_bias, uint64_t modulus,
                                          uint64_t* d_out, void* stream);
/* the layer: the product at modulus q, then EvalFunc with one shared table d_lut[q] over the flat batch of
 * instances c_out oh ow results, every intermediate in HBM: bit for bit what im2col, tfhe_ciphertext_mul_matrix per
 * group (modulus q), an add of bias[o] to b, tfhe_eval_func and a transpose to plane-major order give.  The table
 * is classified as in tfhe_eval_dense_device (an arbitrary-class table with q > N is TFHE_ERR_UNSUPPORTED before
 * anything is launched); more than 65,536 results run EvalFunc in slices; tfhe_info.bootstraps grows by what
 * tfhe_eval_func on instances c_out oh ow ciphertexts adds.  Uses the dense layer's grow-only stores. */
tfhe_status tfhe_eval_conv2d_device(tfhe_ctx* ctx, const tfhe_conv2d* d, size_t instances, const uint64_t* d_ct,
                                    const int64_t* d_weight, const uint64_t* d_bias, uint64_t q, const uint64_t* d_lut,
                                    uint64_t* d_out, void* stream);
/* the same on host arrays, staged through the context's first device as tfhe_eval_dense */
tfhe_status tfhe_eval_conv2d(tfhe_ctx* ctx, const tfhe_conv2d* d, size_t instances, const uint64_t* ct,
                             const int64_t* weight, const uint64_t* bias, uint64_t q, const uint64_t* lut,
                             uint64_t* out);
/* the kernel's tile sizes, for tests and tools: K-tile, output-plane tile, threads per workgroup, output positions
 * per workgroup (any pointer may be NULL) */
void tfhe_conv2d_tiles(int* kt, int* ct, int* threads, int* positions);

/* ---- pooling layers (no reference counterpart; new symbols only, the ABI version stays) ----
 * A windowed pairwise reduction whose pair step is one EvalFunc: with a ReLU table it is max pooling.
 * ct[instances][c][h][w][n+1] mod q -> out[instances][c][oh][ow][n+1], oh = (h + 2 pad_h - kh) / stride_h + 1 and ow
 * likewise: the output layout is the input layout.  Every (instance, plane, oy, ox) is reduced on its own, every
 * step on all n+1 words:
 *   L0 = the window's taps inside [0, h) x [0, w), in order t = ky kw + kx (a tap in the padding is left out: the
 *        -infinity padding of max_pool2d; pad < window leaves at least one);
 *   round l: L_{l+1}[j] = op(L_l[2j], L_l[2j+1]) for every complete pair; an odd last element is carried unchanged
 *        (no bootstrap, no copy); the reduction ends when one element is left;
 *   op(a, b) = b + EvalFunc(a - b mod q, lut) mod q, EvalFunc being tfhe_eval_func with one shared table lut[q].
 * The result equals that tournament composed on host arrays with tfhe_eval_func bit for bit.  All the pairs of a
 * round, over every instance, plane and position, are one flat EvalFunc batch, run in slices beyond 65,536.  The
 * table is classified as in tfhe_eval_dense_device (an arbitrary-class table with q > N is TFHE_ERR_UNSUPPORTED
 * before anything is launched); tfhe_info.bootstraps grows by pairs c instances (1: negacyclic, 2: otherwise),
 * pairs = sum over positions of (valid taps - 1).  A 1 x 1 window is a strided copy with no bootstrap.  No input
 * word is written.  The descriptor's rules and messages are tfhe_conv2d's: no zero field, pad < window, window <=
 * padded plane.  Argument errors -- a null pointer, instances = 0, q < 8, q not a power of two or not dividing 2N,
 * a size product that overflows size_t -- are TFHE_ERR_INVALID_ARGUMENT, reported before any device call; a buffer
 * on a device the context does not use is TFHE_ERR_INVALID_ARGUMENT as for the other _device calls. */
typedef struct tfhe_pool2d {
    uint32_t c, h, w;             /* planes and their size */
    uint32_t kh, kw;              /* window */
    uint32_t stride_h, stride_w;  /* >= 1 */
    uint32_t pad_h, pad_w;        /* left-out rows / columns on each side: pad_h < kh, pad_w < kw */
} tfhe_pool2d;

/* host only, no GPU: validates the descriptor; oh, ow, the rounds of the longest tournament, pairs per plane (any
 * pointer may be NULL) */
tfhe_status tfhe_pool2d_shape(const tfhe_pool2d* d, uint32_t* oh, uint32_t* ow, uint32_t* rounds, size_t* pairs);
/* host only, no GPU: the same tournament on clear values mod q (a power of two >= 8), in[instances][c][h][w] ->
 * out[instances][c][oh][ow] with op(a, b) = b + lut[a - b mod q] mod q; mirrors tfhe_fcircuit_eval_plain */
tfhe_status tfhe_pool2d_eval_plain(const tfhe_pool2d* d, size_t instances, uint64_t q, const uint64_t* lut,
                                   const uint64_t* in, uint64_t* out);
/* device = the one holding d_out; ordered on `stream`.  Uses the dense layer's grow-only store and a slot store
 * of instances c slots (n+1) words for the results that are not outputs; the plan is uploaded once per
 * (descriptor, device) and kept in the context */
tfhe_status tfhe_eval_pool2d_device(tfhe_ctx* ctx, const tfhe_pool2d* d, size_t instances, const uint64_t* d_ct,
                                    uint64_t q, const uint64_t* d_lut, uint64_t* d_out, void* stream);
/* the same on host arrays, staged through the context's first device as tfhe_eval_conv2d */
tfhe_status tfhe_eval_pool2d(tfhe_ctx* ctx, const tfhe_pool2d* d, size_t instances, const uint64_t* ct, uint64_t q,
                             const uint64_t* lut, uint64_t* out);

/* ---- one table per channel: EvalFunc and the three layers (no reference counterpart; new symbols only, the ABI
 * version stays) ----
 * THE RULE.  A call takes luts[num_luts][q] and inner >= 1; ciphertext i of the flat batch uses table
 * t(i) = (i / inner) mod num_luts, i the index in the whole batch.  Every table is classified on its own by the
 * reference's checkInputFunction (as tfhe_fcircuit_compile does; not from the first table, as per_ct_lut does), and
 * the result for ciphertext i equals tfhe_eval_func with the shared table luts[t(i)] on that ciphertext, bit for
 * bit, whatever mixture of classes the batch holds.  tfhe_info.bootstraps grows by 1 per ciphertext on a
 * negacyclic table and 2 per ciphertext on any other.  If any table is of the arbitrary class and q > N the call
 * is TFHE_ERR_UNSUPPORTED before anything is launched and the counter does not move.  num_luts = 1 is the
 * shared-table result.  No input is written; d_out must not overlap an input.  The device forms read the
 * num_luts q table words back once per call.  The layers use the rule on their flat result
 * [instances][channels][positions]: dense inner = 1, num_luts = cols; convolution inner = oh ow, num_luts = c_out;
 * pooling one table per plane, num_luts = c, in every round.  The host forms stage through the context's first
 * device; a tabled batch is not sharded over devices.
 * Errors before any device call, TFHE_ERR_INVALID_ARGUMENT with a message naming the field: a null pointer; B,
 * num_luts or inner = 0; q < 8, q not a power of two or q not dividing 2N; a size product that overflows; for the
 * layers, num_luts other than the channel count (and the layer's own rules). */
/* host only, no GPU (q need only be a power of two >= 8): classes[t] in {0 negacyclic, 1 periodic, 2 arbitrary}
 * (may be NULL); per_class[3] = ciphertexts of a batch of B under (inner, num_luts) in each class; *bootstraps =
 * what the call adds to tfhe_info.bootstraps */
tfhe_status tfhe_lut_tables_info(uint64_t q, const uint64_t* luts, size_t num_luts, size_t inner, size_t B,
                                 uint8_t* classes, size_t per_class[3], uint64_t* bootstraps);
/* device = the one holding d_out; ordered on `stream`; sliced internally at the scratch capacity */
tfhe_status tfhe_eval_func_tables_device(tfhe_ctx* ctx, size_t B, const uint64_t* d_ct, uint64_t q,
                                         const uint64_t* d_luts, size_t num_luts, size_t inner, uint64_t* d_out,
                                         void* stream);
tfhe_status tfhe_eval_func_tables(tfhe_ctx* ctx, size_t B, const uint64_t* ct, uint64_t q, const uint64_t* luts,
                                  size_t num_luts, size_t inner, uint64_t* out);
/* as tfhe_eval_dense_device / tfhe_eval_dense with d_luts[cols][q] */
tfhe_status tfhe_eval_dense_tables_device(tfhe_ctx* ctx, size_t instances, size_t K, const uint64_t* d_ct, size_t cols,
                                          const int64_t* d_matrix, const uint64_t* d_bias, uint64_t q,
                                          const uint64_t* d_luts, size_t num_luts, uint64_t* d_out, void* stream);
tfhe_status tfhe_eval_dense_tables(tfhe_ctx* ctx, size_t instances, size_t K, const uint64_t* ct, size_t cols,
                                   const int64_t* matrix, const uint64_t* bias, uint64_t q, const uint64_t* luts,
                                   size_t num_luts, uint64_t* out);
/* as tfhe_eval_conv2d_device / tfhe_eval_conv2d with d_luts[c_out][q] */
tfhe_status tfhe_eval_conv2d_tables_device(tfhe_ctx* ctx, const tfhe_conv2d* d, size_t instances, const uint64_t* d_ct,
                                           const int64_t* d_weight, const uint64_t* d_bias, uint64_t q,
                                           const uint64_t* d_luts, size_t num_luts, uint64_t* d_out, void* stream);
tfhe_status tfhe_eval_conv2d_tables(tfhe_ctx* ctx, const tfhe_conv2d* d, size_t instances, const uint64_t* ct,
                                    const int64_t* weight, const uint64_t* bias, uint64_t q, const uint64_t* luts,
                                    size_t num_luts, uint64_t* out);
/* as tfhe_eval_pool2d_device / tfhe_eval_pool2d with d_luts[c][q] */
tfhe_status tfhe_eval_pool2d_tables_device(tfhe_ctx* ctx, const tfhe_pool2d* d, size_t instances, const uint64_t* d_ct,
                                           uint64_t q, const uint64_t* d_luts, size_t num_luts, uint64_t* d_out,
                                           void* stream);
tfhe_status tfhe_eval_pool2d_tables(tfhe_ctx* ctx, const tfhe_pool2d* d, size_t instances, const uint64_t* ct,
                                    uint64_t q, const uint64_t* luts, size_t num_luts, uint64_t* out);

/* ---- products of two encrypted tensors: elementwise and matrix (no reference counterpart; new symbols only, the
 * ABI version stays) ----
 * The pair form: with luts[2][q] (luts[0] for the sums, luts[1] for the differences), q a power of two, every step on
 * all n+1 words,
 *   out[i][r][c] = sum_{k < inner} ( EvalFunc(x[i][r][k] + y[i][k][c] mod q, luts[0])
 *                                  - EvalFunc(x[i][r][k] - y[i][k][c] mod q, luts[1]) )  mod q,
 * EvalFunc being tfhe_eval_func with that table shared.  With the quarter-square tables (tfhe_amd.product_tables:
 * both rows the staircase of floor(s^2 / 4)) it is the matrix product of the messages, since x y = floor((x + y)^2 /
 * 4) - floor((x - y)^2 / 4) exactly for integers; other tables give other functions of the sum and the difference.
 * Layouts: x[instances][rows][inner][n+1]; y[instances][inner][cols][n+1], with y_transposed
 * y[instances][cols][inner][n+1] (Q K^T), with y_shared the instances axis is absent and every instance reads the
 * same y (encrypted weights); out[instances][rows][cols][n+1].  Elementwise multiplication is rows = inner = cols = 1
 * with instances = the number of elements.  The result equals the formula composed on host arrays with tfhe_eval_func
 * and wrap-around adds, bit for bit.  Each table is classified on its own by the reference's checkInputFunction, as
 * tfhe_eval_func_tables does, and the two classes may differ; an arbitrary-class table with q > N is
 * TFHE_ERR_UNSUPPORTED before anything is launched and the counter does not move.  tfhe_info.bootstraps grows by
 * P (b0 + b1), P = instances rows inner cols, b = 1 for a negacyclic table and 2 otherwise.
 * Slicing: the 2 P look-ups are one flat EvalFunc batch (sums, then differences) in slices of whole outputs, so no
 * output is reduced across slices: a slice is floor(min(scratch capacity, 65,536) / (2 inner)) outputs; 2 inner above
 * 65,536 is TFHE_ERR_UNSUPPORTED before any launch.  No input word is written; d_out must not overlap an input.
 * Argument errors -- a null pointer, instances or a dimension = 0, a flag other than 0 or 1, q < 8, q not a power of
 * two or not dividing 2N, a size product that overflows size_t, a table entry >= q in eval_plain -- are
 * TFHE_ERR_INVALID_ARGUMENT with a message naming the field, reported before any device call; a buffer on a device
 * the context does not use is TFHE_ERR_INVALID_ARGUMENT as for the other _device calls. */
typedef struct tfhe_ct_matmul {
    uint32_t rows, inner, cols;  /* >= 1 */
    uint32_t y_transposed;       /* 0: y[..][inner][cols]; 1: y[..][cols][inner] */
    uint32_t y_shared;           /* 0: one y per instance; 1: one y for all */
} tfhe_ct_matmul;

/* host only, no GPU (q need only be a power of two >= 8): *products = P, *bootstraps = what the call adds to
 * tfhe_info.bootstraps (either pointer may be NULL) */
tfhe_status tfhe_ct_matmul_info(const tfhe_ct_matmul* d, size_t instances, uint64_t q, const uint64_t* luts,
                                size_t* products, uint64_t* bootstraps);
/* host only, no GPU: the same formula on clear values mod q, EvalFunc(v, t) = t[v]: x[instances][rows][inner],
 * y and out likewise without the n+1 axis */
tfhe_status tfhe_ct_matmul_eval_plain(const tfhe_ct_matmul* d, size_t instances, uint64_t q, const uint64_t* luts,
                                      const uint64_t* x, const uint64_t* y, uint64_t* out);
/* device = the one holding d_out; ordered on `stream`.  Uses the dense layer's grow-only store (four rows per
 * look-up pair of a slice); reads the 2 q table words back once per call */
tfhe_status tfhe_eval_ct_matmul_device(tfhe_ctx* ctx, const tfhe_ct_matmul* d, size_t instances, const uint64_t* d_x,
                                       const uint64_t* d_y, uint64_t q, const uint64_t* d_luts, uint64_t* d_out,
                                       void* stream);
/* the same on host arrays, staged through the context's first device as tfhe_eval_pool2d */
tfhe_status tfhe_eval_ct_matmul(tfhe_ctx* ctx, const tfhe_ct_matmul* d, size_t instances, const uint64_t* x,
                                const uint64_t* y, uint64_t q, const uint64_t* luts, uint64_t* out);

/* ---- key generation, encryption and decryption on the device (no reference counterpart; new symbols only, the
 * ABI version stays) ----
 * FOR TESTS, BENCHMARKS AND REPRODUCIBLE EXPERIMENTS.  The generator is splitmix64 from a 64-bit seed: it
 * reproduces this project's CPU oracle word for word and is NOT a cryptographic generator.  Production keys
 * come from the client's OpenFHE through tfhe_setup_eval.
 *
 * The stream.  `seed` is the generator state: draw k (k = 0, 1, ...) is mix(seed + (k + 1) g),
 * g = 0x9E3779B97F4A7C15, mix(z): z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB;
 * z ^ z >> 31.  Every word of a key sits at a fixed draw, so rows are generated independently.
 *   uniform(m) = draw mod m;   ternary = draw mod 3 - 1;
 *   gauss (two draws d, d'): u1 = ((d >> 11) + 1.0) / 9007199254740993.0, u2 = (d' >> 11) / 9007199254740992.0,
 *     llround(3.19 * (sqrt(-2 log u1) * cos(6.283185307179586 * u2))), every product rounded on its own
 *     (IEEE double, no fused multiply-add); log and cos are the device library's.
 * Order of a key generation:
 *   1. s: n ternaries (sk = s mod qKS);   2. sN: N ternaries;
 *   3. KSK rows in (i, j, k) order, row r at draw n + N + r (n + 2): its gauss e, then n uniforms mod qKS (A);
 *      B = e + sN[i] j baseKS^k + <A, s> mod qKS at index n;
 *   4. BSK rows in (i, key, row) order behind all KSK rows, row r at offset 3 N r: N uniforms mod Q (a), then N
 *      gauss (e); b = a sN + e in Z_Q[X]/(X^N + 1); when the row's message bit is set (key 0: s_i = 1; key 1:
 *      s_i = -1), baseG^((row >> 1) + numDigitsToThrow) is added to coefficient 0 of a (even row) or b (odd row).
 *   The state after the keys is seed + (n + N + rows_KSK (n + 2) + rows_BSK 3 N) g.
 * Encryption of ciphertext b of a call reads draws b (n + 2) ...: its gauss e, then n uniforms mod `mod` (a);
 *   b = (m mod ptxt_mod) (mod / ptxt_mod) + e + <a, s> mod `mod`, m mod ptxt_mod taken non-negative, s switched
 *   from qKS to `mod` by its centred value; B ciphertexts advance the state by B (n + 2) g -- B successive
 *   single encryptions.  Decryption: r = b - <a, s> + mod / (2 ptxt_mod) mod `mod`; m = floor(ptxt_mod r / mod).
 *
 * Argument errors -- a null pointer (the optional ones are named below), B = 0, mod = 0, ptxt_mod = 0 or
 * ptxt_mod > mod, parameters tfhe_params_finish rejects (or a composite Q) -- are TFHE_ERR_INVALID_ARGUMENT,
 * reported before any device call; an N whose BSK row exceeds the LDS (N > 8192) is TFHE_ERR_UNSUPPORTED. */

/* Oracle layouts, device pointers on `device`: d_sk [n] mod qKS, d_bsk_coeff [n][2][dG2][2][N] mod Q (coefficient
 * form), d_ksk [N][baseKS][dKS][n+1] mod qKS.  d_bsk_coeff / d_ksk may be NULL (that key is skipped); seed_after
 * may be NULL, else *seed_after = the stream state after the keys.  Runs on `stream` and returns when the keys
 * are complete. */
tfhe_status tfhe_keygen_device(const tfhe_params* p, uint64_t seed, int device, uint64_t* d_sk, uint64_t* d_bsk_coeff,
                               uint64_t* d_ksk, uint64_t* seed_after, void* stream);
/* The same keys generated straight into a ready context: the rows are written into the key arena in its packed,
 * NTT-domain form on the first device (no coefficient-form key and no host buffer of the keys' size exists), then
 * replicated and finished as by tfhe_setup.  The context equals tfhe_setup's on tfhe_keygen_device's keys, its key
 * image byte for byte.  sk_out: host, n words; seed_after may be NULL. */
tfhe_status tfhe_setup_keygen(tfhe_ctx** out, const tfhe_params* p, uint64_t seed, int num_gpus, uint64_t* sk_out,
                              uint64_t* seed_after);
/* d_m[B] -> d_ct[B][n+1] mod `mod` under d_sk (n words mod qKS); queued on `stream`.  seed_after may be NULL. */
tfhe_status tfhe_encrypt_device(const tfhe_params* p, int device, const uint64_t* d_sk, size_t B, const int64_t* d_m,
                                uint64_t ptxt_mod, uint64_t mod, uint64_t seed, uint64_t* d_ct, uint64_t* seed_after,
                                void* stream);
/* d_ct[B][n+1] mod `mod` -> d_m[B]; queued on `stream` */
tfhe_status tfhe_decrypt_device(const tfhe_params* p, int device, const uint64_t* d_sk, size_t B, const uint64_t* d_ct,
                                uint64_t ptxt_mod, uint64_t mod, int64_t* d_m, void* stream);
/* The same on host arrays, staged through `device` on `stream`; they return when the output is in host memory. */
tfhe_status tfhe_encrypt(const tfhe_params* p, int device, const uint64_t* sk, size_t B, const int64_t* m,
                         uint64_t ptxt_mod, uint64_t mod, uint64_t seed, uint64_t* ct, uint64_t* seed_after,
                         void* stream);
tfhe_status tfhe_decrypt(const tfhe_params* p, int device, const uint64_t* sk, size_t B, const uint64_t* ct,
                         uint64_t ptxt_mod, uint64_t mod, int64_t* m, void* stream);

/* ---- key replication for one-process-per-GPU deployments ----
 * The packed device key image (NTT-domain BSK with Shoup companions, packed
 * KSK, tables) can be copied device-to-device (e.g. broadcast over RCCL/xGMI by
 * torch.distributed) and adopted by another process without host conversion. */
tfhe_status tfhe_export_key_image(tfhe_ctx* ctx, void* d_dst, size_t bytes, void* stream);
tfhe_status tfhe_setup_from_key_image(tfhe_ctx** out, const tfhe_params* p, const void* d_src, size_t bytes,
                                      int device);
/* The same image as a file (cache the packed layout on disk; replaces
 * BTKeyLoad + GPUSetup's host conversion, binfhecontext.h:208-220, bootstrapping.cu:874-1083):
 * header {magic "TFHEKIMG", ABI version, tfhe_params, image bytes, FNV-1a 64 of the image}
 * followed by the image.  Loading checks magic, version, parameters, size and checksum
 * before touching the device. */
tfhe_status tfhe_save_key_image(tfhe_ctx* ctx, const char* path);
tfhe_status tfhe_setup_from_key_file(tfhe_ctx** out, const tfhe_params* p, const char* path, int device);

/* ---- introspection ---- */
tfhe_status tfhe_get_info(tfhe_ctx* ctx, tfhe_info* out);
const char* tfhe_status_string(tfhe_status s);
const char* tfhe_last_error(void);
int tfhe_abi_version(void);
/* host-only self test of the NTT tables and packing (no GPU needed); 0 = pass */
tfhe_status tfhe_host_selftest(const tfhe_params* p);

/* ---- sharding (no reference counterpart; the reference deals SM_count-sized chunks round-robin,
 * bootstrapping.cu:1617): contiguous shard `rank` of `world` over `total` units, sizes differing by at
 * most one -- the split tfhe_setup(num_gpus) contexts use across their devices and bench.py uses across
 * ranks.  tfhe_host_shard_selftest runs the multi-device runner (one host thread per device) on
 * `devices` fake devices with no GPU: spans[2g], spans[2g+1] = the (lo, count) device g was given;
 * fail_device >= 0 makes that device's body fail, and the call returns its status with
 * tfhe_last_error() = "device <g>: ...". ---- */
tfhe_status tfhe_shard_range(size_t total, int world, int rank, size_t* lo, size_t* hi);
tfhe_status tfhe_host_shard_selftest(size_t B, int devices, int fail_device, size_t* spans);
/* The RCCL sequence of tfhe_setup(num_gpus)'s key replication (communicator over the devices, one
 * ncclBroadcast per rank in a group, streams synchronised, communicators destroyed) run on ONE device with
 * a one-rank communicator: `bytes` (a multiple of 8) of a seeded buffer broadcast out of place and the two
 * copies' checksums compared.  lib NULL or "" = the system librccl (what tfhe_setup loads); *version =
 * ncclGetVersion's (0 if the library lacks it).  TFHE_ERR_UNSUPPORTED when the library does not load;
 * TFHE_ERR_DEVICE when a call fails or the copy differs.  Checks the engine's RCCL binding against the
 * real library on a one-GPU box (the reference's GPUSetup(numGPUs) copies per GPU from the host,
 * bootstrapping.cu:1005-1069). */
tfhe_status tfhe_rccl_selftest(int device, size_t bytes, const char* lib, int* version);

/* ---- launch knobs (no reference counterpart): the kernel-form choices earlier rounds measured A/B.
 * Read from the environment once, when a context is set up (TFHE_KS_TILED_MIN, TFHE_KS_CTS,
 * TFHE_KS_SPLIT, TFHE_KS_PK, TFHE_HOST_PARTS, TFHE_WIRE, TFHE_ACC_FLAGS, TFHE_F64W, TFHE_SF2,
 * TFHE_GENERIC, TFHE_DUO, TFHE_SF2P, TFHE_SPLIT4, TFHE_KS40, TFHE_PAIR_MIN, TFHE_TRACE); afterwards only tfhe_set_knobs changes them -- no
 * launch reads the environment.  Every setting computes the same outputs (each is a parity-tested
 * cross-check).  A variable that is not a whole number, or a value out of the field's range, fails
 * the setup with TFHE_ERR_INVALID_ARGUMENT (tfhe_set_knobs checks the same ranges).  tfhe_set_knobs
 * must not run while another call on the same context is in flight (the calls read the knobs
 * without a lock, as OpenFHE's BinFHEContext is not safe to reconfigure mid-call either). ---- */
typedef struct tfhe_knobs {
    int32_t ks_tiled_min; /* smallest batch on the batch-tiled key switch; -1: the default (1); 0: never */
    int32_t ks_cts;       /* ciphertexts per thread in the tiled key switch: 0 (by key width / batch), 1, 2, 4 (4: the packed
                             u16 form only -- STD128's keys, its default from 2048 ciphertexts; other widths take 2) */
    int32_t ks_split;     /* most block groups the key-switch steps split over at small batches (1: none) */
    int32_t ks_pk;        /* 0: 32-bit column sums for u16 keys instead of packed u16 pairs */
    int32_t host_parts;   /* sub-batches per device in the host-array runner (>= 1) */
    int32_t wire;         /* 0: u64 words over PCIe (no narrow wire format) */
    int32_t acc_flags;    /* 0: host-array EvalAcc waits for the whole launch (no completion flags) */
    int32_t f64w;         /* retired: must be 1 (round 5 removed the slot-layout FP64 kernel 0 selected) */
    int32_t sf2;          /* 0: gen3sf special-form blind rotation instead of the wave-local sf2 */
    int32_t generic;      /* generic kernel form: 0 by N; 1 v1 (digits in LDS); 2 v2 also at N = 2048 */
    int32_t trace;        /* host-array runner timeline on stderr; circuit runs: event-timed total and the share of the
                             preparation and output kernels */
    int32_t probe;        /* test library only (lib/libtfhe_hip_test.so): fault-probe / timing builds */
    int32_t duo;          /* one- and two-digit special-form contexts (sfduo) and STD128Q- / STD192-class FP64 contexts (f64wduo):
                             batches up to this size (default 128, at most 256) run each ciphertext on two
                             workgroups, and only while the device holds every pair co-resident (a duo workgroup
                             takes one CU: at most half the CU count, 128 on MI355X); 0: never */
    int32_t sf2p;         /* two-digit special-form contexts, batches of 512 or more: 1 (default) runs two
                             ciphertexts per workgroup (sf2p, whose shared LDS holds the whole monomial factor
                             table); 0: one per workgroup (sf2) */
    int32_t split4;       /* STD128-class contexts: batches up to this size (default 384) run each ciphertext's two
                             polynomials on two groups of four wavefronts (fast4 SPLIT); 0: never */
    int32_t ks40;         /* contexts whose key-switching keys need 8-byte words with qKS = 2^33 .. 2^37 (the logQ
                             contexts: 2^35): 1 (default) runs the tiled key switch on split-word records derived
                             at setup (u32 low word + u8 high part per key, 80 B per 16-column row segment instead
                             of 128 B); 0: on the u64 words */
} tfhe_knobs;
tfhe_status tfhe_get_knobs(tfhe_ctx* ctx, tfhe_knobs* out);
tfhe_status tfhe_set_knobs(tfhe_ctx* ctx, const tfhe_knobs* in);

/* One more launch knob, with calls of its own so that tfhe_knobs keeps its layout (new symbols only, same ABI
 * version).  STD128-class contexts: device-resident batches of at least pair_min ciphertexts (default 3072,
 * from TFHE_PAIR_MIN at setup; 0: never) run the blind rotation's pair instance -- two ciphertexts per
 * wavefront, so every key row loaded feeds both -- unless the batch takes the two-group form (split4) or
 * the host-array runner's completion flags.  Same outputs at every setting; tfhe_set_knobs leaves it alone.
 * pair_launches (may be null, as may pair_min): blind rotations this context has launched on that instance. */
tfhe_status tfhe_get_pair_min(tfhe_ctx* ctx, int32_t* pair_min, uint64_t* pair_launches);
tfhe_status tfhe_set_pair_min(tfhe_ctx* ctx, int32_t pair_min);
/* Dynamic LDS bytes per workgroup of the STD128 blind rotation: pair = 0 the default instance (four workgroups
 * per CU), 1 the pair instance (three per CU: at most 160 KiB / 3). */
size_t tfhe_fast4_lds_bytes(int pair);

/* ---- extension (no reference counterpart): build of the specialised STD128-class blind
 * rotation used by later calls, for A/B runs and tests; 0 restores the default.  Process-wide;
 * initial value from TFHE_FAST_VARIANT.  Every build computes the same output. ---- */
tfhe_status tfhe_set_kernel_variant(int variant);
int tfhe_get_kernel_variant(void);

#ifdef __cplusplus
}
#endif
#endif /* TFHE_HIP_H */
