// kernels.hpp -- launch wrappers for the HIP kernels (definitions in *.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "pool.hpp"

namespace tfhe {

// Scalar parameters every blind-rotation kernel needs (the reference's
// params_CUDA[10], bootstrapping.cu:917-929, plus derived constants).
struct BRParams {
    uint32_t N, logN, n, dG2, digits, thr, logG;
    uint64_t Q;
    uint64_t r1;  // floor(2^b / Q), b = word bits, for lazy-sum reduction
};

// Launch choices of one context: read from the environment once, at setup (engine.hip
// knobs_from_env), changed afterwards only through tfhe_set_knobs (tests, A/B runs).  The C-ABI
// mirror is tfhe_knobs (include/tfhe_hip.h); the launchers below take them by reference.
struct Knobs {
    int32_t ks_tiled_min = -1;  // smallest batch on the tiled key switch; -1: default (1), 0: never
    int32_t ks_cts = 0;         // ciphertexts per thread of the tiled key switch; 0: by key width / batch
    int32_t ks_split = 32;      // most block groups the key-switch steps split over at small batches (u16 / u32 keys: 16 at most); 1: none
    int32_t ks_pk = 1;          // 0: no packed u16 column sums
    int32_t host_parts = 1;     // sub-batches per device of the host-array runner
    int32_t wire = 1;           // 0: u64 PCIe words (no narrow wire format)
    int32_t acc_flags = 1;      // 0: no completion-flagged EvalAcc output
    int32_t f64w = 1;           // retired (round 5: the slot-layout FP64 kernel it selected is gone); must be 1
    int32_t sf2 = 1;            // 0: gen3sf instead of the wave-local sf2
    int32_t generic = 0;        // 0: gen3 / v2 by N; 1: v1 (all digits in LDS); 2: v2 also at N = 2048
    int32_t trace = 0;          // host-array runner timeline on stderr
    int32_t probe = 0;          // test library only (TFHE_TEST_PROBES): f64w fault probe / timing builds
    int32_t duo = 128;          // most ciphertexts per launch on the two-workgroup forms (sf2duo: two digits;
                                // f64wduo: STD128Q class; <= 256); 0: never
    int32_t sf2p = 1;           // 0: sf2 with one ciphertext per workgroup instead of two (sf2p) above the duo batches
    int32_t split4 = 384;       // STD128 class: batches up to this size run fast4's two-group form (SPLIT); 0: never
    int32_t ks40 = 1;           // 8-byte keys with qKS = 2^(33..37): the tiled key switch on split-word records; 0: u64
    // -- not in tfhe_knobs (whose layout is fixed by the ABI version): tfhe_set_pair_min / tfhe_get_pair_min --
    int32_t pair_min = 3072;    // STD128 class: batches from this size run fast4's pair instance (two ciphertexts per
                                // wavefront, blind_rotate_fast4_pair.hip); 0: never
};

// Device tables for one (Q, N), word type W (uint32_t or uint64_t storage).
struct DevTables {
    const void* psi;     // [N]  forward twiddles, bit-reversed order
    const void* psi_sh;  // [N]  Shoup companions
    const void* ipsi;    // [N]  inverse twiddles
    const void* ipsi_sh; // [N]
    const void* mono;    // [2N] psi^k - 1
    const void* mono_sh; // [2N]
    const uint32_t* eidx;// [N]  NTT(X)[x] = psi^eidx[x]
};

// Completion flags of a blind rotation (host-array EvalAcc: engine.hip d2h_flagged).  A launcher
// whose kernel stores flags[ct] = gen in host memory once ciphertext ct's accumulator is in HBM
// sets written; the others leave it false and the caller waits for the whole launch instead.
struct BRDone {
    uint32_t* flags = nullptr;  // pinned host memory, one word per ciphertext
    uint32_t gen = 0;
    bool written = false;
};

// Generic LDS-resident blind rotation: one workgroup per ciphertext.
//   a[B][n] mod amod, acc[B][2][N] (u64, coefficient) in/out, acc0 transposed on exit.
//   bsk/bsk_sh: [n][2][dG2][2][N] in W, NTT domain, scaled by N^-1.
hipError_t launch_blind_rotate_generic(int word_bits, const BRParams& P, const DevTables& T, const void* bsk,
                                       const void* bsk_sh, const uint64_t* a, uint64_t amod, uint64_t* acc, size_t B,
                                       hipStream_t s, const Knobs& kn);

// Fast STD128-class blind rotation (W = u32, N = 1024, dG2 = 8): register-resident
// transforms, one wavefront per ciphertext.  Returns hipErrorNotSupported when the
// parameters do not match its specialisation.
// split_max: batches up to this size run the two-group form (k_blind_rotate_fast4 SPLIT; tfhe_knobs.split4)
// pair_min: larger batches from this size run the pair instance (0: never); *paired: whether this launch did
hipError_t launch_blind_rotate_fast(const BRParams& P, const DevTables& T, const void* bsk_fast, const uint64_t* a,
                                    uint64_t amod, uint64_t* acc, size_t B, hipStream_t s, BRDone* dn = nullptr,
                                    int split_max = 0, int pair_min = 0, bool* paired = nullptr);
bool fast_path_supported(const BRParams& P, int word_bits);
// Converts the generic device BSK and tables into the fast kernel's Montgomery form.
hipError_t launch_pack_bsk_fast(const BRParams& P, const DevTables& T, const void* bsk, void* bsk_fast,
                                hipStream_t s);
size_t bsk_fast_bytes(const BRParams& P);
// build of the specialised kernel (see blind_rotate_fast.hip); 0 = default; false if unknown
bool set_fast_variant(int v);
int get_fast_variant();
// the fast kernels' constants for modulus Q (out: a FastConst, blind_rotate_fast.hip / f4::FastConst)
void fast_const_build(uint32_t Q, void* out);
// 4-wavefront variant (blind_rotate_fast4.hip): its table block, packed behind the fast tables,
// and its launch (K: the fast kernel's FastConst).  Digit shape: dig digits per polynomial
// (dG2 = 2 dig), baseG = 2^logg, thr thrown digits, fold = top digit eliminated.
struct Fast4Shape {
    int dig, logg, thr;
    bool fold;
};
bool fast4_shape_supported(const Fast4Shape& sh);
size_t fast4_table_words();
hipError_t launch_pack_tables_fast4(uint32_t Q, const DevTables& T, void* out, hipStream_t s);
hipError_t launch_blind_rotate_fast4(int variant, const Fast4Shape& sh, const void* K, uint32_t n, uint32_t loga,
                                     const int32_t* tabs4, const int32_t* bsk, const uint64_t* a, uint64_t* acc,
                                     size_t B, hipStream_t s, BRDone* dn = nullptr, int split_max = 0, int pair_min = 0,
                                     bool* paired = nullptr);
size_t fast4_lds_bytes(bool pair);  // dynamic LDS of the default / pair instance at the STD128 shape

// Exact-FP64 blind rotation for 2^32 <= Q < 2^50, N = 2048 (STD192 / STD192Q / STD128Q classes):
// keys/tables as centred doubles derived on device from the generic (u64) arena.
bool f64_path_supported(const BRParams& P, int word_bits);
// an instance exists for this context's (Q width, top-digit fold) combination (f64w or slot layout)
bool f64_instance_available(const BRParams& P, bool fold);
size_t bsk_f64_bytes(const BRParams& P);
// fold: eliminate the top digit's transforms (keys packed accordingly); only when
// f64_fold_enabled(P) (thr = 0; WRAP correction where the top digit is not always exact;
// TFHE_F64_FOLD=1 folds only exact sets, 0 turns it off).
bool f64_fold_enabled(const BRParams& P);
// true only in the test library (blind_rotate_f64.hip built with -DTFHE_TEST_PROBES)
bool f64_test_probes_compiled();
hipError_t launch_pack_bsk_f64(const BRParams& P, const DevTables& T, const void* bsk, bool fold, void* out,
                               hipStream_t s);
struct DuoDev;  // duo.hpp
// duo: the device's duo state (STD128Q-class batches up to kn.duo and the device's co-resident pairs run
// k_blind_rotate_f64wduo)
hipError_t launch_blind_rotate_f64(const BRParams& P, const DevTables& T, const void* keys, bool fold, const uint64_t* a,
                                   uint64_t amod, uint64_t* acc, size_t B, hipStream_t s, const Knobs& kn,
                                   DuoDev* duo = nullptr);
// true when the context's FP64 blind rotation has the two-workgroup form (STD128Q class)
bool f64_duo_form(const BRParams& P, bool fold);

// Special-form u64 blind rotation (blind_rotate_sf.hip) for N = 2048 and
// Q = 2^54 - c, c < 2^20 (the logQ / arbFunc contexts): constants as (w, w 2^31 mod Q), five
// multiplies per product.  sf: the W1 arrays (psi, ipsi, mono, bsk) derived on device.
bool sf_path_supported(const BRParams& P, int word_bits);
size_t sf_bytes(const BRParams& P);
hipError_t launch_pack_sf(const BRParams& P, const DevTables& T, const void* bsk, void* out, hipStream_t s);
hipError_t launch_blind_rotate_sf(const BRParams& P, const DevTables& T, const void* bsk, const void* sf,
                                  const uint64_t* a, uint64_t amod, uint64_t* acc, size_t B, hipStream_t s,
                                  const Knobs& kn, DuoDev* duo);

// MKM: ModSwitch(Q->qKS), KeySwitch, ModSwitch(qKS->fmod).
//   ext[B][N+1] mod Q -> out[B][n+1] mod fmod.
//   kska: [N][baseKS][dKS][n_pad] (A part, rows padded to 16 bytes), kskb: [N][baseKS][dKS] (B),
//   both in ksk_bits words.
struct KSParams {
    uint32_t N, n, baseKS, dKS, n_pad;
    uint64_t Q, qKS;
};
hipError_t launch_mkm(const KSParams& P, int ksk_bits, const void* kska, const void* kskb, const uint64_t* ext,
                      uint64_t fmod, uint64_t* out, size_t B, hipStream_t s);
// Batch-tiled form of the same (ks_tiled.hip): the KSK is staged in LDS once per tile of
// up to 1024 ciphertexts instead of gathered per ciphertext.  scratch: ks_tiled_scratch_bytes
// (transposed digit planes).  hipErrorNotSupported when dKS > 16 or baseKS too large.
size_t ks_tiled_scratch_bytes(const KSParams& P, size_t B);
bool ks_tiled_supported(const KSParams& P);
// ksk40: the split-word records of 8-byte keys (ks40_bytes > 0: qKS = 2^(32+b), 1 <= b <= 5, the logQ contexts;
// derived at setup by launch_pack_ks40 from the arena's u64 KSK); nullptr: the u64 form
hipError_t launch_ks_tiled(const KSParams& P, int ksk_bits, const void* kska, const void* kskb, const uint64_t* ext,
                           uint64_t fmod, uint64_t* out, size_t B, void* scratch, hipStream_t s, const Knobs& kn,
                           const void* ksk40 = nullptr);
size_t ks40_bytes(const KSParams& P);
hipError_t launch_pack_ks40(const KSParams& P, const void* kska, void* out, hipStream_t s);

// ---- test vectors, extraction and LWE glue (binfhe-base-scheme.cpp) ----
enum TvMode : uint32_t {
    TV_GATE = 0,    // BootstrapGateCore: +-(Q/8+1) by range [q1,q2)
    TV_HALF = 1,    // f0/f1: x<q/2 ? fmod-q/4 : q/4
    TV_FLOOR2 = 2,  // f2 of EvalFloor
    TV_SIGN3 = 3,   // f3 of EvalSign
    TV_LUT = 4,     // LUT[x]
    TV_LUT1 = 5,    // x<q/2 ? LUT[x] : fmod - LUT[x-q/2]
    TV_LUT2 = 6,    // LUT2 = LUT++LUT, arbitrary-function second bootstrap
};
struct TvParams {
    uint32_t mode, N, n;
    uint64_t Q, ctmod, fmod;
    uint64_t q1, q2;        // gate range
    uint64_t Q8;            // Q/8 + 1
    const uint64_t* lut;    // TV_LUT*: [q] or [B][q]
    uint64_t lut_stride;    // 0: shared LUT
    uint64_t lut_len;       // original LUT length (q)
};
// ct[B][n+1] -> acc[B][2][N] (acc0 = 0, acc1 = test vector), a_out[B][n] = a part
hipError_t launch_build_testvector(const TvParams& P, const uint64_t* ct, uint64_t* acc, uint64_t* a_out, size_t B,
                                   hipStream_t s);
// ---- one table per channel (func_tables.hip) ----
// Which table of P.lut[T][P.lut_len] row s of a launch reads: ids[s] when ids is set (a class's gathered rows), else
// ((first + s) / inner) mod T, first the row's index in the whole batch.
struct TabSel {
    const uint32_t* ids;
    uint64_t first, inner, T;
};
// launch_build_testvector for the modes TV_LUT, TV_LUT1 and TV_LUT2 with the table chosen by S; q a power of two
hipError_t launch_build_testvector_tab(const TvParams& P, const TabSel& S, const uint64_t* ct, uint64_t* acc,
                                       uint64_t* a_out, size_t B, hipStream_t s);
// A slice [first, first + count) of the batch that holds several classes, moved to and from per-class runs of rows:
// an item of class c goes to row base[c] + its rank among the slice's class-c items.  meta[T] = {class, number of
// class-0 / 1 / 2 tables below t}; ntab[c] the class's tables; lo[c] the class's items below `first`.
struct TabMove {
    const uint4* meta;
    uint64_t first, count, inner, T;
    uint64_t ntab[3], lo[3], base[3];
    uint32_t width;
};
// rows[pos] = flat[s] and ids[pos] = the item's table, for s < count
hipError_t launch_tab_gather(const TabMove& M, const uint64_t* flat, uint64_t* rows, uint32_t* ids, hipStream_t s);
// flat[s] = rows[pos]
hipError_t launch_tab_scatter(const TabMove& M, const uint64_t* rows, uint64_t* flat, hipStream_t s);

// tv[B][tvlen] -> acc[B][2][N]: acc0 = 0, acc1[j * (N / tvlen)] = tv[j], other coefficients 0
hipError_t launch_expand_tv(uint32_t N, uint32_t tvlen, const uint64_t* tv, uint64_t* acc, size_t B, hipStream_t s);
// u16 / u32 (wb = 2 / 4 bytes) <-> u64 words: the narrow PCIe wire format of the host-array runner
hipError_t launch_widen(const void* src, int wb, uint64_t* dst, size_t n, hipStream_t s);
hipError_t launch_narrow(const uint64_t* src, int wb, void* dst, size_t n, hipStream_t s);
// acc[B][2][N] (acc0 transposed) -> ext[B][N+1]: a = acc0, b = acc1[0] + b_add mod Q
hipError_t launch_extract(uint32_t N, uint64_t Q, uint64_t b_add, const uint64_t* acc, uint64_t* ext, size_t B,
                          hipStream_t s);

// ---- circuit path (circuit_kernels.hip; plan records: circuit.hpp) ----
// One launch covers bootstraps [first, first + B) of a level (or outputs, for launch_circuit_out), flat
// index = gate * instances + instance; `in` is [num_inputs][instances][n+1], `store` the wire store
// [bootstraps][instances][n+1].
struct CircuitRec;
struct CircuitOut;
struct CircuitPrep {
    uint32_t N, n;
    uint64_t Q, Q8, q;  // Q8 = Q/8 + 1; q: the ciphertext modulus (divides 2N)
    size_t instances, first;
};
// recs: the level's first record.  acc[B][2][N] (acc0 = 0, acc1 = each gate's test vector), a_out[B][n]
hipError_t launch_circuit_prep(const CircuitPrep& P, const CircuitRec* recs, const uint64_t* in, const uint64_t* store,
                               uint64_t* acc, uint64_t* a_out, size_t B, hipStream_t s);
// out[num_outputs][instances][n+1]
hipError_t launch_circuit_out(const CircuitPrep& P, const CircuitOut* outs, const uint64_t* in, const uint64_t* store,
                              uint64_t* out, size_t B, hipStream_t s);

// ---- function-circuit path (fcircuit_kernels.hip; plan records: fcircuit.hpp) ----
// As above with flat index = record * instances + instance.  q: the circuit's modulus, a power of two that
// divides 2N (records at 2q need q <= N); N = 2^log2N.
struct FuncRec;
struct FuncTerm;
struct FuncOut;
struct FuncPrep {
    uint32_t N, n, log2N;
    uint64_t Q, q;
    size_t instances, first;
};
// recs: the level's first record; terms / luts: the plan's.  acc[B][2][N] (acc0 = 0, acc1 = each record's test
// vector), a_out[B][n] = each mask scaled to modulus 2N
hipError_t launch_fcircuit_prep(const FuncPrep& P, const FuncRec* recs, const FuncTerm* terms, const uint64_t* luts,
                                const uint64_t* in, const uint64_t* store, uint64_t* acc, uint64_t* a_out, size_t B,
                                hipStream_t s);
// out[num_outputs][instances][n+1]
hipError_t launch_fcircuit_out(const FuncPrep& P, const FuncOut* outs, const FuncTerm* terms, const uint64_t* in,
                               const uint64_t* store, uint64_t* out, size_t B, hipStream_t s);

enum LweOp : uint32_t {
    LWE_ADD = 0,        // out = x + y mod m
    LWE_SUB = 1,        // out = x - y mod m
    LWE_DOUBLE_SUB = 2, // out = 2(x - y) mod m   (XOR_FAST prep)
    LWE_NOT = 3,        // out = NOT x (EvalNOT, binfhe-base-scheme.cpp:147-159)
    LWE_ADD_CONST = 4,  // b += c mod m
    LWE_SUB_CONST = 5,  // b -= c mod m
    LWE_SET_MOD = 6,    // every word mod m (LWECiphertextImpl::SetModulus)
    LWE_MODSWITCH = 7,  // RoundqQ(x, m, c)  (lwe-pke.cpp:204-215), c = old modulus
    LWE_COPY = 8,
};
// element-wise over B ciphertexts of n+1 words; y may be null for unary ops
hipError_t launch_lwe_op(uint32_t op, uint32_t n, uint64_t m, uint64_t c, const uint64_t* x, const uint64_t* y,
                         uint64_t* out, size_t B, hipStream_t s);

// Position-mixed checksum of `bytes` (a multiple of 8) of device memory: kChecksumBlocks u64 partials,
// whose sum (mod 2^64) the host forms.  engine.hip compares every key-arena replica with device 0's.
constexpr unsigned kChecksumBlocks = 1024;
hipError_t launch_checksum(const void* p, size_t bytes, uint64_t* partial, hipStream_t s);

// ---- key generation, encryption, decryption (keygen_kernels.hip; the stream: include/tfhe_hip.h) ----
// *_state: the splitmix64 state in front of the first KSK / BSK row's first draw.
struct KeygenParams {
    uint32_t N, n, dG2, baseKS, dKS, n_pad;
    uint64_t Q, qKS;
    uint64_t ksk_state, bsk_state;
    uint64_t Ninv, Ninv_sh;  // N^-1 mod Q and its Shoup companion at the context's word width
    size_t ksk_rows, bsk_rows;
};
// Small device arrays of one key generation (engine.hip keygen_prepare).  W = the context's word class.
struct KeygenTables {
    const void *psi, *psi_sh, *ipsi, *ipsi_sh;  // [N] of W: the context's NTT tables
    const void *snt, *snt_sh;                   // [N] of W: NTT(sN) N^-1 and its Shoup companions
    const int8_t* s;                            // [n] LWE key, ternary
    const int8_t* sN;                           // [N] ring key, ternary
    const uint64_t* g;                          // [dG2 / 2] baseG^(d + numDigitsToThrow) mod Q
    const uint64_t* gN;                         // [dG2 / 2] the same times N^-1
    const uint64_t* pw;                         // [dKS] baseKS^k mod qKS
};
constexpr size_t kKeygenMaxLds = 160 * 1024;
size_t keygen_bsk_lds_bytes(uint32_t N, int word_bits, bool arena);
// ksk_bits 0: out_a is the caller's [rows][n+1] u64 array (out_b unused); 16 / 32 / 64: the arena's packed A
// part [rows][n_pad] and B part [rows] at that width (pad columns are written as zeros)
hipError_t launch_keygen_ksk(const KeygenParams& P, const KeygenTables& T, int ksk_bits, void* out_a, void* out_b,
                             hipStream_t s);
// arena: out / out_sh = the arena's bsk / bsk_sh regions (NTT domain, scaled by N^-1, and Shoup companions) in
// word_bits words; else out = the caller's coefficient-form [rows][2][N] u64 array (out_sh unused).
// hipErrorNotSupported when the row does not fit the LDS (keygen_bsk_lds_bytes > kKeygenMaxLds).
hipError_t launch_keygen_bsk(const KeygenParams& P, const KeygenTables& T, int word_bits, bool arena, void* out,
                             void* out_sh, hipStream_t s);
// or_encrypt / or_decrypt on B ciphertexts [B][n+1] mod `mod`; sk mod qKS; ciphertext b draws from
// seed + b (n + 2) positions
hipError_t launch_lwe_encrypt(uint32_t n, uint64_t qKS, const uint64_t* sk, size_t B, const int64_t* msg,
                              uint64_t ptxt_mod, uint64_t mod, uint64_t seed, uint64_t* ct, hipStream_t s);
hipError_t launch_lwe_decrypt(uint32_t n, uint64_t qKS, const uint64_t* sk, size_t B, const uint64_t* ct,
                              uint64_t ptxt_mod, uint64_t mod, int64_t* msg, hipStream_t s);

// CiphertextMulMatrix (mul_matrix.hip): out[i][c][w] = (bias[c] [w == width - 1] + sum_k matrix[k][c] ct[i][k][w])
// mod modulus; ct [instances][K][width], matrix [K][cols] shared, bias [cols] or null, out [instances][cols][width].
// No input is written; mat_scratch (K cols words) receives the entries' residues.  Tile sizes: a workgroup of
// MM_THREADS threads owns MM_THREADS words of one instance and MM_CT columns, the matrix in LDS tiles of MM_KT rows.
constexpr int MM_THREADS = 256, MM_KT = 32, MM_CT = 16;
hipError_t launch_mul_matrix(uint32_t width, size_t instances, size_t K, const uint64_t* ct, size_t cols,
                             const int64_t* matrix, const uint64_t* bias, uint64_t modulus, uint64_t* mat_scratch,
                             uint64_t* out, hipStream_t s);

// Conv2d on ciphertexts (conv2d.hip): the matrix product with the im2col gather inside the kernel.
// ct [instances][c_in][h][w][width], weight [c_out][c_in/groups][kh][kw] int64 (OIHW) shared, bias [c_out] or null,
// out [instances][c_out][oh][ow][width]; a tap in the zero padding contributes nothing.  No input is written;
// mat_scratch (c_out K words, K = (c_in/groups) kh kw) receives the weights' residues, reordered.  The geometry
// is validated by the caller (tfhe_conv2d_shape).  Tile sizes: a workgroup of CV_THREADS threads owns CV_THREADS
// words of one instance, CV_CT output planes of one group and CV_P output positions, the weights in LDS tiles of
// CV_KT taps.
constexpr int CV_THREADS = 256, CV_KT = 32, CV_CT = 8, CV_P = 2;
struct ConvGeom {
    uint32_t c_in, h, w, c_out, kh, kw, sh, sw, ph, pw, groups;
    uint32_t oh, ow;  // (h + 2 ph - kh) / sh + 1, (w + 2 pw - kw) / sw + 1
};
hipError_t launch_conv2d(uint32_t width, const ConvGeom& g, size_t instances, const uint64_t* ct,
                         const int64_t* weight, const uint64_t* bias, uint64_t modulus, uint64_t* mat_scratch,
                         uint64_t* out, hipStream_t s);

// The windowed pairwise reduction's streaming kernels (pool2d.hip), around each round's EvalFunc.
// Items [first, first + count) of a round's flat batch, item = (instance c + plane) nrec + r over the nrec
// records of one plane (pool.hpp): launch_pool_diff writes z[it] = a - b mod q, launch_pool_add writes
// dst = f[it] + b mod q, launch_pool_copy dst = b, it = item - first.  in [planes][in_plane words] is only read;
// slots [planes][slot_plane] and out [planes][out_plane] are the destinations; mask = q - 1.  A workgroup of
// PL_THREADS threads takes PL_ITEMS items at a time, one per wave.
constexpr int PL_THREADS = 256, PL_ITEMS = PL_THREADS / 64;
struct PoolArgs {
    const PoolRec* recs;
    size_t nrec, first, count;
    uint32_t width;
    uint64_t mask;
    const uint64_t* in;
    size_t in_plane;
    uint64_t* slots;
    size_t slot_plane;
    uint64_t* out;
    size_t out_plane;
};
hipError_t launch_pool_diff(const PoolArgs& p, uint64_t* z, hipStream_t s);
hipError_t launch_pool_add(const PoolArgs& p, const uint64_t* f, hipStream_t s);
hipError_t launch_pool_copy(const PoolArgs& p, hipStream_t s);

// The streaming kernels around the EvalFunc batch of a product of two encrypted tensors (ct_matmul.hip; DESIGN
// 3.13).  A slice holds the whole outputs [first_out, first_out + count / inner), o = (i rows + r) cols + c; item
// `it` < count is product (o, k) = (first_out + it / inner, it mod inner).  launch_ctmm_pairs writes z[it] = x + y
// and z[count + it] = x - y mod q for x = x[i][r][k], y = y[i][k][c] ([c][k] with y_transposed, no i with y_shared);
// launch_ctmm_reduce writes out[o] = sum_k f[o' inner + k] - f[count + o' inner + k] mod q.  x and y are only read;
// mask = q - 1; z and f hold 2 count rows.  A workgroup of CM_THREADS threads takes CM_ITEMS items at a time, one per
// wave.
constexpr int CM_THREADS = 256, CM_ITEMS = CM_THREADS / 64;
struct CtmmArgs {
    const uint64_t* x;
    const uint64_t* y;
    uint32_t rows, inner, cols, y_transposed, y_shared;
    uint32_t width;
    uint64_t mask;
    size_t first_out, count;
};
hipError_t launch_ctmm_pairs(const CtmmArgs& p, uint64_t* z, hipStream_t s);
hipError_t launch_ctmm_reduce(const CtmmArgs& p, const uint64_t* f, uint64_t* out, hipStream_t s);

}  // namespace tfhe
