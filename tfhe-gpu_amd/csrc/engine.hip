// engine.hip -- tfhe_ctx: key ingest (GPUSetup), device pipelines for every batch
// operation, multi-GPU sharding, and the extern "C" entry points of tfhe_hip.h.
//
// Design (MI355X-first):
//  * keys live in one per-device "key arena" (tables + NTT-domain BSK with Shoup
//    companions + packed KSK) so a whole key image is one device-to-device copy
//    (peer copy over xGMI in-process, RCCL broadcast across processes);
//  * every bootstrap of a fused op (gate, EvalFunc, EvalFloor, EvalSign,
//    EvalDecomp) stays in HBM: test vector -> blind rotation -> extraction ->
//    MKM -> LWE glue, one stream per device, host sees only LWE ciphertexts;
//  * a batch is split into contiguous shards, one host thread + stream per
//    device (the reference interleaves SM_count-sized chunks, bootstrapping.cu:1617).
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "circuit.hpp"
#include "fcircuit.hpp"
#include "duo.hpp"
#include "host_math.hpp"
#include "kernels.hpp"
#include "tfhe_hip.h"

using namespace tfhe;

namespace {

thread_local std::string g_last_error;

tfhe_status fail(tfhe_status s, const std::string& msg) {
    g_last_error = msg;
    return s;
}

}  // namespace

tfhe_status tfhe::set_last_error(tfhe_status s, const std::string& msg) { return fail(s, msg); }

namespace {

#define HCHECK(expr)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess)                                                                          \
            return fail(e_ == hipErrorOutOfMemory ? TFHE_ERR_OUT_OF_MEMORY : TFHE_ERR_DEVICE,          \
                        std::string(#expr) + ": " + hipGetErrorString(e_));                            \
    } while (0)

#define SCHECK(expr)                        \
    do {                                    \
        tfhe_status s_ = (expr);            \
        if (s_ != TFHE_OK) return s_;       \
    } while (0)

constexpr size_t kAlign = 256;
inline size_t align_up(size_t x) { return (x + kAlign - 1) / kAlign * kAlign; }

int ksk_bits_for(uint64_t qKS) {
    if (qKS <= (1ull << 16)) return 16;
    if (qKS <= (1ull << 32)) return 32;
    return 64;
}

// Byte offsets of everything inside the key arena; a pure function of the params,
// so an importing process can locate the sections of a broadcast image.
struct ArenaLayout {
    size_t psi, psi_sh, ipsi, ipsi_sh, mono, mono_sh, eidx, bsk, bsk_sh, ksk, kskb, total;
    size_t bsk_words, ksk_words, ksk_rows, n_pad;
};

ArenaLayout arena_layout(const tfhe_params& p, int word_bits) {
    ArenaLayout L{};
    const size_t wb = word_bits / 8, N = p.N;
    const size_t kb = ksk_bits_for(p.qKS) / 8;
    L.bsk_words = (size_t)p.n * 2 * p.dG2 * 2 * N;
    L.ksk_rows = (size_t)N * p.baseKS * p.dKS;
    const size_t vec = 16 / kb;  // KSK row padded to a multiple of 16 bytes
    L.n_pad = (p.n + vec - 1) / vec * vec;
    L.ksk_words = L.ksk_rows * (p.n + 1);  // caller's layout (B at index n)
    size_t o = 0;
    L.psi = o; o = align_up(o + N * wb);
    L.psi_sh = o; o = align_up(o + N * wb);
    L.ipsi = o; o = align_up(o + N * wb);
    L.ipsi_sh = o; o = align_up(o + N * wb);
    L.mono = o; o = align_up(o + 2 * N * wb);
    L.mono_sh = o; o = align_up(o + 2 * N * wb);
    L.eidx = o; o = align_up(o + N * 4);
    L.bsk = o; o = align_up(o + L.bsk_words * wb);
    L.bsk_sh = o; o = align_up(o + L.bsk_words * wb);
    L.ksk = o; o = align_up(o + L.ksk_rows * L.n_pad * kb);
    L.kskb = o; o = align_up(o + L.ksk_rows * kb);
    L.total = o;
    return L;
}

struct Scratch {
    uint64_t* acc = nullptr;  // [cap][2][N]
    uint64_t* a = nullptr;    // [cap][n]
    uint64_t* ext = nullptr;  // [cap][N+1]
    uint64_t* lwe[6] = {};    // [cap][n+1] each
    void* ks = nullptr;       // tiled key switch: digit planes (ks_tiled_scratch_bytes) for ks_cap
    size_t ks_cap = 0;
    size_t cap = 0;
    uint64_t* io = nullptr;   // host-array staging: in1 | in2 | out
    size_t io_words = 0;
    void* pk = nullptr;       // the same arrays in the narrow wire format (u16 / u32 words)
    size_t pk_bytes = 0;
};

// A device has a compute stream (`stream`, scratch `sc`) and a copy stream (`stream2`):
// host-array calls pipeline their sub-batches' PCIe copies on the copy stream against the
// kernels on the compute stream, through two device I/O sets (sc.io, sc2.io).  Device-pointer
// entry points use the compute scratch on the caller's stream (or `stream`).
struct Device {
    int id = 0;
    hipStream_t stream = nullptr;
    unsigned char* arena = nullptr;
    void* bsk_fast = nullptr;
    void* keys_f64 = nullptr;  // exact-FP64 path: centred double tables + BSK
    void* keys_sf = nullptr;   // special-form path: W1 = w 2^32 mod Q of the arena's tables and BSK, factor rows
    void* ks40 = nullptr;      // split-word key-switch records of 8-byte keys (ks_tiled.hip k_pack_ks40)
    DuoDev duo;                // two-workgroup forms (sf2duo, f64wduo): exchange buffers, wait deadline, co-resident
                               // pairs, launch fence (duo.hpp DuoDev; alloc_duo)
    Scratch sc;
    DevTables tables{};
    hipStream_t stream2 = nullptr;  // copy stream of the host-array runner
    Scratch sc2;                    // only its io set is used
    void* pin[2] = {};               // pinned staging blocks for the host-array API
    hipEvent_t pin_ev[2] = {};       // last DMA that used each block
    // Lane 0's scratch (sc) is shared by the host-array path (on `stream`) and the
    // device-resident entry points (on the caller's stream): every user of sc waits on
    // this event before its first kernel and records it after its last one, so work
    // queued on different streams never overlaps on the same scratch.
    hipEvent_t sc_fence = nullptr;
    hipEvent_t h2d_ev[2] = {};  // host-array runner: input of I/O set k landed
    hipEvent_t k_ev[2] = {};    // host-array runner: kernels that use I/O set k done
    // Completion flags of the host-array EvalAcc (d2h_flagged): pinned host words, 4 per ciphertext,
    // set by the blind rotation's waves; br_done.flags is non-null only while such a call queues its op.
    uint32_t* flags = nullptr;
    size_t flags_words = 0;
    BRDone br_done{};
    // Wire store of the circuit path (dev_circuit): [bootstraps][instances][n+1] words, every bootstrap's
    // result of one run.  Grow-only, resized only behind sc_fence (ensure_wires), used inside the
    // run_device_op frame like the scratch.
    uint64_t* wires = nullptr;
    size_t wires_words = 0;
    // The matrix product's stores, under the wire store's rules (ensure_words): the signed entries' residues,
    // K cols words (k_mm_reduce_matrix), and the dense layer's pre-activation z, instances cols (n+1) words.
    uint64_t* mm_mat = nullptr;
    size_t mm_mat_words = 0;
    uint64_t* dense_z = nullptr;
    size_t dense_z_words = 0;
    // The pooling layer's stores (dev_pool2d): the results that are not outputs, instances c slots (n+1) words,
    // under the same rules; and the uploaded plans, one per descriptor, written once and freed only by hipFree
    // (which waits for the kernels still reading them): at most kPoolPlans, the oldest evicted.
    uint64_t* pool_slots = nullptr;
    size_t pool_slots_words = 0;
    struct PoolPlanDev {
        PoolGeom g{};
        PoolRec* recs = nullptr;          // device: the plan's records
        std::vector<size_t> round_first;  // PoolPlan::round_first
        size_t copies = 0, slots = 0, widest = 0;
    };
    std::vector<PoolPlanDev> pool_plans;
    // The class table of a call with one table per channel (dev_func_tables): 2 words per table, under the wire
    // store's rules, written only when the call's tables are of more than one class.
    uint64_t* tab_meta = nullptr;
    size_t tab_meta_words = 0;
};
constexpr size_t kPoolPlans = 16;

// hipMalloc'd buffer owned by one scope (error paths free it too)
struct DevBuf {
    void* p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() {
        if (p) hipFree(p);
    }
    template <typename T>
    T* as() const {
        return static_cast<T*>(p);
    }
};

// drains a stream when its scope ends, so that the DevBufs declared before it free memory no kernel still uses
struct Drain {
    hipStream_t s;
    ~Drain() { hipStreamSynchronize(s); }
};

constexpr size_t kStageBytes = (size_t)8 << 20;

}  // namespace

struct tfhe_ctx;
namespace {
void free_device(Device& d);
}

struct tfhe_ctx {
    tfhe_params p{};
    int word_bits = 64;
    int ksk_bits = 64;
    bool use_fast = false;
    bool use_f64 = false;
    bool f64_fold = false;  // exact-FP64 kernel with the top digit's transforms eliminated
    bool use_sf = false;    // special-form u64 kernel (logQ / arbFunc contexts, default)
    BRParams br{};
    KSParams ks{};
    ArenaLayout layout{};
    std::vector<Device> devs;
    std::atomic<uint64_t> bootstraps{0};
    std::atomic<uint64_t> pair_launches{0};  // blind rotations launched on fast4's pair instance (tfhe_get_pair_min)
    int replicate_method = TFHE_REPLICATE_NONE;
    double replicate_ms = 0;
    size_t max_chunk = 65536;  // the reference's max_bootstapping_num, bootstrapping.cuh:140
    Knobs kn{};                // launch choices: environment at setup, tfhe_set_knobs afterwards
    std::string rccl_lib;      // TFHE_RCCL_LIB at setup ("" = the system librccl)
    ~tfhe_ctx();  // frees every device's arena, scratch, streams (error paths included)
};

namespace {

// ---------------------------------------------------------------------------
// setup helpers
// ---------------------------------------------------------------------------
// Launch knobs from the environment, once per context (tfhe_setup*): the A/B switches of earlier rounds'
// measurements.  Afterwards only tfhe_set_knobs changes them; no launch reads the environment.
// The range every knob must lie in (tfhe_set_knobs and the environment alike); nullptr when valid.
const char* knob_out_of_range(const Knobs& k) {
    if (k.ks_tiled_min < -1) return "ks_tiled_min (TFHE_KS_TILED_MIN) < -1";
    if (k.ks_cts < 0 || k.ks_cts > 4 || k.ks_cts == 3) return "ks_cts (TFHE_KS_CTS) not 0, 1, 2 or 4";
    if (k.ks_split < 1) return "ks_split (TFHE_KS_SPLIT) < 1";
    if (k.host_parts < 1) return "host_parts (TFHE_HOST_PARTS) < 1";
    if (k.generic < 0 || k.generic > 2) return "generic (TFHE_GENERIC) not in 0..2";
    if (k.duo < 0 || k.duo > 256) return "duo (TFHE_DUO) not in 0..256";
    if (k.split4 < 0) return "split4 (TFHE_SPLIT4) < 0";
    if (k.pair_min < 0) return "pair_min (TFHE_PAIR_MIN) < 0";
    if (k.f64w != 1) return "f64w (TFHE_F64W): the slot-layout FP64 kernel it selected was retired in round 5 (must be 1)";
    for (int32_t v : {k.ks_pk, k.wire, k.acc_flags, k.sf2, k.sf2p, k.trace, k.ks40})
        if (v < 0 || v > 1) return "a 0/1 knob (TFHE_KS_PK, TFHE_WIRE, TFHE_ACC_FLAGS, TFHE_SF2, TFHE_SF2P, TFHE_KS40) "
                                   "not 0 or 1";
    if (k.probe < 0) return "probe < 0";
    return nullptr;
}

// bad: the first variable that is not a whole number, or whose value is out of range
Knobs knobs_from_env(std::string& bad) {
    Knobs k;
    auto num = [&bad](const char* name, int32_t& dst) {
        const char* e = std::getenv(name);
        if (!e || !e[0]) return;
        char* end = nullptr;
        const long v = std::strtol(e, &end, 10);
        if (*end != '\0' || v < INT32_MIN || v > INT32_MAX) {
            if (bad.empty()) bad = std::string(name) + "=" + e + " is not a whole number";
            return;
        }
        dst = (int32_t)v;
    };
    num("TFHE_KS_TILED_MIN", k.ks_tiled_min);
    num("TFHE_KS_CTS", k.ks_cts);
    num("TFHE_KS_SPLIT", k.ks_split);
    num("TFHE_KS_PK", k.ks_pk);
    num("TFHE_HOST_PARTS", k.host_parts);
    num("TFHE_WIRE", k.wire);
    num("TFHE_ACC_FLAGS", k.acc_flags);
    {  // retired (round 5): scripts of earlier rounds export TFHE_F64W=0 / 1; accepted and ignored with a
       // warning rather than failing contexts that never touch the FP64 kernel.  tfhe_set_knobs
       // still requires 1.
        int32_t f = 1;
        num("TFHE_F64W", f);
        if (f != 1 && bad.empty())
            std::fprintf(stderr, "[tfhe] TFHE_F64W=%d ignored: the slot-layout FP64 kernel it selected was retired in "
                                 "round 5 (f64w is the only FP64 form)\n", (int)f);
    }
    num("TFHE_SF2", k.sf2);
    num("TFHE_DUO", k.duo);
    num("TFHE_SF2P", k.sf2p);
    num("TFHE_SPLIT4", k.split4);
    num("TFHE_PAIR_MIN", k.pair_min);
    num("TFHE_KS40", k.ks40);
    num("TFHE_GENERIC", k.generic);
    if (const char* e = std::getenv("TFHE_GENERIC_V1"); e && e[0] == '1') k.generic = 1;    // round-3 names
    if (const char* e = std::getenv("TFHE_GENERIC_GEN3"); e && e[0] == '0') k.generic = 2;
    k.trace = std::getenv("TFHE_TRACE") != nullptr;
    if (const char* why = knob_out_of_range(k); why && bad.empty()) bad = why;
    return k;
}

tfhe_status init_derived(tfhe_ctx* c) {
    const tfhe_params& p = c->p;
    std::string bad;
    c->kn = knobs_from_env(bad);
    if (!bad.empty()) return fail(TFHE_ERR_INVALID_ARGUMENT, "launch knob from the environment: " + bad);
    c->word_bits = word_bits_for(p);
    c->ksk_bits = ksk_bits_for(p.qKS);
    c->layout = arena_layout(p, c->word_bits);
    c->br.N = p.N;
    c->br.logN = ilog2(p.N);
    c->br.n = p.n;
    c->br.dG2 = p.dG2;
    c->br.digits = p.digitsG - p.numDigitsToThrow;
    c->br.thr = p.numDigitsToThrow;
    c->br.logG = ilog2(p.baseG);
    c->br.Q = p.Q;
    c->br.r1 = c->word_bits == 32 ? (uint64_t)((((u128)1) << 32) / p.Q) : (uint64_t)((((u128)1) << 64) / p.Q);
    c->ks.N = p.N;
    c->ks.n = p.n;
    c->ks.baseKS = p.baseKS;
    c->ks.dKS = p.dKS;
    c->ks.Q = p.Q;
    c->ks.qKS = p.qKS;
    c->ks.n_pad = (uint32_t)c->layout.n_pad;
    const char* force = std::getenv("TFHE_FORCE_GENERIC");
    c->use_fast = fast_path_supported(c->br, c->word_bits) && !(force && force[0] == '1');
    c->use_f64 = f64_path_supported(c->br, c->word_bits) && !(force && force[0] == '1');
    c->f64_fold = c->use_f64 && f64_fold_enabled(c->br);
    if (c->use_f64 && !f64_instance_available(c->br, c->f64_fold)) c->f64_fold = false;
    if (c->use_f64 && !f64_instance_available(c->br, c->f64_fold)) c->use_f64 = false;
    // Q = 2^54 - c: the special-form kernel (TFHE_SF=0 keeps the Shoup gen3 kernel)
    const char* sfe = std::getenv("TFHE_SF");
    c->use_sf = !c->use_fast && !c->use_f64 && sf_path_supported(c->br, c->word_bits) &&
                !(force && force[0] == '1') && !(sfe && sfe[0] == '0');
    if (p.Q >= (1ull << 58) || (c->word_bits == 64 && (u128)2 * p.dG2 * p.Q >= ((u128)1 << 64)))
        return fail(TFHE_ERR_UNSUPPORTED, "modulus too large for lazy accumulation");
    if (p.baseKS > 256) return fail(TFHE_ERR_UNSUPPORTED, "baseKS > 256 not supported");
    return TFHE_OK;
}

template <typename W>
void fill_words(std::vector<unsigned char>& host, size_t off, const uint64_t* src, size_t count) {
    W* dst = reinterpret_cast<W*>(host.data() + off);
    const size_t blk = 1 << 16;
    parallel_for((count + blk - 1) / blk, [&](size_t b) {
        for (size_t i = b * blk; i < std::min(count, (b + 1) * blk); ++i) dst[i] = (W)src[i];
    });
}

template <typename W>
void fill_companions(std::vector<unsigned char>& host, size_t off, const uint64_t* src, size_t count, uint64_t Q) {
    W* dst = reinterpret_cast<W*>(host.data() + off);
    const int bits = sizeof(W) * 8;
    const size_t blk = 1 << 14;
    parallel_for((count + blk - 1) / blk, [&](size_t b) {
        for (size_t i = b * blk; i < std::min(count, (b + 1) * blk); ++i) dst[i] = (W)shoup_companion(src[i], Q, bits);
    });
}

// KSK [rows][n+1] -> A part [rows][n_pad] (zero padded) + B part [rows]
template <typename W>
void pack_ksk(std::vector<unsigned char>& img, const ArenaLayout& L, uint32_t n, const uint64_t* ksk) {
    W* A = reinterpret_cast<W*>(img.data() + L.ksk);
    W* Bp = reinterpret_cast<W*>(img.data() + L.kskb);
    const size_t blk = 4096;
    parallel_for((L.ksk_rows + blk - 1) / blk, [&](size_t b) {
        for (size_t r = b * blk; r < std::min(L.ksk_rows, (b + 1) * blk); ++r) {
            const uint64_t* src = ksk + r * (n + 1);
            W* dst = A + r * L.n_pad;
            for (uint32_t k = 0; k < n; ++k) dst[k] = (W)src[k];
            for (size_t k = n; k < L.n_pad; ++k) dst[k] = 0;
            Bp[r] = (W)src[n];
        }
    });
}

// The table sections of the key image (psi, ipsi, mono with their companions, eidx: everything below L.bsk)
// and, when bsk_ntt is given, the NTT-domain BSK with its companions.
tfhe_status fill_table_image(tfhe_ctx* c, const NttTables& t, const uint64_t* bsk_ntt, std::vector<unsigned char>& img) {
    const tfhe_params& p = c->p;
    const ArenaLayout& L = c->layout;
    auto put = [&](auto tag, size_t off, size_t off_sh, const uint64_t* v, size_t count) {
        using W = decltype(tag);
        fill_words<W>(img, off, v, count);
        if (off_sh != (size_t)-1) fill_companions<W>(img, off_sh, v, count, p.Q);
    };
    if (c->word_bits == 32) {
        put(uint32_t{}, L.psi, L.psi_sh, t.psi_br.data(), p.N);
        put(uint32_t{}, L.ipsi, L.ipsi_sh, t.ipsi_br.data(), p.N);
        put(uint32_t{}, L.mono, L.mono_sh, t.mono.data(), 2ull * p.N);
        if (bsk_ntt) put(uint32_t{}, L.bsk, L.bsk_sh, bsk_ntt, L.bsk_words);
    } else {
        put(uint64_t{}, L.psi, L.psi_sh, t.psi_br.data(), p.N);
        put(uint64_t{}, L.ipsi, L.ipsi_sh, t.ipsi_br.data(), p.N);
        put(uint64_t{}, L.mono, L.mono_sh, t.mono.data(), 2ull * p.N);
        if (bsk_ntt) put(uint64_t{}, L.bsk, L.bsk_sh, bsk_ntt, L.bsk_words);
    }
    std::memcpy(img.data() + L.eidx, t.eidx.data(), sizeof(uint32_t) * p.N);
    if (c->use_fast)  // the fast kernel derives e_x = 2 bitrev(x) + 1 in registers
        for (uint32_t x = 0; x < p.N; ++x)
            if (t.eidx[x] != 2 * bitrev(x, t.logN) + 1) return fail(TFHE_ERR_INTERNAL, "eidx is not 2 bitrev(x) + 1");
    return TFHE_OK;
}

// Build the whole key image on the host (one-time, GPUSetup_core's job in the
// reference, bootstrapping.cu:874-1083).
tfhe_status build_host_image(tfhe_ctx* c, const uint64_t* bsk, bool bsk_eval, const uint64_t* ksk,
                             std::vector<unsigned char>& img) {
    const tfhe_params& p = c->p;
    const ArenaLayout& L = c->layout;
    img.assign(L.total, 0);
    NttTables t = make_ntt_tables(p.Q, p.N);
    std::vector<uint64_t> bsk_ntt(L.bsk_words);
    if (!bsk_to_ntt_scaled(p, t, bsk, bsk_eval, bsk_ntt.data()))
        return fail(TFHE_ERR_INVALID_ARGUMENT, "evaluation-format BSK entry >= Q");
    SCHECK(fill_table_image(c, t, bsk_ntt.data(), img));
    // KSK: packed to the narrowest word holding qKS (reference keeps u64, bootstrapping.cu:963)
    const uint64_t qks = p.qKS;
    std::atomic<bool> bad{false};
    const size_t blk = 1 << 16;
    parallel_for((L.ksk_words + blk - 1) / blk, [&](size_t b) {
        for (size_t i = b * blk; i < std::min(L.ksk_words, (b + 1) * blk); ++i)
            if (ksk[i] >= qks) bad = true;
    });
    if (bad) return fail(TFHE_ERR_INVALID_ARGUMENT, "KSK entry >= qKS");
    if (c->ksk_bits == 16) pack_ksk<uint16_t>(img, L, p.n, ksk);
    else if (c->ksk_bits == 32) pack_ksk<uint32_t>(img, L, p.n, ksk);
    else pack_ksk<uint64_t>(img, L, p.n, ksk);
    return TFHE_OK;
}

void bind_tables(tfhe_ctx* c, Device& d) {
    const ArenaLayout& L = c->layout;
    d.tables.psi = d.arena + L.psi;
    d.tables.psi_sh = d.arena + L.psi_sh;
    d.tables.ipsi = d.arena + L.ipsi;
    d.tables.ipsi_sh = d.arena + L.ipsi_sh;
    d.tables.mono = d.arena + L.mono;
    d.tables.mono_sh = d.arena + L.mono_sh;
    d.tables.eidx = reinterpret_cast<const uint32_t*>(d.arena + L.eidx);
}

// The duo state of a device: the exchange buffer, the partner-wait deadline (kDuoWaitMs of the wall clock
// s_memrealtime reads), the pairs it holds co-resident (one duo workgroup per CU) and the launch fence
tfhe_status alloc_duo(Device& d) {
    HCHECK(hipMalloc(&d.duo.base, duo_bytes()));
    HCHECK(hipMemsetAsync(d.duo.base, 0, duo_bytes(), d.stream));
    int khz = 0, cus = 0;
    HCHECK(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, d.id));
    HCHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, d.id));
    d.duo.wait_ticks = (uint64_t)(khz > 0 ? khz : 100000) * kDuoWaitMs;
    d.duo.resident_pairs = (uint32_t)std::max(0, cus / 2);
    HCHECK(hipEventCreateWithFlags(&d.duo.fence, hipEventDisableTiming));
    d.duo.mu = new std::mutex;
    return TFHE_OK;
}

tfhe_status finish_device(tfhe_ctx* c, Device& d) {
    bind_tables(c, d);
    if (c->use_fast) {
        HCHECK(hipMalloc(&d.bsk_fast, bsk_fast_bytes(c->br)));
        HCHECK(launch_pack_bsk_fast(c->br, d.tables, d.arena + c->layout.bsk, d.bsk_fast, d.stream));
        HCHECK(hipStreamSynchronize(d.stream));
    }
    if (c->use_f64) {
        HCHECK(hipMalloc(&d.keys_f64, bsk_f64_bytes(c->br)));
        HCHECK(launch_pack_bsk_f64(c->br, d.tables, d.arena + c->layout.bsk, c->f64_fold, d.keys_f64, d.stream));
        if (f64_duo_form(c->br, c->f64_fold)) SCHECK(alloc_duo(d));
        HCHECK(hipStreamSynchronize(d.stream));
    }
    if (c->ksk_bits == 64 && ks40_bytes(c->ks) > 0) {  // the logQ contexts' KSK (qKS = 2^35) as split words
        HCHECK(hipMalloc(&d.ks40, ks40_bytes(c->ks)));
        HCHECK(launch_pack_ks40(c->ks, d.arena + c->layout.ksk, d.ks40, d.stream));
        HCHECK(hipStreamSynchronize(d.stream));
    }
    if (c->use_sf) {
        HCHECK(hipMalloc(&d.keys_sf, sf_bytes(c->br)));
        HCHECK(launch_pack_sf(c->br, d.tables, d.arena + c->layout.bsk, d.keys_sf, d.stream));
        if (c->br.digits == 1 || c->br.digits == 2) SCHECK(alloc_duo(d));  // sfduo<1> / sf2duo
        HCHECK(hipStreamSynchronize(d.stream));
    }
    return TFHE_OK;
}

void free_device(Device& d) {
    if (d.id < 0) return;
    hipSetDevice(d.id);
    if (d.sc_fence) hipEventSynchronize(d.sc_fence), hipEventDestroy(d.sc_fence);
    if (d.stream) hipStreamSynchronize(d.stream);
    hipFree(d.arena);
    hipFree(d.bsk_fast);
    hipFree(d.keys_f64);
    hipFree(d.keys_sf);
    hipFree(d.ks40);
    hipFree(d.wires);
    hipFree(d.mm_mat);
    hipFree(d.dense_z);
    hipFree(d.pool_slots);
    hipFree(d.tab_meta);
    for (auto& pp : d.pool_plans) hipFree(pp.recs);
    d.pool_plans.clear();
    hipFree(d.duo.base);
    if (d.duo.fence) hipEventDestroy(d.duo.fence);
    delete d.duo.mu;
    d.duo = DuoDev{};
    if (d.stream2) hipStreamSynchronize(d.stream2);
    for (Scratch* sc : {&d.sc, &d.sc2}) {
        hipFree(sc->acc);
        hipFree(sc->a);
        hipFree(sc->ext);
        for (auto* p : sc->lwe) hipFree(p);
        hipFree(sc->ks);
        hipFree(sc->io);
        hipFree(sc->pk);
    }
    if (d.flags) hipHostFree(d.flags);
    for (int k = 0; k < 2; ++k) {
        if (d.pin_ev[k]) hipEventSynchronize(d.pin_ev[k]), hipEventDestroy(d.pin_ev[k]);
        if (d.pin[k]) hipHostFree(d.pin[k]);
        if (d.h2d_ev[k]) hipEventDestroy(d.h2d_ev[k]);
        if (d.k_ev[k]) hipEventDestroy(d.k_ev[k]);
    }
    if (d.stream) hipStreamDestroy(d.stream);
    if (d.stream2) hipStreamDestroy(d.stream2);
    d = Device{};
    d.id = -1;
}

tfhe_status create_streams(Device& d) {
    HCHECK(hipStreamCreateWithFlags(&d.stream, hipStreamNonBlocking));
    HCHECK(hipStreamCreateWithFlags(&d.stream2, hipStreamNonBlocking));
    HCHECK(hipEventCreateWithFlags(&d.sc_fence, hipEventDisableTiming));
    return TFHE_OK;
}

// Order `s` after every earlier user of lane 0's scratch (see Device::sc_fence).
tfhe_status sc_acquire(Device& d, hipStream_t s) {
    HCHECK(hipStreamWaitEvent(s, d.sc_fence, 0));
    return TFHE_OK;
}
tfhe_status sc_release(Device& d, hipStream_t s) {
    HCHECK(hipEventRecord(d.sc_fence, s));
    return TFHE_OK;
}

// The context device holding device buffer p (the _device entry points' device index).
tfhe_status device_for(tfhe_ctx* c, const void* p, Device*& out) {
    if (c->devs.size() == 1) {  // nothing to choose: skip the query
        out = &c->devs[0];
        return TFHE_OK;
    }
    hipPointerAttribute_t at{};
    // (the runtime reports plain host memory as success + hipMemoryTypeUnregistered)
    if (hipPointerGetAttributes(&at, p) != hipSuccess || at.type == hipMemoryTypeUnregistered) {
        (void)hipGetLastError();
        return fail(TFHE_ERR_INVALID_ARGUMENT, "not a device buffer");
    }
    for (Device& d : c->devs)
        if (d.id == at.device) {
            out = &d;
            return TFHE_OK;
        }
    return fail(TFHE_ERR_INVALID_ARGUMENT, "buffer is on a device this context does not use");
}

tfhe_status ensure_scratch(tfhe_ctx* c, Device& d, size_t B) {
    if (B <= d.sc.cap) return TFHE_OK;
    const tfhe_params& p = c->p;
    if (d.sc_fence) HCHECK(hipEventSynchronize(d.sc_fence));  // no queued kernel still uses the old buffers
    const size_t cap = std::max(B, std::min(c->max_chunk, (size_t)1024));
    hipFree(d.sc.acc);
    hipFree(d.sc.a);
    hipFree(d.sc.ext);
    for (auto*& q : d.sc.lwe) hipFree(q), q = nullptr;
    hipFree(d.sc.ks);
    uint64_t* io = d.sc.io;
    const size_t io_words = d.sc.io_words;
    void* pk = d.sc.pk;
    const size_t pk_bytes = d.sc.pk_bytes;
    d.sc = Scratch{};
    d.sc.io = io, d.sc.io_words = io_words, d.sc.pk = pk, d.sc.pk_bytes = pk_bytes;
    HCHECK(hipMalloc(&d.sc.acc, cap * 2 * p.N * sizeof(uint64_t)));
    HCHECK(hipMalloc(&d.sc.a, cap * p.n * sizeof(uint64_t)));
    HCHECK(hipMalloc(&d.sc.ext, cap * (p.N + 1) * sizeof(uint64_t)));
    for (auto*& q : d.sc.lwe) HCHECK(hipMalloc(&q, cap * (p.n + 1) * sizeof(uint64_t)));
    if (ks_tiled_supported(c->ks)) {
        HCHECK(hipMalloc(&d.sc.ks, ks_tiled_scratch_bytes(c->ks, cap)));
        d.sc.ks_cap = cap;
    }
    d.sc.cap = cap;
    return TFHE_OK;
}

size_t ks_tiled_min(const tfhe_ctx* c);

// The tiled key switch's digit planes alone, for the device-resident key switch (which needs
// none of the bootstrap scratch): grown to B only when the tiled form will run.
tfhe_status ensure_ks_scratch(tfhe_ctx* c, Device& d, size_t B) {
    const size_t tmin = ks_tiled_min(c);
    if (!ks_tiled_supported(c->ks) || tmin == 0 || B < tmin || B <= d.sc.ks_cap) return TFHE_OK;
    if (d.sc_fence) HCHECK(hipEventSynchronize(d.sc_fence));
    hipFree(d.sc.ks);
    d.sc.ks = nullptr, d.sc.ks_cap = 0;
    HCHECK(hipMalloc(&d.sc.ks, ks_tiled_scratch_bytes(c->ks, B)));
    d.sc.ks_cap = B;
    return TFHE_OK;
}

// ---------------------------------------------------------------------------
// device pipelines (one device, one stream, B <= scratch capacity)
// ---------------------------------------------------------------------------
tfhe_status dev_blind_rotate(tfhe_ctx* c, Device& d, const uint64_t* a, uint64_t amod, uint64_t* acc, size_t B) {
    if (amod == 0 || (2ull * c->p.N) % amod != 0) return fail(TFHE_ERR_INVALID_ARGUMENT, "a-modulus must divide 2N");
    const ArenaLayout& L = c->layout;
    if (c->use_fast && (amod & (amod - 1)) == 0) {
        bool paired = false;
        HCHECK(launch_blind_rotate_fast(c->br, d.tables, d.bsk_fast, a, amod, acc, B, d.stream,
                                        d.br_done.flags ? &d.br_done : nullptr, c->kn.split4, c->kn.pair_min, &paired));
        if (paired) c->pair_launches.fetch_add(1, std::memory_order_relaxed);
    } else if (c->use_f64) {
        HCHECK(launch_blind_rotate_f64(c->br, d.tables, d.keys_f64, c->f64_fold, a, amod, acc, B, d.stream, c->kn,
                                       d.duo.base ? &d.duo : nullptr));
    } else if (c->use_sf) {
        HCHECK(launch_blind_rotate_sf(c->br, d.tables, d.arena + L.bsk, d.keys_sf, a, amod, acc, B, d.stream, c->kn,
                                      d.duo.base ? &d.duo : nullptr));
    } else {
        HCHECK(launch_blind_rotate_generic(c->word_bits, c->br, d.tables, d.arena + L.bsk, d.arena + L.bsk_sh, a,
                                           amod, acc, B, d.stream, c->kn));
    }
    c->bootstraps += B;
    return TFHE_OK;
}

// Smallest batch that takes the tiled key switch (knob ks_tiled_min / TFHE_KS_TILED_MIN; 0 = never).
// Round 2 set it at 4096 (u16 keys) / 256 (wider keys): the tiled workgroups each swept all N dKS rows
// (~1 ms for STD128 at any batch up to 8192).
size_t ks_tiled_min(const tfhe_ctx* c) {
    if (c->kn.ks_tiled_min >= 0) return (size_t)c->kn.ks_tiled_min;  // knob (TFHE_KS_TILED_MIN)
    // round 4 (profiles/r04b/ks_sweep.log): with the steps split up to 16 ways at small batches, the tiled
    // form beats the gather at every batch from 1 to 1024 and every key width (STD128Q B = 128: 0.33 vs
    // 6.3 ms; logQ = 23: 1.68 vs 9.3 ms; STD128 B = 1: 0.105 vs 0.64 ms); the gather stays for key
    // shapes the tiled form does not support
    return 1;
}

// the tiled form runs when d.sc.ks holds B ciphertexts (ensure_scratch / ensure_ks_scratch)
tfhe_status dev_mkm(tfhe_ctx* c, Device& d, const uint64_t* ext, uint64_t fmod, uint64_t* out, size_t B) {
    if (fmod < 2) return fail(TFHE_ERR_INVALID_ARGUMENT, "fmod < 2");
    const size_t tmin = ks_tiled_min(c);
    if (tmin && B >= tmin && d.sc.ks && B <= d.sc.ks_cap) {
        const hipError_t e = launch_ks_tiled(c->ks, c->ksk_bits, d.arena + c->layout.ksk, d.arena + c->layout.kskb,
                                             ext, fmod, out, B, d.sc.ks, d.stream, c->kn, d.ks40);
        if (e != hipErrorNotSupported) {
            HCHECK(e);
            return TFHE_OK;
        }
    }
    HCHECK(launch_mkm(c->ks, c->ksk_bits, d.arena + c->layout.ksk, d.arena + c->layout.kskb, ext, fmod, out, B,
                      d.stream));
    return TFHE_OK;
}

// BootstrapFunc / BootstrapGate on device: ct[B][n+1] mod tv.ctmod -> out mod fmod
// sel: the table modes read tv.lut[T][q] through it (one table per channel, dev_func_tables)
tfhe_status dev_bootstrap(tfhe_ctx* c, Device& d, TvParams tv, uint64_t b_add, const uint64_t* ct, uint64_t* out,
                          size_t B, const TabSel* sel = nullptr) {
    tv.N = c->p.N;
    tv.n = c->p.n;
    tv.Q = c->p.Q;
    tv.Q8 = c->p.Q / 8 + 1;
    if ((2ull * c->p.N) % tv.ctmod != 0) return fail(TFHE_ERR_INVALID_ARGUMENT, "ciphertext modulus must divide 2N");
    if (sel && tv.mode != TV_HALF) HCHECK(launch_build_testvector_tab(tv, *sel, ct, d.sc.acc, d.sc.a, B, d.stream));
    else HCHECK(launch_build_testvector(tv, ct, d.sc.acc, d.sc.a, B, d.stream));
    SCHECK(dev_blind_rotate(c, d, d.sc.a, tv.ctmod, d.sc.acc, B));
    HCHECK(launch_extract(c->p.N, c->p.Q, b_add, d.sc.acc, d.sc.ext, B, d.stream));
    return dev_mkm(c, d, d.sc.ext, tv.fmod, out, B);
}

uint64_t gate_const(int gate, uint64_t q) {  // rgsw-cryptoparameters.h:130-137
    static const uint64_t k[] = {5, 7, 1, 3, 5, 1};
    return k[gate] * (q >> 3);
}

// vector EvalBinGate, binfhe-base-scheme.cpp:598-677.  Uses lwe[0..2] + lwe[5].
tfhe_status dev_gate(tfhe_ctx* c, Device& d, int gate, const uint64_t* ct1, const uint64_t* ct2, uint64_t q,
                     uint64_t* out, size_t B) {
    const uint32_t n = c->p.n;
    hipStream_t s = d.stream;
    if (gate == TFHE_XOR || gate == TFHE_XNOR) {
        uint64_t *n1 = d.sc.lwe[3], *n2 = d.sc.lwe[4], *t1 = d.sc.lwe[5];
        HCHECK(launch_lwe_op(LWE_NOT, n, q, 0, ct1, nullptr, n1, B, s));
        HCHECK(launch_lwe_op(LWE_NOT, n, q, 0, ct2, nullptr, n2, B, s));
        SCHECK(dev_gate(c, d, TFHE_AND, ct1, n2, q, t1, B));   // AND(ct1, NOT ct2)
        SCHECK(dev_gate(c, d, TFHE_AND, n1, ct2, q, n2, B));   // AND(NOT ct1, ct2)
        SCHECK(dev_gate(c, d, TFHE_OR, t1, n2, q, out, B));
        if (gate == TFHE_XNOR) HCHECK(launch_lwe_op(LWE_NOT, n, q, 0, out, nullptr, out, B, s));
        return TFHE_OK;
    }
    uint64_t* prep = d.sc.lwe[0];
    HCHECK(launch_lwe_op((gate == TFHE_XOR_FAST || gate == TFHE_XNOR_FAST) ? LWE_DOUBLE_SUB : LWE_ADD, n, q, 0, ct1,
                         ct2, prep, B, s));
    TvParams tv{};
    tv.mode = TV_GATE;
    tv.ctmod = q;
    tv.fmod = q;
    tv.q1 = gate_const(gate, q);
    tv.q2 = addmod(tv.q1, q >> 1, q);
    return dev_bootstrap(c, d, tv, c->p.Q / 8 + 1, prep, out, B);
}

// vector EvalFunc, binfhe-base-scheme.cpp:679-924.  d_lut is a device LUT ([q] or [B][q]); with sel, [T][q] of
// class `prop` wherever sel points.
tfhe_status dev_func(tfhe_ctx* c, Device& d, int prop, const uint64_t* ct, uint64_t q, const uint64_t* d_lut,
                     uint64_t lut_stride, uint64_t* out, size_t B, const TabSel* sel = nullptr) {
    const uint32_t n = c->p.n;
    const uint64_t beta = 128;
    hipStream_t s = d.stream;
    uint64_t *ct1 = d.sc.lwe[0], *ct2 = d.sc.lwe[1], *ct3 = d.sc.lwe[2];
    TvParams tv{};
    tv.lut = d_lut;
    tv.lut_stride = lut_stride;
    tv.lut_len = q;
    if (prop == 0) {  // negacyclic: one bootstrap
        HCHECK(launch_lwe_op(LWE_ADD_CONST, n, q, beta, ct, nullptr, ct1, B, s));
        tv.mode = TV_LUT;
        tv.ctmod = q;
        tv.fmod = q;
        return dev_bootstrap(c, d, tv, 0, ct1, out, B, sel);
    }
    if (prop == 2) {  // arbitrary: raise to 2q, two bootstraps
        if (q > c->p.N) return fail(TFHE_ERR_UNSUPPORTED, "arbitrary function needs q <= N");
        const uint64_t dq = q << 1;
        HCHECK(launch_lwe_op(LWE_ADD_CONST, n, dq, beta, ct, nullptr, ct2, B, s));
        tv.mode = TV_HALF;
        tv.ctmod = dq;
        tv.fmod = dq;
        SCHECK(dev_bootstrap(c, d, tv, 0, ct2, ct3, B));
        HCHECK(launch_lwe_op(LWE_SUB, n, dq, 0, ct, ct3, ct3, B, s));  // EvalSubEq2(ct1, ct3)
        HCHECK(launch_lwe_op(LWE_ADD_CONST, n, dq, beta, ct3, nullptr, ct3, B, s));
        HCHECK(launch_lwe_op(LWE_SUB_CONST, n, dq, q >> 1, ct3, nullptr, ct3, B, s));
        tv.mode = TV_LUT2;
        SCHECK(dev_bootstrap(c, d, tv, 0, ct3, out, B, sel));
        HCHECK(launch_lwe_op(LWE_SET_MOD, n, q, 0, out, nullptr, out, B, s));
        return TFHE_OK;
    }
    // periodic
    HCHECK(launch_lwe_op(LWE_ADD_CONST, n, q, beta, ct, nullptr, ct1, B, s));
    tv.mode = TV_HALF;
    tv.ctmod = q;
    tv.fmod = q;
    SCHECK(dev_bootstrap(c, d, tv, 0, ct1, ct2, B));
    HCHECK(launch_lwe_op(LWE_SUB, n, q, 0, ct, ct2, ct2, B, s));  // EvalSubEq2(ct, ct2)
    HCHECK(launch_lwe_op(LWE_ADD_CONST, n, q, beta, ct2, nullptr, ct2, B, s));
    HCHECK(launch_lwe_op(LWE_SUB_CONST, n, q, q >> 2, ct2, nullptr, ct2, B, s));
    tv.mode = TV_LUT1;
    return dev_bootstrap(c, d, tv, 0, ct2, out, B, sel);
}

// ---------------------------------------------------------------------------
// EvalFunc with one table per channel: ciphertext i of a flat batch uses table (i / inner) mod T
// ---------------------------------------------------------------------------
// The tables of one call, classified one by one on the host.  meta[t] = {class, class-0 / 1 / 2 tables below t}.
// T = 0: one table [q] shared by every ciphertext, classified like a first table (its class is cls[0], so
// classes = 1); no index rule applies and dev_func_tables runs plain dev_func.
struct TabCall {
    const uint64_t* d_luts = nullptr;  // device [max(T, 1)][q]
    size_t T = 0;
    std::vector<uint8_t> cls;    // [max(T, 1)]
    std::vector<uint32_t> meta;  // [max(T, 1)][4]
    uint64_t ntab[3] = {};
    int classes = 0;             // how many of the three are present
    const uint4* d_meta = nullptr;  // Device::tab_meta, uploaded by tab_upload when classes > 1
};

void tab_classify(TabCall& tc, const uint64_t* luts, size_t T, uint64_t q) {
    const size_t count = std::max<size_t>(T, 1);
    tc.T = T;
    tc.cls.resize(count);
    tc.meta.resize(4 * count);
    for (size_t t = 0; t < count; ++t) {
        const int k = check_input_function(luts + t * q, q, q);
        tc.cls[t] = (uint8_t)k;
        tc.meta[4 * t] = (uint32_t)k;
        for (int j = 0; j < 3; ++j) tc.meta[4 * t + 1 + j] = (uint32_t)tc.ntab[j];
        ++tc.ntab[k];
    }
    tc.classes = (tc.ntab[0] != 0) + (tc.ntab[1] != 0) + (tc.ntab[2] != 0);
}

// ciphertexts of each class below index i of the whole batch (k_tab_move computes the same number)
void tab_count(const TabCall& tc, uint64_t inner, uint64_t i, uint64_t n[3]) {
    const uint64_t period = inner * tc.T, p = i / period, r = i - p * period, t = r / inner, within = r - t * inner;
    for (int k = 0; k < 3; ++k) n[k] = p * inner * tc.ntab[k] + inner * tc.meta[4 * t + 1 + k];
    n[tc.cls[t]] += within;
}

// the class table on the device, inside the frame (the buffer is the scratch's: earlier users are done once the
// stream reaches the copy); the host waits, so tc may go out of scope and a later call may overwrite tc.meta
tfhe_status tab_upload(Device& d, TabCall& tc) {
    if (tc.classes < 2) return TFHE_OK;  // always so for a shared table (T = 0: one table, one class), so T >= 2 below
    HCHECK(hipMemcpyAsync(d.tab_meta, tc.meta.data(), tc.T * 16, hipMemcpyHostToDevice, d.stream));
    HCHECK(hipStreamSynchronize(d.stream));
    tc.d_meta = reinterpret_cast<const uint4*>(d.tab_meta);
    return TFHE_OK;
}

// One slice (B <= scratch capacity) whose row 0 is ciphertext `first` of the whole batch.  A slice of one class
// runs dev_func on the caller's rows with the table chosen by the index rule: no row is copied.  Otherwise the
// rows are gathered by class into lwe[3] (their tables into lwe[5]), each class present runs dev_func on its run
// of rows into lwe[4], and the results are scattered: 2 + at most 3 pipelines, whatever T and inner are.
// A shared table (T = 0) is plain dev_func: no index rule, no TabSel.
tfhe_status dev_func_tables(tfhe_ctx* c, Device& d, const TabCall& tc, uint64_t inner, uint64_t first,
                            const uint64_t* ct, uint64_t q, uint64_t* out, size_t B) {
    if (tc.T == 0) return dev_func(c, d, tc.cls[0], ct, q, tc.d_luts, 0, out, B);
    uint64_t lo[3], hi[3];
    tab_count(tc, inner, first, lo);
    tab_count(tc, inner, first + B, hi);
    int present = 0, only = 0;
    for (int k = 0; k < 3; ++k)
        if (hi[k] != lo[k]) ++present, only = k;
    if (present == 1) {
        const TabSel sel{nullptr, first, inner, tc.T};
        return dev_func(c, d, only, ct, q, tc.d_luts, 0, out, B, &sel);
    }
    const size_t w = c->p.n + 1;
    uint64_t *rows = d.sc.lwe[3], *res = d.sc.lwe[4];
    uint32_t* ids = reinterpret_cast<uint32_t*>(d.sc.lwe[5]);
    TabMove mv{};
    mv.meta = tc.d_meta, mv.first = first, mv.count = B, mv.inner = inner, mv.T = tc.T, mv.width = (uint32_t)w;
    uint64_t base = 0;
    for (int k = 0; k < 3; ++k) mv.ntab[k] = tc.ntab[k], mv.lo[k] = lo[k], mv.base[k] = base, base += hi[k] - lo[k];
    HCHECK(launch_tab_gather(mv, ct, rows, ids, d.stream));
    for (int k = 0; k < 3; ++k) {
        const size_t cnt = hi[k] - lo[k], at = mv.base[k];
        if (cnt == 0) continue;
        const TabSel sel{ids + at, 0, inner, tc.T};
        SCHECK(dev_func(c, d, k, rows + at * w, q, tc.d_luts, 0, res + at * w, cnt, &sel));
    }
    HCHECK(launch_tab_scatter(mv, res, out, d.stream));
    return TFHE_OK;
}

// a whole flat batch in slices of the scratch; the table index is the index in the batch, not in the slice
tfhe_status dev_func_tables_batch(tfhe_ctx* c, Device& d, const TabCall& tc, uint64_t inner, const uint64_t* ct,
                                  uint64_t q, uint64_t* out, size_t total) {
    const size_t w = c->p.n + 1, slice = std::min(d.sc.cap, c->max_chunk);
    for (size_t first = 0; first < total; first += slice)
        SCHECK(dev_func_tables(c, d, tc, inner, first, ct + first * w, q, out + first * w, std::min(slice, total - first)));
    return TFHE_OK;
}

// vector EvalFloor, binfhe-base-scheme.cpp:926-987.  out may alias nothing; uses lwe[3], lwe[4].
tfhe_status dev_floor(tfhe_ctx* c, Device& d, const uint64_t* ct, uint64_t mod, uint32_t roundbits, uint64_t* out,
                      size_t B) {
    const uint32_t n = c->p.n;
    const uint64_t beta = 128;
    const uint64_t q = roundbits == 0 ? c->p.q : beta * 2 * (1ull << roundbits);
    hipStream_t s = d.stream;
    uint64_t *ctq = d.sc.lwe[3], *t = d.sc.lwe[4];
    HCHECK(launch_lwe_op(LWE_ADD_CONST, n, mod, beta, ct, nullptr, out, B, s));  // ct1
    HCHECK(launch_lwe_op(LWE_SET_MOD, n, q, 0, out, nullptr, ctq, B, s));
    TvParams tv{};
    tv.mode = TV_HALF;
    tv.ctmod = q;
    tv.fmod = mod;
    SCHECK(dev_bootstrap(c, d, tv, 0, ctq, t, B));
    HCHECK(launch_lwe_op(LWE_SUB, n, mod, 0, out, t, out, B, s));
    HCHECK(launch_lwe_op(LWE_SET_MOD, n, q, 0, out, nullptr, ctq, B, s));
    tv.mode = TV_FLOOR2;
    SCHECK(dev_bootstrap(c, d, tv, 0, ctq, t, B));
    HCHECK(launch_lwe_op(LWE_SUB, n, mod, 0, out, t, out, B, s));
    return TFHE_OK;
}

// vector EvalSign, binfhe-base-scheme.cpp:989-1037 (in: lwe[1] holds the input copy)
tfhe_status dev_sign(tfhe_ctx* c, Device& d, const uint64_t* ct, uint64_t mod, uint64_t* out, size_t B) {
    const uint32_t n = c->p.n;
    const uint64_t beta = 128, q = c->p.q;
    hipStream_t s = d.stream;
    uint64_t *tmp = d.sc.lwe[1], *fl = d.sc.lwe[2];
    HCHECK(hipMemcpyAsync(tmp, ct, B * (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
    while (mod > q) {
        SCHECK(dev_floor(c, d, tmp, mod, 0, fl, B));
        const uint64_t nm = mod / q * 2 * beta;
        HCHECK(launch_lwe_op(LWE_MODSWITCH, n, nm, mod, fl, nullptr, tmp, B, s));
        mod = nm;
    }
    HCHECK(launch_lwe_op(LWE_ADD_CONST, n, mod, beta, tmp, nullptr, tmp, B, s));
    TvParams tv{};
    tv.mode = TV_SIGN3;
    tv.ctmod = mod;
    tv.fmod = q;
    SCHECK(dev_bootstrap(c, d, tv, 0, tmp, out, B));
    HCHECK(launch_lwe_op(LWE_SUB_CONST, n, q, q >> 2, out, nullptr, out, B, s));
    return TFHE_OK;
}

// ---------------------------------------------------------------------------
// circuits (tfhe_circuit, circuit.cpp): every level is one mixed batch
// ---------------------------------------------------------------------------
// The wire store of a run: grow-only; no queued kernel uses the old buffer once sc_fence has passed
// (every user runs inside a run_device_op frame).  A failed allocation leaves the device without a store
// and the context usable.
tfhe_status ensure_words(Device& d, uint64_t*& buf, size_t& have, size_t words) {
    if (words <= have) return TFHE_OK;
    if (d.sc_fence) HCHECK(hipEventSynchronize(d.sc_fence));
    hipFree(buf);
    buf = nullptr, have = 0;
    HCHECK(hipMalloc(&buf, words * sizeof(uint64_t)));
    have = words;
    return TFHE_OK;
}
tfhe_status ensure_wires(Device& d, size_t words) { return ensure_words(d, d.wires, d.wires_words, words); }

// ---------------------------------------------------------------------------
// the matrix product and the dense layer on one device (inside run_device_op)
// ---------------------------------------------------------------------------
// out[i][c] = sum_k matrix[k][c] ct[i][k] (+ bias[c] on b) mod modulus; d.mm_mat holds K cols words
tfhe_status dev_mul_matrix(tfhe_ctx* c, Device& d, size_t instances, size_t K, const uint64_t* ct, size_t cols,
                           const int64_t* matrix, const uint64_t* bias, uint64_t modulus, uint64_t* out) {
    HCHECK(launch_mul_matrix(c->p.n + 1, instances, K, ct, cols, matrix, bias, modulus, d.mm_mat, out, d.stream));
    return TFHE_OK;
}

// z = W^T x + bias mod q into d.dense_z, then EvalFunc over the flat batch of instances cols ciphertexts in
// slices of the scratch, as dev_circuit slices a level.  tc: one shared table, or one per column (inner = 1)
tfhe_status dev_dense(tfhe_ctx* c, Device& d, size_t instances, size_t K, const uint64_t* ct, size_t cols,
                      const int64_t* matrix, const uint64_t* bias, uint64_t q, const TabCall& tc, uint64_t* out) {
    SCHECK(dev_mul_matrix(c, d, instances, K, ct, cols, matrix, bias, q, d.dense_z));
    return dev_func_tables_batch(c, d, tc, 1, d.dense_z, q, out, instances * cols);
}

// ---------------------------------------------------------------------------
// Conv2d and the convolution layer on one device (inside run_device_op)
// ---------------------------------------------------------------------------
// out[i][o][oy][ox] = sum over the window of weight[o] ct[i] (+ bias[o] on b) mod modulus, gathered in the kernel;
// d.mm_mat holds c_out K words
tfhe_status dev_conv2d(tfhe_ctx* c, Device& d, const ConvGeom& g, size_t instances, const uint64_t* ct,
                       const int64_t* weight, const uint64_t* bias, uint64_t modulus, uint64_t* out) {
    HCHECK(launch_conv2d(c->p.n + 1, g, instances, ct, weight, bias, modulus, d.mm_mat, out, d.stream));
    return TFHE_OK;
}

// z = conv(x) + bias mod q into d.dense_z, then EvalFunc over the flat batch of instances c_out oh ow ciphertexts
// in slices, as dev_dense.  tc: one shared table, or one per output plane (inner = oh ow)
tfhe_status dev_conv_layer(tfhe_ctx* c, Device& d, const ConvGeom& g, size_t instances, const uint64_t* ct,
                           const int64_t* weight, const uint64_t* bias, uint64_t q, const TabCall& tc, uint64_t* out) {
    SCHECK(dev_conv2d(c, d, g, instances, ct, weight, bias, q, d.dense_z));
    return dev_func_tables_batch(c, d, tc, (uint64_t)g.oh * g.ow, d.dense_z, q, out, instances * g.c_out * g.oh * g.ow);
}

// ---------------------------------------------------------------------------
// the pooling layer on one device (inside run_device_op)
// ---------------------------------------------------------------------------
// Round by round: the round's pairs over every instance and plane are one flat batch, item = plane nrec + record;
// per slice of the scratch, z = a - b into the first half of d.dense_z, EvalFunc into the second, dst = f + b into
// d.pool_slots or out.  A round reads inputs and earlier rounds' slots and writes fresh slots and outputs, so
// its slices are independent.  Positions with one valid tap are copied.  tc: one shared table, or one per plane
// (item = plane nrec + record, so inner is the round's nrec and the table is plane mod c).
tfhe_status dev_pool2d(tfhe_ctx* c, Device& d, const Device::PoolPlanDev& pp, size_t instances, const uint64_t* ct,
                       uint64_t q, const TabCall& tc, uint64_t* out) {
    const PoolGeom& g = pp.g;
    const size_t w = c->p.n + 1, planes = instances * g.c, slice = std::min(d.sc.cap, c->max_chunk);
    PoolArgs a{};
    a.width = (uint32_t)w, a.mask = q - 1;
    a.in = ct, a.in_plane = (size_t)g.h * g.w * w;
    a.slots = d.pool_slots, a.slot_plane = pp.slots * w;
    a.out = out, a.out_plane = (size_t)g.oh * g.ow * w;
    uint64_t *z = d.dense_z, *f = d.dense_z + std::min(planes * pp.widest, c->max_chunk) * w;
    for (size_t l = 0; l + 1 < pp.round_first.size(); ++l) {
        a.recs = pp.recs + pp.round_first[l];
        a.nrec = pp.round_first[l + 1] - pp.round_first[l];
        const size_t total = planes * a.nrec;
        for (a.first = 0; a.first < total; a.first += slice) {
            a.count = std::min(slice, total - a.first);
            HCHECK(launch_pool_diff(a, z, d.stream));
            SCHECK(dev_func_tables(c, d, tc, a.nrec, a.first, z, q, f, a.count));
            HCHECK(launch_pool_add(a, f, d.stream));
        }
    }
    if (pp.copies) {
        a.recs = pp.recs + pp.round_first.back();
        a.nrec = pp.copies, a.first = 0, a.count = planes * pp.copies;
        HCHECK(launch_pool_copy(a, d.stream));
    }
    return TFHE_OK;
}

// ---------------------------------------------------------------------------
// the product of two encrypted tensors on one device (inside run_device_op)
// ---------------------------------------------------------------------------
// out[o] = sum_k EvalFunc(x + y, table 0) - EvalFunc(x - y, table 1) over the products (o, k) of output
// o = (i rows + r) cols + c.  Slices of `slice` whole outputs, so no output is reduced across slices: the sums and
// the differences into the first half of d.dense_z, one EvalFunc batch of 2 count ciphertexts under tc's two tables
// (inner = count: the first half takes table 0, the second table 1) into the second half, the signed sum over k
// into out.  2 inner slice <= the scratch capacity and the chunk limit (ct_matmul_on_device).
tfhe_status dev_ct_matmul(tfhe_ctx* c, Device& d, const tfhe_ct_matmul& m, size_t instances, size_t slice,
                          const uint64_t* x, const uint64_t* y, uint64_t q, uint64_t* out, const TabCall& tc) {
    const size_t w = c->p.n + 1, total = instances * m.rows * m.cols;
    CtmmArgs a{};
    a.x = x, a.y = y, a.rows = m.rows, a.inner = m.inner, a.cols = m.cols;
    a.y_transposed = m.y_transposed, a.y_shared = m.y_shared;
    a.width = (uint32_t)w, a.mask = q - 1;
    for (a.first_out = 0; a.first_out < total; a.first_out += slice) {
        a.count = std::min(slice, total - a.first_out) * m.inner;
        uint64_t *z = d.dense_z, *f = d.dense_z + 2 * a.count * w;
        HCHECK(launch_ctmm_pairs(a, z, d.stream));
        SCHECK(dev_func_tables(c, d, tc, a.count, 0, z, q, f, 2 * a.count));
        HCHECK(launch_ctmm_reduce(a, f, out, d.stream));
    }
    return TFHE_OK;
}

void circuit_plan_free(int device, void* base) {
    int cur = 0;
    const bool have = hipGetDevice(&cur) == hipSuccess;
    if (hipSetDevice(device) == hipSuccess) hipFree(base);  // waits for the kernels still reading it
    if (have) hipSetDevice(cur);
}

// A compiled plan's arrays on HIP device d.id, one after the other in `parts` order (every part's size is a
// multiple of 8 bytes), uploaded on first use and kept with the circuit.  The copies are synchronous: complete
// before any kernel queued afterwards.
struct PlanPart {
    const void* p;
    size_t bytes;
};
tfhe_status plan_on_device(PlanCache& cache, Device& d, std::initializer_list<PlanPart> parts, const char*& base_out) {
    std::lock_guard<std::mutex> lock(cache.mu);
    void* base = nullptr;
    for (const PlanCache::DevPlan& p : cache.plans)
        if (p.device == d.id) base = p.base;
    if (!base) {
        size_t total = 0;
        for (const PlanPart& part : parts) total += part.bytes;
        DevBuf buf;
        HCHECK(hipMalloc(&buf.p, std::max<size_t>(total, 8)));
        size_t at = 0;
        for (const PlanPart& part : parts) {
            if (part.bytes) HCHECK(hipMemcpy((char*)buf.p + at, part.p, part.bytes, hipMemcpyHostToDevice));
            at += part.bytes;
        }
        cache.plans.push_back(PlanCache::DevPlan{d.id, buf.p});
        cache.dev_free = circuit_plan_free;
        base = buf.p;
        buf.p = nullptr;
    }
    base_out = static_cast<const char*>(base);
    return TFHE_OK;
}

tfhe_status circuit_plan(const tfhe_circuit* circ, Device& d, const CircuitRec*& recs, const CircuitOut*& outs) {
    tfhe_circuit* c = const_cast<tfhe_circuit*>(circ);  // the device copies are a cache, not part of the plan
    const size_t rb = c->recs.size() * sizeof(CircuitRec), ob = c->outs.size() * sizeof(CircuitOut);
    const char* base = nullptr;
    SCHECK(plan_on_device(c->cache, d, {{c->recs.data(), rb}, {c->outs.data(), ob}}, base));
    recs = reinterpret_cast<const CircuitRec*>(base);
    outs = reinterpret_cast<const CircuitOut*>(base + rb);
    return TFHE_OK;
}

// trace knob (TFHE_TRACE): event pairs around the launches of the two circuit kernels and the whole run
struct CircuitTrace {
    std::vector<hipEvent_t> ev;  // run begin, then (begin, end) per prep launch, (begin, end) per output launch, run end
    ~CircuitTrace() {
        for (hipEvent_t e : ev) hipEventDestroy(e);
    }
    tfhe_status mark(bool on, hipStream_t s) {
        if (!on) return TFHE_OK;
        hipEvent_t e = nullptr;
        HCHECK(hipEventCreate(&e));
        ev.push_back(e);
        HCHECK(hipEventRecord(e, s));
        return TFHE_OK;
    }
    // after the run-end mark: waits for the stream and prints the circuit line
    tfhe_status report(hipStream_t s, uint32_t bootstraps, size_t instances, size_t preps) {
        HCHECK(hipStreamSynchronize(s));
        auto ms = [&](size_t a, size_t b) {
            float t = 0;
            hipEventElapsedTime(&t, ev[a], ev[b]);
            return (double)t;
        };
        double prep_ms = 0, out_ms = 0;
        for (size_t k = 1; k + 1 < ev.size(); k += 2) (k < 1 + 2 * preps ? prep_ms : out_ms) += ms(k, k + 1);
        std::fprintf(stderr, "[tfhe] circuit: %u bootstraps x %zu instances in %.3f ms; %zu prep launches %.3f ms, output %.3f ms\n",
                     bootstraps, instances, ms(0, ev.size() - 1), preps, prep_ms, out_ms);
        return TFHE_OK;
    }
};

// One run on one device (inside run_device_op): per level one preparation launch, then the blind rotation,
// the extraction and the key switch once for the whole mixed level -- in slices of the scratch capacity
// when width * instances exceeds it; the key switch writes the level's slots of the wire store.
tfhe_status dev_circuit(tfhe_ctx* c, Device& d, const tfhe_circuit* circ, const CircuitRec* recs,
                        const CircuitOut* outs, size_t instances, const uint64_t* in, uint64_t q, uint64_t* out) {
    const tfhe_params& p = c->p;
    CircuitPrep P{};
    P.N = p.N, P.n = p.n, P.Q = p.Q, P.Q8 = p.Q / 8 + 1, P.q = q, P.instances = instances;
    const size_t w = p.n + 1, slice = std::min(d.sc.cap, c->max_chunk);
    const bool trace = c->kn.trace != 0;
    CircuitTrace tr;
    size_t preps = 0;
    SCHECK(tr.mark(trace, d.stream));
    for (const CircuitLevel& L : circ->levels) {
        const size_t total = (size_t)L.width * instances;
        for (size_t first = 0; first < total; first += slice) {
            const size_t B = std::min(slice, total - first);
            P.first = first;
            SCHECK(tr.mark(trace, d.stream));
            HCHECK(launch_circuit_prep(P, recs + L.first, in, d.wires, d.sc.acc, d.sc.a, B, d.stream));
            SCHECK(tr.mark(trace, d.stream));
            ++preps;
            SCHECK(dev_blind_rotate(c, d, d.sc.a, q, d.sc.acc, B));
            HCHECK(launch_extract(p.N, p.Q, P.Q8, d.sc.acc, d.sc.ext, B, d.stream));
            SCHECK(dev_mkm(c, d, d.sc.ext, q, d.wires + ((size_t)L.first * instances + first) * w, B));
        }
    }
    const size_t total = circ->outs.size() * instances, grid = (size_t)1 << 30;
    for (size_t first = 0; first < total; first += grid) {
        P.first = first;
        SCHECK(tr.mark(trace, d.stream));
        HCHECK(launch_circuit_out(P, outs, in, d.wires, out, std::min(grid, total - first), d.stream));
        SCHECK(tr.mark(trace, d.stream));
    }
    SCHECK(tr.mark(trace, d.stream));
    if (trace) SCHECK(tr.report(d.stream, circ->info.bootstraps, instances, preps));
    return TFHE_OK;
}

// The plan of a function circuit on one device (plan_on_device order: recs | terms | outs | luts).
struct FuncPlan {
    const FuncRec* recs;
    const FuncTerm* terms;
    const FuncOut* outs;
    const uint64_t* luts;
};
tfhe_status fcircuit_plan(const tfhe_fcircuit* circ, Device& d, FuncPlan& pl) {
    tfhe_fcircuit* c = const_cast<tfhe_fcircuit*>(circ);  // the device copies are a cache, not part of the plan
    const size_t rb = c->recs.size() * sizeof(FuncRec), tb = c->terms.size() * sizeof(FuncTerm),
                 ob = c->outs.size() * sizeof(FuncOut), lb = c->luts.size() * sizeof(uint64_t);
    const char* base = nullptr;
    SCHECK(plan_on_device(c->cache, d, {{c->recs.data(), rb}, {c->terms.data(), tb}, {c->outs.data(), ob}, {c->luts.data(), lb}},
                          base));
    pl.recs = reinterpret_cast<const FuncRec*>(base);
    pl.terms = reinterpret_cast<const FuncTerm*>(base + rb);
    pl.outs = reinterpret_cast<const FuncOut*>(base + rb + tb);
    pl.luts = reinterpret_cast<const uint64_t*>(base + rb + tb + ob);
    return TFHE_OK;
}

// One run of a function circuit on one device (inside run_device_op): per level (or slice) one preparation
// launch, ONE blind rotation at a-modulus 2N for records of both ciphertext moduli (the preparation kernel
// scales every mask to 2N), one extraction, and the key switch once per output modulus: the records that end
// at q are the level's first width_q slots, those that end at 2q the rest, so each call writes one contiguous
// range of the wire store.
tfhe_status dev_fcircuit(tfhe_ctx* c, Device& d, const tfhe_fcircuit* circ, const FuncPlan& pl, size_t instances,
                         const uint64_t* in, uint64_t* out) {
    const tfhe_params& p = c->p;
    const uint64_t q = circ->info.q;
    FuncPrep P{};
    P.N = p.N, P.n = p.n, P.log2N = ilog2(p.N), P.Q = p.Q, P.q = q, P.instances = instances;
    const size_t w = p.n + 1, slice = std::min(d.sc.cap, c->max_chunk);
    const bool trace = c->kn.trace != 0;
    CircuitTrace tr;
    size_t preps = 0;
    SCHECK(tr.mark(trace, d.stream));
    for (const FuncLevel& L : circ->levels) {
        const size_t total = (size_t)L.width * instances, at_q = (size_t)L.width_q * instances;
        for (size_t first = 0; first < total; first += slice) {
            const size_t B = std::min(slice, total - first);
            P.first = first;
            SCHECK(tr.mark(trace, d.stream));
            HCHECK(launch_fcircuit_prep(P, pl.recs + L.first, pl.terms, pl.luts, in, d.wires, d.sc.acc, d.sc.a, B, d.stream));
            SCHECK(tr.mark(trace, d.stream));
            ++preps;
            SCHECK(dev_blind_rotate(c, d, d.sc.a, 2ull * p.N, d.sc.acc, B));
            HCHECK(launch_extract(p.N, p.Q, 0, d.sc.acc, d.sc.ext, B, d.stream));
            const size_t nq = at_q > first ? std::min(B, at_q - first) : 0;  // of this slice, those that end at q
            uint64_t* dst = d.wires + ((size_t)L.first * instances + first) * w;
            if (nq) SCHECK(dev_mkm(c, d, d.sc.ext, q, dst, nq));
            if (B > nq) SCHECK(dev_mkm(c, d, d.sc.ext + nq * ((size_t)p.N + 1), q << 1, dst + nq * w, B - nq));
        }
    }
    const size_t total = circ->outs.size() * instances, grid = (size_t)1 << 30;
    for (size_t first = 0; first < total; first += grid) {
        P.first = first;
        SCHECK(tr.mark(trace, d.stream));
        HCHECK(launch_fcircuit_out(P, pl.outs, pl.terms, in, d.wires, out, std::min(grid, total - first), d.stream));
        SCHECK(tr.mark(trace, d.stream));
    }
    SCHECK(tr.mark(trace, d.stream));
    if (trace) SCHECK(tr.report(d.stream, circ->info.bootstraps, instances, preps));
    return TFHE_OK;
}

// ---------------------------------------------------------------------------
// host-array front ends: shard over devices, chunk to scratch, H2D/D2H
// ---------------------------------------------------------------------------
// One host thread per device, each on a contiguous shard (shard_span).  select(g) makes device g
// current on the calling thread (hipSetDevice; a no-op in tfhe_host_shard_selftest); body(g, lo, cnt)
// queues and waits for that shard.  Every thread's status and thread-local error message is
// collected; the first failing device's is returned as "device g: ...".
template <typename Select, typename Body>
tfhe_status run_shards(size_t D, size_t B, Select&& select, Body&& body) {
    if (D == 1 || B < 2 * D) {
        SCHECK(select(0));
        return body((size_t)0, (size_t)0, B);
    }
    std::vector<tfhe_status> st(D, TFHE_OK);
    std::vector<std::string> msg(D);
    std::vector<std::thread> th;
    for (size_t g = 0; g < D; ++g) {
        size_t lo, cnt;
        shard_span(B, D, g, &lo, &cnt);
        th.emplace_back([&, g, lo, cnt] {
            try {  // an exception must not leave a worker thread (std::terminate)
                st[g] = select(g);
                if (st[g] == TFHE_OK && cnt > 0) st[g] = body(g, lo, cnt);
                if (st[g] != TFHE_OK) msg[g] = g_last_error;  // thread_local: this thread's message
            } catch (const std::exception& e) {
                st[g] = TFHE_ERR_INTERNAL, msg[g] = e.what();
            } catch (...) {
                st[g] = TFHE_ERR_INTERNAL, msg[g] = "unknown exception";
            }
        });
    }
    for (auto& t : th) t.join();
    for (size_t g = 0; g < D; ++g)
        if (st[g] != TFHE_OK) return fail(st[g], "device " + std::to_string(g) + ": " + msg[g]);
    return TFHE_OK;
}

template <typename F>
tfhe_status for_each_shard(tfhe_ctx* c, size_t B, F&& body) {
    return run_shards(
        c->devs.size(), B,
        [&](size_t g) -> tfhe_status {
            HCHECK(hipSetDevice(c->devs[g].id));
            return TFHE_OK;
        },
        [&](size_t g, size_t lo, size_t cnt) { return body(c->devs[g], lo, cnt); });
}

// Host <-> device copies through two pinned 8 MiB blocks: the host copy pool fills (or
// drains) block k+1 while the DMA engine moves block k.  Pageable hipMemcpyAsync stages
// through the runtime's buffers with one host thread; this path is ~2x faster.
tfhe_status ensure_pinned(Device& d) {
    for (int k = 0; k < 2; ++k) {
        if (!d.pin[k]) HCHECK(hipHostMalloc(&d.pin[k], kStageBytes, hipHostMallocDefault));
        if (!d.pin_ev[k]) HCHECK(hipEventCreateWithFlags(&d.pin_ev[k], hipEventDisableTiming));
    }
    return TFHE_OK;
}
// words u64 host -> device through the pinned blocks; wb < 8: the narrow wire format -- the host
// pool narrows each block into pinned memory, the DMA moves wb bytes per word into `pk` (device),
// and one kernel widens pk into dst.  wb is the caller's guess from the array's modulus; a value
// that does not fit (an unreduced input) sends the whole array again as u64.
tfhe_status h2d_staged(Device& d, uint64_t* dst, const HostIn& src, size_t words, hipStream_t s, int wb = 8,
                       void* pk = nullptr) {
    SCHECK(ensure_pinned(d));
    const size_t per = kStageBytes / wb;  // words per block
    uint64_t seen = 0;
    for (size_t off = 0, k = 0; off < words; off += per, ++k) {
        const int slot = (int)(k & 1);
        const size_t nw = std::min(per, words - off);
        HCHECK(hipEventSynchronize(d.pin_ev[slot]));  // the DMA that last read this block is done
        if (wb == 8) {
            parallel_memcpy_in((uint64_t*)d.pin[slot], src, off, nw);
            HCHECK(hipMemcpyAsync(dst + off, d.pin[slot], nw * 8, hipMemcpyHostToDevice, s));
        } else {
            seen |= parallel_narrow_in(d.pin[slot], src, off, nw, wb);
            HCHECK(hipMemcpyAsync((char*)pk + off * wb, d.pin[slot], nw * wb, hipMemcpyHostToDevice, s));
        }
        HCHECK(hipEventRecord(d.pin_ev[slot], s));
    }
    if (wb == 8) return TFHE_OK;
    if (seen >> (8 * wb)) return h2d_staged(d, dst, src, words, s);
    HCHECK(launch_widen(pk, wb, dst, words, s));
    return TFHE_OK;
}
// words u64 device -> host; wb < 8 (every value below 2^(8 wb)): one kernel narrows src into pk,
// the DMA moves wb bytes per word, the host pool widens each block into dst
tfhe_status d2h_staged(Device& d, const HostOut& dst, const uint64_t* src, size_t words, hipStream_t s, int wb = 8,
                       void* pk = nullptr) {
    SCHECK(ensure_pinned(d));
    if (wb != 8) HCHECK(launch_narrow(src, wb, pk, words, s));
    const char* from = wb == 8 ? (const char*)src : (const char*)pk;
    const size_t per = kStageBytes / wb;
    size_t prev_off = 0, prev_nw = 0;
    for (size_t off = 0, k = 0;; off += per, ++k) {
        const int slot = (int)(k & 1);
        const bool more = off < words;
        const size_t nw = more ? std::min(per, words - off) : 0;
        if (more) {
            HCHECK(hipEventSynchronize(d.pin_ev[slot]));
            HCHECK(hipMemcpyAsync(d.pin[slot], from + off * wb, nw * wb, hipMemcpyDeviceToHost, s));
            HCHECK(hipEventRecord(d.pin_ev[slot], s));
        }
        if (k > 0) {  // drain the previous block while this one is in flight
            const int ps = (int)((k - 1) & 1);
            HCHECK(hipEventSynchronize(d.pin_ev[ps]));
            if (wb == 8) parallel_memcpy_out(dst, prev_off, (const uint64_t*)d.pin[ps], prev_nw);
            else parallel_widen_out(dst, prev_off, d.pin[ps], prev_nw, wb);
        }
        if (!more) break;
        prev_off = off, prev_nw = nw;
    }
    return TFHE_OK;
}

// The host-array EvalAcc's output while its blind rotation still runs.  The launch wrote completion
// flags (BRDone: 4 words per ciphertext, one per wave, stored in pinned host memory after the wave's
// accumulator words reached HBM); workgroups are dispatched in ciphertext order, so the ciphertexts of
// block k finish before most of block k+1's.  For each 8 MiB block the host waits for its flags, the
// DMA copies it (u64, no narrowing kernel: it would have to wait for the whole launch) on the copy
// stream, and the host drains the previous block into dst.  Only the last block or two, which finish
// with the launch's last wave, are exposed after the kernel -- instead of the whole 67 MB.
// The wait never hangs: if the compute stream completes (or fails) with a flag unset, or 120 s pass,
// the call fails.
tfhe_status wait_flags(const uint32_t* flags, size_t lo, size_t hi, hipStream_t cs) {
    const volatile uint32_t* f = flags;
    const auto t0 = std::chrono::steady_clock::now();
    for (size_t i = lo, polls = 0; i < hi; ++polls) {
        if (f[i] != 0) {
            ++i;
            continue;
        }
        // a miss: pause (the spinning thread shares its core with the host pool draining other blocks,
        // ADVICE r3), yield every 64 misses, check the stream every 1024
#if defined(__x86_64__) || defined(__i386__)
        __builtin_ia32_pause();
#elif defined(__aarch64__)
        __builtin_arm_yield();
#endif
        if ((polls & 63) == 63) std::this_thread::yield();
        if ((polls & 1023) == 1023) {
            const hipError_t q = hipStreamQuery(cs);
            if (q == hipSuccess) {
                if (f[i] == 0) return fail(TFHE_ERR_INTERNAL, "blind rotation finished without its completion flag");
            } else if (q != hipErrorNotReady) {
                return fail(TFHE_ERR_DEVICE, std::string("blind rotation: ") + hipGetErrorString(q));
            }
            if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(120))
                return fail(TFHE_ERR_DEVICE, "blind rotation: completion flags not set within 120 s");
        }
    }
    return TFHE_OK;
}

tfhe_status d2h_flagged(Device& d, const HostOut& dst, const uint64_t* src, size_t cts, size_t wpc, hipStream_t xs,
                        hipStream_t cs) {
    SCHECK(ensure_pinned(d));
    const size_t cpb = std::max<size_t>(1, (kStageBytes / 8) / wpc);  // ciphertexts per block
    if (cpb * wpc * 8 > kStageBytes) return fail(TFHE_ERR_UNSUPPORTED, "accumulator larger than a staging block");
    size_t prev_lo = 0, prev_n = 0;
    for (size_t lo = 0, k = 0;; lo += cpb, ++k) {
        const int slot = (int)(k & 1);
        const bool more = lo < cts;
        const size_t n = more ? std::min(cpb, cts - lo) : 0;
        if (more) {
            SCHECK(wait_flags(d.flags, 4 * lo, 4 * (lo + n), cs));
            HCHECK(hipEventSynchronize(d.pin_ev[slot]));
            HCHECK(hipMemcpyAsync(d.pin[slot], src + lo * wpc, n * wpc * 8, hipMemcpyDeviceToHost, xs));
            HCHECK(hipEventRecord(d.pin_ev[slot], xs));
        }
        if (k > 0) {
            const int ps = (int)((k - 1) & 1);
            HCHECK(hipEventSynchronize(d.pin_ev[ps]));
            parallel_memcpy_out(dst, prev_lo * wpc, (const uint64_t*)d.pin[ps], prev_n * wpc);
        }
        if (!more) break;
        prev_lo = lo, prev_n = n;
    }
    return TFHE_OK;
}

tfhe_status ensure_flags(Device& d, size_t words) {
    if (words <= d.flags_words) return TFHE_OK;
    if (d.flags) HCHECK(hipHostFree(d.flags));
    d.flags = nullptr, d.flags_words = 0;
    HCHECK(hipHostMalloc((void**)&d.flags, words * 4, hipHostMallocCoherent | hipHostMallocMapped | hipHostMallocPortable));
    d.flags_words = words;
    return TFHE_OK;
}

// Host-array runner: in-arrays are [B][in_words] (up to 2), out [B][out_words].  Each
// device's shard is cut into sub-batches.  Kernels run in order on the device's compute
// stream (lane-0 scratch); copies run on its copy stream (stream2) into two alternating
// device I/O sets, ordered by events: the kernels of k wait for H2D(k), D2H(k) waits for the
// kernels of k, and H2D(k+2) follows D2H(k) on the copy stream (so it reuses k's I/O set only
// after k's kernels and D2H are done).  The host queues H2D(k+1) and the kernels of k+1
// before it drains D2H(k): the compute stream waits for PCIe only for the first sub-batch's
// input and the last one's output.  op(device, in1, in2, out, count, index of the first
// ciphertext) queues its kernels on d.stream.
// Sub-batches per shard: 1 unless TFHE_HOST_PARTS asks for more.  Measured (STD128 NAND,
// 8192, profiles/r02_host): one sub-batch 45.0 ms, 2: 46.2, 4: 51.5, 8: 59.7 -- the split
// blind rotations (2048 workgroups each: a launch tail apiece), the key switches (~1 ms each at
// any batch) and the runtime's blit kernels for the sub-8 MiB copies, which run beside the
// blind rotation, cost more than the 3.4 ms of PCIe they hide.
size_t host_parts(const tfhe_ctx* c, size_t cnt) {
    const size_t want = (size_t)std::max(1, c->kn.host_parts);  // knob (TFHE_HOST_PARTS)
    return std::min(want, std::max<size_t>(1, cnt / 256));
}

tfhe_status ensure_io_set(Scratch& sc, size_t words, size_t pk_bytes) {
    if (words > sc.io_words) {
        hipFree(sc.io);
        sc.io = nullptr, sc.io_words = 0;
        HCHECK(hipMalloc(&sc.io, words * sizeof(uint64_t)));
        sc.io_words = words;
    }
    if (pk_bytes > sc.pk_bytes) {
        hipFree(sc.pk);
        sc.pk = nullptr, sc.pk_bytes = 0;
        HCHECK(hipMalloc(&sc.pk, pk_bytes));
        sc.pk_bytes = pk_bytes;
    }
    return TFHE_OK;
}

// PCIe wire width of an array: the narrowest of u16 / u32 / u64 that holds every value (inputs:
// the OR of the words; outputs: the op's bound); the wire knob 0 (TFHE_WIRE=0) keeps u64.  The
// completion-flag output of the host-array EvalAcc (d2h_flagged) follows the acc_flags knob.

// Value bounds of the runner's arrays (0: unknown): an array crosses PCIe in the narrowest of u16 /
// u32 / u64 that holds its bound (h2d_staged / d2h_staged).  Inputs are checked as they are packed
// (an unreduced input goes again as u64); outputs must respect their bound (the op's modulus).
struct WireLim {
    uint64_t in1 = 0, in2 = 0, out_in = 0, out = 0;
};

// out_in: the output rows' initial contents (uploaded into the output set before the kernels of
// their sub-batch, for ops that work in place on the output, e.g. the blind rotation).
// Arrays are HostRows views (flat or row pointers); w1 / w2 / wo are their record widths.
template <typename Op>
tfhe_status run_lwe_batch_v(tfhe_ctx* c, size_t B, const HostIn& in1, const HostIn& in2, const HostOut& out, Op&& op,
                            WireLim wl, const HostIn& out_in, bool flag_out = false) {
    const size_t w1 = in1.w, w2 = in2.empty() ? 0 : in2.w, wo = out.w;
    const bool has2 = !in2.empty(), has_oi = !out_in.empty();
    return for_each_shard(c, B, [&](Device& d, size_t lo, size_t cnt) -> tfhe_status {
        const size_t parts = host_parts(c, cnt);
        const size_t sub = std::min((cnt + parts - 1) / parts, c->max_chunk);
        const size_t w_in2 = has2 ? w2 : 0, io_words = sub * (w1 + w_in2 + wo);
        const bool nar = c->kn.wire != 0;
        auto width = [nar](uint64_t lim) { return nar && lim ? wire_bytes(lim - 1) : 8; };
        const int wb1 = width(wl.in1), wb2 = has2 ? width(wl.in2) : 8, wbi = has_oi ? width(wl.out_in) : 8;
        const int wbo = width(wl.out);
        const size_t pk1 = sub * w1 * wb1, pk2 = sub * w_in2 * wb2, pko = sub * wo * std::max(wbi, wbo);
        SCHECK(ensure_scratch(c, d, sub));
        SCHECK(ensure_io_set(d.sc, io_words, pk1 + pk2 + pko));
        SCHECK(ensure_io_set(d.sc2, io_words, pk1 + pk2 + pko));
        for (hipEvent_t* e : {&d.h2d_ev[0], &d.h2d_ev[1], &d.k_ev[0], &d.k_ev[1]})
            if (!*e) HCHECK(hipEventCreateWithFlags(e, hipEventDisableTiming));
        SCHECK(sc_acquire(d, d.stream));
        const hipStream_t cs = d.stream, xs = d.stream2;
        uint64_t* io[2] = {d.sc.io, d.sc2.io};
        char* pk[2] = {(char*)d.sc.pk, (char*)d.sc2.pk};
        const bool trace = c->kn.trace != 0;
        auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
        const double t0 = trace ? now() : 0;
        auto dout_of = [&](int set) { return io[set] + sub * (w1 + w_in2); };
        // D2H of sub-batch k (set k & 1): after its kernels, drained into `out` by the host
        auto d2h = [&](size_t k) -> tfhe_status {
            const size_t off = lo + k * sub, b = std::min(sub, lo + cnt - off);
            const int set = (int)(k & 1);
            HCHECK(hipStreamWaitEvent(xs, d.k_ev[set], 0));
            return d2h_staged(d, out.sub(off), dout_of(set), b * wo, xs, wbo, pk[set] + pk1 + pk2);
        };
        tfhe_status st = TFHE_OK;
        bool done_out = false;  // the flagged path drained the output already
        const size_t n_sub = (cnt + sub - 1) / sub;
        for (size_t k = 0; k < n_sub && st == TFHE_OK; ++k) {
            const size_t off = lo + k * sub, b = std::min(sub, lo + cnt - off);
            const int set = (int)(k & 1);
            uint64_t *din1 = io[set], *din2 = has2 ? io[set] + sub * w1 : nullptr, *dout = dout_of(set);
            st = h2d_staged(d, din1, in1.sub(off), b * w1, xs, wb1, pk[set]);
            if (trace) std::fprintf(stderr, "[tfhe] sub-batch %zu input 1 (%s) staged at %.2f ms\n", k,
                                    in1.flat ? "flat" : "rows", now() - t0);
            if (st == TFHE_OK && has2) st = h2d_staged(d, din2, in2.sub(off), b * w2, xs, wb2, pk[set] + pk1);
            if (st == TFHE_OK && has_oi)
                st = h2d_staged(d, dout, out_in.sub(off), b * wo, xs, wbi, pk[set] + pk1 + pk2);
            if (st != TFHE_OK) break;
            if (trace) std::fprintf(stderr, "[tfhe] sub-batch %zu inputs staged at %.2f ms (wire %d/%d/%d/%d B)\n", k,
                                    now() - t0, wb1, wb2, wbi, wbo);
            // no early return below this point: both streams are synchronised before returning
            if (hipEventRecord(d.h2d_ev[set], xs) != hipSuccess || hipStreamWaitEvent(cs, d.h2d_ev[set], 0) != hipSuccess) {
                st = fail(TFHE_ERR_DEVICE, "host batch: event ordering failed");
                break;
            }
            // flag_out (EvalAcc): one sub-batch lets its blind rotation flag finished ciphertexts
            const bool flagged = flag_out && n_sub == 1 && c->kn.acc_flags != 0;
            if (flagged) {
                st = ensure_flags(d, 4 * b);
                if (st != TFHE_OK) break;
                std::memset(d.flags, 0, 4 * b * sizeof(uint32_t));  // no kernel of an earlier call is left
                d.br_done = BRDone{};
                d.br_done.flags = d.flags;
            }
            st = op(d, din1, din2, dout, b, off);
            const bool written = flagged && d.br_done.written;
            d.br_done = BRDone{};
            if (st != TFHE_OK) break;
            if (written) {  // the blind rotation was the op's last kernel: drain while it runs
                if (trace) std::fprintf(stderr, "[tfhe] sub-batch %zu queued at %.2f ms (flagged output)\n", k, now() - t0);
                st = d2h_flagged(d, out.sub(off), dout, b, wo, xs, cs);
                if (trace) std::fprintf(stderr, "[tfhe] flagged output drained at %.2f ms\n", now() - t0);
                if (st != TFHE_OK) break;
                done_out = true;
                continue;
            }
            if (hipEventRecord(d.k_ev[set], cs) != hipSuccess) {
                st = fail(TFHE_ERR_DEVICE, "host batch: event record failed");
                break;
            }
            if (trace) std::fprintf(stderr, "[tfhe] sub-batch %zu queued at %.2f ms\n", k, now() - t0);
            if (k > 0) st = d2h(k - 1);
        }
        if (st == TFHE_OK && n_sub > 0 && !done_out) {
            if (trace) {
                HCHECK(hipStreamSynchronize(cs));
                std::fprintf(stderr, "[tfhe] last sub-batch's kernels done at %.2f ms\n", now() - t0);
            }
            st = d2h(n_sub - 1);
        }
        const hipError_t e1 = hipStreamSynchronize(cs), e2 = hipStreamSynchronize(xs);
        if (trace) std::fprintf(stderr, "[tfhe] host batch %zu in %zu sub-batches: done %.2f ms\n", cnt, n_sub, now() - t0);
        if (st == TFHE_OK && (e1 != hipSuccess || e2 != hipSuccess))
            st = fail(TFHE_ERR_DEVICE, std::string("host batch: ") + hipGetErrorString(e1 != hipSuccess ? e1 : e2));
        return st;
    });
}

// flat [B][w] arrays
template <typename Op>
tfhe_status run_lwe_batch(tfhe_ctx* c, size_t B, const uint64_t* in1, size_t w1, const uint64_t* in2, size_t w2,
                          uint64_t* out, size_t wo, Op&& op, WireLim wl, const uint64_t* out_in = nullptr,
                          bool flag_out = false) {
    return run_lwe_batch_v(c, B, flat_rows(in1, w1), in2 ? flat_rows(in2, w2) : HostIn{}, flat_rows(out, wo),
                           std::forward<Op>(op), wl, out_in ? flat_rows(out_in, wo) : HostIn{}, flag_out);
}

tfhe_status check_ctx(tfhe_ctx* c) {
    if (!c || c->devs.empty()) return fail(TFHE_ERR_NOT_SET_UP, "context not set up (call tfhe_setup)");
    return TFHE_OK;
}

tfhe_status create_ctx(const tfhe_params* p, int num_gpus, std::unique_ptr<tfhe_ctx>& out) {
    if (!p) return fail(TFHE_ERR_INVALID_ARGUMENT, "null params");
    auto c = std::make_unique<tfhe_ctx>();
    c->p = *p;
    std::string err;
    if (params_finish(&c->p, &err) != TFHE_OK) return fail(TFHE_ERR_INVALID_ARGUMENT, err);
    SCHECK(init_derived(c.get()));
    int count = 0;
    HCHECK(hipGetDeviceCount(&count));
    if (count < 1) return fail(TFHE_ERR_DEVICE, "no HIP device visible");
    // Test hook: TFHE_LOGICAL_DEVICES=k presents k logical devices, all on physical device 0, each
    // with its own arena, streams, scratch and host thread -- the multi-device setup, replication
    // (peer copies: one RCCL communicator cannot hold a device twice), sharding and error paths
    // run on a one-GPU box (tests/test_gpu_multidevice.py).  Read per setup.
    if (const char* rl = std::getenv("TFHE_RCCL_LIB")) c->rccl_lib = rl;
    const char* lg = std::getenv("TFHE_LOGICAL_DEVICES");
    const int logical = lg ? std::atoi(lg) : 0;
    if (logical > 1) count = logical;
    // GPUSetup(numGPUs): numGPUs <= 0 or more than visible uses every visible device
    // (bootstrapping.cu:736-739)
    if (num_gpus < 1 || num_gpus > count) num_gpus = count;
    c->devs.resize(num_gpus);
    for (int g = 0; g < num_gpus; ++g) c->devs[g].id = logical > 1 ? 0 : g;
    out = std::move(c);
    return TFHE_OK;
}

}  // namespace

tfhe_ctx::~tfhe_ctx() {
    for (auto& d : devs) free_device(d);
}

namespace {
// Every extern "C" body runs under this: no C++ exception crosses the C-ABI.
template <typename F>
tfhe_status guarded(F&& body) {
    try {
        return body();
    } catch (const std::bad_alloc&) {
        return fail(TFHE_ERR_OUT_OF_MEMORY, "host allocation failed");
    } catch (const std::exception& e) {
        return fail(TFHE_ERR_INTERNAL, std::string("internal error: ") + e.what());
    } catch (...) {
        return fail(TFHE_ERR_INTERNAL, "internal error");
    }
}
}  // namespace

// ===========================================================================
// extern "C" entry points
// ===========================================================================
extern "C" {

int tfhe_abi_version(void) { return TFHE_HIP_ABI_VERSION; }

tfhe_status tfhe_set_kernel_variant(int variant) {
    if (!set_fast_variant(variant)) return fail(TFHE_ERR_INVALID_ARGUMENT, "unknown kernel variant");
    return TFHE_OK;
}
int tfhe_get_kernel_variant(void) { return get_fast_variant(); }

const char* tfhe_last_error(void) { return g_last_error.c_str(); }

const char* tfhe_status_string(tfhe_status s) {
    switch (s) {
        case TFHE_OK: return "ok";
        case TFHE_ERR_INVALID_ARGUMENT: return "invalid argument";
        case TFHE_ERR_UNSUPPORTED: return "unsupported";
        case TFHE_ERR_NOT_SET_UP: return "not set up";
        case TFHE_ERR_DEVICE: return "device error";
        case TFHE_ERR_OUT_OF_MEMORY: return "out of memory";
        default: return "internal error";
    }
}

tfhe_status tfhe_params_from_set(int paramset, tfhe_params* out) {
    return guarded([&]() -> tfhe_status {
        if (!out) return fail(TFHE_ERR_INVALID_ARGUMENT, "null output");
        tfhe_status s = params_from_set(paramset, out);
        if (s != TFHE_OK) return fail(s, "unknown parameter set");
        return TFHE_OK;
    });
}

tfhe_status tfhe_params_from_logq(int paramset, int arb_func, uint32_t logQ, int64_t N, uint32_t baseG,
                                  uint32_t num_digits_to_throw, tfhe_params* out) {
    return guarded([&]() -> tfhe_status {
        if (!out) return fail(TFHE_ERR_INVALID_ARGUMENT, "null output");
        tfhe_status s = params_from_logq(paramset, arb_func, logQ, N, baseG, num_digits_to_throw, out);
        if (s != TFHE_OK) return fail(s, "unsupported logQ parameter request (STD128/TOY, 11 <= logQ <= 29)");
        return TFHE_OK;
    });
}

tfhe_status tfhe_params_finish(tfhe_params* p) {
    return guarded([&]() -> tfhe_status {
        if (!p) return fail(TFHE_ERR_INVALID_ARGUMENT, "null params");
        std::string err;
        tfhe_status s = params_finish(p, &err);
        return s == TFHE_OK ? s : fail(s, err);
    });
}

extern "C++" {  // (a C++ return type: no C linkage inside the extern "C" block)
namespace {
// RCCL, loaded when a context spans several devices (no link-time dependency for one-GPU use)
struct RcclApi {
    bool ok = false;
    decltype(&ncclCommInitAll) init_all = nullptr;
    decltype(&ncclBroadcast) bcast = nullptr;
    decltype(&ncclGroupStart) group_start = nullptr;
    decltype(&ncclGroupEnd) group_end = nullptr;
    decltype(&ncclCommDestroy) destroy = nullptr;
    decltype(&ncclGetErrorString) err = nullptr;
    decltype(&ncclGetVersion) version = nullptr;  // optional (reported by tfhe_rccl_selftest)
};
// path: "" = the system RCCL (librccl.so.1); otherwise TFHE_RCCL_LIB, read at setup -- a test build of the
// same six entry points (tests/stub_rccl: broadcasts by device copies, so the group / sync / destroy
// sequence below runs on a one-GPU box with logical devices).  Loaded once per path.
const RcclApi& rccl(const std::string& path) {
    static std::mutex mu;
    static std::vector<std::pair<std::string, std::unique_ptr<RcclApi>>> loaded;
    std::lock_guard<std::mutex> lock(mu);
    for (auto& e : loaded)
        if (e.first == path) return *e.second;
    loaded.emplace_back(path, std::make_unique<RcclApi>([&] {
        RcclApi a;
        void* h = path.empty() ? dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL) : dlopen(path.c_str(), RTLD_NOW | RTLD_LOCAL);
        if (!h && path.empty()) h = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
        if (!h) return a;
        a.init_all = (decltype(a.init_all))dlsym(h, "ncclCommInitAll");
        a.bcast = (decltype(a.bcast))dlsym(h, "ncclBroadcast");
        a.group_start = (decltype(a.group_start))dlsym(h, "ncclGroupStart");
        a.group_end = (decltype(a.group_end))dlsym(h, "ncclGroupEnd");
        a.destroy = (decltype(a.destroy))dlsym(h, "ncclCommDestroy");
        a.err = (decltype(a.err))dlsym(h, "ncclGetErrorString");
        a.version = (decltype(a.version))dlsym(h, "ncclGetVersion");
        a.ok = a.init_all && a.bcast && a.group_start && a.group_end && a.destroy && a.err;
        return a;
    }()));
    return *loaded.back().second;
}

// Sum of the checksum partials of `bytes` at p on device `dev` (stream synchronised)
tfhe_status buffer_checksum(int dev, const void* p, size_t bytes, hipStream_t stream, uint64_t& out) {
    DevBuf part;
    HCHECK(hipSetDevice(dev));
    HCHECK(hipMalloc(&part.p, kChecksumBlocks * sizeof(uint64_t)));
    HCHECK(launch_checksum(p, bytes, part.as<uint64_t>(), stream));
    std::vector<uint64_t> h(kChecksumBlocks);
    HCHECK(hipMemcpyAsync(h.data(), part.p, h.size() * 8, hipMemcpyDeviceToHost, stream));
    HCHECK(hipStreamSynchronize(stream));
    out = 0;
    for (uint64_t v : h) out += v;
    return TFHE_OK;
}
tfhe_status arena_checksum(Device& d, size_t bytes, uint64_t& out) {
    return buffer_checksum(d.id, d.arena, bytes, d.stream, out);
}

// One RCCL broadcast of `bytes` at src (on t[0]'s device) into every target buffer: a communicator over the
// targets' devices (ncclCommInitAll), one ncclBroadcast per rank inside a group, every stream synchronised,
// the communicators destroyed.  True when every call succeeded.  The sequence of replicate_arena, and the
// one tfhe_rccl_selftest runs against the real librccl on a one-GPU box (a one-rank communicator).
struct RcclTarget {
    int device;
    void* dst;
    hipStream_t stream;
};
bool rccl_broadcast(const RcclApi& R, const void* src, size_t bytes, const std::vector<RcclTarget>& t) {
    const size_t D = t.size();
    std::vector<ncclComm_t> comms(D);
    std::vector<int> ids(D);
    for (size_t g = 0; g < D; ++g) ids[g] = t[g].device;
    if (R.init_all(comms.data(), (int)D, ids.data()) != ncclSuccess) return false;
    ncclResult_t r = R.group_start();
    for (size_t g = 0; g < D && r == ncclSuccess; ++g)  // no early return inside the group
        r = hipSetDevice(t[g].device) == hipSuccess ? R.bcast(src, t[g].dst, bytes, ncclUint8, 0, comms[g], t[g].stream)
                                                    : ncclUnhandledCudaError;
    const ncclResult_t r2 = R.group_end();
    bool synced = r == ncclSuccess && r2 == ncclSuccess;
    for (size_t g = 0; g < D; ++g) {
        hipSetDevice(t[g].device);
        synced = hipStreamSynchronize(t[g].stream) == hipSuccess && synced;
    }
    for (auto& cm : comms) R.destroy(cm);
    return synced;
}

// Device 0's image -> devices 1..D-1.  GPUSetup(numGPUs) in the reference copies every key from the
// host to each GPU in turn (bootstrapping.cu:1005-1069); here the image crosses PCIe once and is
// broadcast by RCCL over xGMI (one communicator over the context's devices, one ncclBroadcast per
// device in a group), or -- without librccl, or with TFHE_REPLICATE=peer -- copied from device 0 by
// concurrent peer DMAs.  Every device's copy is complete when this returns.
tfhe_status replicate_arena(tfhe_ctx* c, size_t bytes) {
    const size_t D = c->devs.size();
    if (D < 2) return TFHE_OK;
    const auto t0 = std::chrono::steady_clock::now();
    const char* env = std::getenv("TFHE_REPLICATE");
    bool want_rccl = !(env && std::strcmp(env, "peer") == 0);
    // logical devices sharing one GPU (TFHE_LOGICAL_DEVICES): a real communicator cannot hold a device
    // twice; a TFHE_RCCL_LIB test build can (tests/test_gpu_rccl_stub.py)
    for (size_t g = 1; g < D; ++g)
        if (c->devs[g].id == c->devs[0].id && c->rccl_lib.empty()) want_rccl = false;
    bool done = false;
    if (want_rccl && rccl(c->rccl_lib).ok) {
        std::vector<RcclTarget> t(D);
        for (size_t g = 0; g < D; ++g) t[g] = RcclTarget{c->devs[g].id, c->devs[g].arena, c->devs[g].stream};
        done = rccl_broadcast(rccl(c->rccl_lib), c->devs[0].arena, bytes, t);
    }
    if (!done) {
        for (size_t g = 1; g < D; ++g) {
            Device& d = c->devs[g];
            HCHECK(hipSetDevice(d.id));
            HCHECK(hipMemcpyPeerAsync(d.arena, d.id, c->devs[0].arena, c->devs[0].id, bytes, d.stream));
        }
        for (size_t g = 1; g < D; ++g) {
            HCHECK(hipSetDevice(c->devs[g].id));
            HCHECK(hipStreamSynchronize(c->devs[g].stream));
        }
    }
    c->replicate_method = done ? TFHE_REPLICATE_RCCL : TFHE_REPLICATE_PEER;
    c->replicate_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    // every replica must equal device 0's image: a bad broadcast fails setup, not a later call
    uint64_t want = 0, got = 0;
    SCHECK(arena_checksum(c->devs[0], bytes, want));
    for (size_t g = 1; g < D; ++g) {
        SCHECK(arena_checksum(c->devs[g], bytes, got));
        if (got != want)
            return fail(TFHE_ERR_DEVICE, "key arena replica on device " + std::to_string(g) + " differs from device 0's (" +
                                             (done ? "RCCL broadcast" : "peer copy") + ")");
    }
    return TFHE_OK;
}

tfhe_status setup_common(tfhe_ctx** out, const tfhe_params* p, const uint64_t* bsk_coeff, bool bsk_eval,
                         const uint64_t* ksk, int num_gpus) {
    if (!out || !bsk_coeff || !ksk) return fail(TFHE_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    std::unique_ptr<tfhe_ctx> c;
    SCHECK(create_ctx(p, num_gpus, c));
    std::vector<unsigned char> img;
    SCHECK(build_host_image(c.get(), bsk_coeff, bsk_eval, ksk, img));
    const size_t bytes = c->layout.total;
    for (size_t g = 0; g < c->devs.size(); ++g) {
        Device& d = c->devs[g];
        HCHECK(hipSetDevice(d.id));
        SCHECK(create_streams(d));
        HCHECK(hipMalloc(&d.arena, bytes));
    }
    HCHECK(hipSetDevice(c->devs[0].id));
    HCHECK(hipMemcpy(c->devs[0].arena, img.data(), bytes, hipMemcpyHostToDevice));
    img = std::vector<unsigned char>();
    SCHECK(replicate_arena(c.get(), bytes));
    // derived key forms, every device at once (each derives its own from its arena)
    SCHECK(run_shards(
        c->devs.size(), 2 * c->devs.size(),
        [&](size_t g) -> tfhe_status {
            HCHECK(hipSetDevice(c->devs[g].id));
            return TFHE_OK;
        },
        [&](size_t g, size_t, size_t) { return finish_device(c.get(), c->devs[g]); }));
    *out = c.release();
    return TFHE_OK;
}
}  // namespace
}  // extern "C++"

/* One-device run of replicate_arena's RCCL sequence against a real librccl (verdict r5 item 4): the stub
 * of tests/stub_rccl restates the API as declared here, so only the real library checks the dlsym table's
 * prototypes, enums and the communicator / group / broadcast / destroy order against the shipped ABI. */
tfhe_status tfhe_rccl_selftest(int device, size_t bytes, const char* lib, int* version) {
    return guarded([&]() -> tfhe_status {
        if (bytes == 0 || bytes % 8) return fail(TFHE_ERR_INVALID_ARGUMENT, "bytes must be a positive multiple of 8");
        if (version) *version = 0;
        const RcclApi& R = rccl(lib ? lib : "");
        if (!R.ok) return fail(TFHE_ERR_UNSUPPORTED, "librccl did not load (or lacks an entry point)");
        if (version && R.version && R.version(version) != ncclSuccess)
            return fail(TFHE_ERR_DEVICE, "ncclGetVersion failed");
        HCHECK(hipSetDevice(device));
        hipStream_t st = nullptr;
        HCHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        struct StreamGuard {
            hipStream_t s;
            ~StreamGuard() { hipStreamDestroy(s); }
        } sg{st};
        DevBuf src, dst;
        HCHECK(hipMalloc(&src.p, bytes));
        HCHECK(hipMalloc(&dst.p, bytes));
        std::vector<uint64_t> h(bytes / 8);
        uint64_t x = 0x9E3779B97F4A7C15ull;  // splitmix64 stream
        for (auto& v : h) {
            uint64_t z = (x += 0x9E3779B97F4A7C15ull);
            z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
            z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
            v = z ^ (z >> 31);
        }
        HCHECK(hipMemcpy(src.p, h.data(), bytes, hipMemcpyHostToDevice));
        HCHECK(hipMemset(dst.p, 0, bytes));
        // one rank, root 0, out of place: the receive buffer gets the send buffer
        if (!rccl_broadcast(R, src.p, bytes, {RcclTarget{device, dst.p, st}}))
            return fail(TFHE_ERR_DEVICE, "RCCL communicator / broadcast failed");
        uint64_t want = 0, got = 0;
        SCHECK(buffer_checksum(device, src.p, bytes, st, want));
        SCHECK(buffer_checksum(device, dst.p, bytes, st, got));
        if (want != got) return fail(TFHE_ERR_DEVICE, "RCCL broadcast delivered a different buffer");
        return TFHE_OK;
    });
}

tfhe_status tfhe_setup(tfhe_ctx** out, const tfhe_params* p, const uint64_t* bsk_coeff, const uint64_t* ksk,
                       int num_gpus) {
    return guarded([&]() -> tfhe_status {
        return setup_common(out, p, bsk_coeff, false, ksk, num_gpus);
    });
}

tfhe_status tfhe_setup_eval(tfhe_ctx** out, const tfhe_params* p, const uint64_t* bsk_eval, const uint64_t* ksk,
                            int num_gpus) {
    return guarded([&]() -> tfhe_status {
        return setup_common(out, p, bsk_eval, true, ksk, num_gpus);
    });
}

// ---------------------------------------------------------------------------
// key generation, encryption, decryption on the device (keygen_kernels.hip)
// ---------------------------------------------------------------------------
extern "C++" {
namespace {
constexpr uint64_t kGamma = 0x9E3779B97F4A7C15ull;  // splitmix64's increment: draw k reads state + (k + 1) gamma

uint64_t host_draw(uint64_t& state) {
    uint64_t z = (state += kGamma);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// The finished parameters of a keygen / encrypt / decrypt call (argument errors come before any HIP call).
tfhe_status finished_params(const tfhe_params* p, tfhe_params& out) {
    if (!p) return fail(TFHE_ERR_INVALID_ARGUMENT, "null params");
    out = *p;
    std::string err;
    if (params_finish(&out, &err) != TFHE_OK) return fail(TFHE_ERR_INVALID_ARGUMENT, err);
    return TFHE_OK;
}
tfhe_status keygen_params(const tfhe_params* p, tfhe_params& out) {
    SCHECK(finished_params(p, out));
    if (!is_prime(out.Q)) return fail(TFHE_ERR_INVALID_ARGUMENT, "Q must be a prime = 1 mod 2N");
    if (keygen_bsk_lds_bytes(out.N, word_bits_for(out), true) > kKeygenMaxLds)
        return fail(TFHE_ERR_UNSUPPORTED, "key generation: a BSK row of this N does not fit the LDS");
    return TFHE_OK;
}

// Host side of one key generation: s and sN (the stream's first n + N draws), NTT(sN) N^-1, the gadget and
// key-switching powers, and the stream states in front of the KSK and BSK rows.  blob holds the small arrays the
// row kernels read (kernels.hpp KeygenTables), uploaded as one buffer; with own_tables it starts with a copy of
// the NTT tables (tfhe_keygen_device has no arena to take them from).
struct KeygenHost {
    KeygenParams kp{};
    std::vector<uint64_t> sk;  // s mod qKS
    uint64_t end_state = 0;    // the stream state after the keys
    std::vector<unsigned char> blob;
    size_t o_psi = 0, o_psi_sh = 0, o_ipsi = 0, o_ipsi_sh = 0, o_snt = 0, o_snt_sh = 0, o_s = 0, o_sN = 0, o_g = 0,
           o_gN = 0, o_pw = 0;
};

void keygen_prepare(const tfhe_params& p, int word_bits, size_t n_pad, uint64_t seed, const NttTables& t,
                    bool own_tables, KeygenHost& h) {
    const uint32_t n = p.n, N = p.N, digits = p.dG2 / 2;
    const size_t wb = word_bits / 8;
    uint64_t state = seed;
    std::vector<int8_t> s(n), sN(N);
    h.sk.resize(n);
    for (uint32_t i = 0; i < n; ++i) {
        s[i] = (int8_t)((int)(host_draw(state) % 3) - 1);
        h.sk[i] = s[i] < 0 ? p.qKS - 1 : (uint64_t)s[i];
    }
    for (uint32_t i = 0; i < N; ++i) sN[i] = (int8_t)((int)(host_draw(state) % 3) - 1);
    KeygenParams& kp = h.kp;
    kp.N = N, kp.n = n, kp.dG2 = p.dG2, kp.baseKS = p.baseKS, kp.dKS = p.dKS, kp.n_pad = (uint32_t)n_pad;
    kp.Q = p.Q, kp.qKS = p.qKS;
    kp.ksk_rows = (size_t)N * p.baseKS * p.dKS;
    kp.bsk_rows = (size_t)n * 2 * p.dG2;
    kp.ksk_state = state;
    kp.bsk_state = kp.ksk_state + (uint64_t)kp.ksk_rows * (n + 2) * kGamma;
    h.end_state = kp.bsk_state + (uint64_t)kp.bsk_rows * 3 * N * kGamma;
    kp.Ninv = t.Ninv;
    kp.Ninv_sh = shoup_companion(t.Ninv, p.Q, word_bits);
    std::vector<uint64_t> snt(N), g(digits), gN(digits), pw(p.dKS);
    for (uint32_t x = 0; x < N; ++x) snt[x] = sN[x] < 0 ? p.Q - 1 : (uint64_t)sN[x];
    host_ntt_fwd(t, snt.data());
    for (uint32_t x = 0; x < N; ++x) snt[x] = mulmod(snt[x], t.Ninv, p.Q);
    for (uint32_t d = 0; d < digits; ++d) {
        g[d] = powmod(p.baseG, d + p.numDigitsToThrow, p.Q);
        gN[d] = mulmod(g[d], t.Ninv, p.Q);
    }
    uint64_t pk = 1 % p.qKS;
    for (uint32_t k = 0; k < p.dKS; ++k, pk = mulmod(pk, p.baseKS, p.qKS)) pw[k] = pk;

    size_t o = 0;
    auto take = [&o](size_t bytes) {
        const size_t at = o;
        o = align_up(o + bytes);
        return at;
    };
    if (own_tables) h.o_psi = take(N * wb), h.o_psi_sh = take(N * wb), h.o_ipsi = take(N * wb), h.o_ipsi_sh = take(N * wb);
    h.o_snt = take(N * wb), h.o_snt_sh = take(N * wb);
    h.o_s = take(n), h.o_sN = take(N);
    h.o_g = take(digits * 8), h.o_gN = take(digits * 8), h.o_pw = take((size_t)p.dKS * 8);
    h.blob.assign(o, 0);
    auto put = [&](size_t off, size_t off_sh, const uint64_t* v) {
        if (word_bits == 32) fill_words<uint32_t>(h.blob, off, v, N), fill_companions<uint32_t>(h.blob, off_sh, v, N, p.Q);
        else fill_words<uint64_t>(h.blob, off, v, N), fill_companions<uint64_t>(h.blob, off_sh, v, N, p.Q);
    };
    if (own_tables) put(h.o_psi, h.o_psi_sh, t.psi_br.data()), put(h.o_ipsi, h.o_ipsi_sh, t.ipsi_br.data());
    put(h.o_snt, h.o_snt_sh, snt.data());
    std::memcpy(h.blob.data() + h.o_s, s.data(), n);
    std::memcpy(h.blob.data() + h.o_sN, sN.data(), N);
    std::memcpy(h.blob.data() + h.o_g, g.data(), digits * 8);
    std::memcpy(h.blob.data() + h.o_gN, gN.data(), digits * 8);
    std::memcpy(h.blob.data() + h.o_pw, pw.data(), (size_t)p.dKS * 8);
}

// dev: the uploaded blob; arena: the context's tables, or null to use the blob's own copy
KeygenTables keygen_tables(const KeygenHost& h, const unsigned char* dev, const DevTables* arena) {
    KeygenTables T{};
    T.psi = arena ? arena->psi : dev + h.o_psi;
    T.psi_sh = arena ? arena->psi_sh : dev + h.o_psi_sh;
    T.ipsi = arena ? arena->ipsi : dev + h.o_ipsi;
    T.ipsi_sh = arena ? arena->ipsi_sh : dev + h.o_ipsi_sh;
    T.snt = dev + h.o_snt;
    T.snt_sh = dev + h.o_snt_sh;
    T.s = reinterpret_cast<const int8_t*>(dev + h.o_s);
    T.sN = reinterpret_cast<const int8_t*>(dev + h.o_sN);
    T.g = reinterpret_cast<const uint64_t*>(dev + h.o_g);
    T.gN = reinterpret_cast<const uint64_t*>(dev + h.o_gN);
    T.pw = reinterpret_cast<const uint64_t*>(dev + h.o_pw);
    return T;
}

tfhe_status check_lwe_call(const tfhe_params* p, const void* sk, size_t B, const void* in, const void* out,
                           uint64_t ptxt_mod, uint64_t mod, tfhe_params& fp) {
    if (!sk || !in || !out) return fail(TFHE_ERR_INVALID_ARGUMENT, "null argument");
    SCHECK(finished_params(p, fp));
    if (B == 0) return fail(TFHE_ERR_INVALID_ARGUMENT, "B must be at least 1");
    if (mod == 0) return fail(TFHE_ERR_INVALID_ARGUMENT, "mod must not be 0");
    if (ptxt_mod == 0 || ptxt_mod > mod) return fail(TFHE_ERR_INVALID_ARGUMENT, "ptxt_mod must be in 1 .. mod");
    return TFHE_OK;
}
}  // namespace
}  // extern "C++"

tfhe_status tfhe_keygen_device(const tfhe_params* p, uint64_t seed, int device, uint64_t* d_sk, uint64_t* d_bsk_coeff,
                               uint64_t* d_ksk, uint64_t* seed_after, void* stream) {
    return guarded([&]() -> tfhe_status {
        if (!d_sk) return fail(TFHE_ERR_INVALID_ARGUMENT, "null argument");
        tfhe_params fp;
        SCHECK(keygen_params(p, fp));
        const int word_bits = word_bits_for(fp);
        KeygenHost h;
        keygen_prepare(fp, word_bits, 0, seed, make_ntt_tables(fp.Q, fp.N), true, h);
        HCHECK(hipSetDevice(device));
        hipStream_t s = (hipStream_t)stream;
        DevBuf blob;
        HCHECK(hipMalloc(&blob.p, h.blob.size()));
        HCHECK(hipMemcpyAsync(blob.p, h.blob.data(), h.blob.size(), hipMemcpyHostToDevice, s));
        HCHECK(hipMemcpyAsync(d_sk, h.sk.data(), sizeof(uint64_t) * fp.n, hipMemcpyHostToDevice, s));
        const KeygenTables T = keygen_tables(h, blob.as<unsigned char>(), nullptr);
        if (d_ksk) HCHECK(launch_keygen_ksk(h.kp, T, 0, d_ksk, nullptr, s));
        if (d_bsk_coeff) HCHECK(launch_keygen_bsk(h.kp, T, word_bits, false, d_bsk_coeff, nullptr, s));
        HCHECK(hipStreamSynchronize(s));  // the kernels read blob and the copies read h
        if (seed_after) *seed_after = h.end_state;
        return TFHE_OK;
    });
}

tfhe_status tfhe_setup_keygen(tfhe_ctx** out, const tfhe_params* p, uint64_t seed, int num_gpus, uint64_t* sk_out,
                              uint64_t* seed_after) {
    return guarded([&]() -> tfhe_status {
        if (!out || !sk_out) return fail(TFHE_ERR_INVALID_ARGUMENT, "null argument");
        *out = nullptr;
        tfhe_params fp;
        SCHECK(keygen_params(p, fp));
        std::unique_ptr<tfhe_ctx> c;
        SCHECK(create_ctx(p, num_gpus, c));
        const ArenaLayout& L = c->layout;
        // host: the table sections (everything below L.bsk) and the small arrays of the row kernels; no buffer
        // here grows with the keys
        const NttTables t = make_ntt_tables(fp.Q, fp.N);
        std::vector<unsigned char> img(L.bsk, 0);
        SCHECK(fill_table_image(c.get(), t, nullptr, img));
        KeygenHost h;
        keygen_prepare(c->p, c->word_bits, L.n_pad, seed, t, false, h);
        const size_t bytes = L.total;
        for (size_t g = 0; g < c->devs.size(); ++g) {
            Device& d = c->devs[g];
            HCHECK(hipSetDevice(d.id));
            SCHECK(create_streams(d));
            HCHECK(hipMalloc(&d.arena, bytes));
        }
        Device& d = c->devs[0];
        HCHECK(hipSetDevice(d.id));
        {
            DevBuf blob;
            HCHECK(hipMalloc(&blob.p, h.blob.size()));
            // gaps between sections and the pad columns of the KSK are zero, as in build_host_image's image
            HCHECK(hipMemsetAsync(d.arena, 0, bytes, d.stream));
            HCHECK(hipMemcpyAsync(d.arena, img.data(), img.size(), hipMemcpyHostToDevice, d.stream));
            HCHECK(hipMemcpyAsync(blob.p, h.blob.data(), h.blob.size(), hipMemcpyHostToDevice, d.stream));
            bind_tables(c.get(), d);
            const KeygenTables T = keygen_tables(h, blob.as<unsigned char>(), &d.tables);
            hipEvent_t ev[3] = {};  // TFHE_TRACE: the two row kernels' device times (tools/keygen_bench.py)
            if (c->kn.trace)
                for (auto& e : ev) HCHECK(hipEventCreate(&e));
            if (c->kn.trace) HCHECK(hipEventRecord(ev[0], d.stream));
            HCHECK(launch_keygen_ksk(h.kp, T, c->ksk_bits, d.arena + L.ksk, d.arena + L.kskb, d.stream));
            if (c->kn.trace) HCHECK(hipEventRecord(ev[1], d.stream));
            HCHECK(launch_keygen_bsk(h.kp, T, c->word_bits, true, d.arena + L.bsk, d.arena + L.bsk_sh, d.stream));
            if (c->kn.trace) HCHECK(hipEventRecord(ev[2], d.stream));
            HCHECK(hipStreamSynchronize(d.stream));
            if (c->kn.trace) {
                float ksk_ms = 0, bsk_ms = 0;
                HCHECK(hipEventElapsedTime(&ksk_ms, ev[0], ev[1]));
                HCHECK(hipEventElapsedTime(&bsk_ms, ev[1], ev[2]));
                for (auto& e : ev) hipEventDestroy(e);
                std::fprintf(stderr, "[tfhe] keygen: ksk %.3f ms, %zu rows, %zu bytes; bsk %.3f ms, %zu rows, %zu bytes\n",
                             ksk_ms, h.kp.ksk_rows, L.kskb + L.ksk_rows * (c->ksk_bits / 8) - L.ksk, bsk_ms,
                             h.kp.bsk_rows, 2 * L.bsk_words * (size_t)(c->word_bits / 8));
            }
        }
        SCHECK(replicate_arena(c.get(), bytes));
        SCHECK(run_shards(
            c->devs.size(), 2 * c->devs.size(),
            [&](size_t g) -> tfhe_status {
                HCHECK(hipSetDevice(c->devs[g].id));
                return TFHE_OK;
            },
            [&](size_t g, size_t, size_t) { return finish_device(c.get(), c->devs[g]); }));
        std::memcpy(sk_out, h.sk.data(), sizeof(uint64_t) * fp.n);
        if (seed_after) *seed_after = h.end_state;
        *out = c.release();
        return TFHE_OK;
    });
}

tfhe_status tfhe_encrypt_device(const tfhe_params* p, int device, const uint64_t* d_sk, size_t B, const int64_t* d_m,
                                uint64_t ptxt_mod, uint64_t mod, uint64_t seed, uint64_t* d_ct, uint64_t* seed_after,
                                void* stream) {
    return guarded([&]() -> tfhe_status {
        tfhe_params fp;
        SCHECK(check_lwe_call(p, d_sk, B, d_m, d_ct, ptxt_mod, mod, fp));
        HCHECK(hipSetDevice(device));
        HCHECK(launch_lwe_encrypt(fp.n, fp.qKS, d_sk, B, d_m, ptxt_mod, mod, seed, d_ct, (hipStream_t)stream));
        if (seed_after) *seed_after = seed + (uint64_t)B * (fp.n + 2) * kGamma;
        return TFHE_OK;
    });
}

tfhe_status tfhe_decrypt_device(const tfhe_params* p, int device, const uint64_t* d_sk, size_t B, const uint64_t* d_ct,
                                uint64_t ptxt_mod, uint64_t mod, int64_t* d_m, void* stream) {
    return guarded([&]() -> tfhe_status {
        tfhe_params fp;
        SCHECK(check_lwe_call(p, d_sk, B, d_ct, d_m, ptxt_mod, mod, fp));
        HCHECK(hipSetDevice(device));
        HCHECK(launch_lwe_decrypt(fp.n, fp.qKS, d_sk, B, d_ct, ptxt_mod, mod, d_m, (hipStream_t)stream));
        return TFHE_OK;
    });
}

tfhe_status tfhe_encrypt(const tfhe_params* p, int device, const uint64_t* sk, size_t B, const int64_t* m,
                         uint64_t ptxt_mod, uint64_t mod, uint64_t seed, uint64_t* ct, uint64_t* seed_after,
                         void* stream) {
    return guarded([&]() -> tfhe_status {
        tfhe_params fp;
        SCHECK(check_lwe_call(p, sk, B, m, ct, ptxt_mod, mod, fp));
        HCHECK(hipSetDevice(device));
        hipStream_t s = (hipStream_t)stream;
        const size_t skb = sizeof(uint64_t) * fp.n, ctb = sizeof(uint64_t) * B * (fp.n + 1);
        DevBuf dsk, dm, dct;
        HCHECK(hipMalloc(&dsk.p, skb));
        HCHECK(hipMalloc(&dm.p, sizeof(int64_t) * B));
        HCHECK(hipMalloc(&dct.p, ctb));
        HCHECK(hipMemcpyAsync(dsk.p, sk, skb, hipMemcpyHostToDevice, s));
        HCHECK(hipMemcpyAsync(dm.p, m, sizeof(int64_t) * B, hipMemcpyHostToDevice, s));
        HCHECK(launch_lwe_encrypt(fp.n, fp.qKS, dsk.as<uint64_t>(), B, dm.as<int64_t>(), ptxt_mod, mod, seed,
                                  dct.as<uint64_t>(), s));
        HCHECK(hipMemcpyAsync(ct, dct.p, ctb, hipMemcpyDeviceToHost, s));
        HCHECK(hipStreamSynchronize(s));
        if (seed_after) *seed_after = seed + (uint64_t)B * (fp.n + 2) * kGamma;
        return TFHE_OK;
    });
}

tfhe_status tfhe_decrypt(const tfhe_params* p, int device, const uint64_t* sk, size_t B, const uint64_t* ct,
                         uint64_t ptxt_mod, uint64_t mod, int64_t* m, void* stream) {
    return guarded([&]() -> tfhe_status {
        tfhe_params fp;
        SCHECK(check_lwe_call(p, sk, B, ct, m, ptxt_mod, mod, fp));
        HCHECK(hipSetDevice(device));
        hipStream_t s = (hipStream_t)stream;
        const size_t skb = sizeof(uint64_t) * fp.n, ctb = sizeof(uint64_t) * B * (fp.n + 1);
        DevBuf dsk, dm, dct;
        HCHECK(hipMalloc(&dsk.p, skb));
        HCHECK(hipMalloc(&dm.p, sizeof(int64_t) * B));
        HCHECK(hipMalloc(&dct.p, ctb));
        HCHECK(hipMemcpyAsync(dsk.p, sk, skb, hipMemcpyHostToDevice, s));
        HCHECK(hipMemcpyAsync(dct.p, ct, ctb, hipMemcpyHostToDevice, s));
        HCHECK(launch_lwe_decrypt(fp.n, fp.qKS, dsk.as<uint64_t>(), B, dct.as<uint64_t>(), ptxt_mod, mod,
                                  dm.as<int64_t>(), s));
        HCHECK(hipMemcpyAsync(m, dm.p, sizeof(int64_t) * B, hipMemcpyDeviceToHost, s));
        HCHECK(hipStreamSynchronize(s));
        return TFHE_OK;
    });
}

tfhe_status tfhe_setup_from_key_image(tfhe_ctx** out, const tfhe_params* p, const void* d_src, size_t bytes,
                                      int device) {
    return guarded([&]() -> tfhe_status {
        if (!out || !d_src) return fail(TFHE_ERR_INVALID_ARGUMENT, "null argument");
        *out = nullptr;
        std::unique_ptr<tfhe_ctx> c;
        SCHECK(create_ctx(p, 1, c));
        if (bytes != c->layout.total) return fail(TFHE_ERR_INVALID_ARGUMENT, "key image size mismatch");
        Device& d = c->devs[0];
        d.id = device;
        HCHECK(hipSetDevice(device));
        SCHECK(create_streams(d));
        HCHECK(hipMalloc(&d.arena, bytes));
        HCHECK(hipMemcpy(d.arena, d_src, bytes, hipMemcpyDeviceToDevice));
        SCHECK(finish_device(c.get(), d));
        *out = c.release();
        return TFHE_OK;
    });
}

namespace {
struct KeyFileHeader {
    char magic[8];  // "TFHEKIMG"
    uint32_t abi;
    uint32_t reserved;
    tfhe_params params;
    uint64_t bytes;
    uint64_t fnv;
};
uint64_t fnv1a64(const unsigned char* p, size_t n) {
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ p[i]) * 1099511628211ull;
    return h;
}
}  // namespace

tfhe_status tfhe_save_key_image(tfhe_ctx* c, const char* path) {
    return guarded([&]() -> tfhe_status {
        SCHECK(check_ctx(c));
        if (!path) return fail(TFHE_ERR_INVALID_ARGUMENT, "null path");
        std::vector<unsigned char> img(c->layout.total);
        HCHECK(hipSetDevice(c->devs[0].id));
        HCHECK(hipStreamSynchronize(c->devs[0].stream));
        HCHECK(hipMemcpy(img.data(), c->devs[0].arena, img.size(), hipMemcpyDeviceToHost));
        KeyFileHeader hdr{};
        std::memcpy(hdr.magic, "TFHEKIMG", 8);
        hdr.abi = (uint32_t)tfhe_abi_version();
        hdr.params = c->p;
        hdr.bytes = img.size();
        hdr.fnv = fnv1a64(img.data(), img.size());
        FILE* f = std::fopen(path, "wb");
        if (!f) return fail(TFHE_ERR_INVALID_ARGUMENT, std::string("cannot open ") + path);
        const bool ok = std::fwrite(&hdr, sizeof(hdr), 1, f) == 1 && std::fwrite(img.data(), 1, img.size(), f) == img.size();
        if (std::fclose(f) != 0 || !ok) return fail(TFHE_ERR_INVALID_ARGUMENT, std::string("write failed: ") + path);
        return TFHE_OK;
    });
}

tfhe_status tfhe_setup_from_key_file(tfhe_ctx** out, const tfhe_params* p, const char* path, int device) {
    return guarded([&]() -> tfhe_status {
        if (!out || !p || !path) return fail(TFHE_ERR_INVALID_ARGUMENT, "null argument");
        *out = nullptr;
        tfhe_params want = *p;
        std::string err;
        if (params_finish(&want, &err) != TFHE_OK) return fail(TFHE_ERR_INVALID_ARGUMENT, err);
        FILE* f = std::fopen(path, "rb");
        if (!f) return fail(TFHE_ERR_INVALID_ARGUMENT, std::string("cannot open ") + path);
        KeyFileHeader hdr{};
        std::vector<unsigned char> img;
        tfhe_status st = TFHE_OK;
        if (std::fread(&hdr, sizeof(hdr), 1, f) != 1 || std::memcmp(hdr.magic, "TFHEKIMG", 8) != 0)
            st = fail(TFHE_ERR_INVALID_ARGUMENT, "not a key image file");
        else if (hdr.abi != (uint32_t)tfhe_abi_version())
            st = fail(TFHE_ERR_INVALID_ARGUMENT, "key image written by another ABI version");
        else if (std::memcmp(&hdr.params, &want, sizeof(want)) != 0)
            st = fail(TFHE_ERR_INVALID_ARGUMENT, "key image parameters differ from the requested ones");
        else if (hdr.bytes != arena_layout(want, word_bits_for(want)).total)  // before any allocation
            st = fail(TFHE_ERR_INVALID_ARGUMENT, "key image size field does not match the parameters");
        else {
            img.resize(hdr.bytes);
            if (std::fread(img.data(), 1, img.size(), f) != img.size())
                st = fail(TFHE_ERR_INVALID_ARGUMENT, "truncated key image file");
            else if (fnv1a64(img.data(), img.size()) != hdr.fnv)
                st = fail(TFHE_ERR_INVALID_ARGUMENT, "key image checksum mismatch");
        }
        std::fclose(f);
        if (st != TFHE_OK) return st;
        std::unique_ptr<tfhe_ctx> c;
        SCHECK(create_ctx(&want, 1, c));
        if (img.size() != c->layout.total) return fail(TFHE_ERR_INVALID_ARGUMENT, "key image size mismatch");
        Device& d = c->devs[0];
        d.id = device;
        HCHECK(hipSetDevice(device));
        SCHECK(create_streams(d));
        HCHECK(hipMalloc(&d.arena, img.size()));
        HCHECK(hipMemcpy(d.arena, img.data(), img.size(), hipMemcpyHostToDevice));
        SCHECK(finish_device(c.get(), d));
        *out = c.release();
        return TFHE_OK;
    });
}

tfhe_status tfhe_export_key_image(tfhe_ctx* c, void* d_dst, size_t bytes, void* stream) {
    return guarded([&]() -> tfhe_status {
        SCHECK(check_ctx(c));
        if (bytes != c->layout.total) return fail(TFHE_ERR_INVALID_ARGUMENT, "key image size mismatch");
        HCHECK(hipSetDevice(c->devs[0].id));
        hipStream_t s = stream ? (hipStream_t)stream : c->devs[0].stream;
        HCHECK(hipMemcpyAsync(d_dst, c->devs[0].arena, bytes, hipMemcpyDeviceToDevice, s));
        HCHECK(hipStreamSynchronize(s));
        return TFHE_OK;
    });
}

tfhe_status tfhe_clean(tfhe_ctx* c) {
    delete c;  // ~tfhe_ctx frees every device
    return TFHE_OK;
}

tfhe_status tfhe_get_info(tfhe_ctx* c, tfhe_info* out) {
    return guarded([&]() -> tfhe_status {
        SCHECK(check_ctx(c));
        if (!out) return fail(TFHE_ERR_INVALID_ARGUMENT, "null output");
        out->num_devices = (int)c->devs.size();
        out->word_bits = c->word_bits;
        out->bsk_device_bytes = c->layout.ksk - c->layout.bsk + (c->use_fast ? bsk_fast_bytes(c->br) : 0) +
                                (c->use_f64 ? bsk_f64_bytes(c->br) : 0) +
                                (c->use_sf ? sf_bytes(c->br) : 0);
        out->ksk_device_bytes = c->layout.total - c->layout.ksk;
        out->bootstraps = c->bootstraps.load();
        out->key_image_bytes = c->layout.total;
        out->br_kernel = c->use_fast  ? TFHE_BR_FAST
                         : c->use_f64 ? (c->f64_fold ? TFHE_BR_F64_FOLD : TFHE_BR_F64)
                         : c->use_sf  ? TFHE_BR_SF
                                      : TFHE_BR_GENERIC;
        out->replicate_method = c->replicate_method;
        out->replicate_ms = c->replicate_ms;
        out->duo_timeouts = 0;
        for (Device& d : c->devs) {
            if (!d.duo.base) continue;
            uint32_t e = 0;
            HCHECK(hipSetDevice(d.id));
            HCHECK(hipStreamSynchronize(d.stream));
            HCHECK(hipMemcpy(&e, (const uint32_t*)d.duo.base + duo_err_offset_words(), 4, hipMemcpyDeviceToHost));
            out->duo_timeouts += e;
        }
        return TFHE_OK;
    });
}

// pair_min follows the mirrored fields (tfhe_knobs is fixed by the ABI version; tfhe_set_pair_min sets it)
static_assert(sizeof(tfhe_knobs) == offsetof(Knobs, pair_min) && sizeof(Knobs) == sizeof(tfhe_knobs) + sizeof(int32_t),
              "tfhe_knobs mirrors tfhe::Knobs field by field up to pair_min");

tfhe_status tfhe_get_knobs(tfhe_ctx* c, tfhe_knobs* out) {
    return guarded([&]() -> tfhe_status {
        SCHECK(check_ctx(c));
        if (!out) return fail(TFHE_ERR_INVALID_ARGUMENT, "null output");
        std::memcpy(out, &c->kn, sizeof(tfhe_knobs));
        return TFHE_OK;
    });
}

tfhe_status tfhe_set_knobs(tfhe_ctx* c, const tfhe_knobs* in) {
    return guarded([&]() -> tfhe_status {
        SCHECK(check_ctx(c));
        if (!in) return fail(TFHE_ERR_INVALID_ARGUMENT, "null knobs");
        Knobs k = c->kn;  // pair_min stays
        std::memcpy(&k, in, sizeof(tfhe_knobs));
        if (const char* why = knob_out_of_range(k)) return fail(TFHE_ERR_INVALID_ARGUMENT, std::string("knob out of range: ") + why);
        if (k.probe != 0 && !f64_test_probes_compiled())
            return fail(TFHE_ERR_UNSUPPORTED, "probe builds exist only in the test library (libtfhe_hip_test.so)");
        c->kn = k;
        return TFHE_OK;
    });
}

tfhe_status tfhe_get_pair_min(tfhe_ctx* c, int32_t* pair_min, uint64_t* pair_launches) {
    return guarded([&]() -> tfhe_status {
        SCHECK(check_ctx(c));
        if (pair_min) *pair_min = c->kn.pair_min;
        if (pair_launches) *pair_launches = c->pair_launches.load(std::memory_order_relaxed);
        return TFHE_OK;
    });
}

tfhe_status tfhe_set_pair_min(tfhe_ctx* c, int32_t pair_min) {
    return guarded([&]() -> tfhe_status {
        SCHECK(check_ctx(c));
        if (pair_min < 0) return fail(TFHE_ERR_INVALID_ARGUMENT, "knob out of range: pair_min (TFHE_PAIR_MIN) < 0");
        c->kn.pair_min = pair_min;
        return TFHE_OK;
    });
}

size_t tfhe_fast4_lds_bytes(int pair) { return fast4_lds_bytes(pair != 0); }

tfhe_status tfhe_shard_range(size_t total, int world, int rank, size_t* lo, size_t* hi) {
    if (world < 1 || rank < 0 || rank >= world || !lo || !hi) return fail(TFHE_ERR_INVALID_ARGUMENT, "bad world/rank");
    size_t l, cnt;
    shard_span(total, (size_t)world, (size_t)rank, &l, &cnt);
    *lo = l, *hi = l + cnt;
    return TFHE_OK;
}

tfhe_status tfhe_host_shard_selftest(size_t B, int devices, int fail_device, size_t* spans) {
    return guarded([&]() -> tfhe_status {
        if (devices < 1 || !spans) return fail(TFHE_ERR_INVALID_ARGUMENT, "bad arguments");
        for (int g = 0; g < devices; ++g) spans[2 * g] = spans[2 * g + 1] = 0;
        return run_shards(
            (size_t)devices, B, [](size_t) { return TFHE_OK; },
            [&](size_t g, size_t lo, size_t cnt) -> tfhe_status {
                spans[2 * g] = lo, spans[2 * g + 1] = cnt;
                if ((int)g == fail_device) return fail(TFHE_ERR_DEVICE, "injected fault on shard [" + std::to_string(lo) +
                                                                            ", " + std::to_string(lo + cnt) + ")");
                return TFHE_OK;
            });
    });
}

tfhe_status tfhe_eval_acc(tfhe_ctx* c, size_t B, const uint64_t* a, uint64_t a_mod, uint64_t* acc) {
    return guarded([&]() -> tfhe_status {
        SCHECK(check_ctx(c));
        if (B == 0) return TFHE_OK;
        if (!a || !acc) return fail(TFHE_ERR_INVALID_ARGUMENT, "null argument");
        const tfhe_params& p = c->p;
        const size_t wacc = 2 * (size_t)p.N;
        // the accumulators go straight into the output set and are rotated there
        return run_lwe_batch(
            c, B, a, p.n, nullptr, 0, acc, wacc,
            [&](Device& d, const uint64_t* i1, const uint64_t*, uint64_t* o, size_t b, size_t) {
                return dev_blind_rotate(c, d, i1, a_mod, o, b);
            },
            WireLim{a_mod, 0, p.Q, p.Q}, acc, true);
    });
}

tfhe_status tfhe_eval_acc_tv(tfhe_ctx* c, size_t B, const uint64_t* a, uint64_t a_mod, const uint64_t* tv,
                             uint32_t tv_len, uint64_t* acc) {
    return guarded([&]() -> tfhe_status {
        SCHECK(check_ctx(c));
        if (B == 0) return TFHE_OK;
        if (!a || !tv || !acc) return fail(TFHE_ERR_INVALID_ARGUMENT, "null argument");
        const tfhe_params& p = c->p;
        if (tv_len == 0 || tv_len > p.N || p.N % tv_len != 0)
            return fail(TFHE_ERR_INVALID_ARGUMENT, "test-vector length must divide N");
        return run_lwe_batch(c, B, a, p.n, tv, tv_len, acc, 2 * (size_t)p.N,
                             [&](Device& d, const uint64_t* i1, const uint64_t* i2, uint64_t* o, size_t b, size_t) {
                                 HCHECK(launch_expand_tv(p.N, tv_len, i2, o, b, d.stream));
                                 return dev_blind_rotate(c, d, i1, a_mod, o, b);
                             },
                             WireLim{a_mod, p.Q, 0, p.Q}, nullptr, true);
    });
}

tfhe_status tfhe_eval_acc_tv_rows(tfhe_ctx* c, size_t B, const uint64_t* const* a_rows, uint64_t a_mod,
                                  const uint64_t* tv, uint32_t tv_len, uint64_t* const* acc_rows) {
    return guarded([&]() -> tfhe_status {
        SCHECK(check_ctx(c));
        if (B == 0) return TFHE_OK;
        if (!a_rows || !tv || !acc_rows) return fail(TFHE_ERR_INVALID_ARGUMENT, "null argument");
        const tfhe_params& p = c->p;
        if (tv_len == 0 || tv_len > p.N || p.N % tv_len != 0)
            return fail(TFHE_ERR_INVALID_ARGUMENT, "test-vector length must divide N");
        for (size_t s = 0; s < B; ++s)
            if (!a_rows[s] || !acc_rows[2 * s] || !acc_rows[2 * s + 1])
                return fail(TFHE_ERR_INVALID_ARGUMENT, "null row pointer");
        return run_lwe_batch_v(c, B, ptr_rows(a_rows, 1, p.n, (const uint64_t*)nullptr), flat_rows(tv, tv_len),
                               ptr_rows(acc_rows, 2, p.N, (uint64_t*)nullptr),
                               [&](Device& d, const uint64_t* i1, const uint64_t* i2, uint64_t* o, size_t b, size_t) {
                                   HCHECK(launch_expand_tv(p.N, tv_len, i2, o, b, d.stream));
                                   return dev_blind_rotate(c, d, i1, a_mod, o, b);
                               },
                               WireLim{a_mod, p.Q, 0, p.Q}, HostIn{}, true);
    });
}

tfhe_status tfhe_eval_acc_device(tfhe_ctx* c, size_t B, const uint64_t* d_a, uint64_t a_mod, uint64_t* d_acc,
                                 void* stream) {
    return guarded([&]() -> tfhe_status {
        SCHECK(check_ctx(c));
        if (B == 0) return TFHE_OK;
        if (!d_a || !d_acc) return fail(TFHE_ERR_INVALID_ARGUMENT, "null argument");
        Device* dp = nullptr;
        SCHECK(device_for(c, d_acc, dp));
        Device& d = *dp;
        HCHECK(hipSetDevice(d.id));
        hipStream_t saved = d.stream;
        if (stream) d.stream = (hipStream_t)stream;
        tfhe_status st = dev_blind_rotate(c, d, d_a, a_mod, d_acc, B);
        d.stream = saved;
        return st;
    });
}

tfhe_status tfhe_mkm_switch(tfhe_ctx* c, size_t B, const uint64_t* ct_ext, uint64_t fmod, uint64_t* out) {
    return guarded([&]() -> tfhe_status {
        SCHECK(check_ctx(c));
        if (B == 0) return TFHE_OK;
        if (!ct_ext || !out) return fail(TFHE_ERR_INVALID_ARGUMENT, "null argument");
        const tfhe_params& p = c->p;
        return run_lwe_batch(c, B, ct_ext, p.N + 1, nullptr, 0, out, p.n + 1,
                             [&](Device& d, const uint64_t* i1, const uint64_t*, uint64_t* o, size_t b, size_t) {
                                 return dev_mkm(c, d, i1, fmod, o, b);
                             },
                             WireLim{p.Q, 0, 0, fmod});
    });
}

tfhe_status tfhe_mkm_switch_rows(tfhe_ctx* c, size_t B, const uint64_t* const* ext_a_rows, const uint64_t* ext_b,
                                 uint64_t fmod, uint64_t* const* out_a_rows, uint64_t* out_b) {
    return guarded([&]() -> tfhe_status {
        SCHECK(check_ctx(c));
        if (B == 0) return TFHE_OK;
        if (!ext_a_rows || !ext_b || !out_a_rows || !out_b) return fail(TFHE_ERR_INVALID_ARGUMENT, "null argument");
        for (size_t s = 0; s < B; ++s)
            if (!ext_a_rows[s] || !out_a_rows[s]) return fail(TFHE_ERR_INVALID_ARGUMENT, "null row pointer");
        const tfhe_params& p = c->p;
        return run_lwe_batch_v(c, B, ptr_rows(ext_a_rows, 1, p.N, ext_b), HostIn{},
                               ptr_rows(out_a_rows, 1, p.n, out_b),
                               [&](Device& d, const uint64_t* i1, const uint64_t*, uint64_t* o, size_t b, size_t) {
                                   return dev_mkm(c, d, i1, fmod, o, b);
                               },
                               WireLim{p.Q, 0, 0, fmod}, HostIn{});
    });
}

tfhe_status tfhe_mkm_switch_device(tfhe_ctx* c, size_t B, const uint64_t* d_ct_ext, uint64_t fmod, uint64_t* d_out,
                                   void* stream) {
    return guarded([&]() -> tfhe_status {
        SCHECK(check_ctx(c));
        if (B == 0) return TFHE_OK;
        if (!d_ct_ext || !d_out) return fail(TFHE_ERR_INVALID_ARGUMENT, "null argument");
        Device* dp = nullptr;
        SCHECK(device_for(c, d_out, dp));
        Device& d = *dp;
        HCHECK(hipSetDevice(d.id));
        SCHECK(ensure_ks_scratch(c, d, B));
        hipStream_t saved = d.stream;
        if (stream) d.stream = (hipStream_t)stream;
        tfhe_status st = sc_acquire(d, d.stream);
        if (st == TFHE_OK) st = dev_mkm(c, d, d_ct_ext, fmod, d_out, B);
        const tfhe_status rel = sc_release(d, d.stream);
        d.stream = saved;
        return st != TFHE_OK ? st : rel;
    });
}

tfhe_status tfhe_eval_bin_gate(tfhe_ctx* c, int gate, size_t B, const uint64_t* ct1, const uint64_t* ct2, uint64_t q,
                               uint64_t* out) {
    return guarded([&]() -> tfhe_status {
        SCHECK(check_ctx(c));
        if (B == 0) return fail(TFHE_ERR_INVALID_ARGUMENT, "EvalBinGate: input vector is empty");
        if (!ct1 || !ct2 || !out) return fail(TFHE_ERR_INVALID_ARGUMENT, "null argument");
        if (ct1 == ct2) return fail(TFHE_ERR_INVALID_ARGUMENT, "Input ciphertexts should be independant");
        if (gate < TFHE_OR || gate > TFHE_XNOR) return fail(TFHE_ERR_INVALID_ARGUMENT, "unknown gate");
        const size_t w = c->p.n + 1;
        return run_lwe_batch(c, B, ct1, w, ct2, w, out, w,
                             [&](Device& d, const uint64_t* i1, const uint64_t* i2, uint64_t* o, size_t b, size_t) {
                                 return dev_gate(c, d, gate, i1, i2, q, o, b);
                             },
                             WireLim{q, q, 0, q});
    });
}

extern "C++" {  // (templates need C++ linkage inside the extern "C" block)
namespace {
// Frame of the device-resident fused ops: the device holding d_out, scratch for B ciphertexts, the
// caller's stream (ordered after every earlier user of the device's scratch, sc_fence).
template <typename F>
tfhe_status run_device_op(tfhe_ctx* c, size_t B, const void* d_out, void* stream, F&& body) {
    Device* dp = nullptr;
    SCHECK(device_for(c, d_out, dp));
    Device& d = *dp;
    HCHECK(hipSetDevice(d.id));
    SCHECK(ensure_scratch(c, d, B));
    hipStream_t saved = d.stream;
    if (stream) d.stream = (hipStream_t)stream;
    tfhe_status st = sc_acquire(d, d.stream);
    if (st == TFHE_OK) st = body(d);
    const tfhe_status rel = sc_release(d, d.stream);  // even after a failed launch: later users wait on it
    d.stream = saved;
    return st != TFHE_OK ? st : rel;
}

// One input of a host-array call: `words` words at `host`, in rows of `row` words.  A null host (an absent bias)
// keeps its room in the block, is not copied, and reaches the device call as null.
struct HostSeg {
    const void* host;
    size_t row, words;
};

// Frame of the host-array form of a device-resident op, on the context's first device: one block
// "in[0] | in[1] | ... | out" whose size in bytes must fit size_t (the callers check their products, this checks
// the sum), the inputs staged in, on_device(device segments, d_out), the output (rows of n+1 words) staged back,
// and the stream drained before the block is freed, on every path.
template <typename F>
tfhe_status run_from_host(tfhe_ctx* c, const char* op, std::initializer_list<HostSeg> in, uint64_t* out,
                          size_t out_words, F&& on_device) {
    const size_t lim = SIZE_MAX / sizeof(uint64_t);
    size_t total = out_words;
    bool fits = total <= lim;
    for (const HostSeg& seg : in) {
        fits = fits && seg.words <= lim - total;
        if (fits) total += seg.words;
    }
    if (!fits) return fail(TFHE_ERR_INVALID_ARGUMENT, std::string(op) + ": sizes overflow");
    Device& d = c->devs[0];
    HCHECK(hipSetDevice(d.id));
    DevBuf buf;
    HCHECK(hipMalloc(&buf.p, total * sizeof(uint64_t)));
    uint64_t* at = buf.as<uint64_t>();
    std::vector<const uint64_t*> d_in;
    tfhe_status st = TFHE_OK;
    for (const HostSeg& seg : in) {
        d_in.push_back(seg.host ? at : nullptr);
        if (st == TFHE_OK && seg.host)
            st = h2d_staged(d, at, flat_rows(static_cast<const uint64_t*>(seg.host), seg.row), seg.words, d.stream);
        at += seg.words;
    }
    if (st == TFHE_OK) st = on_device(d_in.data(), at);
    if (st == TFHE_OK) st = d2h_staged(d, flat_rows(out, c->p.n + 1), at, out_words, d.stream);
    const hipError_t e = hipStreamSynchronize(d.stream);  // before the block is freed, on every path
    if (st == TFHE_OK && e != hipSuccess) st = fail(TFHE_ERR_DEVICE, std::string(op) + ": " + hipGetErrorString(e));
    return st;
}
}  // namespace
}  // extern "C++"

extern "C++" {
namespace {
// The table size every EvalFunc layer admits (N = 0: no context, only the power of two is checked).
tfhe_status check_table_q(const char* who, uint64_t q, uint64_t N) {
    if (q >= 8 && (q & (q - 1)) == 0 && (N == 0 || (2ull * N) % q == 0)) return TFHE_OK;
    return fail(TFHE_ERR_INVALID_ARGUMENT,
                std::string(who) + ": q must be a power of two >= 8" + (N ? " that divides 2N" : ""));
}

// What every call with one table per channel checks of (q, num_luts, inner) before any device call; every
// message names the field.
tfhe_status check_tables_args(const char* who, uint64_t q, uint64_t N, size_t num_luts, size_t inner) {
    const auto bad = [who](const std::string& what) {
        return fail(TFHE_ERR_INVALID_ARGUMENT, std::string(who) + ": " + what);
    };
    if (num_luts == 0) return bad("num_luts is 0");
    if (inner == 0) return bad("inner is 0");
    SCHECK(check_table_q(who, q, N));
    if (num_luts > UINT32_MAX || num_luts > SIZE_MAX / sizeof(uint64_t) / q) return bad("num_luts q overflows");
    if (inner > SIZE_MAX / num_luts) return bad("inner num_luts overflows");
    return TFHE_OK;
}

// The host tables of a host-array call (num_luts = 0: one shared table; else lut[num_luts][q]), classified once
// into `pre` for tab_prepare: an arbitrary one at q > N is refused before anything is allocated or launched.
tfhe_status check_host_tables(tfhe_ctx* c, const uint64_t* lut, size_t num_luts, uint64_t q, TabCall& pre) {
    tab_classify(pre, lut, num_luts, q);
    if (pre.ntab[2] && q > c->p.N) return fail(TFHE_ERR_UNSUPPORTED, "arbitrary function needs q <= N");
    return TFHE_OK;
}

// `words` words of a device table on the host, once the stream's earlier work is done
tfhe_status tab_read_back(Device& d, void* stream, const uint64_t* d_luts, size_t words, std::vector<uint64_t>& host) {
    host.resize(words);
    hipStream_t s = stream ? (hipStream_t)stream : d.stream;
    HCHECK(hipMemcpyAsync(host.data(), d_luts, words * 8, hipMemcpyDeviceToHost, s));
    HCHECK(hipStreamSynchronize(s));
    return TFHE_OK;
}

// The tables of a device call, before its frame opens: the T q words (T = 0: the q words of the shared table)
// read back once and classified one by one, the call refused when an arbitrary table meets q > N, and the class
// table's store in place.  pre: the classes of the same tables, known already (the host-array forms classify
// their host copy: no read-back, no second pass).
tfhe_status tab_prepare(tfhe_ctx* c, Device& d, void* stream, uint64_t q, const uint64_t* d_luts, size_t T, TabCall& tc,
                        const TabCall* pre = nullptr) {
    if (pre) {
        tc = *pre;
    } else {
        std::vector<uint64_t> host;
        SCHECK(tab_read_back(d, stream, d_luts, std::max<size_t>(T, 1) * q, host));
        tab_classify(tc, host.data(), T, q);
    }
    tc.d_luts = d_luts;
    if (tc.ntab[2] && q > c->p.N) return fail(TFHE_ERR_UNSUPPORTED, "arbitrary function needs q <= N");
    // more than one class needs T >= 2: a shared table (T = 0) never reaches the class table's store
    if (tc.classes > 1) SCHECK(ensure_words(d, d.tab_meta, d.tab_meta_words, 2 * T));
    return TFHE_OK;
}

tfhe_status check_func_tables_call(tfhe_ctx* c, size_t B, const void* ct, uint64_t q, const void* luts, size_t num_luts,
                                   size_t inner, const void* out) {
    SCHECK(check_ctx(c));
    if (!ct) return fail(TFHE_ERR_INVALID_ARGUMENT, "EvalFuncTables: null ct");
    if (!luts) return fail(TFHE_ERR_INVALID_ARGUMENT, "EvalFuncTables: null luts");
    if (!out) return fail(TFHE_ERR_INVALID_ARGUMENT, "EvalFuncTables: null out");
    if (B == 0) return fail(TFHE_ERR_INVALID_ARGUMENT, "EvalFuncTables: B is 0");
    SCHECK(check_tables_args("EvalFuncTables", q, c->p.N, num_luts, inner));
    if (B > SIZE_MAX / sizeof(uint64_t) / (c->p.n + 1)) return fail(TFHE_ERR_INVALID_ARGUMENT, "EvalFuncTables: B (n+1) overflows");
    return TFHE_OK;
}

// d_out selects the device
tfhe_status func_tables_on_device(tfhe_ctx* c, size_t B, const uint64_t* d_ct, uint64_t q, const uint64_t* d_luts,
                                  size_t num_luts, size_t inner, uint64_t* d_out, void* stream,
                                  const TabCall* pre = nullptr) {
    Device* dp = nullptr;
    SCHECK(device_for(c, d_out, dp));
    HCHECK(hipSetDevice(dp->id));
    TabCall tc;
    SCHECK(tab_prepare(c, *dp, stream, q, d_luts, num_luts, tc, pre));
    return run_device_op(c, std::min(B, c->max_chunk), d_out, stream, [&](Device& d) {
        SCHECK(tab_upload(d, tc));
        return dev_func_tables_batch(c, d, tc, inner, d_ct, q, d_out, B);
    });
}
}  // namespace
}  // extern "C++"

tfhe_status tfhe_lut_tables_info(uint64_t q, const uint64_t* luts, size_t num_luts, size_t inner, size_t B,
                                 uint8_t* classes, size_t per_class[3], uint64_t* bootstraps) {
    return guarded([&]() -> tfhe_status {
        if (!luts) return fail(TFHE_ERR_INVALID_ARGUMENT, "LutTablesInfo: null luts");
        if (!per_class) return fail(TFHE_ERR_INVALID_ARGUMENT, "LutTablesInfo: null per_class");
        if (!bootstraps) return fail(TFHE_ERR_INVALID_ARGUMENT, "LutTablesInfo: null bootstraps");
        if (B == 0) return fail(TFHE_ERR_INVALID_ARGUMENT, "LutTablesInfo: B is 0");
        SCHECK(check_tables_args("LutTablesInfo", q, 0, num_luts, inner));
        TabCall tc;
        tab_classify(tc, luts, num_luts, q);
        if (classes) std::copy(tc.cls.begin(), tc.cls.end(), classes);
        uint64_t n[3];
        tab_count(tc, inner, B, n);
        for (int k = 0; k < 3; ++k) per_class[k] = (size_t)n[k];
        *bootstraps = n[0] + 2 * (n[1] + n[2]);
        return TFHE_OK;
    });
}

tfhe_status tfhe_eval_func_tables_device(tfhe_ctx* c, size_t B, const uint64_t* d_ct, uint64_t q, const uint64_t* d_luts,
                                         size_t num_luts, size_t inner, uint64_t* d_out, void* stream) {
    return guarded([&]() -> tfhe_status {
        SCHECK(check_func_tables_call(c, B, d_ct, q, d_luts, num_luts, inner, d_out));
        return func_tables_on_device(c, B, d_ct, q, d_luts, num_luts, inner, d_out, stream);
    });
}

tfhe_status tfhe_eval_func_tables(tfhe_ctx* c, size_t B, const uint64_t* ct, uint64_t q, const uint64_t* luts,
                                  size_t num_luts, size_t inner, uint64_t* out) {
    return guarded([&]() -> tfhe_status {
        SCHECK(check_func_tables_call(c, B, ct, q, luts, num_luts, inner, out));
        TabCall pre;
        SCHECK(check_host_tables(c, luts, num_luts, q, pre));
        const size_t w = c->p.n + 1;
        return run_from_host(c, "EvalFuncTables", {{ct, w, B * w}, {luts, q, num_luts * q}}, out, B * w,
                             [&](const uint64_t* const* in, uint64_t* d_out) {
                                 return func_tables_on_device(c, B, in[0], q, in[1], num_luts, inner, d_out, nullptr, &pre);
                             });
    });
}

tfhe_status tfhe_eval_bin_gate_device(tfhe_ctx* c, int gate, size_t B, const uint64_t* d_ct1, const uint64_t* d_ct2,
                                      uint64_t q, uint64_t* d_out, void* stream) {
    return guarded([&]() -> tfhe_status {
        SCHECK(check_ctx(c));
        if (gate < TFHE_OR || gate > TFHE_XNOR) return fail(TFHE_ERR_INVALID_ARGUMENT, "unknown gate");
        if (B == 0) return TFHE_OK;
        if (!d_ct1 || !d_ct2 || !d_out) return fail(TFHE_ERR_INVALID_ARGUMENT, "null argument");
        return run_device_op(c, B, d_out, stream,
                             [&](Device& d) { return dev_gate(c, d, gate, d_ct1, d_ct2, q, d_out, B); });
    });
}

tfhe_status tfhe_eval_func_device(tfhe_ctx* c, size_t B, const uint64_t* d_ct, uint64_t q, const uint64_t* d_lut,
                                  int per_ct_lut, uint64_t* d_out, void* stream) {
    return guarded([&]() -> tfhe_status {
        SCHECK(check_ctx(c));
        if (B == 0) return TFHE_OK;
        if (!d_ct || !d_lut || !d_out) return fail(TFHE_ERR_INVALID_ARGUMENT, "null argument");
        if (q < 4 || (2ull * c->p.N) % q) return fail(TFHE_ERR_INVALID_ARGUMENT, "q must divide 2N");
        // the first LUT classifies the batch (binfhe-base-scheme.cpp:697-698): q words to the host
        Device* dp = nullptr;
        SCHECK(device_for(c, d_out, dp));
        HCHECK(hipSetDevice(dp->id));
        std::vector<uint64_t> lut0;
        SCHECK(tab_read_back(*dp, stream, d_lut, q, lut0));
        const int prop = check_input_function(lut0.data(), q, q);
        return run_device_op(c, B, d_out, stream, [&](Device& d) {
            return dev_func(c, d, prop, d_ct, q, d_lut, per_ct_lut ? q : 0, d_out, B);
        });
    });
}

tfhe_status tfhe_eval_floor_device(tfhe_ctx* c, size_t B, const uint64_t* d_ct, uint64_t mod, uint32_t roundbits,
                                   uint64_t* d_out, void* stream) {
    return guarded([&]() -> tfhe_status {
        SCHECK(check_ctx(c));
        if (B == 0) return TFHE_OK;
        if (!d_ct || !d_out) return fail(TFHE_ERR_INVALID_ARGUMENT, "null argument");
        return run_device_op(c, B, d_out, stream,
                             [&](Device& d) { return dev_floor(c, d, d_ct, mod, roundbits, d_out, B); });
    });
}

tfhe_status tfhe_eval_sign_device(tfhe_ctx* c, size_t B, const uint64_t* d_ct, uint64_t mod, uint64_t* d_out,
                                  void* stream) {
    return guarded([&]() -> tfhe_status {
        SCHECK(check_ctx(c));
        if (B == 0) return TFHE_OK;
        if (!d_ct || !d_out) return fail(TFHE_ERR_INVALID_ARGUMENT, "null argument");
        return run_device_op(c, B, d_out, stream, [&](Device& d) { return dev_sign(c, d, d_ct, mod, d_out, B); });
    });
}

extern "C++" {
namespace {
// what both circuit kinds check of a call (after the context and the circuit handle)
tfhe_status check_circuit_shape(tfhe_ctx* c, uint32_t num_inputs, uint32_t num_outputs, uint32_t bootstraps,
                                size_t instances, const void* in, uint64_t q, const void* out) {
    if (instances == 0) return fail(TFHE_ERR_INVALID_ARGUMENT, "EvalCircuit: no instances");
    if (!out || (!in && num_inputs > 0)) return fail(TFHE_ERR_INVALID_ARGUMENT, "null argument");
    if (q == 0 || (2ull * c->p.N) % q != 0) return fail(TFHE_ERR_INVALID_ARGUMENT, "ciphertext modulus must divide 2N");
    const size_t w = c->p.n + 1, most = std::max<size_t>({num_inputs, num_outputs, bootstraps});
    if (instances > SIZE_MAX / sizeof(uint64_t) / w / most) return fail(TFHE_ERR_INVALID_ARGUMENT, "EvalCircuit: too many instances");
    return TFHE_OK;
}

tfhe_status check_circuit_call(tfhe_ctx* c, const tfhe_circuit* circ, size_t instances, const void* in, uint64_t q,
                               const void* out) {
    SCHECK(check_ctx(c));
    if (!circ) return fail(TFHE_ERR_INVALID_ARGUMENT, "null circuit");
    return check_circuit_shape(c, circ->info.num_inputs, circ->info.num_outputs, circ->info.bootstraps, instances, in, q, out);
}

tfhe_status check_fcircuit_call(tfhe_ctx* c, const tfhe_fcircuit* circ, size_t instances, const void* in, const void* out) {
    SCHECK(check_ctx(c));
    if (!fcircuit_alive(circ)) return fail(TFHE_ERR_INVALID_ARGUMENT, "null, freed or unknown function circuit");
    const tfhe_fcircuit_info& I = circ->info;
    SCHECK(check_circuit_shape(c, I.num_inputs, I.num_outputs, I.bootstraps, instances, in, I.q, out));
    if (I.arbitrary > 0 && I.q > c->p.N) return fail(TFHE_ERR_UNSUPPORTED, "arbitrary function needs q <= N");
    return TFHE_OK;
}

// the host-array form of both circuit kinds: staged through the context's first device around on_device(d_in, d_out)
template <typename F>
tfhe_status circuit_from_host(tfhe_ctx* c, uint32_t num_inputs, uint32_t num_outputs, size_t instances, const uint64_t* in,
                              uint64_t* out, F&& on_device) {
    const size_t w = c->p.n + 1, wi = (size_t)num_inputs * instances * w, wo = (size_t)num_outputs * instances * w;
    // one block in | out (d_out lies wi words into it); a circuit without inputs stages nothing and hands
    // on_device a null d_in
    return run_from_host(c, "EvalCircuit", {{wi ? in : nullptr, w, wi}}, out, wo,
                         [&](const uint64_t* const* d_in, uint64_t* d_out) { return on_device(d_in[0], d_out); });
}

// d_out selects the device; the wire store and the plan are in place before the frame opens
tfhe_status fcircuit_on_device(tfhe_ctx* c, const tfhe_fcircuit* circ, size_t instances, const uint64_t* d_in,
                               uint64_t* d_out, void* stream) {
    Device* dp = nullptr;
    SCHECK(device_for(c, d_out, dp));
    HCHECK(hipSetDevice(dp->id));
    SCHECK(ensure_wires(*dp, (size_t)circ->info.bootstraps * instances * (c->p.n + 1)));
    FuncPlan pl{};
    SCHECK(fcircuit_plan(circ, *dp, pl));
    const size_t widest = std::min((size_t)circ->info.widest_level * instances, c->max_chunk);
    return run_device_op(c, widest, d_out, stream,
                         [&](Device& d) { return dev_fcircuit(c, d, circ, pl, instances, d_in, d_out); });
}

// d_out selects the device; the wire store and the plan are in place before the frame opens
tfhe_status circuit_on_device(tfhe_ctx* c, const tfhe_circuit* circ, size_t instances, const uint64_t* d_in, uint64_t q,
                              uint64_t* d_out, void* stream) {
    Device* dp = nullptr;
    SCHECK(device_for(c, d_out, dp));
    HCHECK(hipSetDevice(dp->id));
    SCHECK(ensure_wires(*dp, (size_t)circ->info.bootstraps * instances * (c->p.n + 1)));
    const CircuitRec* recs = nullptr;
    const CircuitOut* outs = nullptr;
    SCHECK(circuit_plan(circ, *dp, recs, outs));
    const size_t widest = std::min((size_t)circ->info.widest_level * instances, c->max_chunk);
    return run_device_op(c, widest, d_out, stream,
                         [&](Device& d) { return dev_circuit(c, d, circ, recs, outs, instances, d_in, q, d_out); });
}
}  // namespace
}  // extern "C++"

tfhe_status tfhe_eval_circuit_device(tfhe_ctx* c, const tfhe_circuit* circ, size_t instances, const uint64_t* d_in,
                                     uint64_t q, uint64_t* d_out, void* stream) {
    return guarded([&]() -> tfhe_status {
        SCHECK(check_circuit_call(c, circ, instances, d_in, q, d_out));
        return circuit_on_device(c, circ, instances, d_in, q, d_out, stream);
    });
}

tfhe_status tfhe_eval_circuit(tfhe_ctx* c, const tfhe_circuit* circ, size_t instances, const uint64_t* in, uint64_t q,
                              uint64_t* out) {
    return guarded([&]() -> tfhe_status {
        SCHECK(check_circuit_call(c, circ, instances, in, q, out));
        return circuit_from_host(c, circ->info.num_inputs, circ->info.num_outputs, instances, in, out,
                                 [&](const uint64_t* d_in, uint64_t* d_out) {
                                     return circuit_on_device(c, circ, instances, d_in, q, d_out, nullptr);
                                 });
    });
}

tfhe_status tfhe_eval_fcircuit_device(tfhe_ctx* c, const tfhe_fcircuit* circ, size_t instances, const uint64_t* d_in,
                                      uint64_t* d_out, void* stream) {
    return guarded([&]() -> tfhe_status {
        SCHECK(check_fcircuit_call(c, circ, instances, d_in, d_out));
        return fcircuit_on_device(c, circ, instances, d_in, d_out, stream);
    });
}

tfhe_status tfhe_eval_fcircuit(tfhe_ctx* c, const tfhe_fcircuit* circ, size_t instances, const uint64_t* in,
                               uint64_t* out) {
    return guarded([&]() -> tfhe_status {
        SCHECK(check_fcircuit_call(c, circ, instances, in, out));
        return circuit_from_host(c, circ->info.num_inputs, circ->info.num_outputs, instances, in, out,
                                 [&](const uint64_t* d_in, uint64_t* d_out) {
                                     return fcircuit_on_device(c, circ, instances, d_in, d_out, nullptr);
                                 });
    });
}

tfhe_status tfhe_eval_func(tfhe_ctx* c, size_t B, const uint64_t* ct, uint64_t q, const uint64_t* lut, int per_ct_lut,
                           uint64_t* out) {
    return guarded([&]() -> tfhe_status {
        SCHECK(check_ctx(c));
        if (B == 0) return fail(TFHE_ERR_INVALID_ARGUMENT, "EvalFunc: input vector is empty");
        if (!ct || !lut || !out) return fail(TFHE_ERR_INVALID_ARGUMENT, "null argument");
        if (q < 4 || (2ull * c->p.N) % q) return fail(TFHE_ERR_INVALID_ARGUMENT, "q must divide 2N");
        // LUT classification uses the first LUT, as the reference (binfhe-base-scheme.cpp:697-698, 815-816)
        const int prop = check_input_function(lut, q, q);
        const size_t w = c->p.n + 1;
        const uint64_t stride = per_ct_lut ? q : 0;
        // LUTs go to every device once (all of them when per ciphertext), then the batch runs
        // through the pipelined host-array runner
        const size_t D = c->devs.size();
        std::vector<uint64_t*> d_lut(D, nullptr);
        const size_t lut_words = per_ct_lut ? B * q : q;
        tfhe_status st = TFHE_OK;
        for (size_t g = 0; g < D && st == TFHE_OK; ++g) {
            if (hipSetDevice(c->devs[g].id) != hipSuccess || hipMalloc(&d_lut[g], lut_words * 8) != hipSuccess ||
                hipMemcpy(d_lut[g], lut, lut_words * 8, hipMemcpyHostToDevice) != hipSuccess)
                st = fail(TFHE_ERR_OUT_OF_MEMORY, "LUT upload failed");
        }
        if (st == TFHE_OK)
            st = run_lwe_batch(c, B, ct, w, nullptr, 0, out, w,
                               [&](Device& d, const uint64_t* i1, const uint64_t*, uint64_t* o, size_t b, size_t off) {
                                   const size_t g = (size_t)(&d - c->devs.data());  // the device's index (logical devices share an id)
                                   return dev_func(c, d, prop, i1, q, d_lut[g] + (per_ct_lut ? off * q : 0), stride, o, b);
                               },
                               WireLim{q, 0, 0, 0});
        for (size_t g = 0; g < D; ++g)
            if (d_lut[g]) hipSetDevice(c->devs[g].id), hipFree(d_lut[g]);
        return st;
    });
}

tfhe_status tfhe_eval_floor(tfhe_ctx* c, size_t B, const uint64_t* ct, uint64_t mod, uint32_t roundbits,
                            uint64_t* out) {
    return guarded([&]() -> tfhe_status {
        SCHECK(check_ctx(c));
        if (B == 0) return fail(TFHE_ERR_INVALID_ARGUMENT, "EvalFloor: input vector is empty");
        if (!ct || !out) return fail(TFHE_ERR_INVALID_ARGUMENT, "null argument");
        const size_t w = c->p.n + 1;
        return run_lwe_batch(c, B, ct, w, nullptr, 0, out, w,
                             [&](Device& d, const uint64_t* i1, const uint64_t*, uint64_t* o, size_t b, size_t) {
                                 return dev_floor(c, d, i1, mod, roundbits, o, b);
                             },
                             WireLim{mod, 0, 0, 0});
    });
}

tfhe_status tfhe_eval_sign(tfhe_ctx* c, size_t B, const uint64_t* ct, uint64_t mod, uint64_t* out) {
    return guarded([&]() -> tfhe_status {
        SCHECK(check_ctx(c));
        if (B == 0) return fail(TFHE_ERR_INVALID_ARGUMENT, "EvalSign: input vector is empty");
        if (!ct || !out) return fail(TFHE_ERR_INVALID_ARGUMENT, "null argument");
        const size_t w = c->p.n + 1;
        return run_lwe_batch(c, B, ct, w, nullptr, 0, out, w,
                             [&](Device& d, const uint64_t* i1, const uint64_t*, uint64_t* o, size_t b, size_t) {
                                 return dev_sign(c, d, i1, mod, o, b);
                             },
                             WireLim{mod, 0, 0, 0});
    });
}

tfhe_status tfhe_eval_decomp(tfhe_ctx* c, size_t B, const uint64_t* ct, uint64_t mod, uint32_t max_digits,
                             uint64_t* out, uint64_t* moduli, uint32_t* num_digits) {
    return guarded([&]() -> tfhe_status {
        SCHECK(check_ctx(c));
        if (B == 0) return fail(TFHE_ERR_INVALID_ARGUMENT, "EvalDecomp: input vector is empty");
        if (!ct || !out || !moduli || !num_digits) return fail(TFHE_ERR_INVALID_ARGUMENT, "null argument");
        const uint64_t q = c->p.q, beta = 128;
        if (mod <= q) return fail(TFHE_ERR_UNSUPPORTED, "EvalDecomp is only for large precision");
        // digit count and moduli are data independent (binfhe-base-scheme.cpp:1066-1080)
        std::vector<uint64_t> mods;
        for (uint64_t m = mod; m > q; m = m / q * 2 * beta) mods.push_back(q);
        {
            uint64_t m = mod;
            while (m > q) m = m / q * 2 * beta;
            mods.push_back(m);
        }
        if (mods.size() > max_digits) return fail(TFHE_ERR_INVALID_ARGUMENT, "max_digits too small");
        for (size_t i = 0; i < mods.size(); ++i) moduli[i] = mods[i];
        *num_digits = (uint32_t)mods.size();
        const uint32_t n = c->p.n;
        const size_t w = n + 1;
        return for_each_shard(c, B, [&](Device& d, size_t lo, size_t cnt) -> tfhe_status {
            const size_t chunk = std::min(cnt, c->max_chunk);
            SCHECK(ensure_scratch(c, d, chunk));
            SCHECK(sc_acquire(d, d.stream));
            DevBuf tmp_b, fl_b, dig_b;
            HCHECK(hipMalloc(&tmp_b.p, chunk * w * 8));
            HCHECK(hipMalloc(&fl_b.p, chunk * w * 8));
            HCHECK(hipMalloc(&dig_b.p, chunk * w * 8));
            uint64_t *tmp = tmp_b.as<uint64_t>(), *fl = fl_b.as<uint64_t>(), *dig = dig_b.as<uint64_t>();
            std::vector<uint64_t> host_digit(chunk * w);
            tfhe_status st = TFHE_OK;
            Drain drain{d.stream};  // every exit below leaves the stream drained before the DevBufs free their memory
            for (size_t off = lo; off < lo + cnt && st == TFHE_OK; off += chunk) {
                const size_t b = std::min(chunk, lo + cnt - off);
                HCHECK(hipMemcpyAsync(tmp, ct + off * w, b * w * 8, hipMemcpyHostToDevice, d.stream));
                uint64_t m = mod;
                for (size_t k = 0; k < mods.size() && st == TFHE_OK; ++k) {
                    if (k + 1 < mods.size()) HCHECK(launch_lwe_op(LWE_SET_MOD, n, q, 0, tmp, nullptr, dig, b, d.stream));
                    else HCHECK(hipMemcpyAsync(dig, tmp, b * w * 8, hipMemcpyDeviceToDevice, d.stream));
                    HCHECK(hipMemcpyAsync(host_digit.data(), dig, b * w * 8, hipMemcpyDeviceToHost, d.stream));
                    HCHECK(hipStreamSynchronize(d.stream));
                    for (size_t s = 0; s < b; ++s)
                        std::memcpy(out + ((off + s) * max_digits + k) * w, host_digit.data() + s * w, w * 8);
                    if (k + 1 < mods.size()) {
                        st = dev_floor(c, d, tmp, m, 0, fl, b);
                        if (st != TFHE_OK) break;
                        const uint64_t nm = m / q * 2 * beta;
                        HCHECK(launch_lwe_op(LWE_MODSWITCH, n, nm, m, fl, nullptr, tmp, b, d.stream));
                        m = nm;
                    }
                }
            }
            return st;
        });
    });
}

extern "C++" {
namespace {
// what the matrix-product calls check of their sizes: none zero, no product that overflows size_t in bytes
tfhe_status check_mm_sizes(tfhe_ctx* c, size_t instances, size_t K, size_t cols, uint64_t modulus) {
    if (instances == 0) return fail(TFHE_ERR_INVALID_ARGUMENT, "CiphertextMulMatrix: no instances");
    if (K == 0) return fail(TFHE_ERR_INVALID_ARGUMENT, "Input ciphertexts are empty.");
    if (cols == 0) return fail(TFHE_ERR_INVALID_ARGUMENT, "Input matrix is empty.");
    if (modulus == 0) return fail(TFHE_ERR_INVALID_ARGUMENT, "modulus is 0");
    const size_t w = c->p.n + 1, lim = SIZE_MAX / sizeof(uint64_t);
    if (K > lim / cols || K > lim / w || instances > lim / w / K || cols > lim / w || instances > lim / w / cols)
        return fail(TFHE_ERR_INVALID_ARGUMENT, "CiphertextMulMatrix: sizes overflow");
    return TFHE_OK;
}

// d_out selects the device; the residue store is in place before the frame opens
tfhe_status mul_matrix_on_device(tfhe_ctx* c, size_t instances, size_t K, const uint64_t* d_ct, size_t cols,
                                 const int64_t* d_matrix, const uint64_t* d_bias, uint64_t modulus, uint64_t* d_out,
                                 void* stream) {
    Device* dp = nullptr;
    SCHECK(device_for(c, d_out, dp));
    HCHECK(hipSetDevice(dp->id));
    SCHECK(ensure_words(*dp, dp->mm_mat, dp->mm_mat_words, K * cols));
    return run_device_op(c, 0, d_out, stream, [&](Device& d) {
        return dev_mul_matrix(c, d, instances, K, d_ct, cols, d_matrix, d_bias, modulus, d_out);
    });
}

tfhe_status check_dense_call(tfhe_ctx* c, size_t instances, size_t K, const void* ct, size_t cols, const void* matrix,
                             uint64_t q, const void* lut, const void* out) {
    SCHECK(check_ctx(c));
    if (!ct || !matrix || !lut || !out) return fail(TFHE_ERR_INVALID_ARGUMENT, "null argument");
    SCHECK(check_mm_sizes(c, instances, K, cols, q));
    return check_table_q("EvalDense", q, c->p.N);
}

// d_out selects the device; the tables are read back once and classified (pre: the host-array form's classes of
// its host copy).  num_luts = 0: d_lut is one shared table [q]; else [num_luts = cols][q], one per column
tfhe_status dense_on_device(tfhe_ctx* c, size_t instances, size_t K, const uint64_t* d_ct, size_t cols,
                            const int64_t* d_matrix, const uint64_t* d_bias, uint64_t q, const uint64_t* d_lut,
                            uint64_t* d_out, void* stream, size_t num_luts = 0, const TabCall* pre = nullptr) {
    Device* dp = nullptr;
    SCHECK(device_for(c, d_out, dp));
    HCHECK(hipSetDevice(dp->id));
    TabCall tc;
    SCHECK(tab_prepare(c, *dp, stream, q, d_lut, num_luts, tc, pre));
    SCHECK(ensure_words(*dp, dp->mm_mat, dp->mm_mat_words, K * cols));
    SCHECK(ensure_words(*dp, dp->dense_z, dp->dense_z_words, instances * cols * (c->p.n + 1)));
    return run_device_op(c, std::min(instances * cols, c->max_chunk), d_out, stream, [&](Device& d) {
        SCHECK(tab_upload(d, tc));
        return dev_dense(c, d, instances, K, d_ct, cols, d_matrix, d_bias, q, tc, d_out);
    });
}
}  // namespace
}  // extern "C++"

tfhe_status tfhe_ciphertext_mul_matrix(tfhe_ctx* c, size_t K, const uint64_t* ct, size_t cols, const int64_t* matrix,
                                       uint64_t modulus, uint64_t* out) {
    return guarded([&]() -> tfhe_status {
        SCHECK(check_ctx(c));
        if (K == 0) return fail(TFHE_ERR_INVALID_ARGUMENT, "Input ciphertexts are empty.");
        if (cols == 0) return fail(TFHE_ERR_INVALID_ARGUMENT, "Input matrix is empty.");
        if (!ct || !matrix || !out || modulus == 0) return fail(TFHE_ERR_INVALID_ARGUMENT, "null argument");
        SCHECK(check_mm_sizes(c, 1, K, cols, modulus));
        const uint32_t w = c->p.n + 1;
        Device& d = c->devs[0];
        HCHECK(hipSetDevice(d.id));
        DevBuf dct, dm, dout;
        HCHECK(hipMalloc(&dct.p, K * w * 8));
        HCHECK(hipMalloc(&dm.p, K * cols * 8));
        HCHECK(hipMalloc(&dout.p, cols * w * 8));
        Drain drain{d.stream};
        HCHECK(hipMemcpyAsync(dct.p, ct, K * w * 8, hipMemcpyHostToDevice, d.stream));
        HCHECK(hipMemcpyAsync(dm.p, matrix, K * cols * 8, hipMemcpyHostToDevice, d.stream));
        SCHECK(ensure_words(d, d.mm_mat, d.mm_mat_words, K * cols));
        hipStream_t s = d.stream;  // device 0's own frame (d_out would select among logical devices by id)
        tfhe_status st = sc_acquire(d, s);
        if (st == TFHE_OK)
            st = dev_mul_matrix(c, d, 1, K, dct.as<uint64_t>(), cols, dm.as<int64_t>(), nullptr, modulus,
                                dout.as<uint64_t>());
        const tfhe_status rel = sc_release(d, s);
        if (st != TFHE_OK) return st;
        SCHECK(rel);
        HCHECK(hipMemcpyAsync(out, dout.p, cols * w * 8, hipMemcpyDeviceToHost, d.stream));
        HCHECK(hipStreamSynchronize(d.stream));
        return TFHE_OK;
    });
}

tfhe_status tfhe_ciphertext_mul_matrix_device(tfhe_ctx* c, size_t instances, size_t K, const uint64_t* d_ct,
                                              size_t cols, const int64_t* d_matrix, const uint64_t* d_bias,
                                              uint64_t modulus, uint64_t* d_out, void* stream) {
    return guarded([&]() -> tfhe_status {
        SCHECK(check_ctx(c));
        if (!d_ct || !d_matrix || !d_out) return fail(TFHE_ERR_INVALID_ARGUMENT, "null argument");
        SCHECK(check_mm_sizes(c, instances, K, cols, modulus));
        return mul_matrix_on_device(c, instances, K, d_ct, cols, d_matrix, d_bias, modulus, d_out, stream);
    });
}

tfhe_status tfhe_eval_dense_device(tfhe_ctx* c, size_t instances, size_t K, const uint64_t* d_ct, size_t cols,
                                   const int64_t* d_matrix, const uint64_t* d_bias, uint64_t q, const uint64_t* d_lut,
                                   uint64_t* d_out, void* stream) {
    return guarded([&]() -> tfhe_status {
        SCHECK(check_dense_call(c, instances, K, d_ct, cols, d_matrix, q, d_lut, d_out));
        return dense_on_device(c, instances, K, d_ct, cols, d_matrix, d_bias, q, d_lut, d_out, stream);
    });
}

extern "C++" {
namespace {
// what the layers with one table per channel check on top of the layer's own rules
tfhe_status check_layer_tables(tfhe_ctx* c, const char* who, uint64_t q, size_t num_luts, size_t channels,
                               const char* channels_name) {
    SCHECK(check_tables_args(who, q, c->p.N, num_luts, 1));
    if (num_luts != channels)
        return fail(TFHE_ERR_INVALID_ARGUMENT, std::string(who) + ": num_luts must equal " + channels_name);
    return TFHE_OK;
}

// the host-array dense layer; num_luts = 0: one shared table, else lut[num_luts = cols][q]
tfhe_status dense_from_host(tfhe_ctx* c, size_t instances, size_t K, const uint64_t* ct, size_t cols,
                            const int64_t* matrix, const uint64_t* bias, uint64_t q, const uint64_t* lut,
                            uint64_t* out, size_t num_luts) {
    TabCall pre;
    SCHECK(check_host_tables(c, lut, num_luts, q, pre));
    const size_t w = c->p.n + 1, wl = std::max<size_t>(num_luts, 1) * q;
    return run_from_host(
        c, "EvalDense", {{ct, w, instances * K * w}, {matrix, cols, K * cols}, {bias, cols, cols}, {lut, q, wl}}, out,
        instances * cols * w, [&](const uint64_t* const* in, uint64_t* d_out) {
            return dense_on_device(c, instances, K, in[0], cols, reinterpret_cast<const int64_t*>(in[1]), in[2], q,
                                   in[3], d_out, nullptr, num_luts, &pre);
        });
}
}  // namespace
}  // extern "C++"

tfhe_status tfhe_eval_dense(tfhe_ctx* c, size_t instances, size_t K, const uint64_t* ct, size_t cols,
                            const int64_t* matrix, const uint64_t* bias, uint64_t q, const uint64_t* lut,
                            uint64_t* out) {
    return guarded([&]() -> tfhe_status {
        SCHECK(check_dense_call(c, instances, K, ct, cols, matrix, q, lut, out));
        return dense_from_host(c, instances, K, ct, cols, matrix, bias, q, lut, out, 0);
    });
}

tfhe_status tfhe_eval_dense_tables_device(tfhe_ctx* c, size_t instances, size_t K, const uint64_t* d_ct, size_t cols,
                                          const int64_t* d_matrix, const uint64_t* d_bias, uint64_t q,
                                          const uint64_t* d_luts, size_t num_luts, uint64_t* d_out, void* stream) {
    return guarded([&]() -> tfhe_status {
        SCHECK(check_dense_call(c, instances, K, d_ct, cols, d_matrix, q, d_luts, d_out));
        SCHECK(check_layer_tables(c, "EvalDense", q, num_luts, cols, "cols"));
        return dense_on_device(c, instances, K, d_ct, cols, d_matrix, d_bias, q, d_luts, d_out, stream, num_luts);
    });
}

tfhe_status tfhe_eval_dense_tables(tfhe_ctx* c, size_t instances, size_t K, const uint64_t* ct, size_t cols,
                                   const int64_t* matrix, const uint64_t* bias, uint64_t q, const uint64_t* luts,
                                   size_t num_luts, uint64_t* out) {
    return guarded([&]() -> tfhe_status {
        SCHECK(check_dense_call(c, instances, K, ct, cols, matrix, q, luts, out));
        SCHECK(check_layer_tables(c, "EvalDense", q, num_luts, cols, "cols"));
        return dense_from_host(c, instances, K, ct, cols, matrix, bias, q, luts, out, num_luts);
    });
}

void tfhe_mm_tiles(int* kt, int* ct, int* threads) {
    if (kt) *kt = MM_KT;
    if (ct) *ct = MM_CT;
    if (threads) *threads = MM_THREADS;
}

extern "C++" {
namespace {
// the descriptor's own rules (no context, no device): every message names the field
// (the pooling descriptor passes through here as a depthwise convolution: `who` and the name of its planes field)
tfhe_status conv_geometry(const tfhe_conv2d* d, ConvGeom& g, size_t& K, const char* who = "Conv2d",
                          const char* planes = "c_in") {
    const auto bad = [who](const std::string& what) {
        return fail(TFHE_ERR_INVALID_ARGUMENT, std::string(who) + ": " + what);
    };
    if (!d) return bad("null descriptor");
    const struct {
        uint32_t v;
        const char* name;
    } nonzero[] = {{d->c_in, planes}, {d->h, "h"}, {d->w, "w"}, {d->c_out, "c_out"}, {d->kh, "kh"}, {d->kw, "kw"},
                   {d->stride_h, "stride_h"}, {d->stride_w, "stride_w"}, {d->groups, "groups"}};
    for (const auto& f : nonzero)
        if (f.v == 0) return bad(std::string(f.name) + " is 0");
    if (d->c_in % d->groups != 0) return bad("groups does not divide c_in");
    if (d->c_out % d->groups != 0) return bad("groups does not divide c_out");
    if (d->pad_h >= d->kh) return bad("pad_h must be below kh");
    if (d->pad_w >= d->kw) return bad("pad_w must be below kw");
    if (d->kh > (uint64_t)d->h + 2ull * d->pad_h) return bad("kh exceeds h + 2 pad_h");
    if (d->kw > (uint64_t)d->w + 2ull * d->pad_w) return bad("kw exceeds w + 2 pad_w");
    const uint64_t oh = ((uint64_t)d->h + 2ull * d->pad_h - d->kh) / d->stride_h + 1,
                   ow = ((uint64_t)d->w + 2ull * d->pad_w - d->kw) / d->stride_w + 1;
    if (oh > UINT32_MAX) return bad("h + 2 pad_h overflows");
    if (ow > UINT32_MAX) return bad("w + 2 pad_w overflows");
    g = ConvGeom{d->c_in, d->h, d->w, d->c_out, d->kh, d->kw, d->stride_h, d->stride_w, d->pad_h, d->pad_w, d->groups,
                 (uint32_t)oh, (uint32_t)ow};
    const uint64_t khw = (uint64_t)d->kh * d->kw;  // below 2^64
    const size_t Cg = d->c_in / d->groups;
    if (khw > SIZE_MAX / Cg) return bad("c_in kh kw overflows");
    K = (size_t)(Cg * khw);
    return TFHE_OK;
}

// acc *= f unless that leaves size_t
bool conv_mul(size_t& acc, size_t f) {
    if (f != 0 && acc > SIZE_MAX / f) return false;
    acc *= f;
    return true;
}

// what the convolution calls check before any device call; d_bias may be null
tfhe_status check_conv_call(tfhe_ctx* c, const tfhe_conv2d* desc, size_t instances, const void* ct, const void* weight,
                            uint64_t modulus, const void* out, ConvGeom& g, size_t& K) {
    SCHECK(check_ctx(c));
    if (!desc) return fail(TFHE_ERR_INVALID_ARGUMENT, "Conv2d: null descriptor");
    if (!ct) return fail(TFHE_ERR_INVALID_ARGUMENT, "Conv2d: null ct");
    if (!weight) return fail(TFHE_ERR_INVALID_ARGUMENT, "Conv2d: null weight");
    if (!out) return fail(TFHE_ERR_INVALID_ARGUMENT, "Conv2d: null out");
    if (instances == 0) return fail(TFHE_ERR_INVALID_ARGUMENT, "Conv2d: instances is 0");
    SCHECK(conv_geometry(desc, g, K));
    if (modulus == 0) return fail(TFHE_ERR_INVALID_ARGUMENT, "Conv2d: modulus is 0");
    const size_t w = c->p.n + 1;
    size_t in = sizeof(uint64_t), res = sizeof(uint64_t), wt = sizeof(uint64_t);
    const bool ok = conv_mul(in, instances) && conv_mul(in, g.c_in) && conv_mul(in, g.h) && conv_mul(in, g.w) &&
                    conv_mul(in, w) && conv_mul(res, instances) && conv_mul(res, g.c_out) && conv_mul(res, g.oh) &&
                    conv_mul(res, g.ow) && conv_mul(res, w) && conv_mul(wt, g.c_out) && conv_mul(wt, K);
    if (!ok) return fail(TFHE_ERR_INVALID_ARGUMENT, "Conv2d: sizes overflow");
    return TFHE_OK;
}

tfhe_status check_conv_layer_call(tfhe_ctx* c, const tfhe_conv2d* desc, size_t instances, const void* ct,
                                  const void* weight, uint64_t q, const void* lut, const void* out, ConvGeom& g,
                                  size_t& K) {
    SCHECK(check_conv_call(c, desc, instances, ct, weight, q, out, g, K));
    if (!lut) return fail(TFHE_ERR_INVALID_ARGUMENT, "EvalConv2d: null lut");
    return check_table_q("EvalConv2d", q, c->p.N);
}

// d_out selects the device; the tables as in dense_on_device.  num_luts = 0: d_lut is one shared table [q]; else
// [num_luts = c_out][q], one per output plane
tfhe_status conv_layer_on_device(tfhe_ctx* c, const ConvGeom& g, size_t K, size_t instances, const uint64_t* d_ct,
                                 const int64_t* d_weight, const uint64_t* d_bias, uint64_t q, const uint64_t* d_lut,
                                 uint64_t* d_out, void* stream, size_t num_luts = 0, const TabCall* pre = nullptr) {
    Device* dp = nullptr;
    SCHECK(device_for(c, d_out, dp));
    HCHECK(hipSetDevice(dp->id));
    TabCall tc;
    SCHECK(tab_prepare(c, *dp, stream, q, d_lut, num_luts, tc, pre));
    const size_t total = instances * g.c_out * g.oh * g.ow;
    SCHECK(ensure_words(*dp, dp->mm_mat, dp->mm_mat_words, K * g.c_out));
    SCHECK(ensure_words(*dp, dp->dense_z, dp->dense_z_words, total * (c->p.n + 1)));
    return run_device_op(c, std::min(total, c->max_chunk), d_out, stream, [&](Device& d) {
        SCHECK(tab_upload(d, tc));
        return dev_conv_layer(c, d, g, instances, d_ct, d_weight, d_bias, q, tc, d_out);
    });
}
}  // namespace
}  // extern "C++"

tfhe_status tfhe_conv2d_shape(const tfhe_conv2d* d, uint32_t* oh, uint32_t* ow, size_t* K) {
    return guarded([&]() -> tfhe_status {
        ConvGeom g;
        size_t k = 0;
        SCHECK(conv_geometry(d, g, k));
        if (oh) *oh = g.oh;
        if (ow) *ow = g.ow;
        if (K) *K = k;
        return TFHE_OK;
    });
}

tfhe_status tfhe_ciphertext_conv2d_device(tfhe_ctx* c, const tfhe_conv2d* desc, size_t instances, const uint64_t* d_ct,
                                          const int64_t* d_weight, const uint64_t* d_bias, uint64_t modulus,
                                          uint64_t* d_out, void* stream) {
    return guarded([&]() -> tfhe_status {
        ConvGeom g;
        size_t K = 0;
        SCHECK(check_conv_call(c, desc, instances, d_ct, d_weight, modulus, d_out, g, K));
        Device* dp = nullptr;
        SCHECK(device_for(c, d_out, dp));
        HCHECK(hipSetDevice(dp->id));
        SCHECK(ensure_words(*dp, dp->mm_mat, dp->mm_mat_words, K * g.c_out));
        return run_device_op(c, 0, d_out, stream, [&](Device& d) {
            return dev_conv2d(c, d, g, instances, d_ct, d_weight, d_bias, modulus, d_out);
        });
    });
}

tfhe_status tfhe_eval_conv2d_device(tfhe_ctx* c, const tfhe_conv2d* desc, size_t instances, const uint64_t* d_ct,
                                    const int64_t* d_weight, const uint64_t* d_bias, uint64_t q, const uint64_t* d_lut,
                                    uint64_t* d_out, void* stream) {
    return guarded([&]() -> tfhe_status {
        ConvGeom g;
        size_t K = 0;
        SCHECK(check_conv_layer_call(c, desc, instances, d_ct, d_weight, q, d_lut, d_out, g, K));
        return conv_layer_on_device(c, g, K, instances, d_ct, d_weight, d_bias, q, d_lut, d_out, stream);
    });
}

extern "C++" {
namespace {
// the host-array convolution layer; num_luts = 0: one shared table, else lut[num_luts = c_out][q]
tfhe_status conv_layer_from_host(tfhe_ctx* c, const ConvGeom& g, size_t K, size_t instances, const uint64_t* ct,
                                 const int64_t* weight, const uint64_t* bias, uint64_t q, const uint64_t* lut,
                                 uint64_t* out, size_t num_luts) {
    TabCall pre;
    SCHECK(check_host_tables(c, lut, num_luts, q, pre));
    const size_t w = c->p.n + 1, wi = instances * g.c_in * g.h * g.w * w, nb = g.c_out,
                 wo = instances * g.c_out * g.oh * g.ow * w, wl = std::max<size_t>(num_luts, 1) * q;
    return run_from_host(c, "EvalConv2d", {{ct, w, wi}, {weight, K, K * nb}, {bias, nb, nb}, {lut, q, wl}}, out, wo,
                         [&](const uint64_t* const* in, uint64_t* d_out) {
                             return conv_layer_on_device(c, g, K, instances, in[0], reinterpret_cast<const int64_t*>(in[1]),
                                                         in[2], q, in[3], d_out, nullptr, num_luts, &pre);
                         });
}
}  // namespace
}  // extern "C++"

tfhe_status tfhe_eval_conv2d(tfhe_ctx* c, const tfhe_conv2d* desc, size_t instances, const uint64_t* ct,
                             const int64_t* weight, const uint64_t* bias, uint64_t q, const uint64_t* lut,
                             uint64_t* out) {
    return guarded([&]() -> tfhe_status {
        ConvGeom g;
        size_t K = 0;
        SCHECK(check_conv_layer_call(c, desc, instances, ct, weight, q, lut, out, g, K));
        return conv_layer_from_host(c, g, K, instances, ct, weight, bias, q, lut, out, 0);
    });
}

tfhe_status tfhe_eval_conv2d_tables_device(tfhe_ctx* c, const tfhe_conv2d* desc, size_t instances, const uint64_t* d_ct,
                                           const int64_t* d_weight, const uint64_t* d_bias, uint64_t q,
                                           const uint64_t* d_luts, size_t num_luts, uint64_t* d_out, void* stream) {
    return guarded([&]() -> tfhe_status {
        ConvGeom g;
        size_t K = 0;
        SCHECK(check_conv_layer_call(c, desc, instances, d_ct, d_weight, q, d_luts, d_out, g, K));
        SCHECK(check_layer_tables(c, "EvalConv2d", q, num_luts, g.c_out, "c_out"));
        return conv_layer_on_device(c, g, K, instances, d_ct, d_weight, d_bias, q, d_luts, d_out, stream, num_luts);
    });
}

tfhe_status tfhe_eval_conv2d_tables(tfhe_ctx* c, const tfhe_conv2d* desc, size_t instances, const uint64_t* ct,
                                    const int64_t* weight, const uint64_t* bias, uint64_t q, const uint64_t* luts,
                                    size_t num_luts, uint64_t* out) {
    return guarded([&]() -> tfhe_status {
        ConvGeom g;
        size_t K = 0;
        SCHECK(check_conv_layer_call(c, desc, instances, ct, weight, q, luts, out, g, K));
        SCHECK(check_layer_tables(c, "EvalConv2d", q, num_luts, g.c_out, "c_out"));
        return conv_layer_from_host(c, g, K, instances, ct, weight, bias, q, luts, out, num_luts);
    });
}

void tfhe_conv2d_tiles(int* kt, int* ct, int* threads, int* positions) {
    if (kt) *kt = CV_KT;
    if (ct) *ct = CV_CT;
    if (threads) *threads = CV_THREADS;
    if (positions) *positions = CV_P;
}

extern "C++" {
namespace {
// the descriptor's rules are the convolution's, by the convolution's code: a pooling window is a depthwise one
tfhe_status pool_geometry(const tfhe_pool2d* d, PoolGeom& g, uint32_t& rounds, size_t& pairs) {
    if (!d) return fail(TFHE_ERR_INVALID_ARGUMENT, "Pool2d: null descriptor");
    const tfhe_conv2d cd{d->c, d->h, d->w, d->c, d->kh, d->kw, d->stride_h, d->stride_w, d->pad_h, d->pad_w, d->c};
    ConvGeom cg;
    size_t K = 0;
    SCHECK(conv_geometry(&cd, cg, K, "Pool2d", "c"));
    g = PoolGeom{d->c, d->h, d->w, d->kh, d->kw, d->stride_h, d->stride_w, d->pad_h, d->pad_w, cg.oh, cg.ow};
    if (!pool_counts(g, rounds, pairs)) return fail(TFHE_ERR_INVALID_ARGUMENT, "Pool2d: sizes overflow");
    return TFHE_OK;
}

// what the pooling calls check before any device call (N = 0: no context); `words` is n+1, or 1 for clear values
tfhe_status check_pool_args(const char* who, const tfhe_pool2d* desc, size_t instances, const void* in, uint64_t q,
                            uint64_t N, const void* lut, const void* out, size_t words, PoolGeom& g, size_t& pairs) {
    const auto bad = [who](const std::string& what) {
        return fail(TFHE_ERR_INVALID_ARGUMENT, std::string(who) + ": " + what);
    };
    if (!desc) return bad("null descriptor");
    if (!in) return bad("null ct");
    if (!lut) return bad("null lut");
    if (!out) return bad("null out");
    if (instances == 0) return bad("instances is 0");
    uint32_t rounds = 0;
    SCHECK(pool_geometry(desc, g, rounds, pairs));
    SCHECK(check_table_q(who, q, N));
    size_t src = sizeof(uint64_t), res = sizeof(uint64_t), mid = sizeof(PoolRec);
    // inputs, outputs, and what the pairs can need at most: a record each; a slot and two flat rows each
    const bool ok = conv_mul(src, instances) && conv_mul(src, g.c) && conv_mul(src, g.h) && conv_mul(src, g.w) &&
                    conv_mul(src, words) && conv_mul(res, instances) && conv_mul(res, g.c) && conv_mul(res, g.oh) &&
                    conv_mul(res, g.ow) && conv_mul(res, words) && conv_mul(mid, instances) && conv_mul(mid, g.c) &&
                    conv_mul(mid, pairs ? pairs : 1) && conv_mul(mid, words);
    if (!ok) return bad("sizes overflow");
    return TFHE_OK;
}

// the device copy of the plan of `g`: built and uploaded on first use, then kept
tfhe_status pool_plan_on_device(Device& d, const PoolGeom& g, const Device::PoolPlanDev*& out) {
    for (const auto& pp : d.pool_plans)
        if (std::memcmp(&pp.g, &g, sizeof g) == 0) {
            out = &pp;
            return TFHE_OK;
        }
    const PoolPlan plan = pool_plan(g);
    Device::PoolPlanDev pp;
    pp.g = g, pp.round_first = plan.round_first, pp.copies = plan.copies, pp.slots = plan.slots;
    pp.widest = plan.widest();
    if (!plan.recs.empty()) {
        HCHECK(hipMalloc(&pp.recs, plan.recs.size() * sizeof(PoolRec)));
        const hipError_t e = hipMemcpy(pp.recs, plan.recs.data(), plan.recs.size() * sizeof(PoolRec), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            hipFree(pp.recs);
            HCHECK(e);
        }
    }
    if (d.pool_plans.size() >= kPoolPlans) {
        hipFree(d.pool_plans.front().recs);  // waits for the kernels still reading it
        d.pool_plans.erase(d.pool_plans.begin());
    }
    d.pool_plans.push_back(std::move(pp));
    out = &d.pool_plans.back();
    return TFHE_OK;
}

// d_out selects the device; the tables as in dense_on_device.  num_luts = 0: d_lut is one shared table [q]; else
// [num_luts = c][q], one per plane
tfhe_status pool_on_device(tfhe_ctx* c, const PoolGeom& g, size_t instances, const uint64_t* d_ct, uint64_t q,
                           const uint64_t* d_lut, uint64_t* d_out, void* stream, size_t num_luts = 0,
                           const TabCall* pre = nullptr) {
    Device* dp = nullptr;
    SCHECK(device_for(c, d_out, dp));
    HCHECK(hipSetDevice(dp->id));
    TabCall tc;
    SCHECK(tab_prepare(c, *dp, stream, q, d_lut, num_luts, tc, pre));
    const Device::PoolPlanDev* pp = nullptr;
    SCHECK(pool_plan_on_device(*dp, g, pp));
    const size_t w = c->p.n + 1, planes = instances * g.c, B = std::min(planes * pp->widest, c->max_chunk);
    SCHECK(ensure_words(*dp, dp->dense_z, dp->dense_z_words, 2 * B * w));
    SCHECK(ensure_words(*dp, dp->pool_slots, dp->pool_slots_words, planes * pp->slots * w));
    return run_device_op(c, B, d_out, stream, [&](Device& d) {
        SCHECK(tab_upload(d, tc));
        return dev_pool2d(c, d, *pp, instances, d_ct, q, tc, d_out);
    });
}
}  // namespace
}  // extern "C++"

tfhe_status tfhe_pool2d_shape(const tfhe_pool2d* d, uint32_t* oh, uint32_t* ow, uint32_t* rounds, size_t* pairs) {
    return guarded([&]() -> tfhe_status {
        PoolGeom g;
        uint32_t r = 0;
        size_t p = 0;
        SCHECK(pool_geometry(d, g, r, p));
        if (oh) *oh = g.oh;
        if (ow) *ow = g.ow;
        if (rounds) *rounds = r;
        if (pairs) *pairs = p;
        return TFHE_OK;
    });
}

tfhe_status tfhe_pool2d_eval_plain(const tfhe_pool2d* desc, size_t instances, uint64_t q, const uint64_t* lut,
                                   const uint64_t* in, uint64_t* out) {
    return guarded([&]() -> tfhe_status {
        PoolGeom g;
        size_t pairs = 0;
        SCHECK(check_pool_args("Pool2dEvalPlain", desc, instances, in, q, 0, lut, out, 1, g, pairs));
        pool_eval_plain(g, pool_plan(g), instances, q, lut, in, out);
        return TFHE_OK;
    });
}

tfhe_status tfhe_eval_pool2d_device(tfhe_ctx* c, const tfhe_pool2d* desc, size_t instances, const uint64_t* d_ct,
                                    uint64_t q, const uint64_t* d_lut, uint64_t* d_out, void* stream) {
    return guarded([&]() -> tfhe_status {
        SCHECK(check_ctx(c));
        PoolGeom g;
        size_t pairs = 0;
        SCHECK(check_pool_args("EvalPool2d", desc, instances, d_ct, q, c->p.N, d_lut, d_out, c->p.n + 1, g, pairs));
        return pool_on_device(c, g, instances, d_ct, q, d_lut, d_out, stream);
    });
}

extern "C++" {
namespace {
// the host-array pooling layer; num_luts = 0: one shared table, else lut[num_luts = c][q]
tfhe_status pool_from_host(tfhe_ctx* c, const PoolGeom& g, size_t instances, const uint64_t* ct, uint64_t q,
                           const uint64_t* lut, uint64_t* out, size_t num_luts) {
    TabCall pre;
    SCHECK(check_host_tables(c, lut, num_luts, q, pre));
    const size_t w = c->p.n + 1, wi = instances * g.c * g.h * g.w * w, wo = instances * g.c * g.oh * g.ow * w,
                 wl = std::max<size_t>(num_luts, 1) * q;
    return run_from_host(c, "EvalPool2d", {{ct, w, wi}, {lut, q, wl}}, out, wo,
                         [&](const uint64_t* const* in, uint64_t* d_out) {
                             return pool_on_device(c, g, instances, in[0], q, in[1], d_out, nullptr, num_luts, &pre);
                         });
}
}  // namespace
}  // extern "C++"

tfhe_status tfhe_eval_pool2d(tfhe_ctx* c, const tfhe_pool2d* desc, size_t instances, const uint64_t* ct, uint64_t q,
                             const uint64_t* lut, uint64_t* out) {
    return guarded([&]() -> tfhe_status {
        SCHECK(check_ctx(c));
        PoolGeom g;
        size_t pairs = 0;
        SCHECK(check_pool_args("EvalPool2d", desc, instances, ct, q, c->p.N, lut, out, c->p.n + 1, g, pairs));
        return pool_from_host(c, g, instances, ct, q, lut, out, 0);
    });
}

tfhe_status tfhe_eval_pool2d_tables_device(tfhe_ctx* c, const tfhe_pool2d* desc, size_t instances, const uint64_t* d_ct,
                                           uint64_t q, const uint64_t* d_luts, size_t num_luts, uint64_t* d_out,
                                           void* stream) {
    return guarded([&]() -> tfhe_status {
        SCHECK(check_ctx(c));
        PoolGeom g;
        size_t pairs = 0;
        SCHECK(check_pool_args("EvalPool2d", desc, instances, d_ct, q, c->p.N, d_luts, d_out, c->p.n + 1, g, pairs));
        SCHECK(check_layer_tables(c, "EvalPool2d", q, num_luts, g.c, "c"));
        return pool_on_device(c, g, instances, d_ct, q, d_luts, d_out, stream, num_luts);
    });
}

tfhe_status tfhe_eval_pool2d_tables(tfhe_ctx* c, const tfhe_pool2d* desc, size_t instances, const uint64_t* ct,
                                    uint64_t q, const uint64_t* luts, size_t num_luts, uint64_t* out) {
    return guarded([&]() -> tfhe_status {
        SCHECK(check_ctx(c));
        PoolGeom g;
        size_t pairs = 0;
        SCHECK(check_pool_args("EvalPool2d", desc, instances, ct, q, c->p.N, luts, out, c->p.n + 1, g, pairs));
        SCHECK(check_layer_tables(c, "EvalPool2d", q, num_luts, g.c, "c"));
        return pool_from_host(c, g, instances, ct, q, luts, out, num_luts);
    });
}

extern "C++" {
namespace {
// The sizes of a product call: P = instances rows inner cols, and the rows of x, y and out.
struct CtmmSizes {
    size_t products, x_rows, y_rows, out_rows;
};

// what the product calls check before any device call (N = 0: no context); `words` is n+1, or 1 for clear values;
// every message names the field
tfhe_status check_ct_matmul_args(const char* who, const tfhe_ct_matmul* m, size_t instances, uint64_t q, uint64_t N,
                                 size_t words, CtmmSizes& sz) {
    const auto bad = [who](const std::string& what) {
        return fail(TFHE_ERR_INVALID_ARGUMENT, std::string(who) + ": " + what);
    };
    if (!m) return bad("null descriptor");
    if (instances == 0) return bad("instances is 0");
    if (m->rows == 0) return bad("rows is 0");
    if (m->inner == 0) return bad("inner is 0");
    if (m->cols == 0) return bad("cols is 0");
    if (m->y_transposed > 1) return bad("y_transposed must be 0 or 1");
    if (m->y_shared > 1) return bad("y_shared must be 0 or 1");
    SCHECK(check_table_q(who, q, N));
    // the inputs and the output in bytes, and what a slice can need at most: four flat rows per product
    size_t xs = 1, ys = 1, os = 1, mid = 4 * sizeof(uint64_t);
    const bool ok = conv_mul(xs, instances) && conv_mul(xs, m->rows) && conv_mul(xs, m->inner) &&
                    conv_mul(ys, m->y_shared ? 1 : instances) && conv_mul(ys, m->inner) && conv_mul(ys, m->cols) &&
                    conv_mul(os, instances) && conv_mul(os, m->rows) && conv_mul(os, m->cols) &&
                    conv_mul(mid, instances) && conv_mul(mid, m->rows) && conv_mul(mid, m->inner) &&
                    conv_mul(mid, m->cols) && conv_mul(mid, words);
    size_t xb = xs, yb = ys, ob = os, all = 0;
    if (!ok || q > SIZE_MAX / (4 * sizeof(uint64_t)) || !conv_mul(xb, words * sizeof(uint64_t)) || !conv_mul(yb, words * sizeof(uint64_t)) ||
        !conv_mul(ob, words * sizeof(uint64_t)) || xb > SIZE_MAX - yb || (all = xb + yb) > SIZE_MAX - ob ||
        (all += ob) > SIZE_MAX - 2 * q * sizeof(uint64_t))
        return bad("sizes overflow");
    sz = CtmmSizes{os * m->inner, xs, ys, os};
    return TFHE_OK;
}

tfhe_status check_ct_matmul_call(tfhe_ctx* c, const tfhe_ct_matmul* m, size_t instances, const void* x, const void* y,
                                 uint64_t q, const void* luts, const void* out, CtmmSizes& sz) {
    SCHECK(check_ctx(c));
    if (!x) return fail(TFHE_ERR_INVALID_ARGUMENT, "EvalCtMatMul: null x");
    if (!y) return fail(TFHE_ERR_INVALID_ARGUMENT, "EvalCtMatMul: null y");
    if (!luts) return fail(TFHE_ERR_INVALID_ARGUMENT, "EvalCtMatMul: null luts");
    if (!out) return fail(TFHE_ERR_INVALID_ARGUMENT, "EvalCtMatMul: null out");
    SCHECK(check_ct_matmul_args("EvalCtMatMul", m, instances, q, c->p.N, c->p.n + 1, sz));
    if (2 * (size_t)m->inner > c->max_chunk)
        return fail(TFHE_ERR_UNSUPPORTED, "EvalCtMatMul: 2 inner exceeds the chunk limit of " +
                                              std::to_string(c->max_chunk) + " ciphertexts: an output's products are one EvalFunc batch");
    return TFHE_OK;
}

// d_out selects the device; the two tables are read back once and classified one by one (pre: the host-array
// form's classes of its host copy)
tfhe_status ct_matmul_on_device(tfhe_ctx* c, const tfhe_ct_matmul& m, size_t instances, const CtmmSizes& sz,
                                const uint64_t* d_x, const uint64_t* d_y, uint64_t q, const uint64_t* d_luts,
                                uint64_t* d_out, void* stream, const TabCall* pre = nullptr) {
    Device* dp = nullptr;
    SCHECK(device_for(c, d_out, dp));
    HCHECK(hipSetDevice(dp->id));
    TabCall tc;
    SCHECK(tab_prepare(c, *dp, stream, q, d_luts, 2, tc, pre));
    // whole outputs per slice: 2 inner look-ups each, as many as the chunk limit admits (the frame grows the
    // scratch to B, so the scratch capacity never binds first)
    const size_t slice = std::min(sz.out_rows, c->max_chunk / (2 * (size_t)m.inner)), B = 2 * slice * m.inner;
    SCHECK(ensure_words(*dp, dp->dense_z, dp->dense_z_words, 2 * B * (c->p.n + 1)));
    return run_device_op(c, B, d_out, stream, [&](Device& d) {
        SCHECK(tab_upload(d, tc));
        return dev_ct_matmul(c, d, m, instances, slice, d_x, d_y, q, d_out, tc);
    });
}
}  // namespace
}  // extern "C++"

tfhe_status tfhe_ct_matmul_info(const tfhe_ct_matmul* m, size_t instances, uint64_t q, const uint64_t* luts,
                                size_t* products, uint64_t* bootstraps) {
    return guarded([&]() -> tfhe_status {
        if (!luts) return fail(TFHE_ERR_INVALID_ARGUMENT, "CtMatMulInfo: null luts");
        CtmmSizes sz;
        SCHECK(check_ct_matmul_args("CtMatMulInfo", m, instances, q, 0, 1, sz));
        uint64_t per = 0;
        for (int t = 0; t < 2; ++t) per += check_input_function(luts + t * q, q, q) == 0 ? 1 : 2;
        if (sz.products > UINT64_MAX / per) return fail(TFHE_ERR_INVALID_ARGUMENT, "CtMatMulInfo: sizes overflow");
        if (products) *products = sz.products;
        if (bootstraps) *bootstraps = sz.products * per;
        return TFHE_OK;
    });
}

tfhe_status tfhe_ct_matmul_eval_plain(const tfhe_ct_matmul* m, size_t instances, uint64_t q, const uint64_t* luts,
                                      const uint64_t* x, const uint64_t* y, uint64_t* out) {
    return guarded([&]() -> tfhe_status {
        if (!luts) return fail(TFHE_ERR_INVALID_ARGUMENT, "CtMatMulEvalPlain: null luts");
        if (!x) return fail(TFHE_ERR_INVALID_ARGUMENT, "CtMatMulEvalPlain: null x");
        if (!y) return fail(TFHE_ERR_INVALID_ARGUMENT, "CtMatMulEvalPlain: null y");
        if (!out) return fail(TFHE_ERR_INVALID_ARGUMENT, "CtMatMulEvalPlain: null out");
        CtmmSizes sz;
        SCHECK(check_ct_matmul_args("CtMatMulEvalPlain", m, instances, q, 0, 1, sz));
        for (uint64_t t = 0; t < 2 * q; ++t)
            if (luts[t] >= q)
                return fail(TFHE_ERR_INVALID_ARGUMENT, "CtMatMulEvalPlain: luts[" + std::to_string(t / q) + "][" +
                                                           std::to_string(t % q) + "] is not below q");
        const uint64_t mask = q - 1;
        const size_t R = m->rows, K = m->inner, Cn = m->cols;
        for (size_t i = 0; i < instances; ++i) {
            const uint64_t* yi = y + (m->y_shared ? 0 : i * K * Cn);
            for (size_t r = 0; r < R; ++r)
                for (size_t cc = 0; cc < Cn; ++cc) {
                    uint64_t acc = 0;
                    for (size_t k = 0; k < K; ++k) {
                        const uint64_t a = x[(i * R + r) * K + k], b = yi[m->y_transposed ? cc * K + k : k * Cn + cc];
                        acc += luts[(a + b) & mask] - luts[q + ((a - b) & mask)];
                    }
                    out[(i * R + r) * Cn + cc] = acc & mask;
                }
        }
        return TFHE_OK;
    });
}

tfhe_status tfhe_eval_ct_matmul_device(tfhe_ctx* c, const tfhe_ct_matmul* m, size_t instances, const uint64_t* d_x,
                                       const uint64_t* d_y, uint64_t q, const uint64_t* d_luts, uint64_t* d_out,
                                       void* stream) {
    return guarded([&]() -> tfhe_status {
        CtmmSizes sz;
        SCHECK(check_ct_matmul_call(c, m, instances, d_x, d_y, q, d_luts, d_out, sz));
        return ct_matmul_on_device(c, *m, instances, sz, d_x, d_y, q, d_luts, d_out, stream);
    });
}

tfhe_status tfhe_eval_ct_matmul(tfhe_ctx* c, const tfhe_ct_matmul* m, size_t instances, const uint64_t* x,
                                const uint64_t* y, uint64_t q, const uint64_t* luts, uint64_t* out) {
    return guarded([&]() -> tfhe_status {
        CtmmSizes sz;
        SCHECK(check_ct_matmul_call(c, m, instances, x, y, q, luts, out, sz));
        TabCall pre;
        SCHECK(check_host_tables(c, luts, 2, q, pre));
        const size_t w = c->p.n + 1;
        return run_from_host(c, "EvalCtMatMul", {{x, w, sz.x_rows * w}, {y, w, sz.y_rows * w}, {luts, q, 2 * q}}, out,
                             sz.out_rows * w, [&](const uint64_t* const* in, uint64_t* d_out) {
                                 return ct_matmul_on_device(c, *m, instances, sz, in[0], in[1], q, in[2], d_out, nullptr, &pre);
                             });
    });
}

// GPULWEOperation::GPUSetup(numGPUs) (lwe-operation.cu:143-146) ignores numGPUs and works on device 0;
// so does this (CiphertextMulMatrix runs on device 0): any count is accepted, as long as a device exists
// (round 4 refused numGPUs above the visible count -- found by the multi-device drop-in test)
tfhe_status tfhe_lwe_gpu_setup(int num_gpus) {
    (void)num_gpus;
    return guarded([&]() -> tfhe_status {
        int count = 0;
        HCHECK(hipGetDeviceCount(&count));
        if (count < 1) return fail(TFHE_ERR_DEVICE, "no HIP device visible");
        return TFHE_OK;
    });
}

tfhe_status tfhe_lwe_gpu_clean(void) { return TFHE_OK; }

tfhe_status tfhe_host_selftest(const tfhe_params* pin) {
    return guarded([&]() -> tfhe_status {
        if (!pin) return fail(TFHE_ERR_INVALID_ARGUMENT, "null params");
        tfhe_params p = *pin;
        std::string err;
        if (params_finish(&p, &err) != TFHE_OK) return fail(TFHE_ERR_INVALID_ARGUMENT, err);
        NttTables t = make_ntt_tables(p.Q, p.N);
        // (1) forward/inverse round trip and (2) product vs schoolbook on a pseudo-random pair
        std::vector<uint64_t> a(p.N), b(p.N), ref(p.N, 0);
        uint64_t s = 0x1234567;
        for (uint32_t i = 0; i < p.N; ++i) {
            s = s * 6364136223846793005ull + 1442695040888963407ull;
            a[i] = (s >> 7) % p.Q;
            s = s * 6364136223846793005ull + 1442695040888963407ull;
            b[i] = (s >> 7) % p.Q;
        }
        for (uint32_t i = 0; i < p.N; ++i)
            for (uint32_t j = 0; j < p.N; ++j) {
                uint64_t v = mulmod(a[i], b[j], p.Q);
                if (i + j < p.N) ref[i + j] = addmod(ref[i + j], v, p.Q);
                else ref[i + j - p.N] = submod(ref[i + j - p.N], v, p.Q);
            }
        std::vector<uint64_t> A = a, Bv = b;
        host_ntt_fwd(t, A.data());
        host_ntt_fwd(t, Bv.data());
        for (uint32_t i = 0; i < p.N; ++i) A[i] = mulmod(A[i], Bv[i], p.Q);
        host_ntt_inv(t, A.data(), true);
        if (A != ref) return fail(TFHE_ERR_INTERNAL, "host NTT product mismatch");
        // (3) monomial table: NTT(X^m)[x] = psi^(e_x * m)
        for (uint32_t m : {1u, 3u, p.N - 1, p.N + 5, 2 * p.N - 1}) {
            std::vector<uint64_t> mon(p.N, 0);
            if (m < p.N) mon[m] = 1;
            else mon[m - p.N] = p.Q - 1;
            host_ntt_fwd(t, mon.data());
            for (uint32_t x = 0; x < p.N; ++x) {
                uint32_t idx = (uint32_t)(((uint64_t)t.eidx[x] * m) % (2ull * p.N));
                if (mon[x] != addmod(t.mono[idx], 1, p.Q)) return fail(TFHE_ERR_INTERNAL, "monomial table mismatch");
            }
        }
        // (3b) the slot exponents are 2 bitrev(x) + 1 (the fast kernel relies on it)
        for (uint32_t x = 0; x < p.N; ++x)
            if (t.eidx[x] != 2 * bitrev(x, t.logN) + 1) return fail(TFHE_ERR_INTERNAL, "eidx is not 2 bitrev(x) + 1");
        // (4) Shoup companions at the chosen word width
        const int wb = word_bits_for(p);
        const u128 R = (u128)1 << wb;
        for (uint32_t x = 0; x < p.N; ++x) {
            const uint64_t w = t.psi_br[x], wp = shoup_companion(w, p.Q, wb);
            const uint64_t aa = a[x] | (wb == 32 ? 0x80000000ull : 0x8000000000000000ull);
            const uint64_t mask = wb == 32 ? 0xFFFFFFFFull : ~0ull;
            const uint64_t qt = (uint64_t)(((u128)aa * wp) >> wb);
            const uint64_t r = (uint64_t)(((u128)aa * w - (u128)qt * p.Q) % R) & mask;
            if (r >= 2 * p.Q || r % p.Q != mulmod(aa % p.Q, w, p.Q)) return fail(TFHE_ERR_INTERNAL, "Shoup bound");
        }
        // (5) the narrow PCIe wire format's host side (pool jobs above and below the 1 MiB cut)
        for (size_t n : {(size_t)1000, (size_t)3 << 17}) {
            std::vector<uint64_t> src(n), back(n, ~0ull);
            for (size_t i = 0; i < n; ++i) src[i] = (i * 2654435761u) & 0xFFFFFFFFu;
            if (parallel_or(src.data(), n) >> 32 || wire_bytes(parallel_or(src.data(), n)) != 4)
                return fail(TFHE_ERR_INTERNAL, "wire width");
            for (int wb : {2, 4}) {
                std::vector<uint8_t> packed(n * wb);
                parallel_narrow(packed.data(), src.data(), n, wb);
                parallel_widen(back.data(), packed.data(), n, wb);
                const uint64_t mask = wb == 2 ? 0xFFFFu : 0xFFFFFFFFu;
                for (size_t i = 0; i < n; ++i)
                    if (back[i] != (src[i] & mask)) return fail(TFHE_ERR_INTERNAL, "wire narrow/widen");
            }
        }
        return TFHE_OK;
    });
}

}  // extern "C"
