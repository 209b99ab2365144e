// duo.hpp -- the two-workgroup ("duo") blind rotations for batches too small to fill the chip
// (k_blind_rotate_sf2duo / k_blind_rotate_sfduo, blind_rotate_sf.hip; k_blind_rotate_f64wduo,
// blind_rotate_f64.hip): the per-device state, its launch fence, and the device side of the per-round hand-off
// between the two members of a pair.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>

namespace tfhe {

// One per-device buffer, allocated at setup for the contexts that have a duo form.
//   xbuf  [pairs][2 members][2 round parities][2048] u64   the per-round hand-off (16 KiB per member)
//   flags [pairs][2 members][32] u32                        word 0: the member's round flag; word 1 of
//                                                           member 0's line: the pair's failed word
//   err   one 128-B line                                    timed-out workgroups since setup
//   save  [pairs][2][2048] u64                              the input accumulators (the rescue's input)
constexpr uint32_t kDuoMaxPairs = 256;
constexpr uint32_t kDuoN = 2048;
// Per device (engine.hip, finish_device): the buffer above; the partner-wait deadline in wall-clock ticks
// (s_memrealtime counts at hipDeviceAttributeWallClockRate: kDuoWaitMs of it); the pairs the device holds
// co-resident (the duo forms take 116-148 KiB of LDS, one workgroup per CU: half the CU count) -- a larger
// batch runs the one-workgroup kernel, so a pair's partner is never queued behind its own launch's pairs;
// and the fence that orders duo launches from different streams on the one buffer (event + host mutex).
constexpr uint32_t kDuoWaitMs = 10;
struct DuoDev {
    void* base = nullptr;
    uint64_t wait_ticks = 0;
    uint32_t resident_pairs = 0;
    hipEvent_t fence = nullptr;
    std::mutex* mu = nullptr;
};
struct DuoBuf {
    uint64_t* xbuf;
    uint32_t* flags;
    uint32_t* err;
    uint64_t* save;
    uint64_t wait_ticks;  // a member waits at most this long for its partner's flag in any round
};
inline DuoBuf duo_layout(const DuoDev& D) {
    DuoBuf X;
    X.xbuf = (uint64_t*)D.base;
    X.flags = (uint32_t*)(X.xbuf + (size_t)kDuoMaxPairs * 4 * kDuoN);
    X.err = X.flags + kDuoMaxPairs * 2 * 32;
    X.save = (uint64_t*)(X.err + 32);
    X.wait_ticks = D.wait_ticks;
    return X;
}
// Runs `launch` (the duo kernel and its rescue, on stream s) after every earlier duo launch on this device's
// buffer, whatever stream it was queued on.
template <class F>
hipError_t duo_serialised(DuoDev& D, hipStream_t s, F&& launch) {
    std::lock_guard<std::mutex> lock(*D.mu);
    if (hipError_t e = hipStreamWaitEvent(s, D.fence, 0); e != hipSuccess) return e;
    if (hipError_t e = launch(); e != hipSuccess) return e;
    return hipEventRecord(D.fence, s);
}
inline size_t duo_bytes() { return (size_t)kDuoMaxPairs * (4 * kDuoN * 8 + 2 * 128) + 128 + (size_t)kDuoMaxPairs * 2 * kDuoN * 8; }
inline uint32_t duo_err_offset_words() { return (uint32_t)((size_t)kDuoMaxPairs * 4 * kDuoN * 2 + kDuoMaxPairs * 2 * 32); }

// ---- the hand-off (device side) ----
// Each round a member publishes 16 KiB to its partner and takes the partner's:
//     duo_store of its values;  s_waitcnt vmcnt(0);  workgroup barrier;
//     thread 0: duo_publish_and_wait (one flag store, then polls of the partner's flag);
//     workgroup barrier;  uniform break if the partner never arrived;  duo_load of the partner's values.
// The waitcnt, the barriers and the break stay in the kernels, in that order.  What the protocol assumes:
//  * ordering: the data stores and the flag are RELAXED agent-scope atomics (write-through past the CU, `sc1`);
//    the data is ordered before the flag by every wave's `s_waitcnt vmcnt(0)` (each store acknowledged) and the
//    workgroup barrier, and on the reader by the poll's load returning before the barrier and the loads behind
//    it.  That is gfx9 ISA behaviour (the MI355X_MICROARCH.md hand-off table's sc1 row;
//    tools/microbench/pair_handoff.hip), not a HIP-memory-model release / acquire pair -- one of those costs
//    about 1.7 us per round, more than the hand-off itself;
//  * pairing: members are blocks b and b + 8, which share an XCD only through round-robin workgroup dispatch;
//    correctness never depends on it (agent scope), the latency does (same-XCD hand-offs measured 1.1-1.3 us,
//    cross-XCD 1.9-2.0);
//  * liveness: both members must be resident at once.  The launchers run a duo form only for batches up to the
//    device's co-resident pairs and fence duo launches of one device's buffer across streams (duo_serialised),
//    so a partner can only be late behind another context's work.  Every wait is bounded by kDuoWaitMs (10 ms)
//    of wall clock (s_memrealtime): a member that times out fails its pair (duo_fail_pair: the pair's failed
//    word, and one more in X.err, a count since setup, tfhe_info.duo_timeouts) and leaves the round loop; its
//    partner then times out too (the flags it waits for never come).  Each member saves its input first
//    (X.save), and the launcher queues the one-workgroup rescue kernel right behind, which recomputes exactly
//    the failed pairs' ciphertexts from X.save -- a late partner never returns wrong accumulators.
// The clock is read every 8th poll and the deadline set at the first read, so a partner within 8 polls costs
// no clock read.  The test library's probe 1 (a partner that never arrives: `gone`) waits a 64th of the bound
// (SHORT).
__device__ __forceinline__ void duo_store(uint64_t* p, uint64_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint64_t duo_load(const uint64_t* p) {
    return __hip_atomic_load(const_cast<uint64_t*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void duo_store(double* p, double v) {
    duo_store(reinterpret_cast<uint64_t*>(p), __builtin_bit_cast(uint64_t, v));
}
__device__ __forceinline__ double duo_load(const double* p) {
    return __builtin_bit_cast(double, duo_load(reinterpret_cast<const uint64_t*>(p)));
}

// One thread of the member: publishes round `round` (unless gone) and waits for the partner's; false on timeout.
template <bool SHORT>
__device__ __forceinline__ bool duo_publish_and_wait(uint32_t* myflag, const uint32_t* peerflag, uint32_t round,
                                                     uint64_t wait_ticks, bool gone) {
    if (!gone) __hip_atomic_store(myflag, round + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    bool ok = !gone;
    uint64_t t_end = 0;
    uint32_t k = 0;
    while (ok && __hip_atomic_load(const_cast<uint32_t*>(peerflag), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < round + 1) {
        if ((++k & 7) == 0) {
            const uint64_t now = wall_clock64();
            if (t_end == 0) t_end = now + (SHORT ? wait_ticks >> 6 : wait_ticks);
            else if (now > t_end) ok = false;
        }
        __builtin_amdgcn_s_sleep(1);
    }
    return ok;
}
// One thread of a member that timed out: the pair's failed word (the rescue's cue) and the error count.
__device__ __forceinline__ void duo_fail_pair(const DuoBuf& X, uint32_t pair) {
    __hip_atomic_store(X.flags + pair * 2 * 32 + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(X.err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace tfhe
