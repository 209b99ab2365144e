// circuit.hpp -- the lowered plan of a levelled Boolean circuit (tfhe_circuit): what circuit.cpp
// compiles from a netlist, what engine.hip uploads once per device, and what the kernels of
// circuit_kernels.hip read.
//
// A plan holds one 16-byte record per bootstrap, in slot order.  Slot s is the s-th bootstrapped gate
// after sorting by level (stable: creation order inside a level), so the results of a level occupy the
// consecutive slots [first, first + width) and the key switch of a whole level writes them with one
// launch.  The wire store of a run is [bootstraps][instances][n+1] words: slot s, instance i at
// (s * instances + i) * (n + 1); the input array has the same shape with the input wire for the slot.
#pragma once

#include <cstdint>
#include <exception>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "tfhe_hip.h"

namespace tfhe {

// Where an operand (or an output) is read from.  A NOT is the `neg` bit of its reader
// (EvalNOT: a -> -a, b -> q/4 - b); a constant is (a = 0, b = value * (q >> 2)) and is never negated
// (a negated constant is stored as the other constant).
enum CircuitKind : uint32_t { CK_INPUT = 0, CK_SLOT = 1, CK_CONST = 2 };

// ctl: bits 0-2 the gate (tfhe_gate OR .. XNOR_FAST); bits 4-5 kind of operand 0, bit 6 its neg;
// bits 8-9 kind of operand 1, bit 10 its neg.  i0 / i1: input wire, slot, or the constant's value.
struct CircuitRec {
    uint32_t ctl, i0, i1, reserved;
};
static_assert(sizeof(CircuitRec) == 16, "one 16-byte load per workgroup");
constexpr uint32_t circuit_ctl(uint32_t op, uint32_t k0, bool n0, uint32_t k1, bool n1) {
    return op | k0 << 4 | (uint32_t)n0 << 6 | k1 << 8 | (uint32_t)n1 << 10;
}

// ctl: bits 0-1 kind, bit 2 neg
struct CircuitOut {
    uint32_t ctl, idx;
};

struct CircuitLevel {
    uint32_t first, width;  // slots [first, first + width)
};

// last-error channel of the C-ABI (engine.hip); returns s
tfhe_status set_last_error(tfhe_status s, const std::string& msg);

// exceptions of a host-only entry point -> status + last error
template <typename F>
tfhe_status host_guarded(F&& body) {
    try {
        return body();
    } catch (const std::bad_alloc&) {
        return set_last_error(TFHE_ERR_OUT_OF_MEMORY, "host allocation failed");
    } catch (const std::exception& e) {
        return set_last_error(TFHE_ERR_INTERNAL, std::string("internal error: ") + e.what());
    }
}

// Device copies of a compiled plan (one byte image), one per HIP device that ran the circuit; uploaded by
// engine.hip on first use (plan_on_device), released through dev_free (set by the uploader; the compilers have
// no HIP dependency) when the circuit is freed.
struct PlanCache {
    struct DevPlan {
        int device;
        void* base;
    };
    std::mutex mu;
    std::vector<DevPlan> plans;
    void (*dev_free)(int device, void* base) = nullptr;
    void release() {
        for (const DevPlan& p : plans)
            if (dev_free) dev_free(p.device, p.base);
        plans.clear();
    }
};

}  // namespace tfhe

struct tfhe_circuit {
    tfhe_circuit_info info{};
    std::vector<tfhe::CircuitRec> recs;      // [bootstraps], slot order
    std::vector<tfhe::CircuitLevel> levels;  // [info.levels]
    std::vector<tfhe::CircuitOut> outs;      // [num_outputs]
    tfhe::PlanCache cache;  // device copies of recs | outs (outs at byte offset recs.size() * 16)
};
