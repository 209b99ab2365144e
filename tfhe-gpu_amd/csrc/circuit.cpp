// circuit.cpp -- netlist compiler of tfhe_circuit (host only, no GPU): validation, lowering to
// bootstrapped gates with negate flags and constant operands, ASAP levels, slot renumbering, and the
// clear-bit evaluation of the lowered plan (tfhe_circuit_eval_plain).
//
// Lowering keeps the result bit-identical to the reference's vector API called gate by gate:
//  * XOR / XNOR are what EvalBinGate runs for them (binfhe-base-scheme.cpp:619-640):
//    OR(AND(x, NOT y), AND(NOT x, y)), negated for XNOR -- three bootstraps on two levels;
//  * NOT is never a gate: it toggles the negate flag of the wire it yields (EvalNOT,
//    binfhe-base-scheme.cpp:147-159, is an exact involution, so a double negation cancels);
//  * CONST0 / CONST1 are operand kinds (NoiselessEmbedding, lwe-pke.cpp:326-338); NOT of a constant is
//    the other constant (b -> q/4 - b);
//  * nothing else is simplified: no constant folding through a bootstrap, no dead-gate removal, so
//    bootstraps = #(OR, AND, NOR, NAND, XOR_FAST, XNOR_FAST) + 3 #(XOR, XNOR).
// Slots are not reused by liveness: the wire store of a run holds every bootstrap's result.
#include "circuit.hpp"

#include <algorithm>
#include <memory>
#include <new>
#include <numeric>

using namespace tfhe;

namespace {

struct Ref {
    uint32_t kind = CK_INPUT, idx = 0;
    bool neg = false;
    uint32_t level = 0;
};

Ref negated(Ref r) {
    if (r.kind == CK_CONST) r.idx ^= 1u;
    else r.neg = !r.neg;
    return r;
}

struct Boot {
    uint32_t op;
    Ref a, b;
    uint32_t level;
};

tfhe_status bad(const std::string& msg) { return set_last_error(TFHE_ERR_INVALID_ARGUMENT, "tfhe_circuit_compile: " + msg); }

inline uint8_t gate_bit(uint32_t op, uint8_t x, uint8_t y) {
    switch (op) {
        case TFHE_OR: return x | y;
        case TFHE_AND: return x & y;
        case TFHE_NOR: return 1 ^ (x | y);
        case TFHE_NAND: return 1 ^ (x & y);
        case TFHE_XOR_FAST: return x ^ y;
        default: return 1 ^ x ^ y;  // TFHE_XNOR_FAST
    }
}

}  // namespace

extern "C" {

tfhe_status tfhe_circuit_compile(tfhe_circuit** out, uint32_t num_inputs, const tfhe_circuit_gate* gates,
                                 size_t num_gates, const uint32_t* outputs, size_t num_outputs) {
    return host_guarded([&]() -> tfhe_status {
        if (!out) return bad("null output pointer");
        *out = nullptr;
        if (num_gates > 0 && !gates) return bad("null gate array with num_gates > 0");
        if (num_outputs == 0) return bad("a circuit needs at least one output");
        if (!outputs) return bad("null output array");
        // three bootstraps per gate at most, and every wire and slot index is a u32
        if (num_gates > (UINT32_MAX - num_inputs) / 3 || num_outputs > UINT32_MAX) return bad("netlist too large");
        const uint32_t wires = num_inputs + (uint32_t)num_gates;

        std::vector<Ref> wire(wires);
        std::vector<Boot> boots;
        boots.reserve(num_gates);
        auto emit = [&](uint32_t op, const Ref& a, const Ref& b) {
            const uint32_t level = 1 + std::max(a.level, b.level);
            boots.push_back(Boot{op, a, b, level});
            Ref r;
            r.kind = CK_SLOT, r.idx = (uint32_t)boots.size() - 1, r.level = level;
            return r;
        };
        for (uint32_t i = 0; i < num_inputs; ++i) wire[i].idx = i;
        for (size_t g = 0; g < num_gates; ++g) {
            const tfhe_circuit_gate& G = gates[g];
            const uint32_t self = num_inputs + (uint32_t)g;
            const std::string name = "gate " + std::to_string(g);
            if (G.op > TFHE_C_CONST1) return bad(name + ": unknown op " + std::to_string(G.op));
            Ref& w = wire[self];
            if (G.op == TFHE_C_CONST0 || G.op == TFHE_C_CONST1) {
                w.kind = CK_CONST, w.idx = G.op == TFHE_C_CONST1;
                continue;
            }
            const uint32_t operands = G.op == TFHE_C_NOT ? 1 : 2;
            const uint32_t in[2] = {G.in0, G.in1};
            for (uint32_t k = 0; k < operands; ++k) {
                if (in[k] >= wires)
                    return bad(name + ": operand " + std::to_string(k) + " names wire " + std::to_string(in[k]) +
                               ", out of range (the netlist has " + std::to_string(wires) + " wires)");
                if (in[k] >= self)
                    return bad(name + ": operand " + std::to_string(k) + " names wire " + std::to_string(in[k]) +
                               ", not below its own wire " + std::to_string(self) + " (forward reference)");
            }
            if (G.op == TFHE_C_NOT) {
                w = negated(wire[G.in0]);
                continue;
            }
            const Ref a = wire[G.in0], b = wire[G.in1];
            if (G.op == TFHE_XOR || G.op == TFHE_XNOR) {
                const Ref t1 = emit(TFHE_AND, a, negated(b));
                const Ref t2 = emit(TFHE_AND, negated(a), b);
                const Ref o = emit(TFHE_OR, t1, t2);
                w = G.op == TFHE_XNOR ? negated(o) : o;
            } else {
                w = emit(G.op, a, b);
            }
        }
        for (size_t o = 0; o < num_outputs; ++o)
            if (outputs[o] >= wires)
                return bad("output " + std::to_string(o) + " names wire " + std::to_string(outputs[o]) +
                           ", out of range (the netlist has " + std::to_string(wires) + " wires)");

        // slots: bootstraps sorted by level, creation order inside a level
        std::vector<uint32_t> order(boots.size()), slot_of(boots.size());
        std::iota(order.begin(), order.end(), 0u);
        std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return boots[x].level < boots[y].level; });
        for (uint32_t s = 0; s < order.size(); ++s) slot_of[order[s]] = s;
        auto index_of = [&](const Ref& r) { return r.kind == CK_SLOT ? slot_of[r.idx] : r.idx; };

        auto c = std::make_unique<tfhe_circuit>();
        c->recs.resize(boots.size());
        for (uint32_t s = 0; s < order.size(); ++s) {
            const Boot& b = boots[order[s]];
            c->recs[s] = CircuitRec{circuit_ctl(b.op, b.a.kind, b.a.neg, b.b.kind, b.b.neg), index_of(b.a), index_of(b.b), 0};
            if (c->levels.size() < b.level) c->levels.push_back(CircuitLevel{s, 0});  // levels are dense: ASAP
            c->levels.back().width++;
        }
        c->outs.resize(num_outputs);
        for (size_t o = 0; o < num_outputs; ++o) {
            const Ref& r = wire[outputs[o]];
            c->outs[o] = CircuitOut{r.kind | (uint32_t)r.neg << 2, index_of(r)};
        }
        tfhe_circuit_info& I = c->info;
        I.num_inputs = num_inputs;
        I.num_outputs = (uint32_t)num_outputs;
        I.num_gates = (uint32_t)num_gates;
        I.bootstraps = (uint32_t)boots.size();
        I.levels = (uint32_t)c->levels.size();
        I.widest_level = 0;
        for (const CircuitLevel& L : c->levels) I.widest_level = std::max(I.widest_level, L.width);
        *out = c.release();
        return TFHE_OK;
    });
}

tfhe_status tfhe_circuit_free(tfhe_circuit* c) {
    if (!c) return TFHE_OK;
    c->cache.release();
    delete c;
    return TFHE_OK;
}

tfhe_status tfhe_circuit_get_info(const tfhe_circuit* c, tfhe_circuit_info* out) {
    if (!c || !out) return set_last_error(TFHE_ERR_INVALID_ARGUMENT, "tfhe_circuit_get_info: null argument");
    *out = c->info;
    return TFHE_OK;
}

tfhe_status tfhe_circuit_level_widths(const tfhe_circuit* c, uint32_t* widths, size_t cap) {
    if (!c || (!widths && cap > 0))
        return set_last_error(TFHE_ERR_INVALID_ARGUMENT, "tfhe_circuit_level_widths: null argument");
    if (cap < c->levels.size())
        return set_last_error(TFHE_ERR_INVALID_ARGUMENT, "tfhe_circuit_level_widths: room for " + std::to_string(cap) +
                                                             " widths, the circuit has " +
                                                             std::to_string(c->levels.size()) + " levels");
    for (size_t l = 0; l < c->levels.size(); ++l) widths[l] = c->levels[l].width;
    return TFHE_OK;
}

tfhe_status tfhe_circuit_eval_plain(const tfhe_circuit* c, size_t instances, const uint8_t* in, uint8_t* out) {
    return host_guarded([&]() -> tfhe_status {
        if (!c || !out || (!in && c->info.num_inputs > 0 && instances > 0))
            return set_last_error(TFHE_ERR_INVALID_ARGUMENT, "tfhe_circuit_eval_plain: null argument");
        std::vector<uint8_t> store(c->recs.size() * instances);
        auto read = [&](uint32_t kind, bool neg, uint32_t idx, size_t i) -> uint8_t {
            const uint8_t v = kind == CK_CONST   ? (uint8_t)idx
                              : kind == CK_INPUT ? (uint8_t)(in[idx * instances + i] != 0)
                                                 : store[idx * instances + i];
            return v ^ (uint8_t)neg;
        };
        for (size_t s = 0; s < c->recs.size(); ++s) {
            const CircuitRec& r = c->recs[s];
            for (size_t i = 0; i < instances; ++i)
                store[s * instances + i] = gate_bit(r.ctl & 7, read(r.ctl >> 4 & 3, r.ctl >> 6 & 1, r.i0, i),
                                                    read(r.ctl >> 8 & 3, r.ctl >> 10 & 1, r.i1, i));
        }
        for (size_t o = 0; o < c->outs.size(); ++o)
            for (size_t i = 0; i < instances; ++i)
                out[o * instances + i] = read(c->outs[o].ctl & 3, c->outs[o].ctl >> 2 & 1, c->outs[o].idx, i);
        return TFHE_OK;
    });
}

}  // extern "C"
