// fcircuit.cpp -- netlist compiler of tfhe_fcircuit (host only, no GPU): validation, classification of the
// tables, folding of the linear forms, lowering of LUT nodes to bootstrap records, ASAP levels, slot
// renumbering, and the clear-value evaluation of the lowered plan (tfhe_fcircuit_eval_plain).
//
// Lowering keeps the result bit-identical to tfhe_eval_func (shared table) called node by node
// (binfhe-base-scheme.cpp:679-924; engine.hip dev_func):
//  * a negacyclic table is one bootstrap: TV_LUT at modulus q;
//  * a periodic table is two: TV_HALF, then TV_LUT1 on ct - first - q/4, both at modulus q;
//  * an arbitrary table is two at modulus 2q: TV_HALF, then TV_LUT2 on ct - first - q/2; the result is read
//    mod q (SetModulus) by whatever reads it;
//  * LIN nodes are folded into their readers: mod a power of two the folded form and the node-by-node
//    evaluation are the same ring expression, so the words are equal, whatever the order of the sums;
//  * nothing else is simplified: no dead-node removal, no sharing of equal bootstraps.
#include "fcircuit.hpp"

#include <algorithm>
#include <memory>
#include <mutex>
#include <numeric>
#include <set>

using namespace tfhe;

namespace tfhe {

int check_input_function(const uint64_t* lut, uint64_t len, uint64_t mod) {
    const uint64_t h = len / 2;
    if (lut[0] == mod - lut[h]) {
        for (uint64_t i = 1; i < h; ++i)
            if (lut[i] != mod - lut[h + i]) return 2;
        return 0;
    }
    if (lut[0] == lut[h]) {
        for (uint64_t i = 1; i < h; ++i)
            if (lut[i] != lut[h + i]) return 2;
        return 1;
    }
    return 2;
}

}  // namespace tfhe

namespace {

std::mutex g_live_mu;
std::set<const tfhe_fcircuit*>& live() {
    static std::set<const tfhe_fcircuit*> s;
    return s;
}

tfhe_status bad(const std::string& msg) { return set_last_error(TFHE_ERR_INVALID_ARGUMENT, "tfhe_fcircuit_compile: " + msg); }
tfhe_status dead(const char* where) {
    return set_last_error(TFHE_ERR_INVALID_ARGUMENT, std::string(where) + ": null, freed or unknown function circuit");
}

// a wire: sum of coef * base over bases (kind << 32 | idx, ascending), + k, mod q
struct Form {
    std::vector<std::pair<uint64_t, uint64_t>> terms;
    uint64_t k = 0;
    uint32_t level = 0;
};

void add_scaled(Form& dst, const Form& src, uint64_t c, uint64_t mask) {
    std::vector<std::pair<uint64_t, uint64_t>> out;
    out.reserve(dst.terms.size() + src.terms.size());
    size_t i = 0, j = 0;
    while (i < dst.terms.size() || j < src.terms.size()) {
        std::pair<uint64_t, uint64_t> t;
        if (j == src.terms.size() || (i < dst.terms.size() && dst.terms[i].first < src.terms[j].first)) {
            t = dst.terms[i++];
        } else if (i == dst.terms.size() || src.terms[j].first < dst.terms[i].first) {
            t = {src.terms[j].first, (src.terms[j].second * c) & mask};
            ++j;
        } else {
            t = {dst.terms[i].first, (dst.terms[i].second + src.terms[j].second * c) & mask};
            ++i, ++j;
        }
        if (t.second) out.push_back(t);
    }
    dst.terms.swap(out);
    dst.k = (dst.k + src.k * c) & mask;
}

struct Boot {
    uint32_t ctl, lut, form, level, stage1;  // form: index of the node's form; stage1: creation index
};

}  // namespace

namespace tfhe {
bool fcircuit_alive(const tfhe_fcircuit* c) {
    std::lock_guard<std::mutex> lock(g_live_mu);
    return c && live().count(c) != 0;
}
}  // namespace tfhe

extern "C" {

tfhe_status tfhe_fcircuit_compile(tfhe_fcircuit** out, uint32_t num_inputs, const tfhe_fcircuit_node* nodes,
                                  size_t num_nodes, uint64_t q, const uint64_t* luts, size_t num_luts,
                                  const uint32_t* outputs, size_t num_outputs) {
    return host_guarded([&]() -> tfhe_status {
        if (!out) return bad("null output pointer");
        *out = nullptr;
        if (num_nodes > 0 && !nodes) return bad("null node array with num_nodes > 0");
        if (num_luts > 0 && !luts) return bad("null table array with num_luts > 0");
        if (num_outputs == 0) return bad("a circuit needs at least one output");
        if (!outputs) return bad("null output array");
        if (q < 8 || (q & (q - 1)) != 0 || q > (1ull << 62))
            return bad("q = " + std::to_string(q) + " is not a power of two from 8 to 2^62");
        // two bootstraps per node at most, and every wire, slot and table index is a u32
        if (num_nodes > (UINT32_MAX - num_inputs) / 2 || num_outputs > UINT32_MAX || num_luts > UINT32_MAX)
            return bad("netlist too large");
        const uint64_t mask = q - 1;
        const uint32_t wires = num_inputs + (uint32_t)num_nodes;

        auto c = std::make_unique<tfhe_fcircuit>();
        tfhe_fcircuit_info& I = c->info;
        c->lut_class.resize(num_luts);
        for (size_t t = 0; t < num_luts; ++t) {
            const uint64_t* T = luts + t * q;
            for (uint64_t i = 0; i < q; ++i)
                if (T[i] >= q)
                    return bad("table " + std::to_string(t) + ": entry " + std::to_string(i) + " is " + std::to_string(T[i]) +
                               ", not below q = " + std::to_string(q));
            const int cls = check_input_function(T, q, q);
            c->lut_class[t] = (uint8_t)cls;
            ++(cls == 0 ? I.negacyclic : cls == 1 ? I.periodic : I.arbitrary);
        }
        c->luts.assign(luts, luts + num_luts * q);

        std::vector<Form> wire(wires);
        std::vector<Form> forms;  // of the LUT nodes, by Boot::form
        std::vector<Boot> boots;
        for (uint32_t i = 0; i < num_inputs; ++i) wire[i].terms = {{(uint64_t)CK_INPUT << 32 | i, 1}};
        for (size_t g = 0; g < num_nodes; ++g) {
            const tfhe_fcircuit_node& G = nodes[g];
            const uint32_t self = num_inputs + (uint32_t)g;
            const std::string name = "node " + std::to_string(g);
            if (G.op > TFHE_F_LUT) return bad(name + ": unknown op " + std::to_string(G.op));
            const uint32_t in[2] = {G.in0, G.in1};
            const int64_t cf[2] = {G.c0, G.c1};
            const uint32_t operands = G.c1 == 0 ? 1 : 2;
            for (uint32_t k = 0; k < operands; ++k) {
                if (in[k] >= wires)
                    return bad(name + ": operand " + std::to_string(k) + " names wire " + std::to_string(in[k]) +
                               ", out of range (the netlist has " + std::to_string(wires) + " wires)");
                if (in[k] >= self)
                    return bad(name + ": operand " + std::to_string(k) + " names wire " + std::to_string(in[k]) +
                               ", not below its own wire " + std::to_string(self) + " (forward reference)");
            }
            if (G.k >= q) return bad(name + ": k = " + std::to_string(G.k) + " is not below q = " + std::to_string(q));
            if (G.op == TFHE_F_LUT && G.lut >= num_luts)
                return bad(name + ": names table " + std::to_string(G.lut) + ", out of range (the circuit has " +
                           std::to_string(num_luts) + " tables)");
            Form f;
            f.k = G.k;
            for (uint32_t k = 0; k < operands; ++k) {
                // a negative coefficient multiplies by q - |c|
                const uint64_t mag = (uint64_t)(cf[k] < 0 ? -cf[k] : cf[k]) & mask;
                add_scaled(f, wire[in[k]], cf[k] < 0 ? (q - mag) & mask : mag, mask);
                f.level = std::max(f.level, wire[in[k]].level);
            }
            if (G.op == TFHE_F_LIN) {
                wire[self] = std::move(f);
                continue;
            }
            const int cls = c->lut_class[G.lut];
            const uint32_t fi = (uint32_t)forms.size(), lvl = f.level;
            forms.push_back(std::move(f));
            if (cls == 0) {
                boots.push_back(Boot{FM_LUT, G.lut, fi, lvl + 1, 0});
            } else {
                const uint32_t mods = cls == 2 ? FR_CT2Q | FR_OUT2Q : 0;
                boots.push_back(Boot{FM_HALF | mods, G.lut, fi, lvl + 1, 0});
                boots.push_back(Boot{(cls == 2 ? FM_LUT2 : FM_LUT1) | mods | FR_SECOND, G.lut, fi, lvl + 2,
                                     (uint32_t)boots.size() - 1});
            }
            Form& w = wire[self];
            w.terms = {{(uint64_t)CK_SLOT << 32 | (uint32_t)(boots.size() - 1), 1}};
            w.level = boots.back().level;
        }
        for (size_t o = 0; o < num_outputs; ++o)
            if (outputs[o] >= wires)
                return bad("output " + std::to_string(o) + " names wire " + std::to_string(outputs[o]) +
                           ", out of range (the netlist has " + std::to_string(wires) + " wires)");

        // slots: records sorted by level, then output modulus q before 2q, creation order otherwise
        std::vector<uint32_t> order(boots.size()), slot_of(boots.size());
        std::iota(order.begin(), order.end(), 0u);
        std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
            if (boots[x].level != boots[y].level) return boots[x].level < boots[y].level;
            return (boots[x].ctl & FR_OUT2Q) < (boots[y].ctl & FR_OUT2Q);
        });
        for (uint32_t s = 0; s < order.size(); ++s) slot_of[order[s]] = s;
        auto emit_terms = [&](const Form& f, uint32_t& term0, uint32_t& nterms) {
            term0 = (uint32_t)c->terms.size(), nterms = (uint32_t)f.terms.size();
            for (const auto& t : f.terms) {
                const uint32_t kind = (uint32_t)(t.first >> 32), idx = (uint32_t)t.first;
                c->terms.push_back(FuncTerm{kind, kind == CK_SLOT ? slot_of[idx] : idx, t.second});
            }
        };
        std::vector<std::pair<uint32_t, uint32_t>> form_terms(forms.size());  // both stages of a node share them
        for (size_t f = 0; f < forms.size(); ++f) emit_terms(forms[f], form_terms[f].first, form_terms[f].second);
        c->recs.resize(boots.size());
        for (uint32_t s = 0; s < order.size(); ++s) {
            const Boot& b = boots[order[s]];
            c->recs[s] = FuncRec{b.ctl, b.lut, form_terms[b.form].first, form_terms[b.form].second, forms[b.form].k,
                                 b.ctl & FR_SECOND ? slot_of[b.stage1] : 0, 0};
            if (c->levels.size() < b.level) c->levels.push_back(FuncLevel{s, 0, 0});  // levels are dense: ASAP
            c->levels.back().width++;
            if (!(b.ctl & FR_OUT2Q)) c->levels.back().width_q++;
        }
        c->outs.resize(num_outputs);
        for (size_t o = 0; o < num_outputs; ++o) {
            const Form& f = wire[outputs[o]];
            emit_terms(f, c->outs[o].term0, c->outs[o].nterms);
            c->outs[o].k = f.k;
        }
        I.num_inputs = num_inputs;
        I.num_outputs = (uint32_t)num_outputs;
        I.num_nodes = (uint32_t)num_nodes;
        I.bootstraps = (uint32_t)boots.size();
        I.levels = (uint32_t)c->levels.size();
        for (const FuncLevel& L : c->levels) I.widest_level = std::max(I.widest_level, L.width);
        I.num_luts = (uint32_t)num_luts;
        I.q = q;
        {
            std::lock_guard<std::mutex> lock(g_live_mu);
            live().insert(c.get());
        }
        *out = c.release();
        return TFHE_OK;
    });
}

tfhe_status tfhe_fcircuit_free(tfhe_fcircuit* c) {
    if (!c) return TFHE_OK;
    {
        std::lock_guard<std::mutex> lock(g_live_mu);
        if (!live().erase(c)) return dead("tfhe_fcircuit_free");
    }
    c->cache.release();
    delete c;
    return TFHE_OK;
}

tfhe_status tfhe_fcircuit_get_info(const tfhe_fcircuit* c, tfhe_fcircuit_info* out) {
    if (!fcircuit_alive(c)) return dead("tfhe_fcircuit_get_info");
    if (!out) return set_last_error(TFHE_ERR_INVALID_ARGUMENT, "tfhe_fcircuit_get_info: null argument");
    *out = c->info;
    return TFHE_OK;
}

tfhe_status tfhe_fcircuit_level_widths(const tfhe_fcircuit* c, uint32_t* widths, size_t cap) {
    if (!fcircuit_alive(c)) return dead("tfhe_fcircuit_level_widths");
    if (!widths && cap > 0) return set_last_error(TFHE_ERR_INVALID_ARGUMENT, "tfhe_fcircuit_level_widths: null argument");
    if (cap < c->levels.size())
        return set_last_error(TFHE_ERR_INVALID_ARGUMENT, "tfhe_fcircuit_level_widths: room for " + std::to_string(cap) +
                                                             " widths, the circuit has " +
                                                             std::to_string(c->levels.size()) + " levels");
    for (size_t l = 0; l < c->levels.size(); ++l) widths[l] = c->levels[l].width;
    return TFHE_OK;
}

tfhe_status tfhe_fcircuit_eval_plain(const tfhe_fcircuit* c, size_t instances, const uint64_t* in, uint64_t* out) {
    return host_guarded([&]() -> tfhe_status {
        if (!fcircuit_alive(c)) return dead("tfhe_fcircuit_eval_plain");
        if (!out || (!in && c->info.num_inputs > 0 && instances > 0))
            return set_last_error(TFHE_ERR_INVALID_ARGUMENT, "tfhe_fcircuit_eval_plain: null argument");
        const uint64_t q = c->info.q, mask = q - 1;
        std::vector<uint64_t> store(c->recs.size() * instances);
        auto form = [&](uint32_t term0, uint32_t nterms, uint64_t k, size_t i) {
            uint64_t v = k;
            for (uint32_t t = term0; t < term0 + nterms; ++t) {
                const FuncTerm& T = c->terms[t];
                v += T.coef * (T.kind == CK_SLOT ? store[T.idx * instances + i] : in[T.idx * instances + i]);
            }
            return v & mask;
        };
        // a first stage holds nothing the clear model needs: its second stage looks the form up itself
        for (size_t s = 0; s < c->recs.size(); ++s) {
            const FuncRec& r = c->recs[s];
            if ((r.ctl & 7) == FM_HALF) continue;
            for (size_t i = 0; i < instances; ++i)
                store[s * instances + i] = c->luts[r.lut * q + form(r.term0, r.nterms, r.k, i)];
        }
        for (size_t o = 0; o < c->outs.size(); ++o)
            for (size_t i = 0; i < instances; ++i)
                out[o * instances + i] = form(c->outs[o].term0, c->outs[o].nterms, c->outs[o].k, i);
        return TFHE_OK;
    });
}

}  // extern "C"
