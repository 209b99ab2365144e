// Stand-alone driver of the function-circuit compiler (tfhe-gpu_amd/csrc/fcircuit.cpp), for sanitizer builds on
// the CPU (tests/test_fcircuit_cpu.py builds it with AddressSanitizer and UBSan as host options): compiles the three-digit
// adder and a netlist with every table class, LIN chains and mixed levels, runs eval_plain against a direct
// model, hits every compile error, and frees -- once, twice, and uses a freed handle.  No GPU, no engine: the
// last-error channel the compiler reports through is defined here.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "fcircuit.hpp"

static std::string g_err;
tfhe_status tfhe::set_last_error(tfhe_status s, const std::string& msg) {
    g_err = msg;
    return s;
}

#define REQUIRE(cond)                                                                       \
    do {                                                                                    \
        if (!(cond)) {                                                                      \
            std::fprintf(stderr, "line %d: %s failed (last error: %s)\n", __LINE__, #cond, g_err.c_str()); \
            return 1;                                                                       \
        }                                                                                   \
    } while (0)

namespace {

constexpr uint64_t Q = 2048, P = 8, IV = Q / P;

std::vector<uint64_t> table(int64_t (*f)(int64_t)) {
    std::vector<uint64_t> t(Q);
    for (uint64_t i = 0; i < Q; ++i) t[i] = (uint64_t)(((f((int64_t)(i / IV)) % (int64_t)P + (int64_t)P) % (int64_t)P) * (int64_t)IV);
    return t;
}
int64_t f_mod4(int64_t m) { return m % 4; }
int64_t f_div4(int64_t m) { return m / 4; }
int64_t f_cube(int64_t m) { return m * m * m; }
int64_t f_neg1(int64_t m) { return m < 4 ? m + 1 : -(m - 3); }

using Node = tfhe_fcircuit_node;
Node lin(uint32_t in0, int32_t c0, uint32_t in1 = 0, int32_t c1 = 0, uint64_t k = 0) { return Node{TFHE_F_LIN, in0, in1, c0, c1, 0, k}; }
Node lut(uint32_t t, uint32_t in0, int32_t c0, uint32_t in1 = 0, int32_t c1 = 0, uint64_t k = 0) {
    return Node{TFHE_F_LUT, in0, in1, c0, c1, t, k};
}

// the netlist on clear values, node by node
std::vector<uint64_t> model(uint32_t ni, const std::vector<Node>& nodes, const std::vector<uint64_t>& luts,
                            const std::vector<uint32_t>& outs, const std::vector<uint64_t>& in) {
    std::vector<uint64_t> w(in.begin(), in.begin() + ni);
    for (const Node& n : nodes) {
        int64_t v = (int64_t)n.c0 * (int64_t)w[n.in0] + (n.c1 ? (int64_t)n.c1 * (int64_t)w[n.in1] : 0) + (int64_t)n.k;
        const uint64_t r = (uint64_t)(((v % (int64_t)Q) + (int64_t)Q) % (int64_t)Q);
        w.push_back(n.op == TFHE_F_LIN ? r : luts[n.lut * Q + r]);
    }
    std::vector<uint64_t> o;
    for (uint32_t x : outs) o.push_back(w[x]);
    return o;
}

int check_plain(tfhe_fcircuit* c, uint32_t ni, const std::vector<Node>& nodes, const std::vector<uint64_t>& luts,
                const std::vector<uint32_t>& outs, size_t instances) {
    std::vector<uint64_t> in(ni * instances), out(outs.size() * instances);
    uint64_t x = 12345;
    for (uint64_t& v : in) v = ((x = x * 6364136223846793005ull + 1442695040888963407ull) >> 40) % P * IV;
    REQUIRE(tfhe_fcircuit_eval_plain(c, instances, in.data(), out.data()) == TFHE_OK);
    for (size_t i = 0; i < instances; ++i) {
        std::vector<uint64_t> one(ni);
        for (uint32_t k = 0; k < ni; ++k) one[k] = in[k * instances + i];
        const std::vector<uint64_t> want = model(ni, nodes, luts, outs, one);
        for (size_t o = 0; o < outs.size(); ++o) REQUIRE(out[o * instances + i] == want[o]);
    }
    return 0;
}

}  // namespace

int main() {
    std::vector<uint64_t> luts;
    for (auto f : {f_mod4, f_div4, f_cube, f_neg1}) {
        const std::vector<uint64_t> t = table(f);
        luts.insert(luts.end(), t.begin(), t.end());
    }
    // three-digit base-4 adder: inputs x0 x1 x2 y0 y1 y2
    std::vector<Node> add = {lin(0, 1, 3, 1), lut(0, 6, 1), lut(1, 6, 1),
                             lin(1, 1, 4, 1), lin(9, 1, 8, 1), lut(0, 10, 1), lut(1, 10, 1),
                             lin(2, 1, 5, 1), lin(13, 1, 12, 1), lut(0, 14, 1), lut(1, 14, 1)};
    std::vector<uint32_t> add_out = {7, 11, 15, 16};
    tfhe_fcircuit* a = nullptr;
    REQUIRE(tfhe_fcircuit_compile(&a, 6, add.data(), add.size(), Q, luts.data(), 4, add_out.data(), add_out.size()) == TFHE_OK);
    tfhe_fcircuit_info I{};
    REQUIRE(tfhe_fcircuit_get_info(a, &I) == TFHE_OK && I.bootstraps == 12 && I.levels == 6 && I.widest_level == 2);
    REQUIRE(I.negacyclic == 1 && I.periodic == 1 && I.arbitrary == 2 && I.q == Q);
    uint32_t widths[8];
    REQUIRE(tfhe_fcircuit_level_widths(a, widths, 8) == TFHE_OK && widths[0] == 2 && widths[5] == 2);
    REQUIRE(tfhe_fcircuit_level_widths(a, widths, 5) == TFHE_ERR_INVALID_ARGUMENT);
    if (check_plain(a, 6, add, luts, add_out, 200)) return 1;

    // every class, LIN of LIN, negative and doubled coefficients, k, stages of different nodes in one level
    std::vector<Node> all = {lin(0, 1, 1, 1), lin(3, 2, 2, -1, IV), lut(3, 3, 1), lut(0, 4, 1), lut(2, 0, 1, 2, 1),
                             lut(0, 5, 1, 6, 1), lut(1, 5, 1), lut(2, 7, 1), lin(9, 1, 0, -3), lut(3, 11, 1, 8, 2, 2 * IV)};
    std::vector<uint32_t> all_out = {1, 4, 11, 5, 6, 7, 12, 10, 8};
    tfhe_fcircuit* b = nullptr;
    REQUIRE(tfhe_fcircuit_compile(&b, 3, all.data(), all.size(), Q, luts.data(), 4, all_out.data(), all_out.size()) == TFHE_OK);
    REQUIRE(tfhe_fcircuit_get_info(b, &I) == TFHE_OK && I.bootstraps == 12 && I.levels == 5 && I.widest_level == 3);
    if (check_plain(b, 3, all, luts, all_out, 300)) return 1;

    // every compile error names its node or table and leaves no handle
    tfhe_fcircuit* e = nullptr;
    const uint32_t o2[] = {2}, o9[] = {9};
    auto fails = [&](std::vector<Node> n, uint64_t q, const uint64_t* t, size_t nt, const uint32_t* o, size_t no, const char* names) {
        e = reinterpret_cast<tfhe_fcircuit*>(1);
        const tfhe_status st = tfhe_fcircuit_compile(&e, 2, n.data(), n.size(), q, t, nt, o, no);
        return st == TFHE_ERR_INVALID_ARGUMENT && e == nullptr && g_err.find(names) != std::string::npos;
    };
    Node unknown = lin(0, 1);
    unknown.op = 2;
    REQUIRE(fails({lin(0, 1), unknown}, Q, luts.data(), 4, o2, 1, "node 1"));
    REQUIRE(fails({lin(0, 1), lin(1, 1, 4, 1)}, Q, luts.data(), 4, o2, 1, "node 1"));   // forward
    REQUIRE(fails({lin(2, 1)}, Q, luts.data(), 4, o2, 1, "node 0"));                     // itself
    REQUIRE(fails({lin(77, 1)}, Q, luts.data(), 4, o2, 1, "node 0"));                    // out of range
    REQUIRE(fails({lut(4, 0, 1)}, Q, luts.data(), 4, o2, 1, "node 0"));                  // table index
    std::vector<uint64_t> big(luts.begin(), luts.begin() + 2 * Q);
    big[Q + 5] = Q;
    REQUIRE(fails({lut(0, 0, 1)}, Q, big.data(), 2, o2, 1, "table 1"));
    REQUIRE(fails({lin(0, 1, 0, 0, Q)}, Q, luts.data(), 4, o2, 1, "node 0"));            // k >= q
    REQUIRE(fails({lin(0, 1)}, 48, luts.data(), 4, o2, 1, "q = 48"));
    REQUIRE(fails({lin(0, 1)}, 4, luts.data(), 4, o2, 1, "q = 4"));
    REQUIRE(fails({lin(0, 1)}, Q, luts.data(), 4, o2, 0, "output"));
    REQUIRE(fails({lin(0, 1)}, Q, luts.data(), 4, o9, 1, "output 0"));
    REQUIRE(fails({lin(0, 1)}, Q, luts.data(), 4, nullptr, 1, "null"));
    REQUIRE(fails({lin(0, 1)}, Q, nullptr, 4, o2, 1, "null"));
    e = reinterpret_cast<tfhe_fcircuit*>(1);
    REQUIRE(tfhe_fcircuit_compile(&e, 2, nullptr, 3, Q, luts.data(), 4, o2, 1) == TFHE_ERR_INVALID_ARGUMENT && e == nullptr);
    REQUIRE(tfhe_fcircuit_compile(nullptr, 2, nullptr, 0, Q, luts.data(), 4, o2, 1) == TFHE_ERR_INVALID_ARGUMENT);

    // free; a freed handle is refused by every entry point, a second free included
    REQUIRE(tfhe_fcircuit_free(a) == TFHE_OK);
    REQUIRE(tfhe_fcircuit_free(a) == TFHE_ERR_INVALID_ARGUMENT);
    REQUIRE(tfhe_fcircuit_get_info(a, &I) == TFHE_ERR_INVALID_ARGUMENT);
    REQUIRE(tfhe_fcircuit_level_widths(a, widths, 8) == TFHE_ERR_INVALID_ARGUMENT);
    uint64_t v[6] = {0}, r[4];
    REQUIRE(tfhe_fcircuit_eval_plain(a, 1, v, r) == TFHE_ERR_INVALID_ARGUMENT);
    REQUIRE(tfhe_fcircuit_eval_plain(b, 1, v, nullptr) == TFHE_ERR_INVALID_ARGUMENT);
    REQUIRE(tfhe_fcircuit_free(b) == TFHE_OK);
    REQUIRE(tfhe_fcircuit_free(nullptr) == TFHE_OK);
    std::puts("fcircuit driver ok");
    return 0;
}
