// fcircuit.hpp -- the lowered plan of a function circuit (tfhe_fcircuit): what fcircuit.cpp compiles from a
// netlist of linear forms and LUT bootstraps, what engine.hip uploads once per device, and what the kernels
// of fcircuit_kernels.hip read.
//
// A plan holds one 32-byte record per bootstrap, in slot order.  A LUT node on a negacyclic table is one
// record; on a periodic or an arbitrary table it is two, a first stage (TV_HALF) and a second stage
// (TV_LUT1 / TV_LUT2) that also reads the first stage's slot.  Slot s is the s-th record after sorting by
// level (stable: creation order), and inside a level the records whose key switch ends at modulus q precede
// those that end at 2q, so a level's key switch is at most two launches on two contiguous slot ranges.
// The wire store of a run is [bootstraps][instances][n+1] words, as for tfhe_circuit.
//
// Linear forms are folded at compile time: every wire is sum_t coef_t * base_t + k mod q over base rows
// (inputs and second-stage / one-stage slots), like terms merged, so LIN nodes own no slot and cost no
// launch; q is a power of two, so the sum may wrap in 64 bits before it is masked.  A slot written at
// modulus 2q (an arbitrary table's second stage) is reduced mod q by the same mask whenever it is read
// (SetModulus(q), binfhe-base-scheme.cpp:770).
#pragma once

#include "circuit.hpp"

namespace tfhe {

// binfhe-base-scheme.cpp:162-186 checkInputFunction: 0 negacyclic, 1 periodic, 2 arbitrary
int check_input_function(const uint64_t* lut, uint64_t len, uint64_t mod);

struct FuncTerm {
    uint32_t kind, idx;  // CK_INPUT: input wire; CK_SLOT: slot
    uint64_t coef;       // mod q
};
static_assert(sizeof(FuncTerm) == 16, "one 16-byte load per term");

// ctl: bits 0-2 the test-vector mode (TvMode: TV_HALF, TV_LUT, TV_LUT1, TV_LUT2); bit 4: the ciphertext
// modulus is 2q; bit 5: the output modulus is 2q; bit 6: second stage (reads slot `stage1`).
// The prepared ciphertext is (form + k mod q), then as dev_func (engine.hip) at the ciphertext modulus m:
// first / only stage b += 128; second stage (ct - stage1), b += 128, b -= m / 4.
struct FuncRec {
    uint32_t ctl, lut;
    uint32_t term0, nterms;  // terms[term0 .. term0 + nterms)
    uint64_t k;
    uint32_t stage1, reserved;
};
static_assert(sizeof(FuncRec) == 32, "two 16-byte loads per workgroup");
constexpr uint32_t FR_CT2Q = 1u << 4, FR_OUT2Q = 1u << 5, FR_SECOND = 1u << 6;
// the modes a record can name: TvMode's values (kernels.hpp; fcircuit_kernels.hip asserts the equality),
// restated so that the compiler stays free of HIP headers
enum FuncMode : uint32_t { FM_HALF = 1, FM_LUT = 4, FM_LUT1 = 5, FM_LUT2 = 6 };

// an output wire: its folded form
struct FuncOut {
    uint32_t term0, nterms;
    uint64_t k;
};

struct FuncLevel {
    uint32_t first, width, width_q;  // slots [first, first + width); the first width_q end at modulus q
};

}  // namespace tfhe

struct tfhe_fcircuit {
    tfhe_fcircuit_info info{};
    std::vector<tfhe::FuncRec> recs;      // [bootstraps], slot order
    std::vector<tfhe::FuncTerm> terms;    // of the records, then of the outputs
    std::vector<tfhe::FuncOut> outs;      // [num_outputs]
    std::vector<tfhe::FuncLevel> levels;  // [info.levels]
    std::vector<uint64_t> luts;           // [num_luts][q]
    std::vector<uint8_t> lut_class;       // [num_luts]
    tfhe::PlanCache cache;                // device copies of recs | terms | outs | luts
};

namespace tfhe {
// Handles are looked up in a registry of live circuits before they are followed, so a freed (or never
// compiled) handle is TFHE_ERR_INVALID_ARGUMENT in every entry point, not a use after free.
bool fcircuit_alive(const tfhe_fcircuit* c);
}  // namespace tfhe
