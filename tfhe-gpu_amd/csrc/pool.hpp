// pool.hpp -- the host plan of a windowed pairwise reduction (tfhe_pool2d): what pool.cpp builds from
// the geometry, what engine.hip uploads once per (descriptor, device), and what the kernels of pool2d.hip read.
//
// Every (instance, plane, oy, ox) reduces the taps of its window that fall inside the plane, in order
// t = ky kw + kx, by a tournament: round l pairs the neighbours of its list, op(L[2j], L[2j+1]), and carries an odd
// last element unchanged (no record, no copy) until one element is left.  The geometry depends on (oy, ox) alone,
// so the plan is per plane: one 24-byte record {a, b, dst} per pair, the records of a round contiguous.  A source
// is an input tap or a slot of an earlier round's results, a destination a slot or -- for the last pair of a
// position -- the output position itself.  Every non-final result gets a slot of its own: no slot is written
// twice, so a round never reads what it writes.  Free of HIP headers.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace tfhe {

// a validated descriptor: oh = (h + 2 ph - kh) / sh + 1, ow likewise
struct PoolGeom {
    uint32_t c, h, w, kh, kw, sh, sw, ph, pw;
    uint32_t oh, ow;
};

// A row of n+1 words inside one plane.  a, b >= 0: input tap y w + x; dst >= 0: output position oy ow + ox;
// negative: slot ~v of the plane's slot store.
struct PoolRec {
    int64_t a, b, dst;
};
static_assert(sizeof(PoolRec) == 24, "three 8-byte loads per item");

struct PoolPlan {
    std::vector<PoolRec> recs;        // the pairs, round by round; then the copies
    std::vector<size_t> round_first;  // [rounds + 1]: round l is recs[round_first[l] .. round_first[l + 1])
    size_t copies = 0;                // positions with one valid tap: recs[round_first[rounds] ..) {b, b, dst}
    size_t slots = 0;                 // non-final results per plane
    size_t rounds() const { return round_first.size() - 1; }
    size_t pairs() const { return round_first.back(); }
    size_t widest() const;            // the most pairs of one round
};

// valid taps of output row / column o along one axis: size n, window k, stride s, padding p
inline uint32_t pool_valid(uint32_t o, uint32_t n, uint32_t k, uint32_t s, uint32_t p) {
    const int64_t lo = (int64_t)o * s - p, hi = lo + k;  // [lo, hi) clipped to [0, n)
    return (uint32_t)((hi < (int64_t)n ? hi : (int64_t)n) - (lo > 0 ? lo : 0));
}

// rounds = ceil(log2(most valid taps of a position)), pairs = sum over positions of (valid taps - 1); false when
// pairs leaves size_t.  O(oh + ow), no plan is built.
bool pool_counts(const PoolGeom& g, uint32_t& rounds, size_t& pairs);

PoolPlan pool_plan(const PoolGeom& g);

// the tournament on clear values mod q (a power of two): in[instances][c][h][w] -> out[instances][c][oh][ow],
// op(a, b) = b + lut[a - b mod q] mod q
void pool_eval_plain(const PoolGeom& g, const PoolPlan& plan, size_t instances, uint64_t q, const uint64_t* lut,
                     const uint64_t* in, uint64_t* out);

}  // namespace tfhe
