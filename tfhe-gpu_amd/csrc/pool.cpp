// pool.cpp -- the host plan of tfhe_pool2d (pool.hpp) and the tournament on clear values
// (tfhe_pool2d_eval_plain).  No GPU.
#include "pool.hpp"

#include <algorithm>

namespace tfhe {

size_t PoolPlan::widest() const {
    size_t m = 0;
    for (size_t l = 0; l + 1 < round_first.size(); ++l) m = std::max(m, round_first[l + 1] - round_first[l]);
    return m;
}

bool pool_counts(const PoolGeom& g, uint32_t& rounds, size_t& pairs) {
    // valid taps of a position = (valid rows) (valid columns): the sums and the maxima separate
    uint64_t sy = 0, sx = 0;
    uint32_t my = 0, mx = 0;
    for (uint32_t oy = 0; oy < g.oh; ++oy) {
        const uint32_t v = pool_valid(oy, g.h, g.kh, g.sh, g.ph);
        sy += v, my = std::max(my, v);
    }
    for (uint32_t ox = 0; ox < g.ow; ++ox) {
        const uint32_t v = pool_valid(ox, g.w, g.kw, g.sw, g.pw);
        sx += v, mx = std::max(mx, v);
    }
    const unsigned __int128 taps = (unsigned __int128)sy * sx, npos = (unsigned __int128)g.oh * g.ow;
    if (taps - npos > (unsigned __int128)SIZE_MAX) return false;
    pairs = (size_t)(taps - npos);
    const uint64_t most = (uint64_t)my * mx;
    rounds = 0;
    while (((uint64_t)1 << rounds) < most) ++rounds;
    return true;
}

PoolPlan pool_plan(const PoolGeom& g) {
    std::vector<std::vector<PoolRec>> rounds;
    std::vector<PoolRec> copies;
    std::vector<int64_t> cur, next;
    size_t slots = 0;
    for (uint32_t oy = 0; oy < g.oh; ++oy) {
        for (uint32_t ox = 0; ox < g.ow; ++ox) {
            const int64_t pos = (int64_t)oy * g.ow + ox;
            cur.clear();
            for (uint32_t ky = 0; ky < g.kh; ++ky) {
                const int64_t y = (int64_t)oy * g.sh - g.ph + ky;
                if (y < 0 || y >= (int64_t)g.h) continue;  // a tap in the padding is left out
                for (uint32_t kx = 0; kx < g.kw; ++kx) {
                    const int64_t x = (int64_t)ox * g.sw - g.pw + kx;
                    if (x >= 0 && x < (int64_t)g.w) cur.push_back(y * g.w + x);
                }
            }
            if (cur.size() == 1) copies.push_back(PoolRec{cur[0], cur[0], pos});
            for (size_t l = 0; cur.size() > 1; ++l) {
                if (rounds.size() <= l) rounds.emplace_back();
                next.clear();
                for (size_t j = 0; j + 1 < cur.size(); j += 2) {
                    const int64_t dst = cur.size() == 2 ? pos : ~(int64_t)slots++;
                    rounds[l].push_back(PoolRec{cur[j], cur[j + 1], dst});
                    next.push_back(dst);
                }
                if (cur.size() % 2) next.push_back(cur.back());  // carried: no record
                cur.swap(next);
            }
        }
    }
    PoolPlan p;
    p.round_first.push_back(0);
    for (const auto& r : rounds) {
        p.recs.insert(p.recs.end(), r.begin(), r.end());
        p.round_first.push_back(p.recs.size());
    }
    p.recs.insert(p.recs.end(), copies.begin(), copies.end());
    p.copies = copies.size();
    p.slots = slots;
    return p;
}

void pool_eval_plain(const PoolGeom& g, const PoolPlan& plan, size_t instances, uint64_t q, const uint64_t* lut,
                     const uint64_t* in, uint64_t* out) {
    const uint64_t mask = q - 1;
    const size_t in_plane = (size_t)g.h * g.w, out_plane = (size_t)g.oh * g.ow;
    std::vector<uint64_t> store(plan.slots);
    for (size_t ip = 0; ip < instances * g.c; ++ip) {
        const uint64_t* x = in + ip * in_plane;
        uint64_t* y = out + ip * out_plane;
        const auto src = [&](int64_t r) { return r >= 0 ? x[r] : store[(size_t)~r]; };
        for (size_t i = 0; i < plan.pairs(); ++i) {  // round by round: a slot is written before it is read
            const PoolRec& r = plan.recs[i];
            const uint64_t a = src(r.a), b = src(r.b), v = (b + lut[(a - b) & mask]) & mask;
            if (r.dst >= 0) y[r.dst] = v;
            else store[(size_t)~r.dst] = v;
        }
        for (size_t i = plan.pairs(); i < plan.recs.size(); ++i) y[plan.recs[i].dst] = x[plan.recs[i].b];
    }
}

}  // namespace tfhe
