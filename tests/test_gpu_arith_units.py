"""GPU: the kernels' arithmetic __device__ functions against exact integers.

The lazy-reduction schedules rest on lemmas about small device functions (sf_mul's result formula and carry,
|smul(y, w)| <= |y| (Q/2) / 2^32 + Q/2, fmodmul's residual bound, shoup_lazy in [0, 2Q)); tools/bounds_sf.py,
bounds_fast4.py and bounds_f64.py assume them.  Here the test library's arithmetic probes
(tfhe-gpu_amd/csrc/arith_probes.hpp: one tfhe_test_arith_<family> entry point per source file, each calling the
real functions on operands loaded from memory and storing the raw, unreduced results) run them at the operands
the lemmas are about, and Python integers (Python floats where the function restates an IEEE formula) say what
must come out.  Bounds come from the tools' own functions (bounds_fast4.smul_b, bounds_f64.Arith.fmodmul / fred,
bounds_sf.ct / gs / mulw / fold), never from a probe's output.

Every function runs N_RANDOM random cases plus its corner list, shuffled so that corner and random cases (for
sf_mul: carry and no-carry products) sit in neighbouring lanes of one wavefront, in launches of 256-lane
workgroups; then three more times with the lanes lane % 3 == r branched around the call (sf_mul's carry lives in
a lane mask): the lanes that ran must reproduce the full run, the others must have stored nothing.  No case is
skipped: a case the probe did not store fails the test.

The probes compile the functions into small kernels of their own, so they test the functions' arithmetic, not
the instruction spacing of the product kernels around them.
"""
import ctypes as C
import math
import os
import random
import sys
from fractions import Fraction

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M32, M64 = (1 << 32) - 1, (1 << 64) - 1
SENT = 0xA5A5A5A55A5A5A5A  # what the output buffer holds where a probe stored nothing
N_RANDOM = 20000
TAB = 512  # twiddle-table entries of the radix cores (the largest index the kernels' (m0, g) reach is 511)
FWD_MG = [(1, 0)] + [(8, g) for g in range(8)] + [(64, g) for g in range(64)]      # the kernels' forward (m0, g)
INV_MG = [(256, g) for g in range(64)] + [(32, g) for g in range(8)] + [(4, 0)]    # and inverse (m, g)


def _tool(name):
    """tools/<name>.py as a module (bounds_fast4 reads sys.argv and runs its checks on import)"""
    import importlib

    tools = os.path.join(ROOT, "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    argv, sys.argv = sys.argv, [name + ".py"]
    try:
        return importlib.import_module(name)
    finally:
        sys.argv = argv


def _is_prime(n):
    if n < 2:
        return False
    for p in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        if n % p == 0:
            return n == p
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):  # deterministic below 2^64
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def _prev_prime(n):
    n -= 1
    while not _is_prime(n):
        n -= 1
    return n


def _s64(v):
    return v - (1 << 64) if v >> 63 else v


def _mix(rng, corners, rand, n=N_RANDOM):
    """the corner cases (a list of rows) and n random rows (rand() -> row), shuffled together"""
    rows = list(corners) + [rand() for _ in range(n)]
    rng.shuffle(rows)
    return rows


def _pick(rng, corners, rand, p=0.25):
    """a corner value with probability p, else a random one"""
    return rng.choice(corners) if rng.random() < p else rand()


class Probes:
    FAMILIES = ("dm", "kg", "g3", "sf", "f64", "fast4")

    def __init__(self):
        import torch
        from tfhe_amd import capi

        self.torch = torch
        self.L = capi.lib(capi.TEST_LIB)
        sig = [C.c_int, C.c_uint64, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
        self.fn = {}
        for f in self.FAMILIES:
            fn = getattr(self.L, "tfhe_test_arith_" + f)
            fn.argtypes, fn.restype = sig, C.c_int
            self.fn[f] = fn
        self.counts = {}

    def _dev(self, words):
        a = np.array(words, dtype=np.uint64)
        return self.torch.from_numpy(a.view(np.int64).ravel().copy()).cuda()

    def _call(self, family, op, Q, d_in, cases, ni, no, d_tab, tab_words):
        out = self.torch.full((cases * no,), _s64(SENT), dtype=self.torch.int64, device="cuda")
        self.torch.cuda.synchronize()
        rc = self.fn[family](op, Q, cases, d_in.data_ptr(), cases * ni, d_tab.data_ptr() if d_tab is not None else None,
                             tab_words, out.data_ptr(), cases * no)
        assert rc == 0, (family, op, rc)
        return out.cpu().numpy().view(np.uint64).reshape(cases, no)

    def run(self, family, name, op, Q, rows, no, tab=None):
        """rows: the cases (equal-length lists of words, already reduced mod 2^64) -> their `no` output words each.
        Full run, then the three runs with every third lane branched out."""
        cases, ni = len(rows), len(rows[0])
        d_in = self._dev(rows)
        d_tab = self._dev(tab) if tab is not None else None
        tw = len(tab) if tab is not None else 0
        full = self._call(family, op, Q, d_in, cases, ni, no, d_tab, tw)
        untouched = np.flatnonzero(full[:, 0] == np.uint64(SENT))
        assert untouched.size == 0, f"{name}: {untouched.size} cases not run, first {rows[int(untouched[0])]}"
        lane = np.arange(cases) % 64
        for r in range(3):
            part = self._call(family, op | ((r + 1) << 8), Q, d_in, cases, ni, no, d_tab, tw)
            out_lanes = lane % 3 == r
            assert np.all(part[out_lanes] == np.uint64(SENT)), f"{name}: a branched-out lane stored (r = {r})"
            assert np.array_equal(part[~out_lanes], full[~out_lanes]), f"{name}: differs under the lane mask (r = {r})"
        self.counts[name] = max(self.counts.get(name, 0), cases)
        print(f"{name}: Q = {Q}, {cases} cases x 4 launches")
        return full.tolist()


@pytest.fixture(scope="module")
def probes():
    return Probes()


# ---------------------------------------------------------------- device_math.hpp: Shoup arithmetic
U32_Q = [12289, 134215681, _prev_prime(1 << 30)]
U64_Q = [4294991873, (1 << 54) - 77823, _prev_prime(1 << 58)]


def _a_corners(Q, b):
    return [0, 1, Q - 1, Q, 2 * Q - 1, 2 * Q, 4 * Q - 1, 1 << (b - 1), (1 << b) - 1]


def _w_corners(Q):
    return [0, 1, 2, Q - 2, Q - 1, (Q - 1) // 2, (Q + 1) // 2]


def _shoup_lazy_ref(a, w, wp, Q, b):
    r = a * w - ((a * wp) >> b) * Q
    assert 0 <= r < 2 * Q and r % Q == a * w % Q  # Shoup's lemma, for any a < 2^b and w < Q
    return r


@pytest.mark.parametrize("b,Q", [(32, q) for q in U32_Q] + [(64, q) for q in U64_Q])
def test_shoup_family(probes, b, Q):
    """shoup_lazy (in [0, 2Q), = a w - floor(a w' / 2^b) Q), shoup, reduce_full, addm, subm, csub."""
    assert _is_prime(Q) and 4 * Q < 1 << b
    rng = random.Random(Q)
    wbit = 16 if b == 32 else 0
    ac, wc = _a_corners(Q, b), _w_corners(Q)

    def aw():
        a, w = _pick(rng, ac, lambda: rng.getrandbits(b)), _pick(rng, wc, lambda: rng.randrange(Q))
        return [a, w, (w << b) // Q]

    rows = _mix(rng, [[a, w, (w << b) // Q] for a in ac for w in wc], aw)
    for name, op, ref in (("shoup_lazy", 0, lambda a, w, wp: _shoup_lazy_ref(a, w, wp, Q, b)),
                          ("shoup", 1, lambda a, w, wp: a * w % Q)):
        got = probes.run("dm", f"{name}<u{b}>", op | wbit, Q, rows, 1)
        bad = [(r, g[0]) for r, g in zip(rows, got) if g[0] != ref(*r)]
        assert not bad, (name, len(bad), bad[:3])
    r1 = (1 << b) // Q
    rows = _mix(rng, [[a, r1, 0] for a in ac], lambda: [rng.getrandbits(b), r1, 0])
    got = probes.run("dm", f"reduce_full<u{b}>", 2 | wbit, Q, rows, 1)
    assert all(g[0] == r[0] % Q for r, g in zip(rows, got))
    rows = _mix(rng, [[a, c, 0] for a in wc for c in wc], lambda: [_pick(rng, wc, lambda: rng.randrange(Q)),
                                                                   _pick(rng, wc, lambda: rng.randrange(Q)), 0])
    got = probes.run("dm", f"addm<u{b}>", 3 | wbit, Q, rows, 1)
    assert all(g[0] == (r[0] + r[1]) % Q for r, g in zip(rows, got))
    got = probes.run("dm", f"subm<u{b}>", 4 | wbit, Q, rows, 1)
    assert all(g[0] == (r[0] - r[1]) % Q for r, g in zip(rows, got))
    rows = _mix(rng, [[a, 0, 0] for a in ac], lambda: [rng.getrandbits(b), 0, 0])
    got = probes.run("dm", f"csub<u{b}>", 5 | wbit, Q, rows, 1)
    assert all(g[0] == (r[0] - Q if r[0] >= Q else r[0]) for r, g in zip(rows, got))


def _plain_core(v, m, g, fwd, bf):
    """the radix-8 cores' three stages with the kernels' twiddle indices (g3 / sf / f64 cores share them);
    bf(x, y, index, stage) -> (x', y')"""
    v = list(v)
    if fwd:
        for k in range(4):
            v[k], v[k + 4] = bf(v[k], v[k + 4], m + g, 0)
        for a, c, o in ((0, 2, 0), (1, 3, 0), (4, 6, 1), (5, 7, 1)):
            v[a], v[c] = bf(v[a], v[c], 2 * m + 2 * g + o, 1)
        for j in range(4):
            v[2 * j], v[2 * j + 1] = bf(v[2 * j], v[2 * j + 1], 4 * m + 4 * g + j, 2)
    else:
        for j in range(4):
            v[2 * j], v[2 * j + 1] = bf(v[2 * j], v[2 * j + 1], m + 4 * g + j, 0)
        for a, c, o in ((0, 2, 0), (1, 3, 0), (4, 6, 1), (5, 7, 1)):
            v[a], v[c] = bf(v[a], v[c], (m >> 1) + 2 * g + o, 1)
        for k in range(4):
            v[k], v[k + 4] = bf(v[k], v[k + 4], (m >> 2) + g, 2)
    return v


def _mod_core(v, m, g, fwd, w, Q):
    """the same network in plain modular arithmetic: x + y w, x - y w (forward); x + y, (x - y) w (inverse)"""
    if fwd:
        return _plain_core(v, m, g, True, lambda x, y, i, s: ((x + y * w[i]) % Q, (x - y * w[i]) % Q))
    return _plain_core(v, m, g, False, lambda x, y, i, s: ((x + y) % Q, (x - y) * w[i] % Q))


@pytest.mark.parametrize("b,Q", [(32, q) for q in U32_Q] + [(64, q) for q in U64_Q])
def test_harvey_butterflies_and_gen3_cores(probes, b, Q):
    """ct_lazy: [0, 4Q) -> [0, 4Q); gs_lazy: [0, 2Q) -> [0, 2Q); g3_fwd_core / g3_inv_core: three such stages at
    the kernel's (m0, g) with twiddles and Shoup companions from a table of values below Q."""
    rng = random.Random(Q + 1)
    wbit = 16 if b == 32 else 0
    wc = _w_corners(Q)

    def ct(x, y, w, ws):
        u, v = (x - 2 * Q if x >= 2 * Q else x), _shoup_lazy_ref(y, w, ws, Q, b)
        return u + v, u + 2 * Q - v

    def gs(x, y, w, ws):
        s = x + y
        return (s - 2 * Q if s >= 2 * Q else s), _shoup_lazy_ref(x + 2 * Q - y, w, ws, Q, b)

    for name, op, lim, ref, cong in (("ct_lazy", 0, 4 * Q, ct, lambda x, y, w: (x + y * w, x - y * w)),
                                     ("gs_lazy", 1, 2 * Q, gs, lambda x, y, w: (x + y, (x - y) * w))):
        xc = [v for v in (0, 1, Q - 1, Q, 2 * Q - 1, 2 * Q, 4 * Q - 1) if v < lim]

        def case():
            w = _pick(rng, wc, lambda: rng.randrange(Q))
            return [_pick(rng, xc, lambda: rng.randrange(lim)), _pick(rng, xc, lambda: rng.randrange(lim)), w, (w << b) // Q]

        rows = _mix(rng, [[x, y, w, (w << b) // Q] for x in xc for y in xc for w in wc], case)
        rows = [r + [0] * 6 for r in rows]
        got = probes.run("g3", f"{name}<u{b}>", op | wbit, Q, rows, 8)
        for r, g in zip(rows, got):
            want = ref(*r[:4])
            assert tuple(g[:2]) == want, (name, r, g[:2], want)
            assert all(0 <= v < lim for v in want)
            assert all((a - c) % Q == 0 for a, c in zip(want, cong(*r[:3])))
    w = wc + [rng.randrange(Q) for _ in range(TAB - len(wc))]
    rng.shuffle(w)
    ws = [(x << b) // Q for x in w]
    for name, op, fwd, lim, mgs in (("g3_fwd_core", 2, True, 4 * Q, FWD_MG), ("g3_inv_core", 3, False, 2 * Q, INV_MG)):
        xc = [v for v in (0, 1, Q - 1, Q, 2 * Q - 1, 2 * Q, 4 * Q - 1) if v < lim]
        rows = []
        for i in range(N_RANDOM + len(mgs)):
            m, g = mgs[i % len(mgs)]
            rows.append([_pick(rng, xc, lambda: rng.randrange(lim), 0.2) for _ in range(8)] + [m, g])
        got = probes.run("g3", f"{name}<u{b}>", op | wbit, Q, rows, 8, tab=w + ws)
        bf = (lambda x, y, i, s: ct(x, y, w[i], ws[i])) if fwd else (lambda x, y, i, s: gs(x, y, w[i], ws[i]))
        for r, out in zip(rows, got):
            want = _plain_core(r[:8], r[8], r[9], fwd, bf)
            assert out == want, (name, r)
            assert all(0 <= v < lim for v in want)
            assert [v % Q for v in want] == _mod_core(r[:8], r[8], r[9], fwd, w, Q)


# ---------------------------------------------------------------- round_qQ
def test_round_qQ(probes, oracle):
    """round_qQ(v, q, Q) = the reference's IEEE formula floor(0.5 + (double)v * (double)q / (double)Q) % q in
    Python floats, for the modulus pairs of every parameter set (Q -> qKS, qKS -> q, Q -> q), at 0, 1, Q - 1,
    the neighbours of the rounding boundaries (k + 1/2) Q / q, random v, and values found here where the exact
    rational rounding differs from the double formula."""
    from test_gpu_paramsets import ALL_SETS

    def ref(v, q, Q):
        return int(math.floor(0.5 + float(v) * float(q) / float(Q))) % q

    pairs = set()
    for name in ALL_SETS:
        p = oracle.params_from_set(name)
        pairs |= {(p.qKS, p.Q), (p.q, p.qKS), (p.q, p.Q)}
    for spec in ((True, 12, 0, 0, 1), (False, 23, 0, 0, 1)):
        p = oracle.params_from_logq("STD128", *spec)
        pairs |= {(p.qKS, p.Q), (p.q, p.qKS), (p.q, p.Q)}
    rng = random.Random(5)
    rows, inexact = [], 0
    for q, Q in sorted(pairs):
        rows += [[v, q, Q] for v in (0, 1, Q - 1, Q // 2, Q // 2 + 1)]
        for _ in range(600):
            k = rng.randrange(q)
            mid = (2 * k + 1) * Q // (2 * q)  # floor of the boundary between k and k + 1
            for v in (mid - 1, mid, mid + 1, mid + 2):
                if 0 <= v < Q:
                    rows.append([v, q, Q])
                    if (2 * v * q + Q) // (2 * Q) % q != ref(v, q, Q):
                        inexact += 1
        rows += [[rng.randrange(Q), q, Q] for _ in range(600)]
    rng.shuffle(rows)
    print(f"round_qQ: {len(pairs)} modulus pairs, {inexact} cases where the exact rounding differs from the double formula")
    got = probes.run("dm", "round_qQ", 6, 3, rows, 1)
    bad = [(r, g[0], ref(*r)) for r, g in zip(rows, got) if g[0] != ref(*r)]
    assert not bad, (len(bad), bad[:3])


# ---------------------------------------------------------------- the special-form leaves (blind_rotate_sf.hip)
SF_C = [1, 77823, 876543, (1 << 20) - 1]
INV_FOLDS = [False, True, False, False, True, False, False, True, False, False, False]  # units, C, B, A


def _sf_mul_ref(a, w0, w1, c2):
    S = (a & M32) * w0 + (a >> 32) * w1
    return (S & ((1 << 55) - 1)) + (S >> 55) * c2


def _sf_fold_ref(x, c):
    return (x & ((1 << 54) - 1)) + (x >> 54) * c


class SfBounds:
    """the per-stage input bounds of the sf transforms, from tools/bounds_sf.py's own butterfly functions"""

    def __init__(self, c):
        bs = _tool("bounds_sf")
        bs.A = bs.Arith(c)
        self.bs, self.c, self.Q = bs, c, (1 << 54) - c
        Q = self.Q
        self.fwd, x = [], (28 * Q - Q // 2, 28 * Q + Q // 2)  # digits r + 28Q, |r| <= Q/2
        for _ in range(11):
            self.fwd.append(x)
            a, d = bs.ct(x, x)
            x = (min(a[0], d[0]), max(a[1], d[1]))
        self.fwd_ofs, x = [], (0, 2 * Q)  # sf2p / sf2duo: r + Q, the offset in the difference
        for _ in range(11):
            self.fwd_ofs.append(x)
            a, d = bs.ct_ofs(x, x)
            x = (0, max(a[1], d[1]))
        self.inv, y = [], bs.fold(M64)  # S is a fold's output
        for f in INV_FOLDS:
            self.inv.append(y)
            y = max(bs.gs(y, y, f))
        self.inv_out = y
        assert bs.ok, "tools/bounds_sf.py reports a violation on this schedule"


def _sf_table(rng, Q):
    w = [0, 1, Q - 1, Q - 2, M32, 1 << 32, Q >> 1] + [rng.randrange(Q) for _ in range(TAB - 7)]
    rng.shuffle(w)
    return w, [(x << 32) % Q for x in w]


@pytest.mark.parametrize("c", SF_C)
def test_sf_mul_and_fold(probes, c):
    """sf_mul(a, W0, W1) == (S mod 2^55) + (S >> 55) 2c, S = a0 W0 + a1 W1, bit for bit (and == tools/bounds_sf.py's
    register-level model, and = a w mod Q for (W0, W1) = (w, w 2^32 mod Q)); sf_fold exact and below 2^54 + 2^10 c."""
    Q, c2 = (1 << 54) - c, 2 * c
    bs = _tool("bounds_sf")
    rng = random.Random(c)
    # bounds_sf.exactness's corner lists
    ws = [0, 1, Q - 1, Q - 2, M32, 1 << 32, Q >> 1]
    As = [0, 1, M64, M64 - 1, M32, 1 << 32, 1 << 63, Q, 3 * Q]
    corners = [[a, w, (w << 32) % Q] for a in As for w in ws]
    # P = a0 W0lo + a1 W1lo at 2^64 - 1, 2^64, 2^64 + 1 (the carry out of the first mad), any high halves
    for a1, w1lo, P in ((2, M32, M64), (7, 1227133513, 1 << 64), (4, 1 << 31, (1 << 64) + 1)):
        assert M32 * M32 + a1 * w1lo == P
        for _ in range(16):
            corners.append([(a1 << 32) | M32, (rng.getrandbits(22) << 32) | M32, (rng.getrandbits(22) << 32) | w1lo])
        corners.append([(a1 << 32) | M32, ((1 << 22) - 1) << 32 | M32, ((1 << 22) - 1) << 32 | w1lo])

    def case():
        a = _pick(rng, As, lambda: rng.getrandbits(64), 0.1)
        if rng.random() < 0.5:  # a constant as the kernels hold it
            w = _pick(rng, ws, lambda: rng.randrange(Q), 0.1)
            return [a, w, (w << 32) % Q]
        return [a, rng.getrandbits(54), rng.getrandbits(54)]  # arithmetic only: any W0, W1 < 2^54

    def carry_case():  # all four low factors >= 3/4 2^32: P >= 9/8 2^64 (uniform operands carry once in ten)
        r, top = case(), 3 << 30
        return [r[0] | top << 32 | top, r[1] | top, r[2] | top]

    rows = corners + [case() if i % 5 < 3 else carry_case() for i in range(N_RANDOM)]
    carry = [r for r in rows if (r[0] & M32) * (r[1] & M32) + (r[0] >> 32) * (r[2] & M32) >> 64]
    plain = [r for r in rows if not (r[0] & M32) * (r[1] & M32) + (r[0] >> 32) * (r[2] & M32) >> 64]
    rng.shuffle(carry), rng.shuffle(plain)
    assert min(len(carry), len(plain)) > len(rows) // 5
    k = min(len(carry), len(plain))
    rows = [r for pair in zip(carry[:k], plain[:k]) for r in pair] + carry[k:] + plain[k:]  # neighbours differ in the carry
    got = probes.run("sf", "sf_mul", 0, Q, [r + [0] * 7 for r in rows], 8)
    for r, g in zip(rows, got):
        want = _sf_mul_ref(*r, c2)
        assert g[0] == want, (r, g[0], want)
        assert want == bs.sf_mul_model(*r, c2) and want < (1 << 55) + (1 << 32) * c2
        if r[2] == (r[1] << 32) % Q and r[1] < Q:
            assert want % Q == r[0] * r[1] % Q
    xc = [0, 1, (1 << 54) - 1, 1 << 54, (1 << 54) + 1, Q - 1, Q, 2 * Q, 28 * Q, M64, M64 - 1, 1 << 63, (1 << 63) - 1]
    rows = _mix(rng, [[x] for x in xc], lambda: [rng.getrandbits(rng.choice((64, 64, 60, 56, 55)))])
    got = probes.run("sf", "sf_fold", 1, Q, [r + [0] * 9 for r in rows], 8)
    for r, g in zip(rows, got):
        assert g[0] == _sf_fold_ref(r[0], c) and g[0] < (1 << 54) + (1 << 10) * c and g[0] % Q == r[0] % Q


@pytest.mark.parametrize("c", SF_C)
def test_sf_butterflies_and_cores(probes, c):
    """sf_ct (offset-free and OFS), sf_gs (FOLD or not), sf_fwd_core, sf_inv_core at the lower and upper input bounds
    tools/bounds_sf.py derives for every stage: exact results, no difference ever negative, nothing reaches 2^64."""
    B = SfBounds(c)
    Q, c2 = B.Q, 2 * c
    rng = random.Random(c + 1)
    w0, w1 = _sf_table(rng, Q)

    def ct(ofs):
        def bf(x, y, i, s=0):
            v = _sf_mul_ref(y, w0[i], w1[i], c2)
            d = x + 3 * Q - v if ofs else x - v
            assert d >= 0 and x + v <= M64 and d <= M64, "forward difference negative or a value past 2^64"
            return x + v, d
        return bf

    def gs(fold_stage):
        def bf(x, y, i, s=0):
            d, sm = x + 10 * Q - y, x + y
            assert d >= 0 and d <= M64 and sm <= M64, "inverse difference negative or a value past 2^64"
            return (_sf_fold_ref(sm, c) if s == fold_stage else sm), _sf_mul_ref(d, w0[i], w1[i], c2)
        return bf

    def between(lo_hi):
        lo, hi = lo_hi
        return _pick(rng, [lo, hi, lo + 1, hi - 1], lambda: rng.randint(lo, hi), 0.3)

    for name, op, stages, bf in (("sf_ct<OFS=0>", 2, B.fwd, ct(False)), ("sf_ct<OFS=1>", 3, B.fwd_ofs, ct(True)),
                                 ("sf_gs<FOLD=0>", 4, [(0, y) for y in B.inv], gs(None)),
                                 ("sf_gs<FOLD=1>", 5, [(0, y) for y in B.inv], gs(0))):
        corners = [[x, y, i] for st in stages for x in st for y in st for i in range(0, TAB, 37)]
        rows = _mix(rng, corners, lambda: (lambda st: [between(st), between(st), rng.randrange(TAB)])(rng.choice(stages)))
        got = probes.run("sf", name, op, Q, [r + [0] * 7 for r in rows], 8, tab=w0 + w1)
        for r, g in zip(rows, got):
            assert tuple(g[:2]) == bf(*r), (name, r)
    for name, op, fwd, mgs, stages, bf in (
            ("sf_fwd_core<OFS=0>", 9, True, FWD_MG, B.fwd, ct(False)), ("sf_fwd_core<OFS=1>", 10, True, FWD_MG, B.fwd_ofs, ct(True)),
            ("sf_inv_core<FOLD=0>", 11, False, INV_MG, [(0, y) for y in B.inv], gs(None)),
            ("sf_inv_core<FOLD=1>", 12, False, INV_MG, [(0, y) for y in B.inv], gs(2))):
        rows = []
        for i in range(N_RANDOM + len(mgs)):
            m, g = mgs[i % len(mgs)]
            # the transform stage this (m0, g) starts at: forward m0 = 2^s; inverse m = 2^(10 - s)
            s = m.bit_length() - 1 if fwd else 10 - (m.bit_length() - 1)
            rows.append([between(stages[s]) for _ in range(8)] + [m, g])
        got = probes.run("sf", name, op, Q, rows, 8, tab=w0 + w1)
        for r, out in zip(rows, got):
            want = _plain_core(r[:8], r[8], r[9], fwd, bf)
            assert out == want, (name, r)
            assert [v % Q for v in want] == _mod_core(r[:8], r[8], r[9], fwd, w0, Q)


@pytest.mark.parametrize("c", SF_C)
def test_sf_accumulator_and_digits(probes, c):
    """sf_add_acc lands in [0, Q) for an accumulator in [0, Q) and any increment up to the inverse's output bound;
    sf_load_acc = v mod Q; sf_digit = the signed digit of the centred coefficient (SignedDigitDecompose, digit by
    digit) for the contexts' digit shapes (27- and 18-bit digits, thrown digits counted)."""
    B = SfBounds(c)
    Q = B.Q
    rng = random.Random(c + 2)
    half = Q >> 1
    edge = [0, 1, Q - 1, Q - 2, half, half + 1, half - 1, half + 2]
    incs = [0, 1, Q - 1, Q, Q + 1, 2 * Q, B.inv_out, B.inv_out - 1, 18 * Q]
    rows = _mix(rng, [[a, i] for a in edge for i in incs],
                lambda: [_pick(rng, edge, lambda: rng.randrange(Q)), _pick(rng, incs, lambda: rng.randint(0, B.inv_out))])
    got = probes.run("sf", "sf_add_acc", 6, Q, [r + [0] * 8 for r in rows], 8)
    for r, g in zip(rows, got):
        assert g[0] == (r[0] + r[1]) % Q, r
        f = _sf_fold_ref(r[0] + r[1], c)
        assert r[0] + r[1] <= M64 and f < 2 * Q  # one fold, one conditional subtraction (the tool's claim)
    vs = [0, 1, Q - 1, Q, Q + 1, 2 * Q, M64, M64 - 1, 1 << 63]
    rows = _mix(rng, [[v] for v in vs], lambda: [rng.getrandbits(rng.choice((64, 58, 54)))])
    got = probes.run("sf", "sf_load_acc", 8, Q, [r + [0] * 9 for r in rows], 8)
    assert all(g[0] == r[0] % Q for r, g in zip(rows, got))

    def digit(x, logG, lt):
        d, Bg = (x if x < half else x - Q), 1 << logG
        for _ in range(lt + 1):
            r = d & (Bg - 1)
            r = r - Bg if r >= Bg // 2 else r
            d = (d - r) >> logG
        return r

    shapes = [(27, 0), (27, 1), (18, 0), (18, 1), (18, 2)]

    def drow(x, logG, lt):
        Kd = sum((1 << (logG - 1)) << (z * logG) for z in range(lt))
        return [x, half, Kd & M64, (Kd - Q) & M64, lt * logG, 64 - logG]

    rows = _mix(rng, [drow(x, *s) for x in edge for s in shapes],
                lambda: drow(_pick(rng, edge, lambda: rng.randrange(Q), 0.05), *rng.choice(shapes)))
    got = probes.run("sf", "sf_digit", 7, Q, [r + [0] * 4 for r in rows], 8)
    for r, g in zip(rows, got):
        logG = 64 - r[5]
        assert _s64(g[0]) == digit(r[0], logG, r[4] // logG), r


# ---------------------------------------------------------------- the exact-FP64 leaves (blind_rotate_f64.hip)
F64_Q = [4294991873, (1 << 37) - (1 << 17) + 1, (1 << 40) - 36863, 4398044577793, (1 << 50) - (1 << 14) + 1]
F64_Q.append(next(q for q in range((1 << 40) - 36863 - 4096, 0, -4096) if _is_prime(q)))  # a second prime in (2^40 - 2^20, 2^40)


def _f2u(x):
    return int(np.array([float(x)], dtype=np.float64).view(np.uint64)[0])


def _u2f(rows):
    return np.array(rows, dtype=np.uint64).view(np.float64).tolist()


@pytest.fixture(scope="module")
def f64_arith():
    bf = _tool("bounds_f64")
    memo = {}

    def get(Q):
        if Q not in memo:
            reducing = Q >= 1 << 40
            ar, *_ = bf.walk(Q, 1 if reducing else 2, reducing)
            assert ar.worst < 2.0 ** 53
            memo[Q] = (bf.Arith(Q), int(ar.worst))  # the largest operand or sum the schedule's walk reports
        return memo[Q]

    return get


def _as_int(x, what):
    assert x == math.floor(x) and abs(x) < 2.0 ** 53, (what, x)
    return int(x)


@pytest.mark.parametrize("Q", F64_Q)
def test_fmodmul_fred_and_butterflies(probes, f64_arith, Q):
    """fmodmul / fred: an integer, congruent to a b (to x) mod Q exactly, within Arith.fmodmul / Arith.fred of
    tools/bounds_f64.py -- for |b| <= Q/2 and |a| up to the largest operand that tool's walk reports, and for
    products a b = (Q +- 1)/2 mod Q, where the quotient's rounding ties; ct_bf / gs_bf on top of them."""
    assert _is_prime(Q) and Q % 4096 == 1
    ar, A = f64_arith(Q)
    rng = random.Random(Q)
    Qh = Q // 2

    def tie(amax):
        b = rng.randint(1, Qh) * rng.choice((1, -1))
        a0 = ((Q + rng.choice((1, -1))) // 2) * pow(b, -1, Q) % Q
        k = rng.randint(-(amax // Q) + 1, amax // Q - 1)
        return a0 + k * Q, b

    ac, bc = [0, 1, -1, A, -A, A - 1, Q, -Q], [0, 1, -1, Qh, -Qh, Qh - 1]

    def case():
        if rng.random() < 0.3:
            return list(tie(A))
        return [_pick(rng, ac, lambda: rng.randint(-A, A), 0.1), _pick(rng, bc, lambda: rng.randint(-Qh, Qh), 0.1)]

    rows = _mix(rng, [[a, b] for a in ac for b in bc], case)
    assert all(abs(a * b) < 1 << 102 for a, b in rows)
    got = _u2f(probes.run("f64", "fmodmul_f64", 0, Q, [[_f2u(a), _f2u(b)] + [0] * 8 for a, b in rows], 8))
    for (a, b), g in zip(rows, got):
        r = _as_int(g[0], (a, b))
        assert (r - a * b) % Q == 0, (a, b, r)
        assert abs(r) <= ar.fmodmul(float(abs(a)), float(abs(b))), (a, b, r)
    xc = [0, 1, -1, A, -A, Qh, Qh + 1, -Qh, -Qh - 1]
    rows = _mix(rng, [[x] for x in xc], lambda: [rng.randint(-(A // Q) + 1, A // Q - 1) * Q + (Q + rng.choice((1, -1))) // 2
                                                 if rng.random() < 0.3 else rng.randint(-A, A)])
    got = _u2f(probes.run("f64", "fred", 1, Q, [[_f2u(x[0])] + [0] * 9 for x in rows], 8))
    for (x,), g in zip(rows, got):
        r = _as_int(g[0], x)
        assert (r - x) % Q == 0 and abs(r) <= ar.fred(float(abs(x))), (x, r)
    H = A // 2  # operands whose sums stay within the walk's largest sum

    def bcase():
        a, (b, w) = rng.randint(-H, H), (tie(H) if rng.random() < 0.3 else (rng.randint(-H, H), rng.randint(-Qh, Qh)))
        return [a, b, w]

    rows = _mix(rng, [[a, b, w] for a in (0, H, -H) for b in (0, H, -H) for w in bc], bcase)
    words = [[_f2u(v) for v in r] + [0] * 7 for r in rows]
    got = _u2f(probes.run("f64", "ct_bf", 2, Q, words, 8))
    for (a, b, w), g in zip(rows, got):
        x, y = _as_int(g[0], (a, b, w)), _as_int(g[1], (a, b, w))
        assert x + y == 2 * a and (x - y) % 2 == 0
        v = (x - y) // 2
        assert (v - b * w) % Q == 0 and abs(v) <= ar.fmodmul(float(abs(b)), float(abs(w))), (a, b, w)
    got = _u2f(probes.run("f64", "gs_bf", 3, Q, words, 8))
    for (a, b, w), g in zip(rows, got):
        x, y = _as_int(g[0], (a, b, w)), _as_int(g[1], (a, b, w))
        assert x == a + b and (y - (a - b) * w) % Q == 0
        assert abs(y) <= ar.fmodmul(float(abs(a - b)), float(abs(w))), (a, b, w)


@pytest.mark.parametrize("Q", F64_Q)
def test_f64_radix8_cores(probes, f64_arith, Q):
    """f64_r8_fwd_core / f64_r8_inv_core at the kernel's (m0, g), twiddles any centred values: integer outputs,
    congruent to the plain three-stage network, within the magnitudes Arith.fmodmul gives stage by stage."""
    ar, A = f64_arith(Q)
    rng = random.Random(Q + 3)
    Qh = Q // 2
    tw = [0, 1, -1, Qh, -Qh] + [rng.randint(-Qh, Qh) for _ in range(TAB - 5)]
    rng.shuffle(tw)
    tab = [_f2u(w) for w in tw]
    for name, op, fwd, mgs, B0 in (("f64_r8_fwd_core", 4, True, FWD_MG, A // 2), ("f64_r8_inv_core", 5, False, INV_MG, A // 8)):
        bound = float(B0)
        for _ in range(3):  # the magnitude after each stage, by the tool's lemma
            bound = bound + ar.fmodmul(bound, float(Qh)) if fwd else max(2 * bound, ar.fmodmul(2 * bound, float(Qh)))
        assert bound < 2.0 ** 53
        rows = []
        for i in range(N_RANDOM + len(mgs)):
            m, g = mgs[i % len(mgs)]
            rows.append([_pick(rng, [0, B0, -B0], lambda: rng.randint(-B0, B0), 0.2) for _ in range(8)] + [m, g])
        got = probes.run("f64", name, op, Q, [[_f2u(v) for v in r[:8]] + r[8:] for r in rows], 8, tab=tab)
        for r, g in zip(rows, _u2f(got)):
            out = [_as_int(v, r) for v in g]
            assert [v % Q for v in out] == _mod_core(r[:8], r[8], r[9], fwd, tw, Q), (name, r)
            assert max(abs(v) for v in out) <= bound, (name, r)


# ---------------------------------------------------------------- signed Montgomery leaves (blind_rotate_fast4.hip)
@pytest.mark.parametrize("Q", [2101249, 134215681])
def test_fast4_montgomery_leaves(probes, Q):
    """sredc: result 2^32 = T (mod Q), |result| <= |T| / 2^32 + Q/2 for |T| up to 2^63 - 2^58; smul on 32-bit
    operands of both signs (for |w| <= Q/2 within tools/bounds_fast4.py's smul_b); csub32; bfly_ct, bfly_gs<RED>,
    fwd4, inv4<RED>: congruent to the plain butterflies (Montgomery factor 2^-32), products within smul_b."""
    f4 = _tool("bounds_fast4")
    f4.Q, f4.Qh = Q, Q // 2
    smul_b = f4.smul_b
    rng = random.Random(Q)
    Qh, I31 = Q // 2, (1 << 31) - 1
    Rinv = pow(1 << 32, -1, Q)
    TM = (1 << 63) - (1 << 58)
    tc = [0, 1, -1, TM, -TM, TM - 1, Q << 32, -(Q << 32), 1 << 32, -(1 << 32), (1 << 32) - 1, I31 * I31, -I31 * I31]
    rows = _mix(rng, [[t] for t in tc], lambda: [rng.randint(-TM, TM) >> rng.choice((0, 0, 8, 24, 40))])
    got = probes.run("fast4", "sredc", 0, Q, [[r[0] & M64] + [0] * 7 for r in rows], 4)
    for (t,), g in zip(rows, got):
        r = _s64(g[0])
        assert ((r << 32) - t) % Q == 0 and abs(r) << 33 <= 2 * abs(t) + (Q << 32), (t, r)
    vc = [0, 1, -1, I31, -I31, Qh, -Qh, Qh + 1]
    rows = _mix(rng, [[a, w] for a in vc for w in vc],
                lambda: [_pick(rng, vc, lambda: rng.randint(-I31, I31), 0.1), _pick(rng, vc, lambda: rng.randint(-I31, I31), 0.1)
                         if rng.random() < 0.5 else rng.randint(-Qh, Qh)])
    got = probes.run("fast4", "smul", 1, Q, [[a & M64, w & M64] + [0] * 6 for a, w in rows], 4)
    for (a, w), g in zip(rows, got):
        r = _s64(g[0])
        assert ((r << 32) - a * w) % Q == 0 and abs(r) << 33 <= 2 * abs(a * w) + (Q << 32), (a, w, r)
        if abs(w) <= Qh:
            assert abs(r) <= smul_b(abs(a))
    ms = [Q, 2 * Q, 4 * Q]
    rows = _mix(rng, [[a, m] for m in ms for a in (0, 1, m - 1, m, m + 1, 2 * m - 1)],
                lambda: (lambda m: [rng.randrange(2 * m), m])(rng.choice(ms)))
    got = probes.run("fast4", "csub32", 2, Q, [r + [0] * 6 for r in rows], 4)
    assert all(g[0] == r[0] % r[1] == min(r[0], (r[0] - r[1]) & M32) for r, g in zip(rows, got))

    def wrand():
        return _pick(rng, [0, 1, -1, Qh, -Qh], lambda: rng.randint(-Qh, Qh), 0.1)

    amax = I31 - math.ceil(smul_b(I31))  # a +- smul(b, w) stays a 32-bit value
    rows = _mix(rng, [[a, b, w] for a in (0, amax, -amax) for b in (0, I31, -I31) for w in (1, -1, Qh, -Qh)],
                lambda: [rng.randint(-amax, amax), _pick(rng, [I31, -I31], lambda: rng.randint(-I31, I31), 0.1), wrand()])
    got = probes.run("fast4", "bfly_ct", 3, Q, [[v & M64 for v in r] + [0] * 5 for r in rows], 4)
    for (a, b, w), g in zip(rows, got):
        x, y = _s64(g[0]), _s64(g[1])
        assert x + y == 2 * a and (x - y) % 2 == 0
        v = (x - y) // 2
        assert ((v << 32) - b * w) % Q == 0 and abs(v) <= smul_b(abs(b)), (a, b, w)
    hmax = I31 // 2  # a +- b stay 32-bit values
    rows = _mix(rng, [[a, b, w] for a in (0, hmax, -hmax) for b in (0, hmax, -hmax) for w in (1, -1, Qh, -Qh)],
                lambda: [rng.randint(-hmax, hmax), rng.randint(-hmax, hmax), wrand()])
    words = [[v & M64 for v in r] + [0] * 5 for r in rows]
    for red in (False, True):
        got = probes.run("fast4", f"bfly_gs<RED={int(red)}>", 5 if red else 4, Q, words, 4)
        for (a, b, w), g in zip(rows, got):
            x, y = _s64(g[0]), _s64(g[1])
            assert ((y << 32) - (a - b) * w) % Q == 0 and abs(y) <= smul_b(abs(a - b)), (a, b, w)
            if red:
                assert (x - (a + b)) % Q == 0 and abs(x) <= smul_b(abs(a + b)), (a, b, w)
            else:
                assert x == a + b
    # radix-4 passes: x0..x3 with twiddles w1 (first stage), w2, w3 (second); bounds stage by stage
    fmax, imax = 1 << 30, (1 << 29) - 1

    def net_fwd(x, w1, w2, w3):
        x = list(x)
        for a, c, w in ((0, 2, w1), (1, 3, w1), (0, 1, w2), (2, 3, w3)):
            x[a], x[c] = (x[a] + x[c] * w * Rinv) % Q, (x[a] - x[c] * w * Rinv) % Q
        return x

    def net_inv(x, w1, w2, w3):
        x = list(x)
        for a, c, w in ((0, 1, w2), (2, 3, w3), (0, 2, w1), (1, 3, w1)):
            x[a], x[c] = (x[a] + x[c]) % Q, (x[a] - x[c]) * w * Rinv % Q
        return x

    b1 = fmax + smul_b(fmax)
    fb = b1 + smul_b(b1)
    assert fb < 1 << 31
    rows = _mix(rng, [[s * fmax] * 4 + [w, w, -w] for s in (1, -1) for w in (Qh, -Qh, 1)],
                lambda: [_pick(rng, [fmax, -fmax], lambda: rng.randint(-fmax, fmax), 0.1) for _ in range(4)] + [wrand() for _ in range(3)])
    got = probes.run("fast4", "fwd4", 6, Q, [[v & M64 for v in r] + [0] for r in rows], 4)
    for r, g in zip(rows, got):
        out = [_s64(v) for v in g]
        assert [v % Q for v in out] == net_fwd(r[:4], *r[4:]) and max(abs(v) for v in out) <= fb, r
    rows = _mix(rng, [[s * imax] * 4 + [w, w, -w] for s in (1, -1) for w in (Qh, -Qh, 1)],
                lambda: [_pick(rng, [imax, -imax], lambda: rng.randint(-imax, imax), 0.1) for _ in range(4)] + [wrand() for _ in range(3)])
    words = [[v & M64 for v in r] + [0] for r in rows]
    for red in (False, True):
        got = probes.run("fast4", f"inv4<RED={int(red)}>", 8 if red else 7, Q, words, 4)
        ib = max(smul_b(4 * imax), smul_b(2 * imax)) if red else 4 * imax
        for r, g in zip(rows, got):
            out = [_s64(v) for v in g]
            assert [v % Q for v in out] == net_inv(r[:4], *r[4:]) and max(abs(v) for v in out) <= ib, r


# ---------------------------------------------------------------- the keygen helpers (keygen_kernels.hip)
KG_M = [3, 1 << 14, 1 << 35, (1 << 63) + 29, (1 << 64) - 59]
KG_M_SIGNED = [3, 1 << 14, 1 << 35, (1 << 63) - 25]  # to_mod and centred compute in int64: moduli below 2^63


def test_keygen_helpers(probes, oracle):
    """addm64, subm64, mulmod_any, div128 and companion for every modulus up to 2^64 - 59; to_mod over the whole
    int64 range and centred for moduli below 2^63 (they compute in int64; the callers' moduli are below 2^58);
    draw_at against splitmix64 (include/tfhe_hip.h) and the oracle's generator."""
    rng = random.Random(9)

    def mod_rows(extra=lambda m: []):
        corners = [[a, b, m] for m in KG_M for a in (0, 1, m - 1) for b in (0, 1, m - 1)]
        return _mix(rng, corners, lambda: (lambda m: [_pick(rng, [0, 1, m - 1], lambda: rng.randrange(m), 0.1),
                                                      _pick(rng, [0, 1, m - 1], lambda: rng.randrange(m), 0.1), m])(rng.choice(KG_M)))

    rows = mod_rows()
    for name, op, ref in (("addm64", 0, lambda a, b, m: (a + b) % m), ("subm64", 1, lambda a, b, m: (a - b) % m),
                          ("mulmod_any", 4, lambda a, b, m: a * b % m)):
        got = probes.run("kg", name, op, 3, rows, 1)
        bad = [(r, g[0]) for r, g in zip(rows, got) if g[0] != ref(*r)]
        assert not bad, (name, len(bad), bad[:3])
    wc = [0, 1, M64, M64 - 1, 1 << 63]
    rows = _mix(rng, [[h, lo, m] for m in KG_M for h in wc + [m - 1, m] for lo in wc],
                lambda: [_pick(rng, wc, lambda: rng.getrandbits(64), 0.1), _pick(rng, wc, lambda: rng.getrandbits(64), 0.1),
                         rng.choice(KG_M)])
    got = probes.run("kg", "div128", 5, 3, rows, 1)
    assert all(g[0] == ((r[0] << 64 | r[1]) // r[2]) & M64 for r, g in zip(rows, got))
    rows = _mix(rng, [[v, m, 0] for m in KG_M for v in (0, 1, m - 1, m // 2)],
                lambda: (lambda m: [rng.randrange(m), m, 0])(rng.choice(KG_M)))
    got = probes.run("kg", "companion<u64>", 6, 3, rows, 1)
    assert all(g[0] == (r[0] << 64) // r[1] for r, g in zip(rows, got))
    q32 = [3, 1 << 14, 12289, 134215681, _prev_prime(1 << 30)]
    rows = _mix(rng, [[v, m, 0] for m in q32 for v in (0, 1, m - 1, m // 2)],
                lambda: (lambda m: [rng.randrange(m), m, 0])(rng.choice(q32)))
    got = probes.run("kg", "companion<u32>", 7, 3, rows, 1)
    assert all(g[0] == (r[0] << 32) // r[1] for r, g in zip(rows, got))
    I63 = 1 << 63
    rows = _mix(rng, [[v, m, 0] for m in KG_M_SIGNED for v in (-I63, -I63 + 1, -1, 0, 1, I63 - 1, m, -m, m - 1, 1 - m)],
                lambda: [rng.randint(-I63, I63 - 1) >> rng.choice((0, 0, 20, 50)), rng.choice(KG_M_SIGNED), 0])
    got = probes.run("kg", "to_mod", 2, 3, [[r[0] & M64, r[1], 0] for r in rows], 1)
    assert all(g[0] == r[0] % r[1] for r, g in zip(rows, got))
    rows = _mix(rng, [[v, m, 0] for m in KG_M_SIGNED for v in (0, 1, m // 2, m // 2 + 1, m - 1)],
                lambda: (lambda m: [rng.randrange(m), m, 0])(rng.choice(KG_M_SIGNED)))
    got = probes.run("kg", "centred", 3, 3, rows, 1)
    assert all(_s64(g[0]) == (r[0] - r[1] if r[0] > r[1] // 2 else r[0]) for r, g in zip(rows, got))

    def splitmix_draw(state, k):  # draw k (0-based) of the stream: the state after k + 1 steps, mixed
        z = (state + (k + 1) * 0x9E3779B97F4A7C15) & M64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        return z ^ (z >> 31)

    seq = oracle.Rng(1234)
    want = [int(oracle.lib().or_splitmix64(C.byref(seq))) for _ in range(64)]
    assert want == [splitmix_draw(1234, k) for k in range(64)]
    rows = _mix(rng, [[1234, k, 0] for k in range(64)] + [[s, k, 0] for s in (0, M64) for k in (0, 1, M64, M64 - 1)],
                lambda: [rng.getrandbits(64), rng.getrandbits(rng.choice((8, 32, 64))), 0])
    got = probes.run("kg", "draw_at", 8, 3, rows, 1)
    assert all(g[0] == splitmix_draw(r[0], r[1]) for r, g in zip(rows, got))
