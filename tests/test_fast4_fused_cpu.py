"""CPU-only: an integer model of the four-wavefront kernel's transforms with fused radix-4 groups
(blind_rotate_fast4.hip: fwd4f / inv4f, template parameter FU), on Python ints.

N = 1024, the STD128 Q, the kernel's pass order (forward over the index-bit pairs (b9 b8) .. (b1 b0), inverse back),
signed Montgomery reduction exactly as sredc computes it.  Checked against a plain negacyclic NTT (itself checked
against the defining sum), for random inputs and for all-maximal inputs of both signs at the magnitudes
tools/bounds_fast4.py proves; every intermediate must be a 32-bit value and every output within the tool's bound.
Also the table identities the shared twiddle table of passes 1-3 rests on: p21 = w2 w1, n31 = -w3 w1, and the
inverse's block c = the forward's block m - 1 - c negated with w2 and w3 swapped.
"""
import importlib
import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, LOGN, Q = 1024, 10, 134215681
QH = Q // 2
M32 = (1 << 32) - 1
QINV = pow(Q, -1, 1 << 32)
R = (1 << 32) % Q
LIM = 1 << 31


def _tool():
    """tools/bounds_fast4.py as a module (it reads sys.argv and runs its unfused checks on import)"""
    tools = os.path.join(ROOT, "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    argv, sys.argv = sys.argv, ["bounds_fast4.py"]
    try:
        return importlib.import_module("bounds_fast4")
    finally:
        sys.argv = argv


def _s32(v):
    v &= M32
    return v - (1 << 32) if v >> 31 else v


def i32(v):
    assert -LIM <= v < LIM, f"{v} is no 32-bit value"
    return v


def sredc(T):
    assert abs(T) < (1 << 63) - (1 << 58)
    m = _s32((T & M32) * QINV)
    t = m * -Q + T
    assert t & M32 == 0
    return i32(t >> 32)


def smul(a, w):
    return sredc(i32(a) * w)


def centred(v):
    v %= Q
    return v - Q if v > QH else v


def mont(v):
    return centred(v * R)


def bitrev(k, bits=LOGN):
    return int(format(k, f"0{bits}b")[::-1], 2)


def _root():
    for g in range(2, 100):
        x = pow(g, (Q - 1) // (2 * N), Q)
        if pow(x, N, Q) == Q - 1:
            return x
    raise AssertionError("no primitive 2N-th root")


PSI_ROOT = _root()
PSI = [pow(PSI_ROOT, bitrev(k), Q) for k in range(N)]                 # host_math.cpp: psi_br
IPSI = [pow(pow(PSI_ROOT, Q - 2, Q), bitrev(k), Q) for k in range(N)]  # ipsi_br


def block(t, m, c):
    """{w1, w2, w3, p = w2 w1, n = -w3 w1} of block c of a pass with m blocks, centred Montgomery (k_pack_tables4)"""
    w1, w2, w3 = t[m + c], t[2 * m + 2 * c], t[2 * m + 2 * c + 1]
    return [mont(w1), mont(w2), mont(w3), mont(w2 * w1), mont(-w3 * w1)]


FWD_T = {m: [block(PSI, m, c) for c in range(m)] for m in (1, 4, 16, 64, 256)}
INV_T = {m: [block(IPSI, m, c) for c in range(m)] for m in (1, 4, 16, 64, 256)}


# ---- the kernel's groups ----
def fwd4f(x, w1, w2, w3, p21, n31):
    t = smul(x[2], w1)
    a, b = i32(x[0] + t), i32(x[0] - t)
    c = sredc(i32(x[1]) * w2 + i32(x[3]) * p21)
    d = sredc(x[1] * w3 + x[3] * n31)
    return [i32(a + c), i32(a - c), i32(b + d), i32(b - d)]


def inv4f(x, w1, wa, wb, pa, pb, red, mir):
    e = i32(x[1] - x[0]) if mir else i32(x[0] - x[1])
    f = i32(x[3] - x[2]) if mir else i32(x[2] - x[3])
    s0, s2 = i32(x[0] + x[1]), i32(x[2] + x[3])
    y1 = sredc(e * wa + f * wb)
    y3 = sredc(e * pa + f * pb)
    y2 = smul(i32(s2 - s0) if mir else i32(s0 - s2), w1)
    y0 = smul(i32(s0 + s2), mont(1)) if red else i32(s0 + s2)
    return [y0, y1, y2, y3]


def fwd_fused(a, small=False):
    """ntt_fwd with every pass fused; small: pass 0 on digits from the lookup tables (exact products d w mod Q)"""
    x = list(a)
    for p in range(5):
        hi, lo, m = 1 << (9 - 2 * p), 1 << (8 - 2 * p), 4 ** p
        for i in range(N):
            if i & (hi | lo):
                continue
            idx = (i, i | lo, i | hi, i | hi | lo)
            v = [x[k] for k in idx]
            if p == 0 and small:
                w1, w2, w3 = PSI[1], PSI[2], PSI[3]
                t1 = centred(v[2] * w1)
                u = centred(v[1] * w2) + centred(v[3] * w2 * w1)
                d = centred(v[1] * w3) - centred(v[3] * w3 * w1)
                y = [v[0] + t1 + u, v[0] + t1 - u, v[0] - t1 + d, v[0] - t1 - d]
            else:
                y = fwd4f(v, *FWD_T[m][i >> (10 - 2 * p)])
            for k, r in zip(idx, y):
                x[k] = i32(r)
    return x


RED_PASS = (False, True, False, True, False)  # inverse passes L5, L4, L3, L2, L1 (tools/bounds_fast4.py RED)


def inv_fused(a):
    """ntt_inv with every pass fused: L5 and L1 on the inverse's own twiddles, L4 - L2 on the shared (forward) table's
    block m - 1 - c with the differences taken the other way round"""
    x = list(a)
    for p in range(5):
        lo, hi, m = 1 << (2 * p), 1 << (2 * p + 1), 4 ** (4 - p)
        for i in range(N):
            if i & (hi | lo):
                continue
            idx = (i, i | lo, i | hi, i | hi | lo)
            v = [x[k] for k in idx]
            c = i >> (2 * p + 2)
            if p in (1, 2, 3):
                w1, w2, w3, p21, n31 = FWD_T[m][m - 1 - c]
                y = inv4f(v, w1, w3, w2, n31, p21, RED_PASS[p], True)
            else:
                w1, w2, w3, p12, n13 = INV_T[m][c]
                y = inv4f(v, w1, w2, w3, p12, n13, RED_PASS[p], False)
            for k, r in zip(idx, y):
                x[k] = r
    return x


# ---- the plain transforms ----
def ntt_plain(a):
    x, t, m = [v % Q for v in a], N, 1
    while m < N:
        t //= 2
        for i in range(m):
            w = PSI[m + i]
            for j in range(2 * i * t, 2 * i * t + t):
                u, v = x[j], x[j + t] * w % Q
                x[j], x[j + t] = (u + v) % Q, (u - v) % Q
        m *= 2
    return x


def intt_plain_times_n(a):
    x, t, m = [v % Q for v in a], 1, N
    while m > 1:
        h = m // 2
        for i in range(h):
            w = IPSI[h + i]
            for j in range(2 * i * t, 2 * i * t + t):
                u, v = x[j], x[j + t]
                x[j], x[j + t] = (u + v) % Q, (u - v) * w % Q
        t, m = 2 * t, h
    return x


@pytest.fixture(scope="module")
def bounds():
    f4 = _tool()
    assert f4.Q == Q
    return f4, f4.check_fused(f4.FU_ALL, quiet=True)


def test_plain_ntt_is_the_negacyclic_transform():
    rng = random.Random(1)
    a = [rng.randrange(Q) for _ in range(N)]
    X = ntt_plain(a)
    for k in (0, 1, 2, 511, 512, 777, 1023):  # X[bitrev(k)] = sum_j a_j psi^((2k + 1) j)
        assert X[bitrev(k)] == sum(v * pow(PSI_ROOT, (2 * k + 1) * j, Q) for j, v in enumerate(a)) % Q
    assert intt_plain_times_n(X) == [v * N % Q for v in a]


def test_table_identities():
    for m in (1, 4, 16, 64, 256):
        for c in range(m):
            for t, T in ((PSI, FWD_T), (IPSI, INV_T)):
                w1, w2, w3 = t[m + c], t[2 * m + 2 * c], t[2 * m + 2 * c + 1]
                b = T[m][c]
                assert all(abs(v) <= QH for v in b)
                assert [v * pow(R, -1, Q) % Q for v in b] == [w1, w2, w3, w2 * w1 % Q, -w3 * w1 % Q]
    # the mirrored, negated forward table is the inverse table, for every block of passes 1-3 (and every other pass)
    for m in (4, 16, 64, 1, 256):
        for c in range(m):
            assert IPSI[m + c] == (Q - PSI[m + (m - 1 - c)]) % Q
            fw1, fw2, fw3, fp21, fn31 = FWD_T[m][m - 1 - c]
            iw1, iw2, iw3, ip12, in13 = INV_T[m][c]
            assert (iw1, iw2, iw3) == (-fw1, -fw3, -fw2)  # w2 and w3 swap roles
            assert (ip12, in13) == (-fn31, -fp21)          # p12 = w1 w2, n13 = -w1 w3 of the inverse


def _fwd_inputs(rng, bound, lo=None):
    lo = -bound if lo is None else lo
    yield [rng.randint(lo, bound) for _ in range(N)]
    yield [bound] * N
    yield [lo] * N
    yield [bound if rng.random() < 0.5 else lo for _ in range(N)]


def test_fused_forward_matches_plain(bounds):
    f4, B = bounds
    rng = random.Random(2)
    for small, inputs in ((False, _fwd_inputs(rng, QH + 1)), (True, _fwd_inputs(rng, 63, -64))):
        for a in inputs:
            X = fwd_fused(a, small)
            assert [v % Q for v in X] == ntt_plain(a)
            assert max(abs(v) for v in X) <= B["F"]


def test_fused_inverse_matches_plain(bounds):
    f4, B = bounds
    rng = random.Random(3)
    S = int(B["S"])
    for a in _fwd_inputs(rng, S):
        x = inv_fused(a)
        assert [v % Q for v in x] == intt_plain_times_n(a)
        assert max(abs(v) for v in x) <= B["out"] < 3 * Q


def test_fused_round_trip():
    """inverse(forward(a)) = N a (the kernel folds N^-1 into the keys), the forward's outputs reduced in between as
    the external product reduces them"""
    rng = random.Random(4)
    a = [rng.randint(-QH, QH) for _ in range(N)]
    x = inv_fused([centred(v) for v in fwd_fused(a)])
    assert [v % Q for v in x] == [v * N % Q for v in a]


def test_bounds_tool_fused_run_passes(bounds, capsys):
    f4, _ = bounds
    full = f4.check_fused(f4.FU_ALL)
    pair = f4.check_fused(f4.FU_PAIR)
    assert "OK" in capsys.readouterr().out
    for b in (full, pair):
        assert b["F"] < LIM and b["out"] < 3 * Q
    # the fused second-stage term: (|x1| + |x3|) (Q/2) / 2^32 + Q/2
    assert f4.sred2_b(5 * Q, 3 * Q) == 8 * Q * QH / 2 ** 32 + Q / 2


def test_shared_table_reads_are_conflict_free(capsys):
    """tools/lds_tables4.py: the shared table's ds_read_b128 / ds_read_b32 of passes 1-3, forward and mirrored"""
    _tool()  # puts tools/ on sys.path
    importlib.import_module("lds_tables4").check()
    assert "420 of 672 words" in capsys.readouterr().out
