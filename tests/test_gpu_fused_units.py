"""GPU: the fused radix-4 groups of the four-wavefront kernel (blind_rotate_fast4.hip: fwd4f, inv4f<RED, MIR>) through
the test library's arithmetic probes (ops 9 .. 13 of the fast4 family, 10 words in), against the plain groups (fwd4,
inv4<RED>: ops 6 .. 8) on the same operands: equal mod Q, and every result within the magnitudes tools/bounds_fast4.py
derives for the fused schedule.  Operands: random, every sign corner, and the proven input bounds with |w| <= Q/2.
MIR = 1 is the inverse on the shared (forward) table: it takes (w1', w3', w2', n31', p21') of the mirrored forward block
and must equal the plain inverse group on (-w1', -w3', -w2').
"""
import ctypes as C
import importlib
import itertools
import math
import os
import random
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = 134215681
QH = Q // 2
M64 = (1 << 64) - 1
RINV = pow(1 << 32, -1, Q)
N_RANDOM = 3000


def _s64(v):
    return v - (1 << 64) if v >> 63 else v


def centred(v):
    v %= Q
    return v - Q if v > QH else v


@pytest.fixture(scope="module")
def f4():
    tools = os.path.join(ROOT, "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    argv, sys.argv = sys.argv, ["bounds_fast4.py"]
    try:
        mod = importlib.import_module("bounds_fast4")
    finally:
        sys.argv = argv
    assert mod.Q == Q
    return mod


@pytest.fixture(scope="module")
def probe():
    import torch
    from tfhe_amd import capi

    fn = capi.lib(capi.TEST_LIB).tfhe_test_arith_fast4
    fn.argtypes = [C.c_int, C.c_uint64, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    fn.restype = C.c_int

    def run(op, rows, expect=0):
        """rows of signed words -> the 4 signed result words of each"""
        ni = len(rows[0])
        a = np.array([[v & M64 for v in r] for r in rows], dtype=np.uint64)
        d_in = torch.from_numpy(a.view(np.int64).ravel().copy()).cuda()
        out = torch.zeros(len(rows) * 4, dtype=torch.int64, device="cuda")
        rc = fn(op, Q, len(rows), d_in.data_ptr(), len(rows) * ni, None, 0, out.data_ptr(), len(rows) * 4)
        assert rc == expect, (op, rc)
        return out.cpu().numpy().reshape(len(rows), 4).tolist()

    return run


def _rows(rng, bound):
    """[x0..x3, w1, w2, w3]: every sign corner at the bound (x) and at Q/2 (w), the bound with random twiddles, random"""
    rows = [[sx[k] * bound for k in range(4)] + [sw[k] * QH for k in range(3)]
            for sx in itertools.product((1, -1), repeat=4) for sw in itertools.product((1, -1), repeat=3)]
    rows += [[s * bound for s in sx] + [rng.randint(-QH, QH) for _ in range(3)] for sx in itertools.product((1, -1), repeat=4)]
    rows += [[0, 0, 0, 0, 1, -1, QH], [1, -1, 1, -1, 0, 0, 0], [bound, 0, -bound, 0, 1, 1, 1]]
    rows += [[rng.randint(-bound, bound) for _ in range(4)] + [rng.randint(-QH, QH) for _ in range(3)] for _ in range(N_RANDOM)]
    return rows


def _prod(a, b):
    """the centred Montgomery form of the product of two Montgomery forms"""
    return centred(a * b * RINV)


def test_fused_forward_group(probe, f4):
    B = f4.check_fused(f4.FU_ALL, quiet=True)
    bound = math.ceil(B["F"])  # no forward pass sees a larger input than the transform's proven output
    rng = random.Random(9)
    rows = _rows(rng, bound)
    plain = probe(6, [r + [0] for r in rows])
    fused = probe(9, [r + [_prod(r[5], r[4]), _prod(-r[6], r[4]), 0] for r in rows])
    lim = bound + f4.smul_b(bound) + f4.sred2_b(bound, bound)
    assert lim < 1 << 31
    for r, p, g in zip(rows, plain, fused):
        assert [v % Q for v in g] == [v % Q for v in p], r
        assert max(abs(v) for v in g) <= lim, r
        # y0 + y1 = 2 a and y2 + y3 = 2 b with a + b = 2 x0: the first stage is the plain one
        assert g[0] + g[1] + g[2] + g[3] == 4 * r[0], r


@pytest.mark.parametrize("red", [False, True])
@pytest.mark.parametrize("mir", [False, True])
def test_fused_inverse_group(probe, f4, red, mir):
    B = f4.check_fused(f4.FU_ALL, quiet=True)
    bound = math.ceil(B["out"])  # no inverse pass sees a larger input than the transform's proven output
    assert 4 * bound < 1 << 31
    rng = random.Random(10 + 2 * red + mir)
    rows = _rows(rng, bound)
    if mir:  # r[4:7] = the mirrored forward block (w1', w2', w3'); the inverse's twiddles are (-w1', -w3', -w2')
        plain = probe(8 if red else 7, [r[:4] + [-r[4], -r[6], -r[5], 0] for r in rows])
        fused = probe(13 if red else 12, [r[:4] + [r[4], r[6], r[5], _prod(-r[6], r[4]), _prod(r[5], r[4]), 0] for r in rows])
    else:
        plain = probe(8 if red else 7, [r + [0] for r in rows])
        fused = probe(11 if red else 10, [r + [_prod(r[4], r[5]), _prod(-r[4], r[6]), 0] for r in rows])
    y0 = f4.smul_b(4 * bound) if red else 4 * bound
    lims = [y0, f4.sred2_b(2 * bound, 2 * bound), f4.smul_b(4 * bound), f4.sred2_b(2 * bound, 2 * bound)]
    for r, p, g in zip(rows, plain, fused):
        assert [v % Q for v in g] == [v % Q for v in p], r
        assert all(abs(v) <= b for v, b in zip(g, lims)), r
        if not red:
            assert g[0] == sum(r[:4]), r


def test_fused_ops_check_their_word_count(probe):
    """the fused ops take 10 words per case, the plain ones 8; one past the last op is rejected"""
    assert probe(9, [[0] * 10]) == [[0, 0, 0, 0]]
    probe(9, [[0] * 8], expect=-1)
    probe(6, [[0] * 10], expect=-1)
    probe(14, [[0] * 10], expect=-1)
