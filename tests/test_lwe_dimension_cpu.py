"""CPU: the references of the LWE-dimension sweep (tests/test_gpu_lwe_dimension.py) agree with each
other before either meets the device, on STD128, STD192 and the logQ = 23 context.

  * The oracle composes: a blind rotation of n rounds equals one of n - k rounds over the tail slice of the key
    applied to the output of one of k rounds over the head slice (tests/lwe_dim.py), at the (n, k) pairs of the
    GPU module.  This pins the slicing and transposing helpers and rules out an oracle error that depends on n.
  * The integer model of the key switch (tests/ks_model.py) equals Oracle.mkm_switch at n = 1, 2, 7, 8, 9.

(tfhe_params_finish rejects n = 0: tests/test_capi_cpu.py.)
"""
import numpy as np
import pytest

import ks_model as km
import lwe_dim as ld
from phases import lowered_params

BASES = {"STD128": "STD128", "STD192": "STD192", "LOGQ23": ld.LOGQ23}


def test_transpose_is_an_involution():
    rs = np.random.default_rng(1)
    Q = 134215681
    acc = rs.integers(0, Q, (3, 2, 16), dtype=np.uint64)
    acc[0, 0, :3] = [0, 0, Q - 1]
    t = ld.transpose0(acc, Q)
    assert np.array_equal(t[:, 1], acc[:, 1]) and np.array_equal(t[:, 0, 0], acc[:, 0, 0])
    assert all(int(t[b, 0, 16 - k]) == (Q - int(acc[b, 0, k])) % Q for b in range(3) for k in range(1, 16))
    assert np.array_equal(ld.transpose0(t, Q), acc)


@pytest.mark.parametrize("n,k", ld.COMPOSE, ids=[f"n{n}-k{k}" for n, k in ld.COMPOSE])
@pytest.mark.parametrize("base", list(BASES))
def test_oracle_composes_over_key_slices(oracle, base, n, k):
    ops = {m: lowered_params(oracle, BASES[base], m)[1] for m in (n, k, n - k)}
    op = ops[n]
    bsk, ksk = ld.kat_edge_keys(oracle, 100 + n)(None, op)
    a, acc = ld.sweep_inputs(op, 7)
    orcs = []
    try:
        whole = oracle.Oracle(op, bsk, ksk)
        orcs.append(whole)
        for amod in sorted(a):
            (hb, ha), (tb, ta) = ld.split_rounds(n, bsk, a[amod], k)
            assert hb.size == oracle.sizes(ops[k])[0] and tb.size == oracle.sizes(ops[n - k])[0]
            head = oracle.Oracle(ops[k], hb, np.zeros(oracle.sizes(ops[k])[1], dtype=np.uint64))
            tail = oracle.Oracle(ops[n - k], tb, np.zeros(oracle.sizes(ops[n - k])[1], dtype=np.uint64))
            orcs += [head, tail]
            want = whole.eval_acc(a[amod], amod, acc)
            got = ld.compose(head.eval_acc, tail.eval_acc, ha, ta, amod, acc, int(op.Q))
            assert np.array_equal(got, want), (base, n, k, amod)
            # row 3 (a = 0) only changes form; the others must have moved
            assert np.array_equal(want[3], ld.transpose0(acc, int(op.Q))[3])
            assert not np.array_equal(want[0], ld.transpose0(acc, int(op.Q))[0])
    finally:
        for o in orcs:
            o.close()


@pytest.mark.parametrize("name,n", km.small_cases(), ids=[f"{a}-n{b}" for a, b in km.small_cases()])
def test_key_switch_model_equals_oracle_at_small_n(oracle, name, n):
    p = km.edge_params(oracle, name, n)
    assert p.n == n and km.CONTEXTS[name].get("qKS", p.qKS) == p.qKS
    ext = km.make_ext(p, 6, seed=n)
    bsk = np.zeros(oracle.sizes(p)[0], dtype=np.uint64)
    for f, fill in enumerate(km.FILLS):
        ksk = km.make_ksk(p, fill, seed=f)
        orc = oracle.Oracle(p, bsk, ksk)
        try:
            sums = [km.ks_sums(p, ksk, row) for row in ext]
            assert all(len(s) == n + 1 for s, _ in sums)
            if fill == "max":
                assert max(sums[2][0]) == p.N * p.dKS * (int(p.qKS) - 1)
            for fmod in (int(p.q), 2 * p.N, int(p.qKS), 2):
                got = np.stack([km.ks_finish(p, s, xN, fmod) for s, xN in sums])
                assert got.shape == (6, n + 1)
                assert np.array_equal(got, orc.mkm_switch(ext, fmod)), (name, n, fill, fmod)
        finally:
            orc.close()
