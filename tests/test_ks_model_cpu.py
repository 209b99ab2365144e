"""CPU: the integer model of the key switch (tests/ks_model.py) equals the oracle's (Oracle.mkm_switch) on every
edge context of tests/test_gpu_keyswitch_edges.py -- every KSK fill, every output modulus, the four edge rows and
two random ones -- so the GPU module's two references agree with each other before either meets the device.  The
reference itself pins the oracle's key switch on two cases only (std128_mkm_* in tests/golden/ref_vectors.json)."""
import time

import numpy as np
import pytest

import ks_model as km


def fmods(p):
    return (int(p.q), 2 * p.N, int(p.qKS), 2)


def test_round_and_preimage():
    assert km.round_qQ(0, 1 << 14, 134215681) == 0
    assert km.round_qQ(134215680, 1 << 14, 134215681) == 0  # rounds up to qKS, reduced
    for q, Q in ((1 << 14, 134215681), ((1 << 16) + 1, 134215681), (1 << 37, (1 << 54) - 77823)):
        for t in (0, 1, 127, 128, q - 1):
            assert km.round_qQ(km.preimage(t, q, Q), q, Q) == t


def test_dks_matches_the_sets(oracle):
    for name in ("STD128", "STD192", "STD128Q", "STD192Q", "STD256Q", "TOY"):
        p = oracle.params_from_set(name)
        assert km.dks_for(p.qKS, p.baseKS) == p.dKS, name
    p = oracle.params_from_logq(*km.ARB12)
    assert km.dks_for(p.qKS, p.baseKS) == p.dKS == 7


@pytest.mark.parametrize("name,n", km.cases(), ids=[f"{a}-n{b}" for a, b in km.cases()])
def test_model_equals_oracle(oracle, name, n):
    p = km.edge_params(oracle, name, n)
    ext = km.make_ext(p, 6, seed=n)
    bsk = np.zeros(p.n * 2 * p.dG2 * 2 * p.N, dtype=np.uint64)
    t_or = t_mod = 0.0
    for f, fill in enumerate(km.FILLS):
        ksk = km.make_ksk(p, fill, seed=f)
        orc = oracle.Oracle(p, bsk, ksk)
        try:
            sums = [km.ks_sums(p, ksk, row) for row in ext]
            if fill == "max":  # the digit row at its largest selects N dKS maximal entries: the sums' bound
                assert max(sums[2][0]) == p.N * p.dKS * (int(p.qKS) - 1)
            for fmod in fmods(p):
                t0 = time.perf_counter()
                want = orc.mkm_switch(ext, fmod)
                t1 = time.perf_counter()
                got = np.stack([km.ks_finish(p, s, xN, fmod) for s, xN in sums])
                t_or, t_mod = t_or + t1 - t0, t_mod + time.perf_counter() - t1
                assert np.array_equal(got, want), (name, n, fill, fmod)
        finally:
            orc.close()
    print(f"{name} n = {n}: qKS = {p.qKS}, baseKS = {p.baseKS}, dKS = {p.dKS}: model == oracle on "
          f"{len(km.FILLS)} fills x {len(fmods(p))} moduli x {len(ext)} rows (oracle {t_or:.2f} s)")
