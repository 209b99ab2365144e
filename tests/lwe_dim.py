"""The sweep of the LWE dimension n: what tests/test_lwe_dimension_cpu.py and
tests/test_gpu_lwe_dimension.py share -- the values of n, the keys, the blind-rotation inputs and the composition
of two blind rotations over the slices of one key.

n is the number of rounds of the blind rotation and the number of columns of the key switch.  The BSK is
[n][2][dG2][2][N], so the rows of rounds 0 .. k-1 and k .. n-1 are contiguous slices of one key array, and a
blind rotation of n rounds equals one of n - k rounds (the tail slice, a[:, k:]) applied to the output of one of
k rounds (the head slice, a[:, :k]).  EvalAcc returns the first polynomial transposed (X -> X^-1, poly.cpp:762-770),
an involution on polynomials mod X^N + 1, so the intermediate output is transposed back before it goes in again.
"""
import numpy as np

# every class of n mod 8 with both parities, the first round also the last (1), and the second period of the
# eight-round reduction of fast4's folded accumulator
N_SWEEP = (1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17)
# forms without an eight-round period, where a family's items would take much longer than 10 s: n = 1, both
# parities, two n past 8
N_THIN = (1, 2, 3, 4, 5, 9, 16, 17)
# (n, k): a whole reduction period then a partial one and the reverse; one round then a period; a period then one
# round; one round twice
COMPOSE = ((17, 8), (17, 9), (9, 1), (9, 8), (2, 1))
B = 5  # ragged for two ciphertexts per wavefront and for four per workgroup; inside split4 and the duo limits

ARB12 = ("STD128", True, 12, 0, 0, 1)        # one 27-bit digit
LOGQ23 = ("STD128", False, 23, 0, 0, 1)      # two 18-bit digits
CHES18 = ("STD128", True, 12, 0, 1 << 18, 0)  # three


def kat_edge_keys(oracle, seed):
    """keys(cp, op) -> (bsk, ksk): seeded splitmix64 words mod Q and mod qKS (the KAT recipe, or_kat_keys), the
    first four BSK rows at 0, Q - 1, Q/2 and Q/2 + 1; the KSK is random and not zero."""

    def keys(cp, op):
        bsk, ksk = oracle.kat_keys(op, oracle.Rng(seed))
        Q = int(op.Q)
        assert bsk.size >= 4 * op.N
        bsk[: 4 * op.N] = np.array([0, Q - 1, Q >> 1, (Q >> 1) + 1], dtype=np.uint64).repeat(op.N)
        assert ksk.any() and int(bsk.max()) < Q and int(ksk.max()) < int(op.qKS)
        return bsk, ksk

    return keys


def sweep_inputs(op, seed):
    """({a-modulus: a[B][n]}, acc[B][2][N]): test_gpu_modulus_edges._inputs at B = 5 (edge words, the Q/2, Q/2 + 1
    alternation, random rows); a random except row 3 all 0 and row 4 all a-modulus - 1."""
    from test_gpu_modulus_edges import _inputs

    a, acc = _inputs(op, seed, B)
    for amod, x in a.items():
        x[3], x[4] = 0, amod - 1
    return a, acc


def transpose0(acc, Q):
    """acc[B][2][N] with the first polynomial transposed: out[0] = x[0], out[N - k] = -x[k] mod Q."""
    out = np.array(acc, dtype=np.uint64, copy=True)
    x = out[:, 0].copy()
    out[:, 0, 1:] = (np.uint64(Q) - x[:, :0:-1]) % np.uint64(Q)
    return out


def split_rounds(n, bsk, a, k):
    """((head BSK, a[:, :k]), (tail BSK, a[:, k:])): the key rows and a-words of rounds 0 .. k-1 and k .. n-1."""
    assert 0 < k < n and bsk.size % n == 0 and a.shape[1] == n
    rows = np.asarray(bsk).reshape(n, -1)
    return ((np.ascontiguousarray(rows[:k]).ravel(), np.ascontiguousarray(a[:, :k])),
            (np.ascontiguousarray(rows[k:]).ravel(), np.ascontiguousarray(a[:, k:])))


def compose(run_head, run_tail, a_head, a_tail, amod, acc, Q):
    """The tail's rounds applied to the head's output: run_*(a, amod, acc) -> EvalAcc's output."""
    mid = run_head(a_head, amod, acc)
    return run_tail(a_tail, amod, transpose0(mid, Q))
