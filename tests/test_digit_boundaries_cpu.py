"""CPU: the references of the digit-boundary sweep (tests/test_gpu_digit_boundaries.py) agree with each
other before either meets the device, for every case of test_gpu_lwe_dimension.CASES at n = 3.

  (i)   the carry-loop model (digits.digits) equals or_signed_digit_decompose on the tiled accumulators;
  (ii)  the closed form of IDENTITY rounds (digits.identity_model) equals or_eval_acc under IDENTITY keys;
  (iii) every class of boundary value is present, the residual class exactly where the model says some value of
        the centred range leaves a residual, and the list is closed under negation;
  (iv)  every value meets every residue of the coefficient index mod 8 in each polynomial;
  (v)   where the whole list reconstructs, rows 0 .. B - 2 consist of list values after every IDENTITY round.
"""
import numpy as np
import pytest

import digits as dg
import lwe_dim as ld
from phases import lowered_params
from test_gpu_lwe_dimension import CASES

N = dg.N_ROUNDS


@pytest.fixture(scope="module")
def made(oracle):
    cache = {}

    def get(case):
        if case not in cache:
            _, op = lowered_params(oracle, CASES[case]["base"], N)
            values, calls = dg.inputs(op, seed=list(CASES).index(case))
            cache[case] = (op, values, calls)
        return cache[case]

    return get


@pytest.mark.parametrize("case", list(CASES))
def test_model_digits_equal_the_oracle(oracle, made, case):
    op, values, calls = made(case)
    acc = calls[0][3]
    got = dg.digit_words(acc, *dg.shape(op))
    want = oracle.signed_digit_decompose(op, acc)
    assert got.shape == want.shape == (ld.B, op.dG2, op.N)
    assert np.array_equal(got, want)
    assert len(np.unique(want[:-1])) >= 6  # 0, +-1 and both ends of the digit range at the least


@pytest.mark.parametrize("case", list(CASES))
def test_identity_model_equals_the_oracle(oracle, made, case):
    op, values, calls = made(case)
    assert len(calls) == len({int(op.q), 2 * op.N})
    bsk, ksk = dg.identity_keys(oracle, 1)(None, op)
    rows = bsk.reshape(N, -1)
    assert np.array_equal(rows[0], rows[N - 1]) and np.count_nonzero(rows[0]) == op.dG2
    orc = oracle.Oracle(op, bsk, ksk)
    try:
        for what, a, amod, acc in calls:
            m = dg.exponents(a, amod, op.N)
            step = 2 * op.N // amod
            assert (m[0] == op.N).all() and m.all() and (m[1] == step).all() and (m[2] == 2 * op.N - step).all()
            want = orc.eval_acc(a, amod, acc)
            got = dg.identity_model(a, amod, acc, *dg.shape(op))
            assert np.array_equal(got, want), (case, what)
            assert not np.array_equal(want, ld.transpose0(acc, int(op.Q)))
    finally:
        orc.close()


@pytest.mark.parametrize("case", list(CASES))
def test_every_class_is_present(made, case):
    op, values, _ = made(case)
    Q, logG, digitsG, thr = sh = dg.shape(op)
    vals, classes = dg.boundary_values(*sh)
    assert vals == values and len(set(vals)) == len(vals) == len(classes) and all(0 <= v < Q for v in vals)
    count = {k: sum(k in c for c in classes) for k in dg.CLASSES}
    left = [v for v in vals if dg.digits(v, *sh)[1] != 0]
    print(f"{case}: Q = {Q}, {digitsG} digits of {logG} bits, {thr} thrown: {len(vals)} values {count}, "
          f"{len(left)} leave a residual, reconstructs: {dg.reconstructs(vals, *sh)}")
    assert all(classes) and count["centre"] >= 11 and count["ripple"] and (count["window"] or digitsG == 1)
    assert (count["residual"] > 0) == dg.has_residual(*sh) == (len(left) > 0)
    if left:  # both sides of the first residual, on each sign the range reaches
        signs = {np.sign(dg.digits(v, *sh)[1]) for v in left}
        for s in signs:
            edge = min((v if v < Q >> 1 else v - Q for v in left if np.sign(dg.digits(v, *sh)[1]) == s), key=abs)
            assert (edge - int(s)) % Q in vals and dg.digits((edge - int(s)) % Q, *sh)[1] == 0
    assert all((Q - v) % Q in vals for v in vals)
    # ties: some value puts each digit below the top one (whose tie the range need not reach) at -B/2 with a carry,
    # and some ripple carries through all of them, thrown digits included
    half = -(1 << (logG - 1))
    every = [dg.digits(v, Q, logG, digitsG, 0)[0] for v in vals]
    for l in range(digitsG - 1):
        assert any(d[l] == half for d in every), (case, l)
    assert any(all(x == half for x in d[:digitsG - 1]) and d[digitsG - 1] != 0 for d in every)


@pytest.mark.parametrize("case", list(CASES))
def test_tile_reaches_every_register_slot(made, case):
    op, values, calls = made(case)
    acc = calls[0][3]
    assert acc.shape == (ld.B, 2, op.N) and int(acc.max()) < op.Q
    pos = dg.positions(acc, values)
    assert len(pos) == 2 * len(values)
    assert all(r == set(range(8)) for r in pos.values()), (case, [k for k, r in pos.items() if len(r) < 8][:4])
    assert dg.list_share(acc, values) == 1.0 and dg.list_share(acc[[4, 4]], values) < 0.5


@pytest.mark.parametrize("case", list(CASES))
def test_identity_rounds_keep_the_list(made, case):
    op, values, calls = made(case)
    sh = dg.shape(op)
    exact = dg.reconstructs(values, *sh)
    for what, a, amod, acc in calls:
        shares = [dg.list_share(s, values) for s in dg.identity_states(a, amod, acc, *sh)]
        print(f"{case}, {what}: share of list values in rows 0 .. {ld.B - 2} before each round and after the last: "
              + ", ".join(f"{s:.3f}" for s in shares) + ("" if exact else " (the list does not reconstruct)"))
        assert shares[0] == 1.0
        if exact:
            assert shares == [1.0] * (N + 1), (case, what)
