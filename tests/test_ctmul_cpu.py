"""CPU: the model of the product of two encrypted tensors (tests/ctmul_model.py) that the GPU tests compare against
and the host-only calls of the library -- tfhe_ct_matmul_info, tfhe_ct_matmul_eval_plain, tfhe_amd.product_tables
-- which need no GPU: the helper tables' products, classes and entries, the pair form on clear values against the
model for every flag combination, every argument error with its message, the bootstrap counts per class pair, and
decryption through the oracle."""
import ctypes as C
import itertools

import numpy as np
import pytest

import ctmul_model

BETA = 128
QP = [(1024, 4), (2048, 8), (2048, 16), (4096, 32)]


def _signed(p):
    return range(-(p // 2), p // 2 + 1)


@pytest.mark.parametrize("q,p", QP)
def test_product_tables_multiply(q, p):
    """Every admitted pair of signed messages through the look-up the engine does, table[Delta s + beta]: the default
    form gives x y Delta exactly for |x| + |y| <= p/2, the negacyclic form within 2 for |x| + |y| < p/4; and a
    look-up anywhere in [Delta s - Delta/2, Delta s + Delta/2) reads the same step (the helper centres on beta)."""
    import tfhe_amd

    tfhe_amd.build()
    delta = q // p
    for neg in (False, True):
        t = tfhe_amd.product_tables(q, p, negacyclic=neg)
        assert t.shape == (2, q) and t.dtype == np.uint64 and np.array_equal(t[0], t[1])
        look = lambda s, e=0: int(t[0][(delta * s + e + BETA) % q])
        seen = set()
        for x, y in itertools.product(_signed(p), repeat=2):
            if (abs(x) + abs(y) >= p // 4) if neg else (abs(x) + abs(y) > p // 2):
                continue
            got = (look(x + y) - look(x - y)) % q
            err = (got - x * y * delta + q // 2) % q - q // 2
            assert abs(err) <= (2 if neg else 0), (q, p, neg, x, y, got)
            for e in (-(delta // 2), delta // 2 - 1):
                assert look(x + y, e) == look(x + y) and look(x - y, e) == look(x - y), (q, p, neg, x, y, e)
            seen.add(x * y % p)
        assert len(seen) > 1 or (neg and p < 16)  # p = 4, 8 negacyclic admit only products with a zero factor


@pytest.mark.parametrize("q,p", QP)
def test_product_tables_classes_and_entries(q, p):
    import tfhe_amd

    tfhe_amd.build()
    arb, neg = tfhe_amd.product_tables(q, p), tfhe_amd.product_tables(q, p, negacyclic=True)
    assert list(tfhe_amd.lut_classes(arb, q)) == [2, 2] and list(tfhe_amd.lut_classes(neg, q)) == [0, 0]
    assert int(arb.max()) < q and int(neg.max()) < q
    # the staircases as documented, before the rotation by beta - Delta/2
    delta = q // p
    back = lambda t: np.roll(t[0].astype(np.int64), -(BETA - delta // 2))
    s = np.array([j if j < p // 2 else j - p for j in range(p)])
    assert np.array_equal(back(arb), np.repeat(delta * (s * s // 4 % p), delta))
    h = np.arange(p // 2)
    half = np.where(h < p // 4, delta * (h * h // 4 % p), (q - delta * ((h - p // 2) ** 2 // 4 % p)) % q)
    half[half == 0] = 1
    assert np.array_equal(back(neg), np.repeat(np.concatenate([half, q - half]), delta))
    for bad in ((768, 4), (1024, 3), (1024, 2), (1024, 1024)):
        with pytest.raises(ValueError):
            tfhe_amd.product_tables(*bad)


@pytest.mark.parametrize("q", [8, 1 << 10, 1 << 12])
def test_eval_plain_equals_the_model_on_random_tables(q):
    import tfhe_amd

    tfhe_amd.build()
    rs = np.random.default_rng(91 + q)
    for ((R, K, Cn), n), (tr, sh) in itertools.product(ctmul_model.SHAPES, ctmul_model.FLAGS):
        luts = rs.integers(0, q, (2, q), dtype=np.uint64)
        x = rs.integers(0, q, (n, R, K), dtype=np.uint64)
        y = rs.integers(0, q, ctmul_model.y_shape(R, K, Cn, n, tr, sh), dtype=np.uint64)
        bx, by = x.copy(), y.copy()
        d = tfhe_amd.CtMatMul(R, K, Cn, tr, sh)
        assert d.as_dict() == dict(rows=R, inner=K, cols=Cn, y_transposed=int(tr), y_shared=int(sh))
        got = tfhe_amd.ct_matmul_eval_plain(d, x, y, luts, q)
        assert got.shape == (n, R, Cn) and np.array_equal(got, ctmul_model.plain(x, y, luts, q, tr, sh)), (R, K, Cn, n, tr, sh)
        assert np.array_equal(x, bx) and np.array_equal(y, by)


def test_eval_plain_with_the_product_tables_is_the_matrix_product():
    """Clear values x = Delta X + beta + e, y = Delta Y + e' with |e| + |e'| < Delta/2: x + y and x - y are then what
    the engine looks up for phases Delta (X +- Y) + noise, and the default tables give Delta (X Y mod p) exactly, for
    signed messages and a sum over k."""
    import tfhe_amd

    tfhe_amd.build()
    q, p = 2048, 16
    delta = q // p
    rs = np.random.default_rng(92)
    X, Y = rs.integers(-4, 5, (3, 4, 5)), rs.integers(-4, 5, (3, 5, 2))  # |x| + |y| <= 8 = p/2
    x = (delta * X + BETA + rs.integers(-30, 30, X.shape)) % q
    y = (delta * Y + rs.integers(-30, 30, Y.shape)) % q
    got = tfhe_amd.ct_matmul_eval_plain(tfhe_amd.CtMatMul(4, 5, 2), x.astype(np.uint64), y.astype(np.uint64),
                                        tfhe_amd.product_tables(q, p), q)
    assert np.array_equal(got.astype(np.int64), delta * (np.matmul(X, Y) % p) % q)


def test_argument_errors_by_message():
    import tfhe_amd

    tfhe_amd.build()
    L = tfhe_amd.lib()
    q = 16
    luts = np.zeros((2, q), dtype=np.uint64)
    x, y, out = (np.zeros(64, dtype=np.uint64) for _ in range(3))
    P = lambda a: a.ctypes.data
    good = tfhe_amd.CtMatMul(2, 3, 2)
    D = C.byref
    plain, info = L.tfhe_ct_matmul_eval_plain, L.tfhe_ct_matmul_info
    assert plain(D(good), 2, q, P(luts), P(x), P(y), P(out)) == 0
    big = luts.copy()
    big[1, 5] = q
    cases = [((None, 2, q, P(luts), P(x), P(y), P(out)), b"null descriptor"),
             ((D(good), 2, q, None, P(x), P(y), P(out)), b"null luts"),
             ((D(good), 2, q, P(luts), None, P(y), P(out)), b"null x"),
             ((D(good), 2, q, P(luts), P(x), None, P(out)), b"null y"),
             ((D(good), 2, q, P(luts), P(x), P(y), None), b"null out"),
             ((D(good), 0, q, P(luts), P(x), P(y), P(out)), b"instances is 0"),
             ((D(tfhe_amd.CtMatMul(0, 3, 2)), 2, q, P(luts), P(x), P(y), P(out)), b"rows is 0"),
             ((D(tfhe_amd.CtMatMul(2, 0, 2)), 2, q, P(luts), P(x), P(y), P(out)), b"inner is 0"),
             ((D(tfhe_amd.CtMatMul(2, 3, 0)), 2, q, P(luts), P(x), P(y), P(out)), b"cols is 0"),
             ((D(tfhe_amd.CtMatMul(2, 3, 2, 2, 0)), 2, q, P(luts), P(x), P(y), P(out)), b"y_transposed must be 0 or 1"),
             ((D(tfhe_amd.CtMatMul(2, 3, 2, 0, 7)), 2, q, P(luts), P(x), P(y), P(out)), b"y_shared must be 0 or 1"),
             ((D(good), 2, 4, P(luts), P(x), P(y), P(out)), b"q must be a power of two >= 8"),
             ((D(good), 2, 24, P(luts), P(x), P(y), P(out)), b"q must be a power of two >= 8"),
             ((D(good), 2 ** 62, q, P(luts), P(x), P(y), P(out)), b"sizes overflow"),
             ((D(tfhe_amd.CtMatMul(2 ** 31, 2 ** 31, 2 ** 31)), 2, q, P(luts), P(x), P(y), P(out)), b"sizes overflow"),
             ((D(good), 2, q, P(big), P(x), P(y), P(out)), b"luts[1][5] is not below q")]
    for args, word in cases:
        assert plain(*args) == 1, word
        assert b"CtMatMulEvalPlain: " in L.tfhe_last_error() and word in L.tfhe_last_error(), (word, L.tfhe_last_error())
    n, b = C.c_size_t(), C.c_uint64()
    for args, word in cases[:2] + cases[5:15]:
        a = args[:4] + (D(n), D(b))
        assert info(*a) == 1, word
        assert b"CtMatMulInfo: " in L.tfhe_last_error() and word in L.tfhe_last_error(), (word, L.tfhe_last_error())
    assert info(D(good), 2, q, P(luts), None, None) == 0  # null result pointers are allowed
    with pytest.raises(ValueError):
        tfhe_amd.ct_matmul_eval_plain(good, np.zeros((2, 2, 4)), np.zeros((2, 3, 2)), luts, q)
    with pytest.raises(ValueError) as e:
        tfhe_amd.ct_matmul_eval_plain(good, np.zeros((2, 2, 3)), np.zeros((3, 2)), luts, q)  # not shared
    assert "(2, 3, 2)" in str(e.value)
    with pytest.raises(ValueError):
        tfhe_amd.ct_matmul_eval_plain(good, np.zeros((2, 2, 3)), np.zeros((2, 3, 2)), luts[:1], q)


@pytest.mark.parametrize("c0,c1,per", [(0, 0, 2), (0, 2, 3), (1, 2, 4)])
def test_info_counts_bootstraps_by_class_pair(c0, c1, per):
    import tfhe_amd

    tfhe_amd.build()
    q = 1024
    luts = ctmul_model.pair_luts(q, c0, c1)
    assert list(tfhe_amd.lut_classes(luts, q)) == [c0, c1]
    for ((R, K, Cn), n), (tr, sh) in itertools.product(ctmul_model.SHAPES, ctmul_model.FLAGS):
        P = n * R * K * Cn
        assert tfhe_amd.ct_matmul_info(tfhe_amd.CtMatMul(R, K, Cn, tr, sh), n, luts, q) == (P, per * P)


@pytest.mark.slow
def test_decrypts_to_the_clear_product_on_the_oracle(oracle):
    """ctmul_model.DECRYPT_CASES on the oracle alone, for each of 8 key seeds: keygen, encrypt, the model with the
    oracle's EvalFunc under tfhe_amd.product_tables, decrypt -- every output is X Y mod p."""
    import tfhe_amd

    tfhe_amd.build()
    op = oracle.params_from_logq(*ctmul_model.DECRYPT_LOGQ)
    q, w = op.q, op.n + 1
    assert q == 2048
    seen = {k: set() for k in ctmul_model.DECRYPT_CASES}
    for seed in ctmul_model.DECRYPT_SEEDS:
        rng = oracle.Rng(seed)
        sk, bsk, ksk = oracle.keygen(op, rng)
        orc = oracle.Oracle(op, bsk, ksk)
        del bsk, ksk
        try:
            for name, c in ctmul_model.DECRYPT_CASES.items():
                p = c["p"]
                X, Y, want = ctmul_model.decrypt_msgs(name, seed)
                x = np.stack([oracle.encrypt(op, rng, sk, int(m), p, q) for m in X.ravel()]).reshape(X.shape + (w,))
                y = np.stack([oracle.encrypt(op, rng, sk, int(m), p, q) for m in Y.ravel()]).reshape(Y.shape + (w,))
                luts = tfhe_amd.product_tables(q, p, c["negacyclic"])
                out = ctmul_model.ct_matmul(x, y, luts, q, orc.eval_func)
                got = [oracle.decrypt(op, sk, row, p, q) for row in out.reshape(-1, w)]
                assert got == [int(v) for v in want.ravel()], (name, seed)
                seen[name].update(got)
        finally:
            orc.close()
    assert all(len(v) > 1 for v in seen.values()), ("the cases must not be constant", seen)
