"""The product of two encrypted tensors in numpy (no GPU): the pair form, parameterised by the function
that evaluates a table, so that one function serves clear integers, the host-array EvalFunc and the oracle.  What
tfhe_ct_matmul_eval_plain and tfhe_eval_ct_matmul* are compared against.

    out[i][r][c] = sum_k EvalFunc(x[i][r][k] + y[i][k][c] mod q, luts[0]) - EvalFunc(x[i][r][k] - y[i][k][c] mod q, luts[1])

All the sums go through eval_func in one call, then all the differences, in the order o = (i R + r) C + c, k
innermost."""
import numpy as np

from helpers import cube_lut

# (rows, inner, cols) x instances of the CPU and GPU composition tests: the elementwise form, a matrix with every
# dimension above 1 on one and on three instances, a row vector result and a column vector result
SHAPES = [((1, 1, 1), 5), ((2, 3, 2), 1), ((2, 3, 2), 3), ((1, 1, 3), 2), ((3, 1, 1), 2)]
FLAGS = [(t, s) for t in (False, True) for s in (False, True)]  # (transposed, shared)


def y_shape(R, K, Cn, instances, transposed, shared):
    kc = (Cn, K) if transposed else (K, Cn)
    return kc if shared else (instances,) + kc


def operands(x, y, transposed, shared):
    """x [n, R, K, ...], y as the flags say -> a, b [n, R, C, K, ...]: the two factors of every product."""
    x, y = np.asarray(x), np.asarray(y)
    n, R, K = x.shape[:3]
    tail = x.shape[3:]
    if shared:
        y = np.broadcast_to(y, (n,) + y.shape)
    if transposed:
        y = np.swapaxes(y, 1, 2)
    assert y.shape[:2] == (n, K) and y.shape[3:] == tail, (x.shape, y.shape)
    Cn = y.shape[2]
    a = np.broadcast_to(x[:, :, None], (n, R, Cn, K) + tail)
    b = np.broadcast_to(np.moveaxis(y, 1, 2)[:, None], (n, R, Cn, K) + tail)
    return a, b


def ct_matmul(x, y, luts, q, eval_func, transposed=False, shared=False):
    """eval_func(rows [B, ...], lut [q], q) -> [B, ...]: the host-array EvalFunc of a context or of the oracle."""
    a, b = operands(x, y, transposed, shared)
    m = np.uint64(q - 1)
    n, R, Cn, K = a.shape[:4]
    tail = a.shape[4:]
    flat = (n * R * Cn * K,) + tail
    fs = np.asarray(eval_func(np.ascontiguousarray(((a + b) & m).reshape(flat)), luts[0], q), dtype=np.uint64)
    fd = np.asarray(eval_func(np.ascontiguousarray(((a - b) & m).reshape(flat)), luts[1], q), dtype=np.uint64)
    return (fs - fd).reshape((n, R, Cn, K) + tail).sum(axis=3, dtype=np.uint64) & m


def plain(x, y, luts, q, transposed=False, shared=False):
    """The same on clear values mod q: EvalFunc(v, t) = t[v]."""
    x, y = np.asarray(x, dtype=np.uint64), np.asarray(y, dtype=np.uint64)
    return ct_matmul(x, y, np.asarray(luts, dtype=np.uint64), q, lambda v, t, _q: t[v.astype(np.int64)], transposed, shared)


def class_luts(q):
    """One random-word table of each class of checkInputFunction (as tests/test_gpu_pool2d.py's)."""
    h = q // 2  # lut[i] == q - lut[h + i] for every i < h (the negacyclic test)
    neg = np.array([1 + (3 * x) % (q - 1) if x < h else q - 1 - (3 * (x - h)) % (q - 1) for x in range(q)],
                   dtype=np.uint64)
    per = np.array([(x * 5) % (q // 2) for x in range(q)], dtype=np.uint64)
    return {0: neg, 1: per, 2: cube_lut(q)}


def pair_luts(q, c0, c1):
    """luts[2, q] of classes (c0, c1); the second table is the first kind's reversed-offset variant when the classes
    are equal, so that the two rows differ."""
    t = class_luts(q)
    a, b = t[c0], t[c1].copy()
    if c0 == c1 == 0:
        b = np.concatenate([a[:q // 2][::-1], q - a[:q // 2][::-1]]).astype(np.uint64)
    return np.stack([a, b])


# The decrypting cases shared by tests/test_ctmul_cpu.py (oracle alone, 8 key seeds) and tests/test_gpu_ct_matmul.py
# (a from_keygen context), on the logQ = 12 context (q = 2048) with tfhe_amd.product_tables(q, p, negacyclic): one
# instance, R = C = 2, messages in [0, hi).  An output carries 2 K bootstrap-output errors, plus up to 2 units per
# product under the negacyclic table, against Delta / 2 = q / 2p.  On the oracle, over the 8 key seeds, the worst
# output phase errors |phase - Delta (X Y mod p)| were 29 (p = 4, against 256), 44 (p = 8, against 128) and 32
# (p = 16 negacyclic, against 64); every output decrypted correctly.
DECRYPT_LOGQ = ("STD128", True, 12, 0, 0, 1)  # params_from_logq's arguments
DECRYPT_CASES = {
    "default_p4": dict(p=4, K=2, hi=2, negacyclic=False),   # |x| + |y| <= 2 = p/2
    "default_p8": dict(p=8, K=2, hi=3, negacyclic=False),   # |x| + |y| <= 4 = p/2
    "negacyclic_p16": dict(p=16, K=1, hi=2, negacyclic=True),  # |x| + |y| <= 2 < p/4
}
DECRYPT_SEEDS = tuple(range(3001, 3009))


def decrypt_msgs(name, seed):
    """(x [1, 2, K], y [1, K, 2], want [1, 2, 2] = x y mod p) of a case under a key seed."""
    c = DECRYPT_CASES[name]
    rs = np.random.default_rng([seed, c["p"]])
    x = rs.integers(0, c["hi"], (1, 2, c["K"]), dtype=np.int64)
    y = rs.integers(0, c["hi"], (1, c["K"], 2), dtype=np.int64)
    return x, y, np.matmul(x, y) % c["p"]
