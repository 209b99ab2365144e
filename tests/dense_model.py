"""The dense layer y = f(W^T x + b) in numpy and Python integers (no GPU): the exact matrix product, plus the bias
on the b word, then the oracle's EvalFunc with one shared table.  What tfhe_ciphertext_mul_matrix_device and
tfhe_eval_dense* are compared against."""
import numpy as np


def _as_instances(cts):
    x = np.asarray(cts, dtype=np.uint64)
    return (x[None], True) if x.ndim == 2 else (x, False)


def product(cts, matrix, modulus, bias=None):
    """out[i][c][w] = (bias[c] [w == n] + sum_k matrix[k][c] cts[i][k][w]) mod modulus in [0, modulus), exact at
    every modulus.  cts [instances, K, n+1] (or [K, n+1]: one instance) u64, not necessarily reduced; matrix
    [K, cols] int64; bias [cols] u64 (any values) or None.  Returns u64 in the matching shape.

    Where K max|w| max(ct) < 2^63 every sum fits int64 and numpy's integer matmul is exact (GEMM.cpp's own shape:
    2^10 2^6 2^35 = 2^51); otherwise the sums are Python integers (object dtype)."""
    x, one = _as_instances(cts)
    W = np.asarray(matrix, dtype=np.int64)
    K, cols = W.shape
    assert x.shape[1] == K, (x.shape, W.shape)
    m = int(modulus)
    wmax = max(abs(int(W.min())), abs(int(W.max()))) if W.size else 0
    if K * wmax * int(x.max(initial=0)) < 1 << 63 and m < 1 << 63:
        out = np.stack([(W.T @ xi.astype(np.int64)) % m for xi in x]).astype(np.uint64)  # numpy's % is non-negative
    else:
        out = np.stack([_object_product(xi, W, m) for xi in x]).astype(np.uint64)
    if bias is not None:
        b = [int(v) % m for v in np.asarray(bias, dtype=np.uint64)]
        for i in range(out.shape[0]):
            for c in range(cols):
                out[i, c, -1] = (int(out[i, c, -1]) + b[c]) % m
    return out[0] if one else out


def _object_product(xi, W, m):
    A = xi.astype(object)  # Python integers: no overflow
    return (W.T.astype(object) @ A) % m


def dense(orc, cts, matrix, lut, bias=None, q=None):
    """EvalFunc(product(cts, matrix, q, bias), lut) through the oracle `orc` (pyoracle.Oracle), shared table."""
    q = q or orc.p.q
    z = product(cts, matrix, q, bias)
    flat = orc.eval_func(z.reshape(-1, z.shape[-1]), lut, q)
    return flat.reshape(z.shape)


def clear_layer(msgs, matrix, bias_msgs, f, p):
    """The layer on clear messages mod p: out[i][c] = f((sum_k matrix[k][c] msgs[i][k] + bias_msgs[c]) mod p)."""
    M = np.asarray(msgs, dtype=np.int64)
    if M.ndim == 1:
        M = M[None]
    W = np.asarray(matrix, dtype=np.int64)
    return [[f(int((sum(int(W[k, c]) * int(row[k]) for k in range(W.shape[0])) + int(bias_msgs[c])) % p))
             for c in range(W.shape[1])] for row in M]


# The decrypting case shared by tests/test_dense_cpu.py (oracle alone) and tests/test_gpu_dense.py (device): STD128,
# plaintexts mod p = 4, K = 5, cols = 3, two instances, weights in {-1, 0, 1, 2}, a bias, and the arbitrary-class
# table v -> f(floor(v p / q)) q / p with f(m) = m^3 mod 4.  Worst-case noise: a column of five weights of
# magnitude <= 2 scales the fresh ciphertexts' Gaussian (sigma 3.19) by at most sqrt(5 * 4) = sqrt(20), about 14,
# against EvalFunc's margin of beta = 128 (q / 2p) on either side.
DECRYPT_CASE = dict(paramset="STD128", p=4, K=5, cols=3, instances=2, key_seed=2027, data_seed=61)


def decrypt_case():
    """(msgs [2][5], matrix [5][3], bias_msgs [3], f) of DECRYPT_CASE."""
    d = DECRYPT_CASE
    rs = np.random.default_rng(d["data_seed"])
    msgs = rs.integers(0, d["p"], (d["instances"], d["K"]), dtype=np.int64)
    matrix = rs.integers(-1, 3, (d["K"], d["cols"]), dtype=np.int64)  # {-1, 0, 1, 2}
    bias_msgs = rs.integers(0, d["p"], d["cols"], dtype=np.int64)
    return msgs, matrix, bias_msgs, (lambda m: m ** 3 % 4)
