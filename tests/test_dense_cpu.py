"""CPU: the dense-layer model (tests/dense_model.py) that the GPU tests compare against, checked on its own --
against the reference's recorded matrix product, against plain Python-integer arithmetic, and by decryption
through the oracle -- and the tile-size query of the library, which needs no GPU."""
import numpy as np
import pytest

import dense_model
from helpers import cube_lut


def test_model_equals_reference_gemm_fixture(oracle):
    """GEMM.cpp's configuration (K = 1024, entries in [0, 64), modulus qKS = 2^35): the reference is exact there,
    so the model's product is the recorded output word for word."""
    import refvec

    data = refvec.load()
    c = refvec.case("mm_gemm", data)
    x = refvec.inputs(c, data["fixtures"])
    out = dense_model.product(x["in"], x["matrix"], c["args"]["modulus"])
    refvec.check(c, out.ravel(), {})


@pytest.mark.parametrize("mod", [1 << 12, (1 << 54) - 77823, (1 << 63) + 29, (1 << 64) - 59, 1000003])
def test_model_equals_python_integers(mod):
    """Signed entries (INT64_MIN / INT64_MAX among them), unreduced ciphertext words, a bias >= modulus, moduli that
    are no power of two: every word against sums of Python integers written out here."""
    rs = np.random.default_rng(21)
    inst, K, cols, w = 2, 6, 3, 9
    ct = rs.integers(0, np.iinfo(np.uint64).max, (inst, K, w), dtype=np.uint64, endpoint=True)
    ct[0, 0, :] = np.iinfo(np.uint64).max
    mat = rs.integers(np.iinfo(np.int64).min, np.iinfo(np.int64).max, (K, cols), dtype=np.int64, endpoint=True)
    mat[:, 0] = np.iinfo(np.int64).min
    mat[:, 1] = np.iinfo(np.int64).max
    bias = np.array([0, mod - 1, min(mod + 5, (1 << 64) - 1)], dtype=np.uint64)
    got = dense_model.product(ct, mat, mod, bias)
    assert got.shape == (inst, cols, w) and got.dtype == np.uint64
    for i in range(inst):
        for c in range(cols):
            for j in range(w):
                want = sum(int(mat[k, c]) * int(ct[i, k, j]) for k in range(K))
                if j == w - 1:
                    want += int(bias[c])
                assert int(got[i, c, j]) == want % mod, (i, c, j)
    # the int64 path (small operands) and the Python-integer path agree, and one instance keeps its shape
    small_ct = rs.integers(0, 1 << 12, (K, w), dtype=np.uint64)
    small_m = rs.integers(-64, 64, (K, cols), dtype=np.int64)
    import refvec

    if mod < 1 << 63:
        assert np.array_equal(dense_model.product(small_ct, small_m, mod), refvec.mulmatrix_exact(small_ct, small_m, mod))


def test_decrypting_layer_on_the_oracle(oracle):
    """dense_model.DECRYPT_CASE on the oracle alone: keygen, encrypt, the model's layer, decrypt -- every output is
    the clear-text layer's.  Fixes the seeds tests/test_gpu_dense.py reuses."""
    d = dense_model.DECRYPT_CASE
    msgs, matrix, bias_msgs, f = dense_model.decrypt_case()
    op = oracle.params_from_set(d["paramset"])
    p, q = d["p"], op.q
    rng = oracle.Rng(d["key_seed"])
    sk, bsk, ksk = oracle.keygen(op, rng)
    cts = np.stack([np.stack([oracle.encrypt(op, rng, sk, int(m), p, q) for m in row]) for row in msgs])
    lut = cube_lut(q, p)  # v -> f(floor(v p / q)) q / p
    assert [int(lut[m * (q // p)]) // (q // p) for m in range(p)] == [f(m) for m in range(p)]
    bias = (bias_msgs.astype(np.uint64) * np.uint64(q // p))
    orc = oracle.Oracle(op, bsk, ksk)
    try:
        out = dense_model.dense(orc, cts, matrix, lut, bias, q)
    finally:
        orc.close()
    assert out.shape == (d["instances"], d["cols"], op.n + 1)
    got = [[oracle.decrypt(op, sk, out[i, c], p, q) for c in range(d["cols"])] for i in range(d["instances"])]
    want = dense_model.clear_layer(msgs, matrix, bias_msgs, f, p)
    assert got == want
    assert len({v for row in want for v in row}) > 1, "the case must not be constant"


def test_mm_tiles_without_a_gpu():
    """tfhe_mm_tiles: the matrix-product kernel's tile sizes, from the library alone."""
    import tfhe_amd

    tfhe_amd.build()
    kt, ct, threads = tfhe_amd.mm_tiles()
    assert kt > 0 and ct > 0 and threads > 0
    assert threads % 64 == 0
