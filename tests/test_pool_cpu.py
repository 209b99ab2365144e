"""CPU: the pooling model (tests/pool_model.py) that the GPU tests compare against and the host-only calls of the
library -- tfhe_pool2d_shape, tfhe_pool2d_eval_plain, tfhe_amd.max_table -- which need no GPU: shapes and pair
counts, every argument error with its message, the tournament on clear values against the model and against
torch's max_pool2d, the classes of the two helper tables, and decryption through the oracle."""
import ctypes as C
import itertools

import numpy as np
import pytest

import pool_model


def _lib_desc(d):
    import tfhe_amd

    return tfhe_amd.Pool2d(*d)


def test_pool2d_shape_sweep_without_a_gpu():
    """tfhe_pool2d_shape against the model's (oh, ow, rounds, pairs) over small descriptors, and pairs against a count
    over every window written out here: the taps inside the plane, minus one, summed."""
    import tfhe_amd

    tfhe_amd.build()
    carried = 0
    for h, w, kh, kw, sh, sw, ph, pw in itertools.product((3, 5, 6), (4, 7), (1, 2, 3), (1, 2, 3), (1, 2, 3), (1, 2),
                                                          (0, 1, 2), (0, 1)):
        if ph >= kh or pw >= kw or kh > h + 2 * ph or kw > w + 2 * pw:
            continue
        d = pool_model.desc(3, h, w, kh, kw, stride=(sh, sw), padding=(ph, pw))
        got = tfhe_amd.pool2d_shape(_lib_desc(d))
        assert got == pool_model.shape(d), d
        oh, ow = got[:2]
        pairs, most = 0, 0
        for oy, ox in itertools.product(range(oh), range(ow)):
            ys = [y for y in range(oy * sh - ph, oy * sh - ph + kh) if 0 <= y < h]
            xs = [x for x in range(ox * sw - pw, ox * sw - pw + kw) if 0 <= x < w]
            assert len(ys) * len(xs) >= 1  # pad < window leaves a tap
            pairs += len(ys) * len(xs) - 1
            most = max(most, len(ys) * len(xs))
            carried += (len(ys) * len(xs)) % 2
        assert got[3] == pairs and 2 ** got[2] >= most > 2 ** got[2] // 2, d
    assert carried > 0
    # stride defaults to the window; a 1 x 1 window has no pair and no round; stride beyond the window
    assert tfhe_amd.pool2d_shape(_lib_desc(pool_model.desc(6, 28, 28, 2, 2))) == (14, 14, 2, 3 * 196)
    assert tfhe_amd.pool2d_shape(_lib_desc(pool_model.desc(1, 5, 5, 1, 1, stride=(2, 2)))) == (3, 3, 0, 0)
    assert tfhe_amd.pool2d_shape(_lib_desc(pool_model.desc(1, 9, 9, 2, 2, stride=(4, 5)))) == (2, 2, 2, 12)
    assert tfhe_amd.pool2d_shape(_lib_desc(pool_model.desc(1, 5, 4, 3, 3, stride=(2, 2), padding=(1, 1))))[2:] == (4, 29)


GOOD = dict(c=4, h=5, w=4, kh=3, kw=2, stride_h=2, stride_w=1, pad_h=1, pad_w=1)
BAD_DESCRIPTORS = [(dict({f: 0}), f) for f in ("c", "h", "w", "kh", "kw", "stride_h", "stride_w")]
BAD_DESCRIPTORS += [
    (dict(pad_h=3), "pad_h"), (dict(pad_w=2), "pad_w"),    # pad >= window
    (dict(h=1, kh=4, pad_h=1), "kh"), (dict(w=1, kw=4, pad_w=1), "kw"),  # window beyond the padded plane
]


@pytest.mark.parametrize("change,field", BAD_DESCRIPTORS, ids=[f"{c}" for c, _ in BAD_DESCRIPTORS])
def test_pool2d_descriptor_errors(change, field):
    """Every descriptor error by status (TFHE_ERR_INVALID_ARGUMENT) and by the convolution's message, which names the
    field -- from tfhe_pool2d_shape and from tfhe_pool2d_eval_plain alike."""
    import tfhe_amd

    tfhe_amd.build()
    assert tfhe_amd.pool2d_shape(tfhe_amd.Pool2d(**GOOD)) == (3, 5, 3, 41)
    bad = tfhe_amd.Pool2d(**dict(GOOD, **change))
    with pytest.raises(tfhe_amd.TfheError) as e:
        tfhe_amd.pool2d_shape(bad)
    assert e.value.status == 1
    msg = str(e.value).split("Pool2d: ")[1]
    assert msg.split()[0] == field or f" {field}" in msg, str(e.value)
    # the convolution's wording, by the convolution's code
    conv = dict(c_in=GOOD["c"], c_out=GOOD["c"], groups=GOOD["c"], **{k: v for k, v in GOOD.items() if k != "c"})
    cchange = {("c_in" if k == "c" else k): v for k, v in change.items()}
    with pytest.raises(tfhe_amd.TfheError) as ce:
        tfhe_amd.conv2d_shape(tfhe_amd.Conv2d(**dict(conv, **cchange)))
    assert msg == str(ce.value).split("Conv2d: ")[1].replace("c_in", "c")
    x = np.zeros(16, dtype=np.uint64)
    L = tfhe_amd.lib()
    st = L.tfhe_pool2d_eval_plain(C.byref(bad), 1, 8, x.ctypes.data, x.ctypes.data, x.ctypes.data)
    assert st == 1 and msg.encode() in L.tfhe_last_error()


def test_pool2d_host_call_argument_errors():
    """The null pointers, instances = 0, the moduli and an overflowing size product of the host-only calls, message
    included; null result pointers of tfhe_pool2d_shape are allowed."""
    import tfhe_amd

    tfhe_amd.build()
    L = tfhe_amd.lib()
    assert L.tfhe_pool2d_shape(None, None, None, None, None) == 1
    assert b"descriptor" in L.tfhe_last_error()
    d = tfhe_amd.Pool2d(**GOOD)
    assert L.tfhe_pool2d_shape(C.byref(d), None, None, None, None) == 0
    pairs, rounds = C.c_size_t(), C.c_uint32()
    assert L.tfhe_pool2d_shape(C.byref(d), None, None, C.byref(rounds), C.byref(pairs)) == 0
    assert (rounds.value, pairs.value) == (3, 41)
    x = np.zeros(4 * 5 * 4, dtype=np.uint64)
    lut, out = np.zeros(1024, dtype=np.uint64), np.zeros(4 * 3 * 5, dtype=np.uint64)
    P = lambda a: a.ctypes.data
    plain = L.tfhe_pool2d_eval_plain
    assert plain(C.byref(d), 1, 1024, P(lut), P(x), P(out)) == 0
    for args, word in (((None, 1, 1024, P(lut), P(x), P(out)), b"descriptor"),
                       ((C.byref(d), 1, 1024, None, P(x), P(out)), b"null lut"),
                       ((C.byref(d), 1, 1024, P(lut), None, P(out)), b"null ct"),
                       ((C.byref(d), 1, 1024, P(lut), P(x), None), b"null out"),
                       ((C.byref(d), 0, 1024, P(lut), P(x), P(out)), b"instances is 0"),
                       ((C.byref(d), 1, 4, P(lut), P(x), P(out)), b"q must be a power of two >= 8"),
                       ((C.byref(d), 1, 768, P(lut), P(x), P(out)), b"q must be a power of two >= 8"),
                       ((C.byref(d), 2 ** 62, 1024, P(lut), P(x), P(out)), b"sizes overflow")):
        assert plain(*args) == 1, word
        assert word in L.tfhe_last_error(), (word, L.tfhe_last_error())
    with pytest.raises(ValueError):
        tfhe_amd.pool2d_eval_plain(d, np.zeros((1, 4, 5, 5)), lut, 1024)  # plane size against the descriptor
    with pytest.raises(ValueError):
        tfhe_amd.pool2d_eval_plain(d, np.zeros((1, 4, 5, 4)), lut[:-1], 1024)
    with pytest.raises(ValueError):
        tfhe_amd.max_table(768)


SHAPES = [pool_model.desc(2, 4, 4, 2, 2), pool_model.desc(2, 5, 4, 3, 3, stride=(2, 2), padding=(1, 1)),
          pool_model.desc(2, 4, 5, 3, 2, stride=(1, 2)), pool_model.desc(2, 2, 3, 2, 3),
          pool_model.desc(2, 5, 5, 1, 1, stride=(2, 2)), pool_model.desc(1, 1, 2, 2, 1, padding=(1, 0)),
          pool_model.desc(3, 7, 6, 3, 3, stride=(3, 2), padding=(2, 2))]


@pytest.mark.parametrize("q", [8, 1 << 10, 1 << 12])
def test_eval_plain_equals_the_model_on_random_tables(q):
    """tfhe_pool2d_eval_plain against the model with op(a, b) = b + lut[a - b mod q] mod q, random tables and values:
    even and odd tap counts (9, 6 and 4 valid taps in one plane: carries at more than one round), a window equal to
    the plane, a 1 x 1 window (a strided copy) and positions with one valid tap among 2 x 1 windows."""
    import tfhe_amd

    tfhe_amd.build()
    rs = np.random.default_rng(61 + q)
    for d in SHAPES:
        lut = rs.integers(0, q, q, dtype=np.uint64)
        x = rs.integers(0, q, (3, d.c, d.h, d.w), dtype=np.uint64)
        before = x.copy()
        got = tfhe_amd.pool2d_eval_plain(_lib_desc(d), x, lut, q)
        assert np.array_equal(got, pool_model.pool2d(x, d, pool_model.plain_pair(lut, q))), d
        assert np.array_equal(x, before)
        assert np.array_equal(tfhe_amd.pool2d_eval_plain(_lib_desc(d), x[0], lut, q), got[0])  # one instance
    d = SHAPES[4]  # the copy reads no table entry and keeps every word
    assert np.array_equal(tfhe_amd.pool2d_eval_plain(_lib_desc(d), x[:, :2, :5, :5], lut, q), x[:, :2, :5:2, :5:2])


TORCH_CASES = [(k, s, p) for k in ((2, 2), (3, 3), (3, 2)) for s in ((1, 1), (2, 2), (2, 1), (3, 2))
               for p in ((0, 0), (1, 1), (1, 0))]


@pytest.mark.parametrize("kernel,stride,padding", TORCH_CASES, ids=str)
def test_max_table_equals_torch_max_pool2d(kernel, stride, padding):
    """eval_plain with max_table(q) on clear values below q/2 (differences inside (-q/2, q/2)) equals
    torch.nn.functional.max_pool2d in float64, exactly; paddings within PyTorch's pad <= window / 2.

    With max_table(q, negacyclic=True) on values in [4, q/4 - 4) a pair step returns max(a, b) + e with e = +1 where
    a = b, -1 where a < b and 0 where a > b (the helper's 1 for 0).  A maximum moves by at most what its operands
    move, so after r rounds a result is within r of the true maximum.  The rule used here: for every output,
    |result - max| <= ceil(log2(valid taps of its window)), the rounds on its path; the values keep every
    difference, drift included, inside (-q/4, q/4)."""
    import torch

    import tfhe_amd

    tfhe_amd.build()
    q, C_, h, w = 1 << 10, 2, 7, 6
    d = pool_model.desc(C_, h, w, *kernel, stride=stride, padding=padding)
    oh, ow, rounds, _ = pool_model.shape(d)
    rs = np.random.default_rng(62)
    x = rs.integers(0, q // 2, (2, C_, h, w), dtype=np.int64)
    ref = torch.nn.functional.max_pool2d(torch.from_numpy(x).double(), kernel, stride=stride, padding=padding).numpy()
    got = tfhe_amd.pool2d_eval_plain(_lib_desc(d), x.astype(np.uint64), tfhe_amd.max_table(q), q)
    assert got.shape == ref.shape == (2, C_, oh, ow)
    assert np.array_equal(got.astype(np.float64), ref)
    # the negacyclic table: one more bit of headroom, and the documented unit
    xn = rs.integers(4, q // 4 - 4, (2, C_, h, w), dtype=np.int64)
    xn[0, 0, :3, :3] = 77  # ties
    refn = torch.nn.functional.max_pool2d(torch.from_numpy(xn).double(), kernel, stride=stride, padding=padding).numpy()
    gotn = tfhe_amd.pool2d_eval_plain(_lib_desc(d), xn.astype(np.uint64), tfhe_amd.max_table(q, negacyclic=True), q)
    depth = np.array([[(len(pool_model.taps(d, oy, ox)) - 1).bit_length() for ox in range(ow)] for oy in range(oh)])
    assert rounds == depth.max() <= 4
    assert (np.abs(gotn.astype(np.int64) - refn.astype(np.int64)) <= depth[None, None]).all()
    if kernel != (1, 1):
        assert not np.array_equal(gotn.astype(np.float64), refn)  # the unit is there: ties give max + 1


@pytest.mark.parametrize("q", [8, 1 << 10, 1 << 12])
def test_max_tables_land_in_their_classes(q):
    """The default table is arbitrary-class and the negacyclic one negacyclic by checkInputFunction: a one-node
    FuncCircuit per table, its info() read; and the tables' entries as documented."""
    import tfhe_amd

    tfhe_amd.build()
    arb, neg = tfhe_amd.max_table(q), tfhe_amd.max_table(q, negacyclic=True)
    for lut, cls in ((arb, "arbitrary"), (neg, "negacyclic")):
        fc = tfhe_amd.FuncCircuit(1, [("LUT", 0, (0, 1))], lut[None], [1], q)
        info = fc.info()
        fc.free()
        assert {k: info[k] for k in ("negacyclic", "periodic", "arbitrary")} == \
            {k: int(k == cls) for k in ("negacyclic", "periodic", "arbitrary")}
    assert arb.dtype == neg.dtype == np.uint64
    assert [int(arb[x]) for x in range(q)] == [x if x < q // 2 else 0 for x in range(q)]
    want = [max(x, 1) if x < q // 4 else 1 for x in range(q // 2)]
    assert [int(v) for v in neg[:q // 2]] == want and [int(v) for v in neg[q // 2:]] == [q - v for v in want]


@pytest.mark.slow
def test_decrypts_to_the_clear_max_on_the_oracle(oracle):
    """pool_model.POOL_DECRYPT_CASES on the oracle alone, for each of 8 key seeds: keygen, encrypt, the model with the
    oracle's EvalFunc under each helper table, decrypt -- every output is the clear maximum.  On the logQ = 12
    context: STD128 admits no usable p (pool_model).  The first seed also pins the network of the
    decrypting GPU case (pool_model.NET_CASE): convolution layer, then max pooling."""
    import conv_model
    import tfhe_amd

    tfhe_amd.build()
    op = oracle.params_from_logq(*pool_model.POOL_DECRYPT_LOGQ)
    q, w, d = op.q, op.n + 1, pool_model.POOL_DECRYPT_DESC
    seen = set()
    for seed in pool_model.POOL_DECRYPT_SEEDS:
        rng = oracle.Rng(seed)
        sk, bsk, ksk = oracle.keygen(op, rng)
        orc = oracle.Oracle(op, bsk, ksk)
        del bsk, ksk
        try:
            for kind, c in pool_model.POOL_DECRYPT_CASES.items():
                p = c["p"]
                msgs = pool_model.pool_decrypt_msgs(kind, seed)
                cts = np.stack([oracle.encrypt(op, rng, sk, int(m), p, q) for m in msgs.ravel()])
                lut = tfhe_amd.max_table(q, c["negacyclic"])
                out = pool_model.pool2d(cts.reshape(msgs.shape + (w,)), d, pool_model.func_pair(orc.eval_func, lut, q))
                got = [oracle.decrypt(op, sk, row, p, q) for row in out.reshape(-1, w)]
                want = [int(v) for v in pool_model.clear_max(msgs, d).ravel()]
                assert got == want, (kind, seed)
                seen.update(want)
            if seed == pool_model.NET_CASE["key_seed"]:
                p = pool_model.NET_CASE["p"]
                msgs, weight, want = pool_model.net_case()
                cts = np.stack([oracle.encrypt(op, rng, sk, int(m), p, q) for m in msgs.ravel()])
                y = conv_model.conv_layer(orc, cts.reshape(msgs.shape + (w,)), weight, pool_model.parity_lut(q, p),
                                          conv_model.desc(1, 3, 3, 2, 2, 2), None, q)
                out = pool_model.pool2d(y, pool_model.desc(2, 2, 2, 1, 2),
                                        pool_model.func_pair(orc.eval_func, tfhe_amd.max_table(q), q))
                got = [oracle.decrypt(op, sk, row, p, q) for row in out.reshape(-1, w)]
                assert got == [int(v) for v in want.ravel()] and len(set(got)) > 1
        finally:
            orc.close()
    assert seen == {0, 1}, "the cases must not be constant"
