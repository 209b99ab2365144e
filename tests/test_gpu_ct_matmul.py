"""GPU: the product of two encrypted tensors (tfhe_eval_ct_matmul_device / tfhe_eval_ct_matmul):
out[i][r][c] = sum_k EvalFunc(x + y, luts[0]) - EvalFunc(x - y, luts[1]), the 2 P look-ups one flat EvalFunc batch
between two streaming kernels.  It must equal, bit for bit, the same formula composed of host-array EvalFunc calls
(tests/ctmul_model.py with ctx.EvalFunc) and, through the model, the oracle -- for table pairs of equal and of mixed
classes, every layout flag, on STD128 and the arbFunc logQ = 12 context; it must count its bootstraps, slice at whole
outputs beyond 65,536 look-ups, write no input word and nothing past its output, order two streams, chain between
dense layers by pointer, equal the five-node function circuit, and decrypt to the clear product."""
import itertools

import numpy as np
import pytest

import ctmul_model
import dense_model

pytestmark = pytest.mark.gpu

PAIRS = [(0, 0), (1, 2), (2, 0)]  # (negacyclic, negacyclic), (periodic, arbitrary), (arbitrary, negacyclic)
PER_LOOKUP = {0: 1, 1: 2, 2: 2}


@pytest.fixture(scope="module", params=["STD128", "ARB12"])
def env(request, shared_kat):
    s = shared_kat(request.param)  # the session's shared contexts
    return s["op"], s["ctx"], s["orc"]


def _dev(x):
    import torch

    x = np.ascontiguousarray(x)
    if x.dtype == np.uint64:
        x = x.view(np.int64)
    return torch.from_numpy(x).to(torch.device("cuda", 0))


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _inputs(rs, q, w, shape, n, tr, sh):
    R, K, Cn = shape
    x = rs.integers(0, q, (n, R, K, w), dtype=np.uint64)
    y = rs.integers(0, q, ctmul_model.y_shape(R, K, Cn, n, tr, sh) + (w,), dtype=np.uint64)
    return x, y


def _ctmm_device(ctx, w, shape, x, y, luts, q, tr=False, sh=False, stream=None):
    """The device call on an output pre-filled with -1 and followed by a guard row, which must stay; the inputs and
    the tables must come back bit-identical."""
    import torch

    import tfhe_amd

    R, K, Cn = shape
    n = x.shape[0]
    d_x, d_y, d_l = _dev(x), _dev(y), _dev(luts)
    rows = n * R * Cn
    d_out = torch.full((rows + 1, w), -1, dtype=torch.int64, device=d_x.device)
    torch.cuda.synchronize()
    ctx.EvalCtMatMulDevice(tfhe_amd.CtMatMul(R, K, Cn, tr, sh), n, d_x.data_ptr(), d_y.data_ptr(), d_l.data_ptr(),
                           d_out.data_ptr(), q=q, stream=stream.cuda_stream if stream is not None else 0)
    torch.cuda.synchronize()
    out = _host(d_out)
    assert (out[rows] == np.uint64(2**64 - 1)).all(), "the guard row was written"
    assert np.array_equal(_host(d_x), x) and np.array_equal(_host(d_y), y), "an input word was written"
    assert np.array_equal(_host(d_l), luts)
    return out[:rows].reshape(n, R, Cn, w)


@pytest.mark.parametrize("pair", PAIRS, ids=str)
def test_layer_equals_the_host_array_composition(env, pair):
    """Every word of every shape and flag combination against the model with ctx.EvalFunc (one host-array call for
    the sums, one for the differences), the host-array entry, and the bootstraps counter: P (b0 + b1)."""
    op, ctx, _ = env
    q, w = op.q, op.n + 1
    luts = ctmul_model.pair_luts(q, *pair)
    per = PER_LOOKUP[pair[0]] + PER_LOOKUP[pair[1]]
    rs = np.random.default_rng(101 + 10 * pair[0] + pair[1])
    for (shape, n), (tr, sh) in itertools.product(ctmul_model.SHAPES, ctmul_model.FLAGS):
        x, y = _inputs(rs, q, w, shape, n, tr, sh)
        before = ctx.info().bootstraps
        got = _ctmm_device(ctx, w, shape, x, y, luts, q, tr, sh)
        assert ctx.info().bootstraps - before == per * n * shape[0] * shape[1] * shape[2], (shape, n, tr, sh)
        assert (got < q).all()
        comp = ctmul_model.ct_matmul(x, y, luts, q, ctx.EvalFunc, tr, sh)
        assert np.array_equal(got, comp), (shape, n, tr, sh)
        assert np.array_equal(got, ctx.EvalCtMatMul(x, y, luts, transposed=tr, q=q)), (shape, n, tr, sh)


def test_small_case_equals_the_oracle(env):
    """(1, 1, 3) x 2, y transposed, tables (arbitrary, negacyclic): the model with the oracle's EvalFunc."""
    op, ctx, orc = env
    q, w = op.q, op.n + 1
    luts = ctmul_model.pair_luts(q, 2, 0)
    x, y = _inputs(np.random.default_rng(111), q, w, (1, 1, 3), 2, True, False)
    got = _ctmm_device(ctx, w, (1, 1, 3), x, y, luts, q, True, False)
    assert np.array_equal(got, ctmul_model.ct_matmul(x, y, luts, q, orc.eval_func, True, False))


def test_elementwise_equals_the_five_node_circuit(env):
    """EvalCtMul on 5 products against the FuncCircuit x + y, x - y, two LUT nodes, their difference: bit for bit."""
    import tfhe_amd

    op, ctx, _ = env
    q, w = op.q, op.n + 1
    luts = ctmul_model.pair_luts(q, 0, 0)
    rs = np.random.default_rng(112)
    x, y = (rs.integers(0, q, (5, w), dtype=np.uint64) for _ in range(2))
    fc = tfhe_amd.FuncCircuit(2, [("LIN", (0, 1), (1, 1)), ("LIN", (0, 1), (1, -1)), ("LUT", 0, (2, 1)),
                                  ("LUT", 1, (3, 1)), ("LIN", (4, 1), (5, -1))], luts, [6], q)
    try:
        want = ctx.EvalFuncCircuit(fc, np.stack([x, y]))
    finally:
        fc.free()
    before = ctx.info().bootstraps
    got = ctx.EvalCtMul(x, y, luts, q=q)
    assert ctx.info().bootstraps - before == 10
    assert got.shape == x.shape and np.array_equal(got, want[0])
    # any leading shape, through the same entry point
    assert np.array_equal(ctx.EvalCtMul(x[:4].reshape(2, 2, w), y[:4].reshape(2, 2, w), luts, q=q), got[:4].reshape(2, 2, w))
    assert np.array_equal(got, _ctmm_device(ctx, w, (1, 1, 1), x.reshape(5, 1, 1, w), y.reshape(5, 1, 1, w), luts, q).reshape(5, w))


def test_slices_at_whole_outputs(shared_kat):
    """STD128, K = 3, R = C = 1, 11,000 instances, negacyclic tables: 66,000 look-ups, two slices cut at output
    floor(65,536 / 6) = 10,922, and the kernels' grids stride over the items.  The outputs either side of the cut, the
    first and the last, against EvalFuncDevice on sums and differences computed by torch; every row written, the
    guard, the counter."""
    import torch

    import tfhe_amd

    s = shared_kat("STD128")
    op, ctx = s["op"], s["ctx"]
    q, w, n, K, cut = op.q, op.n + 1, 11000, 3, 10922
    gen = torch.Generator(device="cuda")
    gen.manual_seed(113)
    d_x = torch.randint(0, q, (n, 1, K, w), dtype=torch.int64, device="cuda", generator=gen)
    d_y = torch.randint(0, q, (n, K, 1, w), dtype=torch.int64, device="cuda", generator=gen)
    kx, ky = d_x.clone(), d_y.clone()
    luts = ctmul_model.pair_luts(q, 0, 0)
    d_l = _dev(luts)
    d_out = torch.full((n + 1, w), -1, dtype=torch.int64, device=d_x.device)
    torch.cuda.synchronize()
    before = ctx.info().bootstraps
    ctx.EvalCtMatMulDevice(tfhe_amd.CtMatMul(1, K, 1), n, d_x.data_ptr(), d_y.data_ptr(), d_l.data_ptr(), d_out.data_ptr())
    torch.cuda.synchronize()
    assert ctx.info().bootstraps - before == 2 * n * K == 66000
    assert torch.equal(d_x, kx) and torch.equal(d_y, ky) and bool((d_out[n] == -1).all())
    assert bool((d_out[:n] >= 0).all()) and bool((d_out[:n] < q).all())  # every row was written
    idx = torch.tensor([0, cut - 1, cut, n - 1], device=d_x.device)
    a, b = d_x[idx, 0], d_y[idx, :, 0]  # [4, K, w]
    zs, zd = ((a + b) & (q - 1)).reshape(-1, w).contiguous(), ((a - b) & (q - 1)).reshape(-1, w).contiguous()
    fs, fd = torch.empty_like(zs), torch.empty_like(zd)
    ctx.EvalFuncDevice(len(zs), zs.data_ptr(), d_l[0].data_ptr(), fs.data_ptr())
    ctx.EvalFuncDevice(len(zd), zd.data_ptr(), d_l[1].data_ptr(), fd.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(d_out[idx], (fs - fd).reshape(4, K, w).sum(dim=1) & (q - 1))


def test_arbitrary_table_needs_q_up_to_N(env):
    """q = 2N with an arbitrary-class table in either place: TFHE_ERR_UNSUPPORTED before anything is launched, and the
    bootstraps counter does not move."""
    import tfhe_amd as capi

    op, ctx, _ = env
    q, w = 2 * op.N, op.n + 1
    x, y = _inputs(np.random.default_rng(114), q, w, (2, 3, 2), 1, False, False)
    before = ctx.info().bootstraps
    for pair in ((0, 2), (2, 0)):
        luts = ctmul_model.pair_luts(q, *pair)
        for call in (lambda: _ctmm_device(ctx, w, (2, 3, 2), x, y, luts, q), lambda: ctx.EvalCtMatMul(x, y, luts, q=q)):
            with pytest.raises(capi.TfheError) as e:
                call()
            assert e.value.status == 2  # TFHE_ERR_UNSUPPORTED
    assert ctx.info().bootstraps == before


def test_an_output_beyond_the_chunk_is_unsupported(env):
    """2 inner > 65,536: one output's products no longer fit one EvalFunc batch.  The check precedes any read, so
    small valid pointers stand in for the buffers."""
    import tfhe_amd as capi

    op, ctx, _ = env
    t = _dev(np.zeros((4, op.n + 1), dtype=np.uint64))
    P = t.data_ptr()
    before = ctx.info().bootstraps
    with pytest.raises(capi.TfheError) as e:
        ctx.EvalCtMatMulDevice(capi.CtMatMul(1, 32769, 1), 1, P, P, P, P)
    assert e.value.status == 2 and "inner" in str(e.value)
    assert ctx.info().bootstraps == before


def test_shape_and_argument_errors(env):
    import tfhe_amd as capi

    op, ctx, _ = env
    q, w = op.q, op.n + 1
    luts = ctmul_model.pair_luts(q, 0, 0)
    x, y = _inputs(np.random.default_rng(115), q, w, (2, 3, 2), 2, False, False)
    for bad_x, bad_y, kw in ((x[..., :-1], y, {}), (x[0], y, {}), (x, y[:1], {}), (x, y[:, :2], {}),
                             (x, y, dict(transposed=True)), (x, y[0, :2], {})):
        with pytest.raises(ValueError):
            ctx.EvalCtMatMul(bad_x, bad_y, luts, **kw)
    with pytest.raises(ValueError) as ve:
        ctx.EvalCtMatMul(x, y[:, :2], luts)
    assert f"(2, 3, C, {w})" in str(ve.value)
    with pytest.raises(ValueError):
        ctx.EvalCtMatMul(x, y, luts[:1])
    with pytest.raises(ValueError):
        ctx.EvalCtMul(x, y, luts)  # unequal shapes
    t = _dev(x)
    P, good = t.data_ptr(), capi.CtMatMul(2, 3, 2)
    before = ctx.info().bootstraps
    for bad_q in (4, 3 * 256, 4 * op.N):  # below 8; no power of two; not a divisor of 2N
        with pytest.raises(capi.TfheError) as e:
            ctx.EvalCtMatMulDevice(good, 2, P, P, P, P, q=bad_q)
        assert e.value.status == 1 and "q must be a power of two >= 8 that divides 2N" in str(e.value), bad_q
    for args, word in (((good, 2, 0, P, P, P), "null x"), ((good, 2, P, 0, P, P), "null y"),
                       ((good, 2, P, P, 0, P), "null luts"), ((good, 2, P, P, P, 0), "null out"),
                       ((good, 0, P, P, P, P), "instances is 0"), ((good, 2**62, P, P, P, P), "sizes overflow"),
                       ((capi.CtMatMul(0, 3, 2), 2, P, P, P, P), "rows is 0"),
                       ((capi.CtMatMul(2, 0, 2), 2, P, P, P, P), "inner is 0"),
                       ((capi.CtMatMul(2, 3, 0), 2, P, P, P, P), "cols is 0"),
                       ((capi.CtMatMul(2, 3, 2, 2, 0), 2, P, P, P, P), "y_transposed must be 0 or 1"),
                       ((capi.CtMatMul(2, 3, 2, 0, 2), 2, P, P, P, P), "y_shared must be 0 or 1")):
        with pytest.raises(capi.TfheError) as e:
            ctx.EvalCtMatMulDevice(*args)
        assert e.value.status == 1 and word in str(e.value), word
    L = capi.lib()
    assert L.tfhe_eval_ct_matmul_device(ctx._h, None, 2, P, P, q, P, P, None) == 1 and b"descriptor" in L.tfhe_last_error()
    assert ctx.info().bootstraps == before


def test_two_streams_are_ordered(env):
    """Two calls on two user streams and a host-array call, with no synchronisation between them: they share the
    device's scratch and flat rows, which the engine orders; each equals its sequential run."""
    import torch

    import tfhe_amd

    op, ctx, _ = env
    q, w = op.q, op.n + 1
    luts = ctmul_model.pair_luts(q, 1, 2)
    rs = np.random.default_rng(116)
    x1, y1 = _inputs(rs, q, w, (2, 3, 2), 3, False, True)
    x2, y2 = _inputs(rs, q, w, (3, 2, 1), 2, True, False)
    want1 = _ctmm_device(ctx, w, (2, 3, 2), x1, y1, luts, q, False, True)
    want2 = _ctmm_device(ctx, w, (3, 2, 1), x2, y2, luts, q, True, False)
    a1, b1, a2, b2, d_l = (_dev(v) for v in (x1, y1, x2, y2, luts))
    o1 = torch.full(want1.shape, -1, dtype=torch.int64, device=a1.device)
    o2 = torch.full(want2.shape, -1, dtype=torch.int64, device=a1.device)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    ctx.EvalCtMatMulDevice(tfhe_amd.CtMatMul(2, 3, 2, 0, 1), 3, a1.data_ptr(), b1.data_ptr(), d_l.data_ptr(), o1.data_ptr(),
                           stream=s1.cuda_stream)
    ctx.EvalCtMatMulDevice(tfhe_amd.CtMatMul(3, 2, 1, 1, 0), 2, a2.data_ptr(), b2.data_ptr(), d_l.data_ptr(), o2.data_ptr(),
                           stream=s2.cuda_stream)
    host = ctx.EvalCtMatMul(x2, y2, luts, transposed=True)
    s1.synchronize()
    s2.synchronize()
    assert np.array_equal(_host(o1), want1) and np.array_equal(_host(o2), want2) and np.array_equal(host, want2)


def test_chains_between_dense_layers(shared_kat):
    """EvalDenseDevice -> EvalCtMatMulDevice (y_shared: encrypted weights) -> EvalDenseDevice by pointer, no relayout
    (STD128, negacyclic tables): 3 -> 4 dense on two instances, read as 2 x 2 matrices times a shared 2 x 2 of
    ciphertexts, then 4 -> 2 dense.  Each stage equals the model through the oracle."""
    import torch

    import tfhe_amd

    s = shared_kat("STD128")
    op, ctx, orc = s["op"], s["ctx"], s["orc"]
    q, w = op.q, op.n + 1
    rs = np.random.default_rng(117)
    ct = rs.integers(0, q, (2, 3, w), dtype=np.uint64)
    yw = rs.integers(0, q, (2, 2, w), dtype=np.uint64)
    m1, m2 = rs.integers(-4, 4, (3, 4), dtype=np.int64), rs.integers(-4, 4, (4, 2), dtype=np.int64)
    luts = ctmul_model.pair_luts(q, 0, 0)
    d_ct, d_yw, d_m1, d_m2, d_l = (_dev(a) for a in (ct, yw, m1, m2, luts))
    d_a = torch.full((2, 4, w), -1, dtype=torch.int64, device=d_ct.device)
    d_b = torch.full((2, 2, 2, w), -1, dtype=torch.int64, device=d_ct.device)
    d_o = torch.full((2, 2, w), -1, dtype=torch.int64, device=d_ct.device)
    torch.cuda.synchronize()
    ctx.EvalDenseDevice(2, 3, d_ct.data_ptr(), 4, d_m1.data_ptr(), d_l[0].data_ptr(), d_a.data_ptr())
    ctx.EvalCtMatMulDevice(tfhe_amd.CtMatMul(2, 2, 2, 0, 1), 2, d_a.data_ptr(), d_yw.data_ptr(), d_l.data_ptr(),
                           d_b.data_ptr())
    ctx.EvalDenseDevice(2, 4, d_b.data_ptr(), 2, d_m2.data_ptr(), d_l[1].data_ptr(), d_o.data_ptr())
    torch.cuda.synchronize()
    a = dense_model.dense(orc, ct, m1, luts[0], None, q)
    assert np.array_equal(_host(d_a), a)
    b = ctmul_model.ct_matmul(a.reshape(2, 2, 2, w), yw, luts, q, orc.eval_func, shared=True)
    assert np.array_equal(_host(d_b), b)
    assert np.array_equal(_host(d_o), dense_model.dense(orc, b.reshape(2, 4, w), m2, luts[1], None, q))


def test_decrypts_to_the_clear_product():
    """tests/test_ctmul_cpu.py's decrypting cases of the first key seed on a from_keygen context of the logQ = 12
    parameters: Encrypt -> EvalCtMatMul with tfhe_amd.product_tables -> Decrypt equals X Y mod p, and EvalCtMul on
    the same messages, element by element, their products."""
    import tfhe_amd

    seed = ctmul_model.DECRYPT_SEEDS[0]
    cp = tfhe_amd.params_from_logq(*ctmul_model.DECRYPT_LOGQ)
    q, w = cp.q, cp.n + 1
    ctx, sk = tfhe_amd.BinFHEContextHIP.from_keygen(cp, seed)
    try:
        for name, c in ctmul_model.DECRYPT_CASES.items():
            p = c["p"]
            X, Y, want = ctmul_model.decrypt_msgs(name, seed)
            x = ctx.Encrypt(sk, X.ravel(), p=p, seed=ctx.seed_after).reshape(X.shape + (w,))
            y = ctx.Encrypt(sk, Y.ravel(), p=p, seed=ctx.seed_after).reshape(Y.shape + (w,))
            luts = tfhe_amd.product_tables(q, p, c["negacyclic"])
            before = ctx.info().bootstraps
            out = ctx.EvalCtMatMul(x, y, luts)
            assert ctx.info().bootstraps - before == (2 if c["negacyclic"] else 4) * 4 * c["K"]
            assert ctx.Decrypt(sk, out.reshape(-1, w), p=p) == [int(v) for v in want.ravel()], name
            e = ctx.EvalCtMul(x.reshape(-1, w), y.reshape(-1, w), luts)
            assert ctx.Decrypt(sk, e, p=p) == [int(v) for v in (X.ravel() * Y.ravel()) % p], name
    finally:
        ctx.GPUClean()
