"""GPU: the dense layer y = f(W^T x + b) on encrypted x (tfhe_eval_dense_device / tfhe_eval_dense): the tiled matrix
product at modulus q, the bias on the b word, then EvalFunc with one shared table over the instances * cols results,
every intermediate in HBM.  It must equal, bit for bit, the composition of the host-array calls and the model of
tests/dense_model.py through the oracle, for the three table classes of checkInputFunction, on STD128 (fast4) and the
arbFunc logQ = 12 context (sf2); it must slice a batch beyond 65,536 like a circuit level,
count its bootstraps like EvalFunc, and decrypt to the clear-text layer."""
import numpy as np
import pytest

import dense_model
from helpers import cube_lut

pytestmark = pytest.mark.gpu

KINDS = ["negacyclic", "periodic", "arbitrary"]
BOOTSTRAPS_PER_CT = {"negacyclic": 1, "periodic": 2, "arbitrary": 2}


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


def _luts(q):
    h = q // 2  # lut[i] == q - lut[h + i] for every i < h (checkInputFunction's negacyclic test)
    neg = np.array([1 + (3 * x) % (q - 1) if x < h else q - 1 - (3 * (x - h)) % (q - 1) for x in range(q)],
                   dtype=np.uint64)
    per = np.array([(x * 5) % (q // 2) for x in range(q)], dtype=np.uint64)
    return {"negacyclic": neg, "periodic": per, "arbitrary": cube_lut(q)}


def _layer(op, seed=31):
    """instances = 3, K = 7, cols = CT + 1 (one full column tile and a tail of one), random ciphertexts mod q"""
    import tfhe_amd

    cols = tfhe_amd.mm_tiles()[1] + 1
    rs = np.random.default_rng(seed)
    ct = rs.integers(0, op.q, (3, 7, op.n + 1), dtype=np.uint64)
    mat = rs.integers(-8, 8, (7, cols), dtype=np.int64)
    bias = rs.integers(0, op.q, cols, dtype=np.uint64)
    return ct, mat, bias


def _dense_device(ctx, w, ct, mat, lut, bias, q):
    import torch

    inst, K, cols = ct.shape[0], mat.shape[0], mat.shape[1]
    d_ct, d_m, d_l = _dev(ct), _dev(mat), _dev(lut)
    d_b = _dev(bias) if bias is not None else None
    d_out = torch.full((inst, cols, w), -1, dtype=torch.int64, device=d_ct.device)
    torch.cuda.synchronize()
    ctx.EvalDenseDevice(inst, K, d_ct.data_ptr(), cols, d_m.data_ptr(), d_l.data_ptr(), d_out.data_ptr(),
                        d_bias=d_b.data_ptr() if d_b is not None else 0, q=q)
    torch.cuda.synchronize()
    return _host(d_out)


@pytest.mark.parametrize("kind", KINDS)
def test_dense_equals_composition_and_model(env, kind):
    op, ctx, orc = env
    q, w = op.q, op.n + 1
    if kind == "arbitrary" and q > op.N:
        pytest.skip("arbitrary LUTs need q <= N")
    ct, mat, bias = _layer(op)
    lut = _luts(q)[kind]
    before = ctx.info().bootstraps
    got = _dense_device(ctx, w, ct, mat, lut, bias, q)
    total = ct.shape[0] * mat.shape[1]
    assert ctx.info().bootstraps - before == BOOTSTRAPS_PER_CT[kind] * total  # what EvalFunc on that many adds
    assert np.array_equal(got, ctx.EvalDense(ct, mat, lut, bias=bias, q=q))
    # the host-array composition: CiphertextMulMatrix per instance, the bias added to b, one EvalFunc
    z = np.stack([ctx.CiphertextMulMatrix(x, mat, q) for x in ct])
    z[:, :, -1] = (z[:, :, -1] + bias[None, :]) % np.uint64(q)
    comp = ctx.EvalFunc(z.reshape(-1, w), lut, q).reshape(z.shape)
    assert np.array_equal(got, comp)
    # rows 0 and last through the model and the oracle
    zm = dense_model.product(ct, mat, q, bias).reshape(-1, w)
    assert np.array_equal(zm, z.reshape(-1, w))
    idx = [0, total - 1]
    assert np.array_equal(got.reshape(-1, w)[idx], orc.eval_func(zm[idx], lut, q))


def test_arbitrary_table_needs_q_up_to_N(env):
    """q = 2N (a valid ciphertext modulus, above N) with an arbitrary-class table: TFHE_ERR_UNSUPPORTED before
    anything is launched, and the bootstraps counter does not move.  (Both shared contexts have q <= N, so the
    three classes above all run there.)"""
    import tfhe_amd as capi

    op, ctx, _ = env
    q = 2 * op.N
    ct, mat, bias = _layer(op)
    lut = _luts(q)["arbitrary"]
    before = ctx.info().bootstraps
    for call in (lambda: _dense_device(ctx, op.n + 1, ct, mat, lut, bias, q),
                 lambda: ctx.EvalDense(ct, mat, lut, bias=bias, q=q)):
        with pytest.raises(capi.TfheError) as e:
            call()
        assert e.value.status == 2  # TFHE_ERR_UNSUPPORTED
    assert ctx.info().bootstraps == before


def test_no_bias_equals_zero_bias(env):
    op, ctx, _ = env
    ct, mat, _ = _layer(op, seed=32)
    lut = _luts(op.q)["negacyclic"]
    zero = np.zeros(mat.shape[1], dtype=np.uint64)
    a = _dense_device(ctx, op.n + 1, ct, mat, lut, None, op.q)
    assert np.array_equal(a, _dense_device(ctx, op.n + 1, ct, mat, lut, zero, op.q))
    assert np.array_equal(a, ctx.EvalDense(ct, mat, lut))
    assert np.array_equal(a[0], ctx.EvalDense(ct[0], mat, lut, bias=zero))  # one instance: [K, n+1] -> [cols, n+1]


def test_shape_and_argument_errors(env):
    import tfhe_amd as capi

    op, ctx, _ = env
    ct, mat, bias = _layer(op)
    lut = _luts(op.q)["negacyclic"]
    with pytest.raises(ValueError):
        ctx.EvalDense(ct[:, :6], mat, lut)  # K mismatch
    with pytest.raises(ValueError):
        ctx.EvalDense(ct, mat, lut[:-1])
    with pytest.raises(ValueError):
        ctx.EvalDense(ct, mat, lut, bias=bias[:-1])
    with pytest.raises(ValueError):
        ctx.EvalDense(ct, mat[:, :0], lut)
    d = _dev(ct)
    for q in (4, 3 * 256, 4 * op.N):  # below 8; no power of two; not a divisor of 2N
        with pytest.raises(capi.TfheError) as e:
            ctx.EvalDenseDevice(3, 7, d.data_ptr(), mat.shape[1], d.data_ptr(), d.data_ptr(), d.data_ptr(), q=q)
        assert e.value.status == 1, q  # TFHE_ERR_INVALID_ARGUMENT
    with pytest.raises(capi.TfheError) as e:
        ctx.EvalDenseDevice(3, 7, d.data_ptr(), mat.shape[1], d.data_ptr(), 0, d.data_ptr())  # null table
    assert e.value.status == 1


def test_host_block_sum_overflow_is_refused(env):
    """Sizes whose every product passes the matrix-product checks but whose sum, the one block
    ct | matrix | bias | lut | out of the host-array form, leaves size_t in bytes: refused as an argument error
    before anything is allocated or copied (the arrays passed are far smaller than the sizes claim), and the
    bootstraps counter does not move."""
    op, ctx, _ = env
    q, w = op.q, op.n + 1
    lim = (2**64 - 1) // 8  # words whose bytes fit size_t
    K = cols = 2**30
    instances = lim // w // K  # the most the per-product checks admit
    wi, wm, wl, wo = instances * K * w, K * cols, q, instances * cols * w
    assert instances >= 1 and max(wi, wm, wo, K * w, cols * w) <= lim  # each product fits ...
    assert wi + wm + cols + wl + wo > lim  # ... their sum does not
    ct = np.zeros((1, 1, w), dtype=np.uint64)
    mat = np.zeros((1, 1), dtype=np.int64)
    out = np.zeros((1, 1, w), dtype=np.uint64)
    lut = _luts(q)["negacyclic"]
    L = ctx._L
    before = ctx.info().bootstraps
    assert L.tfhe_eval_dense(ctx._h, instances, K, ct.ravel(), cols, mat.ravel(), None, q, lut, out.ravel()) == 1
    assert b"EvalDense: sizes overflow" in L.tfhe_last_error()
    assert ctx.info().bootstraps == before
    assert not out.any()


def test_slices_beyond_the_chunk(shared_kat):
    """70,001 results on STD128 (K = 2, one instance): EvalFunc runs in two slices, cut at 65,536 like a circuit
    level (the scratch never exceeds max_chunk, so no smaller batch crosses a slice).  Compared with EvalFuncDevice
    on the same z, itself in two calls of at most 65,536: samples on both sides of the cut, and the FNV digest."""
    import torch

    s = shared_kat("STD128")
    op, ctx, orc = s["op"], s["ctx"], s["orc"]
    q, w, cols, cut = op.q, op.n + 1, 70001, 65536
    rs = np.random.default_rng(33)
    ct = rs.integers(0, q, (1, 2, w), dtype=np.uint64)
    mat = rs.integers(-8, 8, (2, cols), dtype=np.int64)
    bias = rs.integers(0, q, cols, dtype=np.uint64)
    lut = _luts(q)["negacyclic"]
    d_ct, d_m, d_b, d_l = _dev(ct), _dev(mat), _dev(bias), _dev(lut)
    d_out = torch.full((cols, w), -1, dtype=torch.int64, device=d_ct.device)
    d_z, d_ref = torch.empty_like(d_out), torch.empty_like(d_out)
    torch.cuda.synchronize()
    before = ctx.info().bootstraps
    ctx.EvalDenseDevice(1, 2, d_ct.data_ptr(), cols, d_m.data_ptr(), d_l.data_ptr(), d_out.data_ptr(),
                        d_bias=d_b.data_ptr())
    torch.cuda.synchronize()
    assert ctx.info().bootstraps - before == cols
    ctx.CiphertextMulMatrixDevice(1, 2, d_ct.data_ptr(), cols, d_m.data_ptr(), q, d_z.data_ptr(), d_bias=d_b.data_ptr())
    for first, cnt in ((0, cut), (cut, cols - cut)):
        ctx.EvalFuncDevice(cnt, d_z[first:].data_ptr(), d_l.data_ptr(), d_ref[first:].data_ptr())
    torch.cuda.synchronize()
    idx = [0, cut - 1, cut, cols - 1]
    got = _host(d_out[idx])
    assert np.array_equal(got, _host(d_ref[idx]))
    assert np.array_equal(got, orc.eval_func(_host(d_z[idx]), lut, q))
    assert torch.equal(d_out, d_ref)
    import pyoracle

    assert pyoracle.fnv1a64(_host(d_out).ravel()) == pyoracle.fnv1a64(_host(d_ref).ravel())


def test_decrypts_to_the_clear_layer():
    """tests/test_dense_cpu.py's decrypting case on a from_keygen context: Encrypt -> EvalDense -> Decrypt equals the
    clear-text layer for every output."""
    import tfhe_amd

    d = dense_model.DECRYPT_CASE
    msgs, matrix, bias_msgs, f = dense_model.decrypt_case()
    cp = tfhe_amd.params_from_set(d["paramset"])
    p, q, w = d["p"], cp.q, cp.n + 1
    ctx, sk = tfhe_amd.BinFHEContextHIP.from_keygen(cp, d["key_seed"])
    try:
        cts = ctx.Encrypt(sk, msgs.ravel(), p=p, seed=ctx.seed_after).reshape(d["instances"], d["K"], w)
        bias = bias_msgs.astype(np.uint64) * np.uint64(q // p)
        out = ctx.EvalDense(cts, matrix, cube_lut(q, p), bias=bias)
        got = ctx.Decrypt(sk, out.reshape(-1, w), p=p)
    finally:
        ctx.GPUClean()
    want = dense_model.clear_layer(msgs, matrix, bias_msgs, f, p)
    assert got == [v for row in want for v in row]
