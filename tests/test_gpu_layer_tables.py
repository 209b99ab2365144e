"""GPU: the dense, convolution and pooling layers with one table per channel (tfhe_eval_dense_tables*,
tfhe_eval_conv2d_tables*, tfhe_eval_pool2d_tables*): column, output plane or plane c uses table c, the
classes cycling over the channels.  Each must equal, bit for bit, the layer's linear part followed by the shared-table
host-array EvalFunc per channel, count its bootstraps, leave its inputs alone, keep the (q,) shape's meaning, refuse a
table count other than the channel count, chain by pointer, and decrypt to the clear-text layer."""
import numpy as np
import pytest

import conv_model
import dense_model
import pool_model
import tables_model

pytestmark = pytest.mark.gpu

KINDS = tables_model.KINDS
PER_CT = {"negacyclic": 1, "periodic": 2, "arbitrary": 2}


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


def _layer(op, seed=31):
    """tests/test_gpu_dense.py's shape: instances = 3, K = 7, cols = CT + 1 (one full column tile and a tail of one)"""
    import tfhe_amd

    cols = tfhe_amd.mm_tiles()[1] + 1
    rs = np.random.default_rng(seed)
    ct = rs.integers(0, op.q, (3, 7, op.n + 1), dtype=np.uint64)
    mat = rs.integers(-8, 8, (7, cols), dtype=np.int64)
    bias = rs.integers(0, op.q, cols, dtype=np.uint64)
    return ct, mat, bias


def _cycle(channels, start=0):
    return [KINDS[(start + c) % 3] for c in range(channels)]


def _out(shape, like):
    """-1 everywhere, one guard row behind the result"""
    import torch

    rows = int(np.prod(shape[:-1]))
    return torch.full((rows + 1, shape[-1]), -1, dtype=torch.int64, device=like.device), rows


def _finish(d_out, rows, shape, inputs):
    import torch

    torch.cuda.synchronize()
    out = _host(d_out)
    assert (out[rows] == np.uint64(2**64 - 1)).all(), "the guard row was written"
    for t, a in inputs:
        assert np.array_equal(_host(t) if a.dtype == np.uint64 else t.cpu().numpy(), a), "an input word was written"
    return out[:rows].reshape(shape)


def _dense_device(ctx, w, ct, mat, luts, bias, q, num_luts=None):
    import torch

    inst, K, cols = ct.shape[0], mat.shape[0], mat.shape[1]
    d_ct, d_m, d_l, d_b = _dev(ct), _dev(mat), _dev(luts), _dev(bias)
    d_out, rows = _out((inst, cols, w), d_ct)
    torch.cuda.synchronize()
    ctx.EvalDenseDevice(inst, K, d_ct.data_ptr(), cols, d_m.data_ptr(), d_l.data_ptr(), d_out.data_ptr(),
                        d_bias=d_b.data_ptr(), q=q, num_luts=luts.shape[0] if num_luts is None else num_luts)
    return _finish(d_out, rows, (inst, cols, w), [(d_ct, ct), (d_m, mat), (d_l, luts), (d_b, bias)])


def _conv_device(ctx, w, d, ct, wt, luts, bias, q, num_luts=None):
    import torch

    import tfhe_amd

    oh, ow, _ = conv_model.shape(d)
    d_ct, d_w, d_l, d_b = _dev(ct), _dev(wt), _dev(luts), _dev(bias)
    shape = (ct.shape[0], d.c_out, oh, ow, w)
    d_out, rows = _out(shape, d_ct)
    torch.cuda.synchronize()
    ctx.EvalConv2dDevice(tfhe_amd.Conv2d(*d), ct.shape[0], d_ct.data_ptr(), d_w.data_ptr(), d_l.data_ptr(),
                         d_out.data_ptr(), d_bias=d_b.data_ptr(), q=q,
                         num_luts=luts.shape[0] if num_luts is None else num_luts)
    return _finish(d_out, rows, shape, [(d_ct, ct), (d_w, wt), (d_l, luts), (d_b, bias)])


def _pool_device(ctx, w, d, ct, luts, q, num_luts=None):
    import torch

    import tfhe_amd

    oh, ow, _, _ = pool_model.shape(d)
    d_ct, d_l = _dev(ct), _dev(luts)
    shape = (ct.shape[0], d.c, oh, ow, w)
    d_out, rows = _out(shape, d_ct)
    torch.cuda.synchronize()
    ctx.EvalPool2dDevice(tfhe_amd.Pool2d(*d), ct.shape[0], d_ct.data_ptr(), d_l.data_ptr(), d_out.data_ptr(), q=q,
                         num_luts=luts.shape[0] if num_luts is None else num_luts)
    return _finish(d_out, rows, shape, [(d_ct, ct), (d_l, luts)])


def _per_channel(eval_func, z, luts, q):
    """z[instances, channels, ..., n+1]: the shared-table eval_func per channel, on that channel's rows."""
    out = np.empty_like(z)
    for c in range(z.shape[1]):
        rows = np.ascontiguousarray(z[:, c]).reshape(-1, z.shape[-1])
        out[:, c] = np.asarray(eval_func(rows, luts[c], q)).reshape(z[:, c].shape)
    return out


def _invalid(call):
    import tfhe_amd as capi

    with pytest.raises(capi.TfheError) as e:
        call()
    assert e.value.status == 1 and "num_luts" in str(e.value)  # TFHE_ERR_INVALID_ARGUMENT


def test_dense(env):
    op, ctx, orc = env
    q, w = op.q, op.n + 1
    ct, mat, bias = _layer(op)
    cols = mat.shape[1]
    kinds = _cycle(cols)
    luts = tables_model.tables(q, kinds)
    before = ctx.info().bootstraps
    got = _dense_device(ctx, w, ct, mat, luts, bias, q)
    assert ctx.info().bootstraps - before == ct.shape[0] * sum(PER_CT[k] for k in kinds)
    z = np.stack([ctx.CiphertextMulMatrix(x, mat, q) for x in ct])
    z[:, :, -1] = (z[:, :, -1] + bias[None, :]) % np.uint64(q)
    assert np.array_equal(got, _per_channel(ctx.EvalFunc, z, luts, q))
    assert np.array_equal(got, ctx.EvalDense(ct, mat, luts, bias=bias, q=q))
    assert np.array_equal(got[-1, -1:], orc.eval_func(z[-1, -1:], luts[-1], q))
    # the (q,) shape keeps its meaning
    assert np.array_equal(ctx.EvalDense(ct, mat, luts[0], bias=bias, q=q), _per_channel(ctx.EvalFunc, z, [luts[0]] * cols, q))
    for n in (cols - 1, cols + 1):
        _invalid(lambda: _dense_device(ctx, w, ct, mat, luts, bias, q, num_luts=n))


@pytest.mark.parametrize("instances", [1, 3])
def test_convolution(env, instances):
    op, ctx, orc = env
    q, w = op.q, op.n + 1
    d = conv_model.desc(2, 4, 5, 3, 3, 3, stride=(1, 2), padding=(1, 1))
    oh, ow, _ = conv_model.shape(d)
    rs = np.random.default_rng(101 + instances)
    ct = rs.integers(0, q, (instances, d.c_in, d.h, d.w, w), dtype=np.uint64)
    wt = rs.integers(-4, 4, (d.c_out, d.c_in, d.kh, d.kw), dtype=np.int64)
    bias = rs.integers(0, q, d.c_out, dtype=np.uint64)
    kinds = _cycle(d.c_out, start=1)  # one class per plane
    luts = tables_model.tables(q, kinds)
    before = ctx.info().bootstraps
    got = _conv_device(ctx, w, d, ct, wt, luts, bias, q)
    assert ctx.info().bootstraps - before == instances * oh * ow * sum(PER_CT[k] for k in kinds)
    import torch

    import tfhe_amd

    d_ct, d_w, d_b = _dev(ct), _dev(wt), _dev(bias)
    d_z = torch.empty((instances, d.c_out, oh, ow, w), dtype=torch.int64, device=d_ct.device)
    ctx.CiphertextConv2dDevice(tfhe_amd.Conv2d(*d), instances, d_ct.data_ptr(), d_w.data_ptr(), q, d_z.data_ptr(),
                               d_bias=d_b.data_ptr())
    torch.cuda.synchronize()
    z = _host(d_z)
    assert np.array_equal(got, _per_channel(ctx.EvalFunc, z, luts, q))
    kw = dict(stride=(d.stride_h, d.stride_w), padding=(d.pad_h, d.pad_w))
    assert np.array_equal(got, ctx.EvalConv2d(ct, wt, luts, bias=bias, q=q, **kw))
    assert np.array_equal(got[-1, -1, -1, -1:], orc.eval_func(z[-1, -1, -1, -1:], luts[-1], q))
    assert np.array_equal(ctx.EvalConv2d(ct, wt, luts[1], bias=bias, q=q, **kw),
                          _per_channel(ctx.EvalFunc, z, [luts[1]] * d.c_out, q))
    for n in (d.c_out - 1, d.c_out + 1):
        _invalid(lambda: _conv_device(ctx, w, d, ct, wt, luts, bias, q, num_luts=n))


# 3 x 3 stride 2 padding 1 on 5 x 4 (odd carries; positions with 4, 6 and 9 valid taps) and 2 x 2 stride 2 on 4 x 4
POOLS = [pool_model.desc(3, 5, 4, 3, 3, stride=(2, 2), padding=(1, 1)), pool_model.desc(3, 4, 4, 2, 2)]


def _pool_per_plane(eval_func, ct, d, luts, q):
    """tests/pool_model.py's tournament, func_pair called per plane on that plane's table"""
    one = pool_model.desc(1, d.h, d.w, d.kh, d.kw, (d.stride_h, d.stride_w), (d.pad_h, d.pad_w))
    return np.concatenate([pool_model.pool2d(ct[:, c:c + 1], one, pool_model.func_pair(eval_func, luts[c], q))
                           for c in range(d.c)], axis=1)


@pytest.mark.parametrize("instances", [1, 3])
@pytest.mark.parametrize("d", POOLS, ids=["3x3s2p1", "2x2s2"])
def test_pooling(env, d, instances):
    op, ctx, orc = env
    q, w = op.q, op.n + 1
    kinds = _cycle(d.c, start=2)  # one class per plane
    luts = tables_model.tables(q, kinds)
    ct = np.random.default_rng(103 + instances).integers(0, q, (instances, d.c, d.h, d.w, w), dtype=np.uint64)
    pairs = pool_model.shape(d)[3]
    before = ctx.info().bootstraps
    got = _pool_device(ctx, w, d, ct, luts, q)
    assert ctx.info().bootstraps - before == instances * pairs * sum(PER_CT[k] for k in kinds)
    assert np.array_equal(got, _pool_per_plane(ctx.EvalFunc, ct, d, luts, q))
    kw = dict(kernel=(d.kh, d.kw), stride=(d.stride_h, d.stride_w), padding=(d.pad_h, d.pad_w))
    assert np.array_equal(got, ctx.EvalPool2d(ct, luts, q=q, **kw))
    if instances == 1:
        assert np.array_equal(ctx.EvalPool2d(ct, luts[0], q=q, **kw), _pool_per_plane(ctx.EvalFunc, ct, d, [luts[0]] * d.c, q))
        for n in (d.c - 1, d.c + 1):
            _invalid(lambda: _pool_device(ctx, w, d, ct, luts, q, num_luts=n))


def test_chains_by_pointer(shared_kat):
    """EvalConv2dDevice -> EvalPool2dDevice -> EvalDenseDevice by pointer, each with one table per channel (STD128):
    1 -> 2 planes of 3 x 3 by a 2 x 2 window; a 1 x 2 pool: 2 x 2 x 1 = 4 results; 4 -> 2 dense.  The first and last
    rows of every stage against the oracle."""
    import torch

    import tfhe_amd

    s = shared_kat("STD128")
    op, ctx, orc = s["op"], s["ctx"], s["orc"]
    q, w = op.q, op.n + 1
    rs = np.random.default_rng(105)
    dc, dp = conv_model.desc(1, 3, 3, 2, 2, 2), pool_model.desc(2, 2, 2, 1, 2)
    ct = rs.integers(0, q, (1, 1, 3, 3, w), dtype=np.uint64)
    wt, mat = rs.integers(-4, 4, (2, 1, 2, 2), dtype=np.int64), rs.integers(-4, 4, (4, 2), dtype=np.int64)
    bc, bd = (rs.integers(0, q, 2, dtype=np.uint64) for _ in range(2))
    lc, lp, ld = (tables_model.tables(q, k) for k in (["periodic", "negacyclic"], ["negacyclic", "arbitrary"],
                                                      ["arbitrary", "periodic"]))
    d_ct, d_wt, d_m, d_bc, d_bd, d_lc, d_lp, d_ld = (_dev(a) for a in (ct, wt, mat, bc, bd, lc, lp, ld))
    d_y = torch.full((1, 2, 2, 2, w), -1, dtype=torch.int64, device=d_ct.device)
    d_p = torch.full((1, 2, 2, 1, w), -1, dtype=torch.int64, device=d_ct.device)
    d_o = torch.full((1, 2, w), -1, dtype=torch.int64, device=d_ct.device)
    torch.cuda.synchronize()
    ctx.EvalConv2dDevice(tfhe_amd.Conv2d(*dc), 1, d_ct.data_ptr(), d_wt.data_ptr(), d_lc.data_ptr(), d_y.data_ptr(),
                         d_bias=d_bc.data_ptr(), num_luts=2)
    ctx.EvalPool2dDevice(tfhe_amd.Pool2d(*dp), 1, d_y.data_ptr(), d_lp.data_ptr(), d_p.data_ptr(), num_luts=2)
    ctx.EvalDenseDevice(1, 4, d_p.data_ptr(), 2, d_m.data_ptr(), d_ld.data_ptr(), d_o.data_ptr(), d_bias=d_bd.data_ptr(),
                        num_luts=2)
    torch.cuda.synchronize()
    y, p, o = _host(d_y), _host(d_p), _host(d_o)
    z = conv_model.conv2d(ct, wt, q, dc, bc)
    for c, pos in ((0, (0, 0)), (1, (1, 1))):
        assert np.array_equal(y[0, c][pos][None], orc.eval_func(z[0, c][pos][None], lc[c], q))
    for c, row in ((0, 0), (1, 1)):  # one round: op(a, b) = b + EvalFunc(a - b) on the plane's table
        pair = pool_model.func_pair(orc.eval_func, lp[c], q)
        assert np.array_equal(p[0, c, row, 0][None], pair(y[0, c, row, 0][None], y[0, c, row, 1][None]))
    zd = dense_model.product(p.reshape(1, 4, w), mat, q, bd)
    for c in (0, 1):
        assert np.array_equal(o[0, c][None], orc.eval_func(zd[0, c][None], ld[c], q))


def test_decrypts_to_the_clear_layer():
    """tests/dense_model.py's decrypting layer on a from_keygen context, column c's table the cube composed with
    m -> (m + c) mod p: every output is the clear-text layer's, and the columns' tables differ where it matters."""
    import tfhe_amd

    d = dense_model.DECRYPT_CASE
    msgs, matrix, bias_msgs, f = dense_model.decrypt_case()
    cp = tfhe_amd.params_from_set(d["paramset"])
    p, q, w = d["p"], cp.q, cp.n + 1
    luts = np.stack([np.array([f((v // (q // p) + c) % p) * (q // p) for v in range(q)], dtype=np.uint64)
                     for c in range(d["cols"])])
    ctx, sk = tfhe_amd.BinFHEContextHIP.from_keygen(cp, d["key_seed"])
    try:
        cts = ctx.Encrypt(sk, msgs.ravel(), p=p, seed=ctx.seed_after).reshape(d["instances"], d["K"], w)
        bias = bias_msgs.astype(np.uint64) * np.uint64(q // p)
        out = ctx.EvalDense(cts, matrix, luts, bias=bias)
        got = ctx.Decrypt(sk, out.reshape(-1, w), p=p)
    finally:
        ctx.GPUClean()
    want = [[f((m + c) % p) for c, m in enumerate(row)] for row in dense_model.clear_layer(msgs, matrix, bias_msgs, int, p)]
    flat = [v for row in want for v in row]
    assert got == flat
    shared = [v for row in dense_model.clear_layer(msgs, matrix, bias_msgs, f, p) for v in row]
    assert flat != shared  # not constant across columns: the shared cube would decrypt differently
