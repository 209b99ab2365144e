"""GPU: the convolution layer y = f(conv(x) + b) on encrypted x (tfhe_eval_conv2d_device / tfhe_eval_conv2d): the
gathered product at modulus q, the bias on the b word, then EvalFunc with one shared table over the
instances * c_out * oh * ow results, every intermediate in HBM.  It must equal, bit for bit, the composition of the
host-array calls (im2col on the host, CiphertextMulMatrix per group, the bias, EvalFunc, a transpose) and the model of
tests/conv_model.py through the oracle, for the three table classes of checkInputFunction, on STD128 and the arbFunc
logQ = 12 context; it must slice a batch beyond 65,536, count its bootstraps like EvalFunc, chain into a dense
layer and into a second convolution without a relayout, and decrypt to the clear-text layer."""
import numpy as np
import pytest

import conv_model
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


def _layer(op, seed=51):
    """Two instances, 4 planes of 2 x 3, a 2 x 2 window with padding (1, 0): 3 x 2 positions; two groups of CT + 1
    output planes (one full tile and a tail of one in each); random ciphertexts mod q."""
    import tfhe_amd

    Og = tfhe_amd.conv2d_tiles()[1] + 1
    d = conv_model.desc(4, 2, 3, 2 * Og, 2, 2, padding=(1, 0), groups=2)
    rs = np.random.default_rng(seed)
    ct = rs.integers(0, op.q, (2, d.c_in, d.h, d.w, op.n + 1), dtype=np.uint64)
    wt = rs.integers(-8, 8, (d.c_out, d.c_in // d.groups, d.kh, d.kw), dtype=np.int64)
    bias = rs.integers(0, op.q, d.c_out, dtype=np.uint64)
    return d, ct, wt, bias


def _conv_device(ctx, w, d, ct, wt, lut, bias, q):
    import torch

    import tfhe_amd

    oh, ow, _ = conv_model.shape(d)
    d_ct, d_w, d_l = _dev(ct), _dev(wt), _dev(lut)
    d_b = _dev(bias) if bias is not None else None
    d_out = torch.full((ct.shape[0], d.c_out, oh, ow, w), -1, dtype=torch.int64, device=d_ct.device)
    torch.cuda.synchronize()
    ctx.EvalConv2dDevice(tfhe_amd.Conv2d(*d), ct.shape[0], d_ct.data_ptr(), d_w.data_ptr(), d_l.data_ptr(),
                         d_out.data_ptr(), d_bias=d_b.data_ptr() if d_b is not None else 0, q=q)
    torch.cuda.synchronize()
    return _host(d_out)


def _kw(d):
    return dict(stride=(d.stride_h, d.stride_w), padding=(d.pad_h, d.pad_w), groups=d.groups)


@pytest.mark.parametrize("kind", KINDS)
def test_layer_equals_composition_and_model(env, kind):
    op, ctx, orc = env
    q, w = op.q, op.n + 1
    if kind == "arbitrary" and q > op.N:
        pytest.skip("arbitrary LUTs need q <= N")
    d, ct, wt, bias = _layer(op)
    lut = _luts(q)[kind]
    oh, ow, K = conv_model.shape(d)
    Og, inst = d.c_out // d.groups, ct.shape[0]
    total = inst * d.c_out * oh * ow
    before = ctx.info().bootstraps
    got = _conv_device(ctx, w, d, ct, wt, lut, bias, q)
    assert ctx.info().bootstraps - before == BOOTSTRAPS_PER_CT[kind] * total  # what EvalFunc on that many adds
    assert np.array_equal(got, ctx.EvalConv2d(ct, wt, lut, bias=bias, q=q, **_kw(d)))
    # the host-array composition: im2col, CiphertextMulMatrix per group (and per position: it takes one input set),
    # the bias added to b, one EvalFunc over position-major rows, a transpose to plane-major order
    cols = conv_model.im2col(ct, d)  # [inst, npos, groups, K, w]
    z = np.empty((inst, oh * ow, d.c_out, w), dtype=np.uint64)
    for i in range(inst):
        for pos in range(oh * ow):
            for g in range(d.groups):
                mat = wt[g * Og:(g + 1) * Og].reshape(Og, K).T
                z[i, pos, g * Og:(g + 1) * Og] = ctx.CiphertextMulMatrix(cols[i, pos, g], mat, q)
    z[..., -1] = (z[..., -1] + bias[None, None, :]) % np.uint64(q)
    comp = ctx.EvalFunc(z.reshape(-1, w), lut, q).reshape(z.shape).transpose(0, 2, 1, 3)
    assert np.array_equal(got.reshape(inst, d.c_out, oh * ow, w), comp)
    # the first and the last result through the model and the oracle
    zm = conv_model.conv2d(ct, wt, q, d, bias).reshape(-1, w)
    assert np.array_equal(zm.reshape(inst, d.c_out, oh * ow, w), z.transpose(0, 2, 1, 3))
    idx = [0, total - 1]
    assert np.array_equal(got.reshape(-1, w)[idx], orc.eval_func(zm[idx], lut, q))


def test_arbitrary_table_needs_q_up_to_N(env):
    """q = 2N with an arbitrary-class table: TFHE_ERR_UNSUPPORTED before anything is launched, and the bootstraps
    counter does not move."""
    import tfhe_amd as capi

    op, ctx, _ = env
    q = 2 * op.N
    d, ct, wt, bias = _layer(op)
    lut = _luts(q)["arbitrary"]
    before = ctx.info().bootstraps
    for call in (lambda: _conv_device(ctx, op.n + 1, d, ct, wt, lut, bias, q),
                 lambda: ctx.EvalConv2d(ct, wt, lut, bias=bias, q=q, **_kw(d))):
        with pytest.raises(capi.TfheError) as e:
            call()
        assert e.value.status == 2  # TFHE_ERR_UNSUPPORTED
    assert ctx.info().bootstraps == before


def test_no_bias_equals_zero_bias_and_one_instance_keeps_its_shape(env):
    op, ctx, _ = env
    d, ct, wt, _ = _layer(op, seed=52)
    lut = _luts(op.q)["negacyclic"]
    zero = np.zeros(d.c_out, dtype=np.uint64)
    a = _conv_device(ctx, op.n + 1, d, ct, wt, lut, None, op.q)
    assert np.array_equal(a, _conv_device(ctx, op.n + 1, d, ct, wt, lut, zero, op.q))
    assert np.array_equal(a, ctx.EvalConv2d(ct, wt, lut, **_kw(d)))
    one = ctx.EvalConv2d(ct[0], wt, lut, bias=zero, **_kw(d))  # [C, H, W, n+1] -> [C_out, oh, ow, n+1]
    assert one.shape == a.shape[1:] and np.array_equal(one, a[0])


def test_shape_and_argument_errors(env):
    import tfhe_amd as capi

    op, ctx, _ = env
    d, ct, wt, bias = _layer(op)
    lut = _luts(op.q)["negacyclic"]
    kw = _kw(d)
    with pytest.raises(ValueError):
        ctx.EvalConv2d(ct[:, :3], wt, lut, **kw)  # planes against weight and groups
    with pytest.raises(ValueError):
        ctx.EvalConv2d(ct[..., :-1], wt, lut, **kw)  # ciphertext width
    with pytest.raises(ValueError):
        ctx.EvalConv2d(ct, wt, lut[:-1], **kw)
    with pytest.raises(ValueError):
        ctx.EvalConv2d(ct, wt, lut, bias=bias[:-1], **kw)
    with pytest.raises(ValueError):
        ctx.EvalConv2d(ct, wt[:, :, :0], lut, **kw)
    with pytest.raises(ValueError):
        ctx.EvalConv2d(ct, wt, lut, stride=0, padding=kw["padding"], groups=2)
    with pytest.raises(ValueError):
        ctx.EvalConv2d(ct, wt, lut, padding=(2, 0), groups=2)  # pad_h >= kh
    # stride and padding as one int
    a = ctx.EvalConv2d(ct, wt, lut, stride=1, padding=1, groups=2)
    assert np.array_equal(a, ctx.EvalConv2d(ct, wt, lut, stride=(1, 1), padding=(1, 1), groups=2))
    t = _dev(ct)
    desc = capi.Conv2d(*d)
    for q in (4, 3 * 256, 4 * op.N):  # below 8; no power of two; not a divisor of 2N
        with pytest.raises(capi.TfheError) as e:
            ctx.EvalConv2dDevice(desc, 2, t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), q=q)
        assert e.value.status == 1 and "q" in str(e.value), q  # TFHE_ERR_INVALID_ARGUMENT
    with pytest.raises(capi.TfheError) as e:
        ctx.EvalConv2dDevice(desc, 2, t.data_ptr(), t.data_ptr(), 0, t.data_ptr())  # null table
    assert e.value.status == 1 and "lut" in str(e.value)


def test_slices_beyond_the_chunk(shared_kat):
    """70,001 results on STD128 (c_in = c_out = 1, h = 1, w = 70001, a 1 x 1 window): the positions cross any 65,535
    grid limit and EvalFunc runs in two slices, cut at 65,536.  Compared with CiphertextMulMatrixDevice (70,001 input
    sets of K = 1) and EvalFuncDevice in two calls: samples on both sides of the cut, and the FNV digest."""
    import torch

    import pyoracle
    import tfhe_amd

    s = shared_kat("STD128")
    op, ctx, orc = s["op"], s["ctx"], s["orc"]
    q, w, npos, cut = op.q, op.n + 1, 70001, 65536
    d = conv_model.desc(1, 1, npos, 1, 1, 1)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(53)
    d_ct = torch.randint(0, q, (1, 1, 1, npos, w), dtype=torch.int64, device="cuda", generator=gen)
    wt, bias, lut = np.array([[[[-3]]]], dtype=np.int64), np.array([q - 5], dtype=np.uint64), _luts(q)["negacyclic"]
    d_w, d_b, d_l = _dev(wt), _dev(bias), _dev(lut)
    d_out = torch.full((npos, w), -1, dtype=torch.int64, device=d_ct.device)
    d_z, d_ref = torch.empty_like(d_out), torch.empty_like(d_out)
    torch.cuda.synchronize()
    before = ctx.info().bootstraps
    ctx.EvalConv2dDevice(tfhe_amd.Conv2d(*d), 1, d_ct.data_ptr(), d_w.data_ptr(), d_l.data_ptr(), d_out.data_ptr(),
                         d_bias=d_b.data_ptr())
    torch.cuda.synchronize()
    assert ctx.info().bootstraps - before == npos
    ctx.CiphertextMulMatrixDevice(npos, 1, d_ct.data_ptr(), 1, d_w.data_ptr(), q, d_z.data_ptr(), d_bias=d_b.data_ptr())
    for first, cnt in ((0, cut), (cut, npos - cut)):
        ctx.EvalFuncDevice(cnt, d_z[first:].data_ptr(), d_l.data_ptr(), d_ref[first:].data_ptr())
    torch.cuda.synchronize()
    idx = [0, cut - 1, cut, npos - 1]
    got = _host(d_out[idx])
    assert np.array_equal(got, _host(d_ref[idx]))
    zm = conv_model.conv2d(_host(d_ct[0, :, :, idx]), wt, q, conv_model.desc(1, 1, len(idx), 1, 1, 1), bias)
    assert np.array_equal(zm.reshape(len(idx), w), _host(d_z[idx]))
    assert np.array_equal(got, orc.eval_func(_host(d_z[idx]), lut, q))
    assert torch.equal(d_out, d_ref)
    assert pyoracle.fnv1a64(_host(d_out).ravel()) == pyoracle.fnv1a64(_host(d_ref).ravel())


def test_chains_without_a_relayout(shared_kat):
    """The output pointer of a convolution passed to EvalDenseDevice as [instances][c_out oh ow][n+1] and to a second
    convolution as [instances][c_out][oh][ow][n+1] equals the model of each chain through the oracle (STD128, a
    negacyclic table).  1 -> 2 planes of 3 x 3 by a 2 x 2 window: 2 x 2 x 2 = 8 results; then 8 -> 2 dense, and a
    2 x 2 window over the 2 planes of 2 x 2: 2 x 1 x 1."""
    import torch

    import tfhe_amd

    s = shared_kat("STD128")
    op, ctx, orc = s["op"], s["ctx"], s["orc"]
    q, w = op.q, op.n + 1
    rs = np.random.default_rng(54)
    d1, d2 = conv_model.desc(1, 3, 3, 2, 2, 2), conv_model.desc(2, 2, 2, 2, 2, 2)
    ct = rs.integers(0, q, (1, 1, 3, 3, w), dtype=np.uint64)
    w1, w2 = rs.integers(-4, 4, (2, 1, 2, 2), dtype=np.int64), rs.integers(-4, 4, (2, 2, 2, 2), dtype=np.int64)
    mat = rs.integers(-4, 4, (8, 2), dtype=np.int64)
    b1, b2, bd = (rs.integers(0, q, 2, dtype=np.uint64) for _ in range(3))
    lut = _luts(q)["negacyclic"]
    d_ct, d_w1, d_w2, d_m, d_b1, d_b2, d_bd, d_l = (_dev(a) for a in (ct, w1, w2, mat, b1, b2, bd, lut))
    d_y1 = torch.full((1, 2, 2, 2, w), -1, dtype=torch.int64, device=d_ct.device)
    d_dense = torch.full((1, 2, w), -1, dtype=torch.int64, device=d_ct.device)
    d_y2 = torch.full((1, 2, 1, 1, w), -1, dtype=torch.int64, device=d_ct.device)
    torch.cuda.synchronize()
    ctx.EvalConv2dDevice(tfhe_amd.Conv2d(*d1), 1, d_ct.data_ptr(), d_w1.data_ptr(), d_l.data_ptr(), d_y1.data_ptr(),
                         d_bias=d_b1.data_ptr())
    ctx.EvalDenseDevice(1, 8, d_y1.data_ptr(), 2, d_m.data_ptr(), d_l.data_ptr(), d_dense.data_ptr(),
                        d_bias=d_bd.data_ptr())
    ctx.EvalConv2dDevice(tfhe_amd.Conv2d(*d2), 1, d_y1.data_ptr(), d_w2.data_ptr(), d_l.data_ptr(), d_y2.data_ptr(),
                         d_bias=d_b2.data_ptr())
    torch.cuda.synchronize()
    y1 = conv_model.conv_layer(orc, ct, w1, lut, d1, b1, q)
    assert np.array_equal(_host(d_y1), y1)
    assert np.array_equal(_host(d_dense), dense_model.dense(orc, y1.reshape(1, 8, w), mat, lut, bd, q))
    assert np.array_equal(_host(d_y2), conv_model.conv_layer(orc, y1, w2, lut, d2, b2, q))


def test_decrypts_to_the_clear_layer():
    """tests/test_conv_cpu.py's decrypting case on a from_keygen context: Encrypt -> EvalConv2d -> Decrypt equals the
    clear-text layer for every output."""
    import tfhe_amd

    c = conv_model.CONV_DECRYPT_CASE
    d = c["desc"]
    msgs, weight, bias_msgs, f = conv_model.conv_decrypt_case()
    cp = tfhe_amd.params_from_set(c["paramset"])
    p, q, w = c["p"], cp.q, cp.n + 1
    ctx, sk = tfhe_amd.BinFHEContextHIP.from_keygen(cp, c["key_seed"])
    try:
        cts = ctx.Encrypt(sk, msgs.ravel(), p=p, seed=ctx.seed_after).reshape(msgs.shape + (w,))
        bias = bias_msgs.astype(np.uint64) * np.uint64(q // p)
        out = ctx.EvalConv2d(cts, weight, cube_lut(q, p), bias=bias, stride=(d.stride_h, d.stride_w),
                             padding=(d.pad_h, d.pad_w), groups=d.groups)
        got = ctx.Decrypt(sk, out.reshape(-1, w), p=p)
    finally:
        ctx.GPUClean()
    want = conv_model.clear_conv(msgs, weight, bias_msgs, f, p, d)
    flat = [v for inst in want for plane in inst for row in plane for v in row]
    assert len(flat) == 16 and got == flat
