"""GPU: the pooling layer (tfhe_eval_pool2d_device / tfhe_eval_pool2d): a windowed pair tournament whose
pair step op(a, b) = b + EvalFunc(a - b) is one shared-table EvalFunc, every round's pairs one flat batch, every
intermediate in HBM.  It must equal, bit for bit, the same tournament composed of host-array EvalFunc calls
(tests/pool_model.py with ctx.EvalFunc) and, through the model, the oracle -- for the three table classes of
checkInputFunction, on STD128 and the arbFunc logQ = 12 context; it must count its bootstraps, slice a round beyond
65,536 pairs, write no input word and nothing past its output, order two streams, chain from a convolution into a
dense layer by pointer, and decrypt to the clear-text network."""
import numpy as np
import pytest

import conv_model
import dense_model
import pool_model
from helpers import cube_lut

pytestmark = pytest.mark.gpu

KINDS = ["negacyclic", "periodic", "arbitrary"]
BOOTSTRAPS_PER_PAIR = {"negacyclic": 1, "periodic": 2, "arbitrary": 2}

# 2 x 2 stride 2 on 4 x 4; 3 x 3 stride 2 padding 1 on 5 x 4 (9, 6 and 4 valid taps: carries at more than one round);
# 3 x 2 stride (1, 2); a window equal to a 2 x 3 plane (global pooling); 1 x 1 stride 2 (a copy); c = 2 throughout
SHAPES = [pool_model.desc(2, 4, 4, 2, 2), pool_model.desc(2, 5, 4, 3, 3, stride=(2, 2), padding=(1, 1)),
          pool_model.desc(2, 4, 5, 3, 2, stride=(1, 2)), pool_model.desc(2, 2, 3, 2, 3),
          pool_model.desc(2, 5, 5, 1, 1, stride=(2, 2))]


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


def _pool_device(ctx, w, d, ct, lut, q, stream=None):
    """The device call on an output pre-filled with -1 and followed by a guard row, which must stay; the input must
    come back bit-identical."""
    import torch

    import tfhe_amd

    oh, ow, _, _ = pool_model.shape(d)
    d_ct, d_l = _dev(ct), _dev(lut)
    rows = ct.shape[0] * d.c * oh * ow
    d_out = torch.full((rows + 1, w), -1, dtype=torch.int64, device=d_ct.device)
    torch.cuda.synchronize()
    ctx.EvalPool2dDevice(tfhe_amd.Pool2d(*d), ct.shape[0], d_ct.data_ptr(), d_l.data_ptr(), d_out.data_ptr(), q=q,
                         stream=stream.cuda_stream if stream is not None else 0)
    torch.cuda.synchronize()
    out = _host(d_out)
    assert (out[rows] == np.uint64(2**64 - 1)).all(), "the guard row was written"
    assert np.array_equal(_host(d_ct), ct), "an input word was written"
    return out[:rows].reshape(ct.shape[0], d.c, oh, ow, w)


def _kw(d):
    return dict(kernel=(d.kh, d.kw), stride=(d.stride_h, d.stride_w), padding=(d.pad_h, d.pad_w))


@pytest.mark.parametrize("instances", [1, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_layer_equals_the_host_array_composition(env, kind, instances):
    """Every word of every shape against the model with ctx.EvalFunc as the pair step's function (one host-array
    call per round), the host-array entry, and the bootstraps counter: pairs * c * instances * (1 | 2); the 1 x 1
    window leaves the counter alone."""
    op, ctx, _ = env
    q, w = op.q, op.n + 1
    lut = _luts(q)[kind]
    rs = np.random.default_rng(71 + instances)
    for d in SHAPES:
        pairs = pool_model.shape(d)[3]
        ct = rs.integers(0, q, (instances, d.c, d.h, d.w, w), dtype=np.uint64)
        before = ctx.info().bootstraps
        got = _pool_device(ctx, w, d, ct, lut, q)
        assert ctx.info().bootstraps - before == BOOTSTRAPS_PER_PAIR[kind] * pairs * d.c * instances, d
        assert (got < q).all()
        comp = pool_model.pool2d(ct, d, pool_model.func_pair(ctx.EvalFunc, lut, q))
        assert np.array_equal(got, comp), d
        assert np.array_equal(got, ctx.EvalPool2d(ct, lut, q=q, **_kw(d))), d
    assert pairs == 0 and np.array_equal(got, ct[:, :, ::2, ::2])  # the copy


def test_global_pooling_equals_the_oracle(env):
    """A window equal to the 2 x 3 plane, one instance, two planes (10 pairs, three rounds with a carry), a
    negacyclic table: the model with the oracle's EvalFunc."""
    op, ctx, orc = env
    q, w, d = op.q, op.n + 1, SHAPES[3]
    lut = _luts(q)["negacyclic"]
    ct = np.random.default_rng(73).integers(0, q, (1, d.c, d.h, d.w, w), dtype=np.uint64)
    got = _pool_device(ctx, w, d, ct, lut, q)
    assert np.array_equal(got, pool_model.pool2d(ct, d, pool_model.func_pair(orc.eval_func, lut, q)))


def test_one_instance_keeps_its_shape_and_stride_defaults_to_the_kernel(env):
    op, ctx, _ = env
    q, w, d = op.q, op.n + 1, SHAPES[0]
    lut = _luts(q)["negacyclic"]
    ct = np.random.default_rng(74).integers(0, q, (2, d.c, d.h, d.w, w), dtype=np.uint64)
    a = ctx.EvalPool2d(ct, lut, 2)
    assert a.shape == (2, d.c, 2, 2, w) and np.array_equal(a, _pool_device(ctx, w, d, ct, lut, q))
    one = ctx.EvalPool2d(ct[1], lut, (2, 2), stride=2)
    assert one.shape == a.shape[1:] and np.array_equal(one, a[1])


def test_max_pool_helper_is_the_layer_with_the_helper_table(env):
    import tfhe_amd

    op, ctx, _ = env
    q, w, d = op.q, op.n + 1, SHAPES[0]
    ct = np.random.default_rng(75).integers(0, q, (1, d.c, d.h, d.w, w), dtype=np.uint64)
    for neg, per_pair in ((False, 2), (True, 1)):
        before = ctx.info().bootstraps
        got = ctx.EvalMaxPool2d(ct, 2, negacyclic=neg)
        assert ctx.info().bootstraps - before == per_pair * pool_model.shape(d)[3] * d.c
        assert np.array_equal(got, _pool_device(ctx, w, d, ct, tfhe_amd.max_table(q, neg), q))


def test_arbitrary_table_needs_q_up_to_N(env):
    """q = 2N with an arbitrary-class table: TFHE_ERR_UNSUPPORTED before anything is launched, and the bootstraps
    counter does not move."""
    import tfhe_amd as capi

    op, ctx, _ = env
    q, w, d = 2 * op.N, op.n + 1, SHAPES[0]
    lut = _luts(q)["arbitrary"]
    ct = np.random.default_rng(76).integers(0, q, (1, d.c, d.h, d.w, w), dtype=np.uint64)
    before = ctx.info().bootstraps
    for call in (lambda: _pool_device(ctx, w, d, ct, lut, q), lambda: ctx.EvalPool2d(ct, lut, q=q, **_kw(d))):
        with pytest.raises(capi.TfheError) as e:
            call()
        assert e.value.status == 2  # TFHE_ERR_UNSUPPORTED
    assert ctx.info().bootstraps == before


def test_shape_and_argument_errors(env):
    import tfhe_amd as capi

    op, ctx, _ = env
    q, w, d = op.q, op.n + 1, SHAPES[1]
    lut = _luts(q)["negacyclic"]
    ct = np.random.default_rng(77).integers(0, q, (2, d.c, d.h, d.w, w), dtype=np.uint64)
    kw = _kw(d)
    with pytest.raises(ValueError):
        ctx.EvalPool2d(ct[..., :-1], lut, **kw)  # ciphertext width
    with pytest.raises(ValueError):
        ctx.EvalPool2d(ct[0, 0], lut, **kw)  # not [C, H, W, n+1]
    with pytest.raises(ValueError):
        ctx.EvalPool2d(ct, lut[:-1], **kw)
    with pytest.raises(ValueError):
        ctx.EvalPool2d(ct, lut, 0)
    with pytest.raises(ValueError):
        ctx.EvalPool2d(ct, lut, 3, stride=0)
    with pytest.raises(ValueError) as ve:
        ctx.EvalPool2d(ct, lut, 3, padding=(3, 0))  # pad_h >= kh
    assert "pad_h" in str(ve.value)
    with pytest.raises(ValueError) as ve:
        ctx.EvalPool2d(ct, lut, (3, 7))  # window beyond the plane
    assert "kw" in str(ve.value)
    # kernel, stride and padding as one int
    assert np.array_equal(ctx.EvalPool2d(ct, lut, 3, stride=2, padding=1), ctx.EvalPool2d(ct, lut, **kw))
    t = _dev(ct)
    desc, P = capi.Pool2d(*d), t.data_ptr()
    before = ctx.info().bootstraps
    for bad_q in (4, 3 * 256, 4 * op.N):  # below 8; no power of two; not a divisor of 2N
        with pytest.raises(capi.TfheError) as e:
            ctx.EvalPool2dDevice(desc, 2, P, P, P, q=bad_q)
        assert e.value.status == 1 and "q must be a power of two >= 8 that divides 2N" in str(e.value), bad_q
    for args, word in (((desc, 2, 0, P, P), "null ct"), ((desc, 2, P, 0, P), "null lut"), ((desc, 2, P, P, 0), "null out"),
                       ((desc, 0, P, P, P), "instances is 0"), ((desc, 2**62, P, P, P), "sizes overflow"),
                       ((capi.Pool2d(*d._replace(stride_w=0)), 2, P, P, P), "stride_w is 0"),
                       ((capi.Pool2d(*d._replace(pad_w=3)), 2, P, P, P), "pad_w must be below kw"),
                       ((capi.Pool2d(*d._replace(kh=8)), 2, P, P, P), "kh exceeds h + 2 pad_h")):
        with pytest.raises(capi.TfheError) as e:
            ctx.EvalPool2dDevice(*args)
        assert e.value.status == 1 and word in str(e.value), word
    L = capi.lib()
    assert L.tfhe_eval_pool2d_device(ctx._h, None, 2, P, q, P, P, None) == 1 and b"descriptor" in L.tfhe_last_error()
    assert ctx.info().bootstraps == before


def test_slices_a_round_beyond_the_chunk(shared_kat):
    """One round of 70,001 pairs on STD128 (a 1 x 2 window of stride 2 on a one-row plane of 140,002): EvalFunc runs
    in two slices, cut at 65,536, and the kernels' grids stride over the items.  The items either side of the cut,
    the first and the last, against EvalFuncDevice on differences computed by torch; the counter."""
    import torch

    import tfhe_amd

    s = shared_kat("STD128")
    op, ctx = s["op"], s["ctx"]
    q, w, npos, cut = op.q, op.n + 1, 70001, 65536
    d = pool_model.desc(1, 1, 2 * npos, 1, 2)
    assert pool_model.shape(d) == (1, npos, 1, npos)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(78)
    d_ct = torch.randint(0, q, (1, 1, 1, 2 * npos, w), dtype=torch.int64, device="cuda", generator=gen)
    keep = d_ct.clone()
    d_l = _dev(_luts(q)["negacyclic"])
    d_out = torch.full((npos + 1, w), -1, dtype=torch.int64, device=d_ct.device)
    torch.cuda.synchronize()
    before = ctx.info().bootstraps
    ctx.EvalPool2dDevice(tfhe_amd.Pool2d(*d), 1, d_ct.data_ptr(), d_l.data_ptr(), d_out.data_ptr())
    torch.cuda.synchronize()
    assert ctx.info().bootstraps - before == npos
    assert torch.equal(d_ct, keep) and bool((d_out[npos] == -1).all())
    assert bool((d_out[:npos] >= 0).all()) and bool((d_out[:npos] < q).all())  # every row was written
    idx = torch.tensor([0, cut - 1, cut, npos - 1], device=d_ct.device)
    rows = d_ct.reshape(npos, 2, w)[idx]
    a, b = rows[:, 0], rows[:, 1]
    z = ((a - b) & (q - 1)).contiguous()
    f = torch.empty_like(z)
    ctx.EvalFuncDevice(len(idx), z.data_ptr(), d_l.data_ptr(), f.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(d_out[idx], (f + b) & (q - 1))


def test_two_streams_are_ordered(env):
    """Two layers on two user streams and a host-array call, with no synchronisation between them: they share the
    device's scratch, slot store and flat rows, which the engine orders; each equals its sequential run."""
    import torch

    import tfhe_amd

    op, ctx, _ = env
    q, w = op.q, op.n + 1
    lut = _luts(q)["negacyclic"]
    rs = np.random.default_rng(79)
    d1, d2 = SHAPES[1], SHAPES[2]
    c1 = rs.integers(0, q, (3, d1.c, d1.h, d1.w, w), dtype=np.uint64)
    c2 = rs.integers(0, q, (2, d2.c, d2.h, d2.w, w), dtype=np.uint64)
    want1, want2 = _pool_device(ctx, w, d1, c1, lut, q), _pool_device(ctx, w, d2, c2, lut, q)
    t1, t2, d_l = _dev(c1), _dev(c2), _dev(lut)
    o1 = torch.full(want1.shape, -1, dtype=torch.int64, device=t1.device)
    o2 = torch.full(want2.shape, -1, dtype=torch.int64, device=t1.device)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    ctx.EvalPool2dDevice(tfhe_amd.Pool2d(*d1), 3, t1.data_ptr(), d_l.data_ptr(), o1.data_ptr(), stream=s1.cuda_stream)
    ctx.EvalPool2dDevice(tfhe_amd.Pool2d(*d2), 2, t2.data_ptr(), d_l.data_ptr(), o2.data_ptr(), stream=s2.cuda_stream)
    host = ctx.EvalPool2d(c2, lut, **_kw(d2))
    s1.synchronize()
    s2.synchronize()
    assert np.array_equal(_host(o1), want1) and np.array_equal(_host(o2), want2) and np.array_equal(host, want2)


def test_chains_from_a_convolution_into_a_dense_layer(shared_kat):
    """EvalConv2dDevice -> EvalPool2dDevice -> EvalDenseDevice by pointer, no relayout (STD128, a negacyclic table):
    1 -> 2 planes of 3 x 3 by a 2 x 2 window: two planes of 2 x 2; a 1 x 2 pool: 2 x 2 x 1 = 4 results; 4 -> 2
    dense.  Each stage equals the model through the oracle."""
    import torch

    import tfhe_amd

    s = shared_kat("STD128")
    op, ctx, orc = s["op"], s["ctx"], s["orc"]
    q, w = op.q, op.n + 1
    rs = np.random.default_rng(80)
    dc, dp = conv_model.desc(1, 3, 3, 2, 2, 2), pool_model.desc(2, 2, 2, 1, 2)
    ct = rs.integers(0, q, (1, 1, 3, 3, w), dtype=np.uint64)
    wt, mat = rs.integers(-4, 4, (2, 1, 2, 2), dtype=np.int64), rs.integers(-4, 4, (4, 2), dtype=np.int64)
    bc, bd = (rs.integers(0, q, 2, dtype=np.uint64) for _ in range(2))
    lut = _luts(q)["negacyclic"]
    d_ct, d_wt, d_m, d_bc, d_bd, d_l = (_dev(a) for a in (ct, wt, mat, bc, bd, lut))
    d_y = torch.full((1, 2, 2, 2, w), -1, dtype=torch.int64, device=d_ct.device)
    d_p = torch.full((1, 2, 2, 1, w), -1, dtype=torch.int64, device=d_ct.device)
    d_o = torch.full((1, 2, w), -1, dtype=torch.int64, device=d_ct.device)
    torch.cuda.synchronize()
    ctx.EvalConv2dDevice(tfhe_amd.Conv2d(*dc), 1, d_ct.data_ptr(), d_wt.data_ptr(), d_l.data_ptr(), d_y.data_ptr(),
                         d_bias=d_bc.data_ptr())
    ctx.EvalPool2dDevice(tfhe_amd.Pool2d(*dp), 1, d_y.data_ptr(), d_l.data_ptr(), d_p.data_ptr())
    ctx.EvalDenseDevice(1, 4, d_p.data_ptr(), 2, d_m.data_ptr(), d_l.data_ptr(), d_o.data_ptr(), d_bias=d_bd.data_ptr())
    torch.cuda.synchronize()
    y = conv_model.conv_layer(orc, ct, wt, lut, dc, bc, q)
    assert np.array_equal(_host(d_y), y)
    pooled = pool_model.pool2d(y, dp, pool_model.func_pair(orc.eval_func, lut, q))
    assert np.array_equal(_host(d_p), pooled)
    assert np.array_equal(_host(d_o), dense_model.dense(orc, pooled.reshape(1, 4, w), mat, lut, bd, q))


def test_network_decrypts_to_the_clear_network():
    """tests/test_pool_cpu.py's decrypting cases of the first key seed on a from_keygen context of the logQ = 12
    parameters, in its order on one stream: each helper table at the p found on the oracle, Encrypt -> EvalMaxPool2d
    -> Decrypt equals the clear maximum; then pool_model.NET_CASE, Encrypt -> EvalConv2d (m -> m mod 2) ->
    EvalMaxPool2d -> Decrypt equals the clear-text network."""
    import tfhe_amd

    c = pool_model.NET_CASE
    cp = tfhe_amd.params_from_logq(*pool_model.POOL_DECRYPT_LOGQ)
    q, w, p = cp.q, cp.n + 1, c["p"]
    ctx, sk = tfhe_amd.BinFHEContextHIP.from_keygen(cp, c["key_seed"])
    try:
        d = pool_model.POOL_DECRYPT_DESC
        for kind, k in pool_model.POOL_DECRYPT_CASES.items():
            m = pool_model.pool_decrypt_msgs(kind, c["key_seed"])
            e = ctx.Encrypt(sk, m.ravel(), p=k["p"], seed=ctx.seed_after).reshape(m.shape + (w,))
            o = ctx.EvalMaxPool2d(e, (d.kh, d.kw), stride=(d.stride_h, d.stride_w), negacyclic=k["negacyclic"])
            assert ctx.Decrypt(sk, o.reshape(-1, w), p=k["p"]) == [int(v) for v in pool_model.clear_max(m, d).ravel()], kind
        msgs, weight, want = pool_model.net_case()
        cts = ctx.Encrypt(sk, msgs.ravel(), p=p, seed=ctx.seed_after).reshape(msgs.shape + (w,))
        y = ctx.EvalConv2d(cts, weight, pool_model.parity_lut(q, p))
        out = ctx.EvalMaxPool2d(y, (1, 2))
        got = ctx.Decrypt(sk, out.reshape(-1, w), p=p)
        assert got == [int(v) for v in want.ravel()] and len(set(got)) > 1
    finally:
        ctx.GPUClean()
