"""GPU: EvalFunc with one table per channel (tfhe_eval_func_tables_device / tfhe_eval_func_tables).
Ciphertext i of a flat batch uses table (i // inner) % T; each table is classified on its own; every result must equal,
bit for bit, the shared-table EvalFunc with that table on that ciphertext, whatever classes the batch mixes -- on
STD128 and the arbFunc logQ = 12 context.  It must count its bootstraps as tfhe_lut_tables_info says, index tables by
the position in the whole batch across a slice, write no input and nothing past its output, and order streams."""
import numpy as np
import pytest

import tables_model

pytestmark = pytest.mark.gpu

MIXED = ["negacyclic", "periodic", "arbitrary", "negacyclic"]  # class order (neg, per, arb, neg')


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


def _tables_device(ctx, ct, luts, inner, q, stream=None):
    """The device call on an output pre-filled with -1 and followed by a guard row, which must stay; the input must
    come back bit-identical."""
    import torch

    B, w = ct.shape
    d_ct, d_l = _dev(ct), _dev(luts)
    d_out = torch.full((B + 1, w), -1, dtype=torch.int64, device=d_ct.device)
    torch.cuda.synchronize()
    ctx.EvalFuncTablesDevice(B, d_ct.data_ptr(), d_l.data_ptr(), luts.shape[0], d_out.data_ptr(), inner=inner, q=q,
                             stream=stream.cuda_stream if stream is not None else 0)
    torch.cuda.synchronize()
    out = _host(d_out)
    assert (out[B] == np.uint64(2**64 - 1)).all(), "the guard row was written"
    assert np.array_equal(_host(d_ct), ct), "an input word was written"
    return out[:B]


def _func_device(ctx, ct, lut, q):
    import torch

    d_ct, d_l = _dev(ct), _dev(lut)
    d_out = torch.full(ct.shape, -1, dtype=torch.int64, device=d_ct.device)
    torch.cuda.synchronize()
    ctx.EvalFuncDevice(ct.shape[0], d_ct.data_ptr(), d_l.data_ptr(), d_out.data_ptr(), q=q)
    torch.cuda.synchronize()
    return _host(d_out)


@pytest.mark.parametrize("inner", [1, 2, 3])
def test_mixed_classes_equal_the_shared_table_calls(env, inner):
    import tfhe_amd

    op, ctx, orc = env
    q, w, B = op.q, op.n + 1, 13
    luts = tables_model.tables(q, MIXED)
    assert tfhe_amd.lut_classes(luts, q).tolist() == [0, 1, 2, 0]
    ct = np.random.default_rng(90 + inner).integers(0, q, (B, w), dtype=np.uint64)
    before = ctx.info().bootstraps
    got = _tables_device(ctx, ct, luts, inner, q)
    assert ctx.info().bootstraps - before == tfhe_amd.lut_tables_info(luts, q, inner, B)[2]
    assert (got < q).all()
    assert np.array_equal(got, tables_model.compose(ctx.EvalFunc, ct, luts, inner, q))
    t = tables_model.table_of(B, inner, len(luts))
    for i in (0, B - 1):
        assert np.array_equal(got[i:i + 1], orc.eval_func(ct[i:i + 1], luts[t[i]], q)), i
    assert np.array_equal(got, ctx.EvalFuncTables(ct, luts, inner=inner, q=q))


@pytest.mark.parametrize("kind", tables_model.KINDS)
def test_one_table_is_the_shared_table_call(env, kind):
    op, ctx, _ = env
    q, w = op.q, op.n + 1
    lut = tables_model.luts3(q)[kind][1]
    ct = np.random.default_rng(94).integers(0, q, (5, w), dtype=np.uint64)
    assert np.array_equal(_tables_device(ctx, ct, lut[None], 3, q), _func_device(ctx, ct, lut, q))


@pytest.mark.parametrize("kind", tables_model.KINDS)
def test_single_class_batches(env, kind):
    """T = 3 different tables of one class, B = 7: the path that copies no row."""
    import tfhe_amd

    op, ctx, _ = env
    q, w, B = op.q, op.n + 1, 7
    luts = tables_model.tables(q, [kind] * 3)
    assert len({t.tobytes() for t in luts}) == 3 and tfhe_amd.lut_classes(luts, q).tolist() == [tables_model.CLASS[kind]] * 3
    ct = np.random.default_rng(95).integers(0, q, (B, w), dtype=np.uint64)
    before = ctx.info().bootstraps
    got = _tables_device(ctx, ct, luts, 2, q)
    assert ctx.info().bootstraps - before == tfhe_amd.lut_tables_info(luts, q, 2, B)[2]
    assert np.array_equal(got, tables_model.compose(ctx.EvalFunc, ct, luts, 2, q))


def test_the_table_index_is_the_index_in_the_whole_batch(shared_kat):
    """B = 70,001, T = 3, inner = 5, negacyclic tables, STD128: two slices, cut at 65,536, which 5 does not divide, so
    an index taken inside the slice would pick wrong tables from ciphertext 65,536 on.  Against three shared-table
    EvalFuncDevice calls on index-gathers of each table's ciphertexts."""
    import torch

    s = shared_kat("STD128")
    op, ctx = s["op"], s["ctx"]
    q, w, B, T, inner = op.q, op.n + 1, 70001, 3, 5
    luts = tables_model.tables(q, ["negacyclic"] * T)
    import tfhe_amd

    assert tfhe_amd.lut_classes(luts, q).tolist() == [0, 0, 0] and len({l.tobytes() for l in luts}) == 3
    d_ct = _dev(np.random.default_rng(96).integers(0, q, (B, w), dtype=np.uint64))
    d_l = _dev(luts)
    d_out = torch.full((B, w), -1, dtype=torch.int64, device=d_ct.device)
    d_ref = torch.empty_like(d_out)
    torch.cuda.synchronize()
    before = ctx.info().bootstraps
    ctx.EvalFuncTablesDevice(B, d_ct.data_ptr(), d_l.data_ptr(), T, d_out.data_ptr(), inner=inner)
    torch.cuda.synchronize()
    assert ctx.info().bootstraps - before == B
    t = torch.from_numpy(tables_model.table_of(B, inner, T)).to(d_ct.device)
    for k in range(T):
        rows = torch.nonzero(t == k).squeeze(1)
        part = d_ct[rows].contiguous()
        res = torch.empty_like(part)
        ctx.EvalFuncDevice(part.shape[0], part.data_ptr(), d_l[k].data_ptr(), res.data_ptr())
        torch.cuda.synchronize()
        d_ref[rows] = res
    assert torch.equal(d_out[65530:65550], d_ref[65530:65550])
    assert torch.equal(d_out, d_ref)


def test_two_streams_are_ordered(env):
    """Two calls on two user streams and a host-array call, with no synchronisation between them: they share the
    device's scratch and class table, which the engine orders; each equals its sequential run."""
    import torch

    op, ctx, _ = env
    q, w = op.q, op.n + 1
    l1, l2 = tables_model.tables(q, MIXED), tables_model.tables(q, ["periodic", "negacyclic", "arbitrary"])
    rs = np.random.default_rng(97)
    c1, c2 = rs.integers(0, q, (13, w), dtype=np.uint64), rs.integers(0, q, (9, w), dtype=np.uint64)
    want1, want2 = _tables_device(ctx, c1, l1, 2, q), _tables_device(ctx, c2, l2, 1, q)
    t1, t2, d1, d2 = _dev(c1), _dev(c2), _dev(l1), _dev(l2)
    o1 = torch.full(c1.shape, -1, dtype=torch.int64, device=t1.device)
    o2 = torch.full(c2.shape, -1, dtype=torch.int64, device=t1.device)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    ctx.EvalFuncTablesDevice(13, t1.data_ptr(), d1.data_ptr(), 4, o1.data_ptr(), inner=2, stream=s1.cuda_stream)
    ctx.EvalFuncTablesDevice(9, t2.data_ptr(), d2.data_ptr(), 3, o2.data_ptr(), inner=1, stream=s2.cuda_stream)
    host = ctx.EvalFuncTables(c2, l2)
    s1.synchronize()
    s2.synchronize()
    assert np.array_equal(_host(o1), want1) and np.array_equal(_host(o2), want2) and np.array_equal(host, want2)


def test_argument_errors(env):
    import tfhe_amd as capi

    op, ctx, _ = env
    q, w = op.q, op.n + 1
    luts = tables_model.tables(q, MIXED)
    ct = np.zeros((4, w), dtype=np.uint64)
    d = _dev(ct).data_ptr()
    dl = _dev(luts)
    before = ctx.info().bootstraps

    def dev(B=4, ct=d, lut=dl.data_ptr(), T=4, out=d, inner=1, q=q):
        return lambda: ctx.EvalFuncTablesDevice(B, ct, lut, T, out, inner=inner, q=q)

    cases = [(dev(ct=0), "ct"), (dev(lut=0), "luts"), (dev(out=0), "out"), (dev(B=0), "B"), (dev(T=0), "num_luts"),
             (dev(inner=0), "inner"), (dev(q=4), "q"), (dev(q=3 * 256), "q"), (dev(q=4 * op.N), "q"),
             (dev(B=1 << 61), "B (n+1)"), (dev(T=1 << 60), "num_luts q"), (dev(inner=1 << 63), "inner num_luts")]
    for call, field in cases:
        with pytest.raises(capi.TfheError) as e:
            call()
        assert e.value.status == 1 and field in str(e.value), field  # TFHE_ERR_INVALID_ARGUMENT
    with pytest.raises(capi.TfheError) as e:
        ctx._check(ctx._L.tfhe_eval_func_tables(ctx._h, 0, ct.ravel(), q, luts.ravel(), 4, 1, ct.ravel()), "host")
    assert e.value.status == 1
    with pytest.raises(ValueError):
        ctx.EvalFuncTables(ct, luts[:, :-1])
    assert ctx.info().bootstraps == before


def test_an_arbitrary_table_needs_q_up_to_N(env):
    """q = 2N with one arbitrary table among negacyclic ones: TFHE_ERR_UNSUPPORTED before anything is launched, and
    the bootstraps counter does not move."""
    import tfhe_amd as capi

    op, ctx, _ = env
    q, w = 2 * op.N, op.n + 1
    luts = tables_model.tables(q, ["negacyclic", "negacyclic", "arbitrary", "negacyclic"])
    ct = np.random.default_rng(98).integers(0, q, (6, w), dtype=np.uint64)
    before = ctx.info().bootstraps
    for call in (lambda: _tables_device(ctx, ct, luts, 1, q), lambda: ctx.EvalFuncTables(ct, luts, q=q)):
        with pytest.raises(capi.TfheError) as e:
            call()
        assert e.value.status == 2  # TFHE_ERR_UNSUPPORTED
    assert ctx.info().bootstraps == before
