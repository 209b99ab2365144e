"""GPU: the pair instance of the STD128 blind rotation (k_blind_rotate_fast4<MINW = 3, NCT = 2, ..., RING = 2>,
blind_rotate_fast4_pair.hip): two ciphertexts per wavefront, three workgroups per CU.

Device-resident batches of at least `pair_min` ciphertexts (tfhe_set_pair_min, default 3072) run it; here it is
forced with pair_min = 1 (and split4 = 0, because the two-group form of small batches takes precedence).  Checked
through the C-ABI: tfhe_eval_acc_device and EvalBinGate(NAND) against the oracle bit for bit at 1 (the wavefront's
second ciphertext masked), 2, 3 (odd tail) and 9 ciphertexts and both power-of-two a-moduli; 65 ciphertexts
against the default kernel word for word; rows of a that are all 0 and all q - 1 (both ends of the monomial
table) in both ciphertexts of a wavefront; the setting's round trip and the dispatch below / from pair_min
(the context counts its launches on the pair instance).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def std128(shared_kat):
    s = shared_kat("STD128")  # the session's shared context
    assert s["ctx"].info().br_kernel == 1
    return s


def _eval_acc_device(ctx, a, amod, acc):
    """tfhe_eval_acc_device on device copies of a[B][n], acc[B][2][N]; returns the new acc"""
    import torch

    import tfhe_amd

    dev = torch.device("cuda", 0)
    d_a = torch.from_numpy(a.astype(np.int64)).to(dev)
    d_acc = torch.from_numpy(acc.astype(np.int64)).to(dev)
    s = torch.cuda.Stream(dev)
    tfhe_amd.capi.check(ctx._L.tfhe_eval_acc_device(ctx.handle, a.shape[0], d_a.data_ptr(), int(amod), d_acc.data_ptr(),
                                                    s.cuda_stream), "tfhe_eval_acc_device")
    s.synchronize()
    return d_acc.cpu().numpy().astype(np.uint64)


def _inputs(op, B, seed, amod):
    rs = np.random.default_rng(seed)
    a = rs.integers(0, amod, (B, op.n), dtype=np.uint64)
    acc = rs.integers(0, op.Q, (B, 2, op.N), dtype=np.uint64)
    return a, acc


def _paired(ctx, fn):
    """fn() with the pair instance forced; asserts that every blind rotation in it ran on that instance"""
    with ctx.knobs_set(pair_min=1, split4=0):
        before = ctx.pair_launches()
        out = fn()
        assert ctx.pair_launches() > before
    return out


@pytest.mark.parametrize("B", [1, 2, 3, 9])
@pytest.mark.parametrize("amod", ["q", "2N"])
def test_pair_eval_acc_matches_oracle(std128, B, amod):
    op, ctx, orc = std128["op"], std128["ctx"], std128["orc"]
    amod = int(op.q) if amod == "q" else 2 * int(op.N)
    a, acc = _inputs(op, B, 1700 + B + amod, amod)
    got = _paired(ctx, lambda: _eval_acc_device(ctx, a, amod, acc))
    assert np.array_equal(got, orc.eval_acc(a, amod, acc))


@pytest.mark.parametrize("B", [1, 2, 3, 9])
def test_pair_nand_matches_oracle(std128, B):
    op, ctx, orc = std128["op"], std128["ctx"], std128["orc"]
    rs = np.random.default_rng(1800 + B)
    c1 = rs.integers(0, op.q, (B, op.n + 1), dtype=np.uint64)
    c2 = rs.integers(0, op.q, (B, op.n + 1), dtype=np.uint64)
    got = _paired(ctx, lambda: ctx.EvalBinGate("NAND", c1, c2))
    assert np.array_equal(got, orc.eval_bin_gate("NAND", c1, c2))


def test_pair_equals_default_kernel_at_65(std128):
    """33 workgroups, the last one with its second ciphertext masked: every output word equal"""
    op, ctx = std128["op"], std128["ctx"]
    a, acc = _inputs(op, 65, 1965, int(op.q))
    pair = _paired(ctx, lambda: _eval_acc_device(ctx, a, op.q, acc))
    with ctx.knobs_set(pair_min=0, split4=0):
        before = ctx.pair_launches()
        one = _eval_acc_device(ctx, a, op.q, acc)
        assert ctx.pair_launches() == before
    assert np.array_equal(pair, one)
    assert not np.array_equal(pair, acc)


@pytest.mark.parametrize("amod", ["q", "2N"])
def test_pair_monomial_table_ends(std128, amod):
    """a rows of all 0 (X^0 - 1 = 0: the accumulator only changes form) and all amod - 1, in the first and in
    the second ciphertext of a wavefront"""
    op, ctx, orc = std128["op"], std128["ctx"], std128["orc"]
    amod = int(op.q) if amod == "q" else 2 * int(op.N)
    a, acc = _inputs(op, 4, 2100 + amod, amod)
    a[0], a[1], a[2], a[3] = 0, amod - 1, amod - 1, 0
    got = _paired(ctx, lambda: _eval_acc_device(ctx, a, amod, acc))
    assert np.array_equal(got, orc.eval_acc(a, amod, acc))


def test_pair_min_round_trip_and_dispatch(std128):
    op, ctx = std128["op"], std128["ctx"]
    assert ctx.knobs()["pair_min"] == 3072  # the measured default
    a, acc = _inputs(op, 6, 2200, int(op.q))
    with ctx.knobs_set(pair_min=6, split4=0):
        assert ctx.knobs()["pair_min"] == 6 and ctx.knobs()["split4"] == 0
        ctx.set_knobs(duo=ctx.knobs()["duo"])  # tfhe_set_knobs leaves pair_min alone
        assert ctx.knobs()["pair_min"] == 6
        n0 = ctx.pair_launches()
        below = _eval_acc_device(ctx, a[:5], op.q, acc[:5])  # B < pair_min: the default kernel
        assert ctx.pair_launches() == n0
        at = _eval_acc_device(ctx, a, op.q, acc)  # B = pair_min: the pair instance
        assert ctx.pair_launches() == n0 + 1
        assert np.array_equal(below, at[:5])
    with ctx.knobs_set(pair_min=1):  # split4 (default 384) takes precedence: the two-group form
        n0 = ctx.pair_launches()
        assert np.array_equal(_eval_acc_device(ctx, a, op.q, acc), at)
        assert ctx.pair_launches() == n0
    assert ctx.knobs()["pair_min"] == 3072
    with pytest.raises(Exception):
        ctx.set_knobs(pair_min=-1)
    assert ctx.knobs()["pair_min"] == 3072
