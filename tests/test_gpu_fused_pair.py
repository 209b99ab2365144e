"""GPU: the pair instance of the STD128 blind rotation with fused radix-4 groups (kernel variant 71,
blind_rotate_fast4_pair.hip: k_blind_rotate_fast4<..., FU>), forced through tfhe_set_kernel_variant.

Full blind rotations (all n rounds) against the oracle word for word at 1 ciphertext (the lone ciphertext of a
wavefront), 2 (one pair), 3 (a pair and an odd last one) and 5 with both power-of-two a-moduli; one
EvalBinGateDevice at 3 ciphertexts, equal between the fused (71) and the plain (70) pair.  Variant 61, the
one-ciphertext build with the inverse's fused groups, gets the 5-ciphertext case too.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def std128(shared_kat):
    s = shared_kat("STD128")  # the session's shared context
    assert s["ctx"].info().br_kernel == 1
    return s


class _variant:
    def __init__(self, v):
        import tfhe_amd

        self.lib, self.v = tfhe_amd.lib(), v

    def __enter__(self):
        assert self.lib.tfhe_set_kernel_variant(self.v) == 0
        assert self.lib.tfhe_get_kernel_variant() == self.v

    def __exit__(self, *exc):
        self.lib.tfhe_set_kernel_variant(0)


def _eval_acc_device(ctx, a, amod, acc):
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
    return rs.integers(0, amod, (B, op.n), dtype=np.uint64), rs.integers(0, op.Q, (B, 2, op.N), dtype=np.uint64)


@pytest.mark.parametrize("B", [1, 2, 3])
def test_fused_pair_matches_oracle(std128, B):
    op, ctx, orc = std128["op"], std128["ctx"], std128["orc"]
    a, acc = _inputs(op, B, 7100 + B, int(op.q))
    with _variant(71):
        before = ctx.pair_launches()
        got = _eval_acc_device(ctx, a, op.q, acc)
        assert ctx.pair_launches() == before + 1
    assert np.array_equal(got, orc.eval_acc(a, int(op.q), acc))


@pytest.mark.parametrize("variant", [71, 61])
@pytest.mark.parametrize("amod", ["q", "2N"])
def test_fused_matches_oracle_at_5(std128, amod, variant):
    op, ctx, orc = std128["op"], std128["ctx"], std128["orc"]
    amod = int(op.q) if amod == "q" else 2 * int(op.N)
    a, acc = _inputs(op, 5, 7200 + amod, amod)
    with _variant(variant), ctx.knobs_set(split4=0):  # 61: its own kernel, not the two-group form of small batches
        got = _eval_acc_device(ctx, a, amod, acc)
    assert np.array_equal(got, orc.eval_acc(a, amod, acc))


def test_fused_and_plain_pair_gate_equal(std128):
    import torch

    op, ctx = std128["op"], std128["ctx"]
    rs = np.random.default_rng(7300)
    B = 3
    d1 = torch.from_numpy(rs.integers(0, op.q, (B, op.n + 1), dtype=np.uint64).astype(np.int64)).cuda()
    d2 = torch.from_numpy(rs.integers(0, op.q, (B, op.n + 1), dtype=np.uint64).astype(np.int64)).cuda()
    out = {}
    for v in (71, 70):
        do = torch.zeros_like(d1)
        with _variant(v):
            before = ctx.pair_launches()
            ctx.EvalBinGateDevice("NAND", B, d1.data_ptr(), d2.data_ptr(), do.data_ptr())
            torch.cuda.synchronize()
            assert ctx.pair_launches() > before
        out[v] = do.cpu().numpy()
    assert np.array_equal(out[71], out[70])
    assert not np.array_equal(out[71], np.zeros_like(out[71]))
