"""GPU: the two-workgroup exact-FP64 blind rotation (k_blind_rotate_f64wduo, blind_rotate_f64.hip); since round 6
also its STD192-class instance (bottom of the file).

STD128Q-class contexts (C5a: Q = 2^50 - 2^14 + 1, two digits, the top one eliminated with the WRAP
correction) run batches of at most `tfhe_knobs.duo` (default 128) ciphertexts with each ciphertext's
round split over two workgroups by NTT half: member h keeps the slots of half h after the first forward
stage, and the pair exchanges 16 KiB of stage-1 inverse values per round.  Checked through the C-ABI:
  * EvalAcc bit-exact against the oracle at batches that leave pair groups ragged (1, 7, 9);
  * accumulators in the WRAP range (centred c in [2^49 - 2^24, Q/2): every round runs the correction
    digit) against the oracle;
  * the same outputs as the one-workgroup f64w (duo = 0) at 64 and 128 ciphertexts;
  * EvalSign at C5's per-GPU shard of an 8-GPU node (1024 / 8 = 128), decrypting with valid keys;
  * a partner that never arrives (test library, probe 5): the rescue recomputes the pair exactly;
  * no partner ever timed out in a normal run (tfhe_info.duo_timeouts).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
QIN = 1 << 23


@pytest.fixture(scope="module")
def f64duo(shared_kat):
    s = shared_kat("STD128Q")  # the session's shared context
    ctx = s["ctx"]
    assert ctx.info().br_kernel == 3 and ctx.knobs()["duo"] == 128  # f64w with the WRAP fold
    yield s
    assert ctx.info().duo_timeouts == 0


def _inputs(op, B, seed, amod=None):
    rs = np.random.default_rng(seed)
    a = rs.integers(0, amod or 2 * op.N, (B, op.n), dtype=np.uint64)
    acc = rs.integers(0, op.Q, (B, 2, op.N), dtype=np.uint64)
    return a, acc


@pytest.mark.parametrize("B", [1, 7, 9])
def test_f64duo_eval_acc_matches_oracle(f64duo, B):
    op, ctx, orc = f64duo["op"], f64duo["ctx"], f64duo["orc"]
    a, acc = _inputs(op, B, 500 + B)
    out = ctx.EvalAcc(a, 2 * op.N, acc)
    assert np.array_equal(out.reshape(B, -1), orc.eval_acc(a, 2 * op.N, acc).reshape(B, -1))


def test_f64duo_wrap_rounds_match_oracle(f64duo):
    """Accumulators whose centred coefficients sit in the WRAP range: the reference's digits sum to
    c - 2^50 there, so round 0 (and more) runs the correction digit through the split transform."""
    op, ctx, orc = f64duo["op"], f64duo["ctx"], f64duo["orc"]
    rs = np.random.default_rng(77)
    B = 3
    a = rs.integers(0, 2 * op.N, (B, op.n), dtype=np.uint64)
    lo, hi = (1 << 49) - (1 << 24), op.Q // 2
    acc = rs.integers(lo, hi, (B, 2, op.N), dtype=np.uint64)
    acc[1, :, ::3] = rs.integers(0, op.Q, (2, (op.N + 2) // 3), dtype=np.uint64)
    out = ctx.EvalAcc(a, 2 * op.N, acc)
    assert np.array_equal(out, orc.eval_acc(a, 2 * op.N, acc))
    with ctx.knobs_set(duo=0):
        assert np.array_equal(out, ctx.EvalAcc(a, 2 * op.N, acc))


@pytest.mark.parametrize("B", [64, 128])
def test_f64duo_equals_one_workgroup_form(f64duo, B):
    op, ctx = f64duo["op"], f64duo["ctx"]
    a, acc = _inputs(op, B, 600 + B, amod=1024)
    two = ctx.EvalAcc(a, 1024, acc)
    with ctx.knobs_set(duo=0):
        one = ctx.EvalAcc(a, 1024, acc)
    assert np.array_equal(two, one)
    idx = [0, B // 2, B - 1]
    assert np.array_equal(two[idx], f64duo["orc"].eval_acc(a[idx], 1024, acc[idx]))


def test_f64duo_evalsign_shard_decrypts(oracle):
    """EvalSign (15 chained bootstraps) at C5's per-GPU shard, 128: duo = one-workgroup form = oracle on a
    sample, and every output decrypts to the sign away from the boundaries."""
    import tfhe_amd

    op, cp = oracle.params_from_set("STD128Q"), tfhe_amd.params_from_set("STD128Q")
    rng = oracle.Rng(33)
    sk, bsk, ksk = oracle.keygen(op, rng)
    ctx = tfhe_amd.BinFHEContextHIP(cp).GPUSetup(bsk, ksk)
    orc = oracle.Oracle(op, bsk, ksk)
    del bsk, ksk
    try:
        p = (op.q // 128 // 2) * (QIN // op.q)
        rs = np.random.default_rng(10)
        ms = rs.integers(0, p, 128)
        ct = np.stack([oracle.encrypt(op, rng, sk, int(m), p, QIN) for m in ms])
        out = ctx.EvalSign(ct, QIN)
        with ctx.knobs_set(duo=0):
            ref = ctx.EvalSign(ct, QIN)
        assert np.array_equal(out, ref)
        assert np.array_equal(out[[0, 77]], orc.eval_sign(ct[[0, 77]], QIN))
        dec = np.array([oracle.decrypt(op, sk, r, 2, op.q) for r in out])
        dist = np.minimum(np.abs(ms - p // 2), np.minimum(ms, p - ms))
        bad = np.flatnonzero(dec != (ms >= p // 2))
        assert np.all(dist[bad] < 64), (bad, ms[bad])
        assert ctx.info().duo_timeouts == 0
    finally:
        ctx.GPUClean()
        orc.close()


def test_f64duo_partner_timeout_is_recomputed(oracle):
    """Probe 5 (test library): member 1 of pair 0 stops publishing at round 2; both members time out, and
    the rescue launch (f64w from the saved inputs) returns the exact result; duo_timeouts counts both."""
    import tfhe_amd

    op, cp = oracle.params_from_set("STD128Q"), tfhe_amd.params_from_set("STD128Q")
    bsk, ksk = oracle.kat_keys(op, oracle.Rng(92))
    ctx = tfhe_amd.BinFHEContextHIP(cp, library=tfhe_amd.capi.TEST_LIB).GPUSetup(bsk, ksk)
    orc = oracle.Oracle(op, bsk, ksk)
    del bsk, ksk
    try:
        a, acc = _inputs(op, 9, 700)
        want = orc.eval_acc(a, 2 * op.N, acc)
        assert np.array_equal(ctx.EvalAcc(a, 2 * op.N, acc), want)
        with ctx.knobs_set(probe=5):
            got = ctx.EvalAcc(a, 2 * op.N, acc)
        assert np.array_equal(got, want)
        assert ctx.info().duo_timeouts == 2
        assert np.array_equal(ctx.EvalAcc(a, 2 * op.N, acc), want)
        assert ctx.info().duo_timeouts == 2
    finally:
        ctx.GPUClean()
        orc.close()



def test_f64duo_two_streams_and_two_contexts(oracle):
    """Verdict r5 item 7: the duo form outside its usual single-stream use.
    * One context, two streams, no host sync between the launches: the device's one exchange buffer is
      fenced (duo.hpp duo_serialised), so both batches are exact and no partner times out.
    * Two contexts (two exchange buffers), 128 + 128 ciphertexts launched at once on two streams: 512
      workgroups that need one CU each, so some members may run while their partners wait behind the other
      launch.  The partner wait is bounded by time (10 ms of s_memrealtime per round), a timed-out pair is
      recomputed by the rescue launch: outputs exact, the whole thing done in well under a second (the
      round-5 bound of 2^24 polls was seconds per stuck member).  duo_timeouts is reported, any value."""
    import time

    import torch

    import tfhe_amd

    op, cp = oracle.params_from_set("STD128Q"), tfhe_amd.params_from_set("STD128Q")
    bsk, ksk = oracle.kat_keys(op, oracle.Rng(93))
    ctxs = [tfhe_amd.BinFHEContextHIP(cp).GPUSetup(bsk, ksk) for _ in range(2)]
    orc = oracle.Oracle(op, bsk, ksk)
    del bsk, ksk
    lib = tfhe_amd.lib()
    dev = torch.device("cuda", 0)
    streams = [torch.cuda.Stream(dev) for _ in range(2)]
    try:
        B = 128
        ins = [_inputs(op, B, 800 + k, amod=1024) for k in range(2)]
        with ctxs[0].knobs_set(duo=0):
            want = [ctxs[0].EvalAcc(a, 1024, acc) for a, acc in ins]
        for k in range(2):
            assert np.array_equal(want[k][[0, B - 1]], orc.eval_acc(ins[k][0][[0, B - 1]], 1024, ins[k][1][[0, B - 1]]))
        d_a = [torch.from_numpy(a.astype(np.int64)).to(dev) for a, _ in ins]

        def run(pairs):
            d_acc = [torch.from_numpy(acc.astype(np.int64)).to(dev) for _, acc in ins]
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for k, ctx in enumerate(pairs):
                tfhe_amd.capi.check(lib.tfhe_eval_acc_device(ctx.handle, B, d_a[k].data_ptr(), 1024, d_acc[k].data_ptr(),
                                                             streams[k].cuda_stream), "eval_acc_device")
            torch.cuda.synchronize(dev)
            dt = time.perf_counter() - t0
            return [x.cpu().numpy().astype(np.uint64) for x in d_acc], dt

        got, dt1 = run([ctxs[0], ctxs[0]])  # one context, two streams
        assert all(np.array_equal(g, w) for g, w in zip(got, want))
        assert ctxs[0].info().duo_timeouts == 0
        got, dt2 = run(ctxs)  # two contexts at once
        assert all(np.array_equal(g, w) for g, w in zip(got, want))
        timeouts = sum(c.info().duo_timeouts for c in ctxs)
        print(f"one context two streams {dt1 * 1e3:.1f} ms; two contexts {dt2 * 1e3:.1f} ms, duo_timeouts {timeouts}")
        assert dt2 < 1.0
    finally:
        for c in ctxs:
            c.GPUClean()
        orc.close()


# ---- round 6: the STD192 class (k_blind_rotate_f64wduo<0, false, false, 2>: Q < 2^40, no reductions, two
# transformed digits + C', the top digit eliminated exactly) -- "What's missing" 2 of the round-5 verdict ----
@pytest.fixture(scope="module")
def f64duo192(shared_kat):
    s = shared_kat("STD192")  # the session's shared context
    ctx = s["ctx"]
    assert ctx.info().br_kernel == 3 and ctx.knobs()["duo"] == 128
    yield s
    assert ctx.info().duo_timeouts == 0


@pytest.mark.parametrize("B", [1, 9])
def test_std192_duo_eval_acc_matches_oracle(f64duo192, B):
    op, ctx, orc = f64duo192["op"], f64duo192["ctx"], f64duo192["orc"]
    a, acc = _inputs(op, B, 900 + B)
    half = op.Q >> 1
    acc[0, :, :6] = [0, op.Q - 1, half, half + 1, half - 1, 1]  # boundary coefficients (centring, extreme digits)
    assert np.array_equal(ctx.EvalAcc(a, 2 * op.N, acc), orc.eval_acc(a, 2 * op.N, acc))


@pytest.mark.parametrize("B", [64, 128])
def test_std192_duo_equals_one_workgroup_form(f64duo192, B):
    op, ctx = f64duo192["op"], f64duo192["ctx"]
    a, acc = _inputs(op, B, 950 + B, amod=1024)
    two = ctx.EvalAcc(a, 1024, acc)
    with ctx.knobs_set(duo=0):
        one = ctx.EvalAcc(a, 1024, acc)
    assert np.array_equal(two, one)
    idx = [0, B - 1]
    assert np.array_equal(two[idx], f64duo192["orc"].eval_acc(a[idx], 1024, acc[idx]))


def test_std192_duo_gates_decrypt(oracle):
    """STD192 NAND / XOR at 128 gates (the duo form) with valid keys: every output decrypts, and equals the
    one-workgroup form and the oracle on a sample."""
    import tfhe_amd

    op, cp = oracle.params_from_set("STD192"), tfhe_amd.params_from_set("STD192")
    rng = oracle.Rng(35)
    sk, bsk, ksk = oracle.keygen(op, rng)
    ctx = tfhe_amd.BinFHEContextHIP(cp).GPUSetup(bsk, ksk)
    orc = oracle.Oracle(op, bsk, ksk)
    del bsk, ksk
    try:
        rs = np.random.default_rng(12)
        m1, m2 = rs.integers(0, 2, 128), rs.integers(0, 2, 128)
        c1 = np.stack([oracle.encrypt(op, rng, sk, int(m), 4, op.q) for m in m1])
        c2 = np.stack([oracle.encrypt(op, rng, sk, int(m), 4, op.q) for m in m2])
        out = ctx.EvalBinGate("NAND", c1, c2)
        with ctx.knobs_set(duo=0):
            assert np.array_equal(out, ctx.EvalBinGate("NAND", c1, c2))
        assert np.array_equal(out[[0, 127]], orc.eval_bin_gate("NAND", c1[[0, 127]], c2[[0, 127]]))
        dec = [oracle.decrypt(op, sk, r, 4, op.q) for r in out]
        assert dec == [1 - (int(x) & int(y)) for x, y in zip(m1, m2)]
        assert ctx.info().duo_timeouts == 0
    finally:
        ctx.GPUClean()
        orc.close()


def test_std192_duo_partner_timeout_is_recomputed(oracle):
    """Probe 5 on the STD192 instance (test library): the rescue is f64w<false, false, 2>'s."""
    import tfhe_amd

    op, cp = oracle.params_from_set("STD192"), tfhe_amd.params_from_set("STD192")
    bsk, ksk = oracle.kat_keys(op, oracle.Rng(95))
    ctx = tfhe_amd.BinFHEContextHIP(cp, library=tfhe_amd.capi.TEST_LIB).GPUSetup(bsk, ksk)
    orc = oracle.Oracle(op, bsk, ksk)
    del bsk, ksk
    try:
        a, acc = _inputs(op, 9, 960)
        want = orc.eval_acc(a, 2 * op.N, acc)
        with ctx.knobs_set(probe=5):
            assert np.array_equal(ctx.EvalAcc(a, 2 * op.N, acc), want)
        assert ctx.info().duo_timeouts == 2
    finally:
        ctx.GPUClean()
        orc.close()
