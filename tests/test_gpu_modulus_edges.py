"""GPU: blind-rotation parity at the edges of each kernel family's admitted moduli.

The dispatch predicates (fast_path_supported, f64_path_supported / f64_instance_available,
sf_path_supported) admit a range of Q per family; the standard sets reach one or two moduli of each.
tfhe_params_finish is public, so a caller can reach the others.  Every case here takes a standard
set, overwrites Q (and baseG where the digit shape needs it), lowers n to 32 (the keys stay a few MB;
the key switch is not under test and gets a zero KSK), finishes the parameters through the C-ABI,
mirrors them into the oracle, asserts the kernel family the context routes to (tfhe_info.br_kernel:
0 generic, 1 fast4, 3 f64, 5 sf) and compares EvalAcc with the oracle bit for bit for every launch
form of that family.

Moduli (all prime, = 1 mod 2N; digit counts as tfhe_params_finish derives them):
  fast4   STD128, Q = 2101249 (22 bits; the smallest prime = 1 mod 2048 that keeps four 7-bit digits)
  f64     STD192, Q = 4294991873 (the smallest admitted: 2^32 + 24577), three 14-bit digits, <0, 0, 2>
  f64     STD192, Q = 1099511590913 = 2^40 - 36863 (the largest non-reducing), three 14-bit digits
  f64     STD128Q, Q = 4398044577793 = 2^42 - 1933311, baseG = 2^21: two digits, top digit inexact,
          reducing with the WRAP correction <1, 1, 1> at its smallest Q class
  generic STD128Q, Q = 2^40 - 36863, baseG = 2^20: two digits, inexact top digit, not reducing -- no
          f64w instance, must fall back
  sf      Q = 2^54 - 876543 (the largest c of the 20 NTT-friendly primes in range), logQ = 12 arbFunc
          throw = 1 (baseG 2^27, one digit) and logQ = 23 throw = 1 (baseG 2^18, two digits)
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N32 = 32  # the lowered LWE dimension


def _edge_pair(oracle, base, Q=None, baseG_log=None, expect_digits=None, n=N32, keys=None):
    """(cp, op, ctx, orc) for `base` (a set name or a params_from_logq argument tuple) with Q / baseG
    overridden (Q = None: the base's own) and the LWE dimension lowered to n; first BSK rows at the key edges,
    zero KSK.  keys: a function (cp, op) -> (bsk, ksk) that supplies the keys instead
    (tests/test_gpu_lwe_dimension.py: a random KSK, slices of another context's BSK)."""
    import tfhe_amd
    from phases import lowered_params

    cp, op = lowered_params(oracle, base, n, Q, baseG_log)
    Q = int(cp.Q)
    if expect_digits is not None:
        assert cp.digitsG - cp.numDigitsToThrow == expect_digits, cp.as_dict()
    if keys is not None:
        bsk, ksk = keys(cp, op)
    else:
        rs = np.random.default_rng(Q % (1 << 32))
        bsk = rs.integers(0, Q, cp.bsk_words(), dtype=np.uint64)
        bsk[: 4 * cp.N] = np.array([0, Q - 1, Q >> 1, (Q >> 1) + 1], dtype=np.uint64).repeat(cp.N)
        ksk = np.zeros(cp.ksk_words(), dtype=np.uint64)
    ctx = tfhe_amd.BinFHEContextHIP(cp).GPUSetup(bsk, ksk)
    orc = oracle.Oracle(op, bsk, ksk)
    return cp, op, ctx, orc


def _inputs(op, seed, B=3):
    """acc: edge rows, one ciphertext alternating Q/2, Q/2 + 1 (extreme digits), one random."""
    rs = np.random.default_rng(seed)
    Q, half = op.Q, op.Q >> 1
    acc = rs.integers(0, Q, (B, 2, op.N), dtype=np.uint64)
    acc[0, :, :8] = [0, 1, Q - 1, Q - 2, half, half + 1, half - 1, half + 2]
    alt = np.where(np.arange(op.N) % 2 == 0, half, half + 1).astype(np.uint64)
    acc[1, 0], acc[1, 1] = alt, alt[::-1]
    a = {amod: rs.integers(0, amod, (B, op.n), dtype=np.uint64) for amod in (op.q, 2 * op.N)}
    return a, acc


def _late_wrap_inputs(op, seed, B=3):
    """test_wrap_correction_late_round's construction: a_i = 0 for i < n - 1 keeps the accumulator's
    boundary values (centred c in [G^2/2 - G/2, Q/2): the top digit leaves a residual) until the last round."""
    rs = np.random.default_rng(seed)
    half, G = op.Q >> 1, op.baseG
    width = half - (G * G // 2 - G // 2)
    assert width > 1
    a = np.zeros((B, op.n), dtype=np.uint64)
    a[:, -1] = rs.integers(1, op.q, B, dtype=np.uint64)
    acc = rs.integers(0, op.Q, (B, 2, op.N), dtype=np.uint64)
    acc[:, :, 10:20] = (half - 1 - rs.integers(0, width - 1, (B, 2, 10))).astype(np.uint64)
    acc[2] = rs.integers(0, op.Q, (2, op.N), dtype=np.uint64)  # a ciphertext without residuals
    return a, acc


class _Case:
    """One edge context; check(form, **knobs) compares EvalAcc at both a-moduli with the oracle's (memoised) answer."""

    def __init__(self, name, oracle, base, Q, kernel, baseG_log=None, digits=None):
        self.name, self.kernel = name, kernel
        self.cp, self.op, self.ctx, self.orc = _edge_pair(oracle, base, Q, baseG_log, digits)
        self.a, self.acc = _inputs(self.op, 7)
        self.calls = [(self.a[m], m, self.acc) for m in sorted({self.op.q, 2 * self.op.N})]
        self._want = {}
        k = self.ctx.info().br_kernel
        print(f"{name}: Q = {Q}, digits = {self.cp.digitsG - self.cp.numDigitsToThrow} of {self.op.logG} bits, "
              f"n = {self.cp.n}, br_kernel = {k}")
        assert k == kernel, (name, k)

    def want(self, i):
        if i not in self._want:
            a, amod, acc = self.calls[i]
            self._want[i] = self.orc.eval_acc(a, amod, acc)
        return self._want[i]

    def check(self, form, **knobs):
        assert self.ctx.info().br_kernel == self.kernel
        with self.ctx.knobs_set(**knobs):
            for i, (a, amod, acc) in enumerate(self.calls):
                got = self.ctx.EvalAcc(a, amod, acc)
                bad = int(np.count_nonzero(got != self.want(i)))
                print(f"{self.name}: form {form} (knobs {knobs}), a-modulus {amod}: br_kernel = {self.kernel}, "
                      f"{bad} of {got.size} words differ from the oracle")
                assert bad == 0, (self.name, form, amod)

    def close(self):
        self.ctx.GPUClean()
        self.orc.close()


@pytest.fixture
def case(oracle):
    made = []

    def make(*args, **kw):
        made.append(_Case(*args, oracle=oracle, **kw))
        return made[-1]

    yield make
    for c in made:
        c.close()


def test_fast4_smallest_modulus(case):
    """fast4 at Q = 2101249 (STD128's four 7-bit digits hold down to 22-bit Q; the standard sets run it at
    134215681 only): the two-group form (split4 covers B = 3 by default), the one-group form (split4 = 0)
    and the multi-ciphertext builds 70 and 86."""
    import tfhe_amd

    c = case("fast4-min", base="STD128", Q=2101249, kernel=1, digits=4)
    assert c.ctx.knobs()["split4"] >= 3
    c.check("split4")
    c.check("one-group", split4=0)
    lib = tfhe_amd.lib()
    try:
        for v in (70, 86):
            assert lib.tfhe_set_kernel_variant(v) == 0
            c.check(f"variant {v}", split4=0)
    finally:
        lib.tfhe_set_kernel_variant(0)


@pytest.mark.parametrize("Q", [4294991873, 1099511590913])
def test_f64_plain_modulus_ends(case, Q):
    """f64w <RED = false, WRAP = false, 2> at the smallest admitted Q (2^32 + 24577) and the largest
    (2^40 - 36863: unreduced sums 8x those of STD192's 2^37 - 2^17 + 1; tools/bounds_f64.py walks this
    schedule at this Q); the two-workgroup form (default at this batch) and the one-workgroup form."""
    c = case(f"f64-plain-{Q}", base="STD192", Q=Q, kernel=3, digits=3)
    t0 = c.ctx.info().duo_timeouts
    c.check("f64wduo")
    assert c.ctx.info().duo_timeouts == t0 == 0
    c.check("f64w", duo=0)


def test_f64_wrap_smallest_class(case):
    """f64w <RED, WRAP, 1> at Q = 4398044577793 = 2^42 - 1933311, baseG = 2^21 (two digits, Q in (G^2 - G, G^2),
    the top digit inexact): the lower end of the instance STD128Q runs at 2^50 - 2^14 + 1.  f64wduo (default)
    and f64w (duo = 0); also the late-round WRAP construction."""
    Q = 4398044577793
    assert (1 << 42) - (1 << 21) < Q < (1 << 42)
    c = case("f64-wrap-42", base="STD128Q", Q=Q, baseG_log=21, kernel=3, digits=2)
    a, acc = _late_wrap_inputs(c.op, 11)
    c.calls.append((a, c.op.q, acc))
    c.check("f64wduo")
    assert c.ctx.info().duo_timeouts == 0
    c.check("f64w", duo=0)


def test_two_inexact_digits_below_2_40_fall_back(case, oracle):
    """Two digits with an inexact top digit at Q < 2^40 (Q = 2^40 - 36863, a prime = 1 mod 4096 in
    (2^40 - 2^20, 2^40); baseG = 2^20) would need <RED = false, WRAP = true, 1>, which is not shipped: the
    context must run the generic kernel, and equal the oracle there."""
    Q = (1 << 40) - 36863
    assert (1 << 40) - (1 << 20) < Q < (1 << 40) and Q % 4096 == 1 and oracle.lib().or_is_prime(Q)
    c = case("f64-fallback-40", base="STD128Q", Q=Q, baseG_log=20, kernel=0, digits=2)
    c.check("generic")


SF_Q = (1 << 54) - 876543


def test_sf_one_digit_largest_c(case):
    """sf at c = 876543 (the standard contexts run c = 77823 only; every fold term is 11x larger here),
    logQ = 12 arbFunc throw = 1: one 27-bit digit.  sfduo<1> (default at B <= 128), sf2<1> (duo = 0) and
    gen3sf (sf2 = 0)."""
    c = case("sf-1digit", base=("STD128", True, 12, 0, 0, 1), Q=SF_Q, kernel=5, digits=1)
    assert c.ctx.knobs()["duo"] >= 3
    c.check("sfduo<1>")
    assert c.ctx.info().duo_timeouts == 0
    c.check("sf2<1>", duo=0)
    c.check("gen3sf", duo=0, sf2=0)


def test_sf_two_digits_largest_c(case):
    """sf at c = 876543, logQ = 23 throw = 1: two 18-bit digits.  sfduo<2> (default), sf2<2> (duo = 0),
    and the pair form sf2p at B = 513 (odd: the last workgroup's second half is inactive): the whole
    batch equals sf2 and three ciphertexts of it equal the oracle (n = 32 keeps the device run in
    seconds; the oracle's 513 would not be)."""
    c = case("sf-2digit", base=("STD128", False, 23, 0, 0, 1), Q=SF_Q, kernel=5, digits=2)
    c.check("sfduo<2>")
    assert c.ctx.info().duo_timeouts == 0
    c.check("sf2<2>", duo=0)
    op, ctx = c.op, c.ctx
    B = 513
    assert ctx.knobs()["sf2p"] != 0
    rs = np.random.default_rng(513)
    a = rs.integers(0, 2 * op.N, (B, op.n), dtype=np.uint64)
    acc = rs.integers(0, op.Q, (B, 2, op.N), dtype=np.uint64)
    acc[[0, 256, 512]] = c.acc
    with ctx.knobs_set(duo=0):
        pair = ctx.EvalAcc(a, 2 * op.N, acc)
        with ctx.knobs_set(sf2p=0):
            one = ctx.EvalAcc(a, 2 * op.N, acc)
    idx = [0, 256, 512]
    want = c.orc.eval_acc(a[idx], 2 * op.N, acc[idx])
    print(f"sf-2digit: form sf2p at B = {B}: br_kernel = {ctx.info().br_kernel}, "
          f"{int(np.count_nonzero(pair != one))} words differ from sf2, "
          f"{int(np.count_nonzero(pair[idx] != want))} from the oracle on ciphertexts {idx}")
    assert np.array_equal(pair, one)
    assert np.array_equal(pair[idx], want)
