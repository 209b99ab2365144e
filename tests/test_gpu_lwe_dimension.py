"""GPU: the LWE dimension n swept through every blind rotation and key switch.

n is the number of rounds of the blind rotation and the number of columns of the key switch.  tfhe_params_finish
admits any n >= 1 and so does every dispatch predicate, while every kernel's round loop has structure that depends
on n: fast4's folded accumulator is reduced every eighth round and its key prefetch re-reads the last round's
rows; f64w's vote flags and the exchange buffers of the two-workgroup kernels are indexed by round parity; sf2,
gen2 and gen3 stage n rotation exponents behind their polynomials; n_pad, the column tiles of the tiled key switch
and the chunks of the gather are functions of n.  The rest of the suite runs n = 32 and the sets' own (502 .. 2048).

Every case below is a standard set or a params_from_logq context with n overwritten (test_gpu_modulus_edges.
_edge_pair: tfhe_params_finish through the C-ABI, the fields mirrored into the oracle's parameters), seeded random
keys (lwe_dim.kat_edge_keys: a random KSK, the first four BSK rows at 0, Q - 1, Q/2, Q/2 + 1), and asserts the
kernel family it routes to (tfhe_info.br_kernel).  n runs through lwe_dim.N_SWEEP = 1 .. 9, 15, 16, 17 (the generic
kernels, which have no eight-round period, through N_THIN = 1 .. 5, 9, 16, 17: SWEEP below).

Three references, none of them the code under test:
  (a) the oracle: EvalAcc word for word for every form of the case (FORMS below), both a-moduli, B = 5;
  (b) composition: the n-round context equals the (n - k)-round context (tail slice of the same BSK) applied to the
      output of the k-round context (head slice), at lwe_dim.COMPOSE, on the default form and for STD128 also on
      variant 71 -- the kernel's final state at an intermediate n against the kernel itself, no oracle involved;
  (c) end to end through the real key switch against the oracle: NAND and XOR (three rotations back to back), the
      two-stage EvalFunc of helpers.cube_lut on the arbFunc contexts, EvalSign at 2^23 on the logQ = 23 context;
      under the default key switch, the gather (ks_tiled_min = 0) and the tiled form (ks_tiled_min = 1, its `[ks]`
      trace line asserted).
Then the key switch alone at n = 1, 2, 7, 8, 9 (ks_model.small_cases: n_pad smaller than one column tile) against
the gather, the oracle and the integer model, and keys generated on the device at n = 1, 2, 9.

One family's contexts are alive at a time (the module-scoped `family` fixture; the items are listed family by
family).  The last test asserts that every form of every case ran at every n and prints the seconds per family.
"""
import os
import time

import numpy as np
import pytest

import ks_model as km
import lwe_dim as ld
from helpers import cube_lut

pytestmark = pytest.mark.gpu

QIN = 1 << 23


def F(label, variant=0, pair=None, host=False, **knobs):
    """One launch form: knobs for knobs_set, a tfhe_set_kernel_variant build, whether the pair instance must (True)
    or must not (False) count the launch, host: the host-array EvalAcc (completion flags)."""
    return dict(label=label, variant=variant, pair=pair, host=host, knobs=knobs)


STD128_FORMS = [
    F("two-group", pair=False),                       # split4 (default 384) covers B = 5
    F("one-group", pair=False, split4=0),
    F("pair", pair=True, pair_min=1, split4=0),       # as the default takes it from pair_min on: the fused pair
    F("variant 70", 70, pair=True, split4=0),
    F("variant 71", 71, pair=True, split4=0),
    F("variant 61", 61, pair=False, split4=0),
    F("variant 86", 86, pair=False, split4=0),
    F("flagged", pair=False, host=True, acc_flags=1, trace=1),
]
SF_FORMS = lambda d: [F(f"sfduo<{d}>"), F(f"sf2<{d}>", duo=0), F("gen3sf", duo=0, sf2=0)]  # noqa: E731
F64_FORMS = [F("f64wduo"), F("f64w", duo=0)]

# case -> family, base, br_kernel, forms; env: read at setup; e2e: the ops of reference (c)
CASES = {
    "std128": dict(family="fast4", base="STD128", kernel=1, forms=STD128_FORMS, e2e=("NAND", "XOR"), also=71),
    "logq11": dict(family="fast4", base=("STD128", False, 11, 0, 0, 0), kernel=1, forms=[F("d6")], e2e=("NAND", "XOR")),
    "logq11-thr1": dict(family="fast4", base=("STD128", False, 11, 0, 0, 1), kernel=1, forms=[F("5 x 5 thrown")],
                        e2e=("NAND", "XOR")),
    "std128ap": dict(family="fast4", base="STD128_AP", kernel=1, forms=[F("3 x 9 unfolded")], e2e=("NAND", "XOR")),
    "std192": dict(family="f64", base="STD192", kernel=3, forms=F64_FORMS, e2e=("NAND", "XOR")),
    "std128q": dict(family="f64", base="STD128Q", kernel=3, forms=F64_FORMS, e2e=("NAND", "XOR"), late_wrap=True),
    "arb12": dict(family="sf", base=ld.ARB12, kernel=5, forms=SF_FORMS(1), e2e=("FUNC",)),
    "logq23": dict(family="sf", base=ld.LOGQ23, kernel=5, forms=SF_FORMS(2), e2e=("NAND", "XOR", "SIGN")),
    "ches18": dict(family="sf", base=ld.CHES18, kernel=5, forms=[F("sf2<3>")], e2e=("FUNC",)),
    "toy": dict(family="generic", base="TOY", kernel=0, forms=[F("generic v1")], e2e=("NAND", "XOR")),
    "std128-generic": dict(family="generic", base="STD128", kernel=0, env=("TFHE_FORCE_GENERIC", "1"),
                           forms=[F("gen2 u32")], e2e=("NAND", "XOR")),
    "arb12-generic": dict(family="generic", base=ld.ARB12, kernel=0, env=("TFHE_SF", "0"), forms=[F("gen3 u64")],
                          e2e=("FUNC",)),
    "logq11-n2048": dict(family="generic", base=("TOY", False, 11, 2048, 0, 0), kernel=0,
                         forms=[F("gen3 u32", generic=0), F("gen2 u32", generic=2)], e2e=("NAND", "XOR")),
    "arb12-n4096": dict(family="generic", base=("TOY", True, 12, 4096, 0, 1), kernel=0, forms=[F("gen2 x 1024")],
                        e2e=("FUNC",)),
    "logq23-n8192": dict(family="generic", base=("TOY", False, 23, 8192, 0, 1), kernel=0, forms=[F("gen2 x 1024")],
                         e2e=("NAND", "XOR")),
}
FAMILIES = ("fast4", "f64", "sf", "generic")
SF2P_N = (1, 2, 9)
# The generic family (six contexts per n, KSKs of up to 264 MB at N = 8192) measured 17 s over N_SWEEP; its kernels
# have no eight-round period, so it takes lwe_dim.N_THIN.  Nothing else is thinned.
SWEEP = {"fast4": ld.N_SWEEP, "f64": ld.N_SWEEP, "sf": ld.N_SWEEP, "generic": ld.N_THIN}

RAN = {}      # (case, form label) -> the n it ran at
SECONDS = {}  # family -> seconds in its items


class Ctx:
    """One context of a case at one n with its oracle, the inputs of (a) and the oracle's memoised answers."""

    def __init__(self, oracle, case, n, keys, tag, calls=None):
        from test_gpu_modulus_edges import _edge_pair, _late_wrap_inputs

        self.case, self.n, self.spec = case, n, CASES[case]
        env = self.spec.get("env")
        if env:
            os.environ[env[0]] = env[1]
        try:  # the environment is read at setup
            self.cp, self.op, self.ctx, self.orc = _edge_pair(oracle, self.spec["base"], n=n, keys=self._keep(keys))
        finally:
            if env:
                os.environ.pop(env[0], None)
        assert self.cp.n == self.op.n == n
        k = self.ctx.info().br_kernel
        print(f"{case} n = {n}{tag}: N = {self.cp.N}, Q = {self.cp.Q}, br_kernel = {k}")
        assert k == self.spec["kernel"], (case, n, k)
        self._want = {}
        if calls is not None:  # calls(op) -> [(what, a, amod, acc)]: another module's inputs
            self.calls = calls(self.op)
            return
        a, self.acc = ld.sweep_inputs(self.op, 7 + n)
        self.calls = [(f"a mod {m}", a[m], m, self.acc) for m in sorted(a)]
        if self.spec.get("late_wrap") and n >= 2:  # a_i = 0 for i < n - 1: the vote flag of parity (n - 1) & 1
            la, lacc = _late_wrap_inputs(self.op, 11 + n, ld.B)
            assert not la[:, :-1].any() and la[:, -1].all()
            self.calls.append(("late wrap", la, int(self.op.q), lacc))

    def _keep(self, keys):
        def wrapped(cp, op):
            self.bsk, ksk = keys(cp, op)
            return self.bsk, ksk

        return wrapped

    def want(self, i):
        if i not in self._want:
            _, a, amod, acc = self.calls[i]
            self._want[i] = self.orc.eval_acc(a, amod, acc)
        return self._want[i]

    def close(self):
        self.ctx.GPUClean()
        self.orc.close()


class Pool:
    """The contexts of one family, built on first use and closed together."""

    def __init__(self, oracle, name):
        self.oracle, self.name, self.made = oracle, name, {}

    def get(self, case, n, keys=None, tag="", calls=None):
        assert CASES[case]["family"] == self.name
        key = (case, n, tag)
        if key not in self.made:
            seed = 1000 * (list(CASES).index(case) + 1) + n
            self.made[key] = Ctx(self.oracle, case, n, keys or ld.kat_edge_keys(self.oracle, seed), tag, calls)
        return self.made[key]

    def close(self):
        for c in self.made.values():
            c.close()
        self.made = {}


@pytest.fixture(scope="module")
def family(request, oracle):
    pool = Pool(oracle, request.param)
    yield pool
    pool.close()


def _stderr(capfd):
    """What the library wrote to stderr since the last call; the test's own stdout is printed again."""
    cap = capfd.readouterr()
    print(cap.out, end="")
    return cap.err


def _run(c, form, a, amod, acc, capfd=None):
    """EvalAcc under one form -> the new accumulators; asserts what tells that the form ran."""
    import tfhe_amd
    from test_gpu_fast4_pair import _eval_acc_device

    ctx, lib = c.ctx, tfhe_amd.lib()
    fast = c.spec["kernel"] == 1
    if form["variant"]:
        assert lib.tfhe_set_kernel_variant(form["variant"]) == 0
    try:
        with ctx.knobs_set(**form["knobs"]):
            kn = ctx.knobs()
            if form["label"] == "two-group":
                assert kn["split4"] >= ld.B
            if form["label"].startswith(("sfduo", "f64wduo")):
                assert kn["duo"] >= ld.B
            before = ctx.pair_launches() if fast else 0
            if form["host"]:
                _stderr(capfd)
                got = ctx.EvalAcc(a, amod, acc)
                assert "(flagged output)" in _stderr(capfd), (c.case, c.n, "the completion flags did not run")
            else:
                got = _eval_acc_device(ctx, a, amod, acc)
            if fast and form["pair"] is not None:
                assert (ctx.pair_launches() > before) == form["pair"], (c.case, c.n, form["label"])
    finally:
        if form["variant"]:
            lib.tfhe_set_kernel_variant(0)
    assert ctx.info().br_kernel == c.spec["kernel"]
    return got


def _oracle_item(pool, case, n, capfd):
    """(a): every form of the case at this n against the oracle."""
    c = pool.get(case, n)
    t0 = c.ctx.info().duo_timeouts
    for form in c.spec["forms"]:
        for i, (what, a, amod, acc) in enumerate(c.calls):
            got = _run(c, form, a, amod, acc, capfd)
            bad = int(np.count_nonzero(got != c.want(i)))
            print(f"{case} n = {n}: form {form['label']}, {what}: {bad} of {got.size} words differ from the oracle")
            assert bad == 0, (case, n, form["label"], what)
        RAN.setdefault((case, form["label"]), set()).add(n)
    assert c.ctx.info().duo_timeouts == t0 == 0
    # a = 0 only changes the accumulator's form, every other row moves
    w = c.want(0)
    assert np.array_equal(w[3], ld.transpose0(c.acc, int(c.op.Q))[3]) and not np.array_equal(w[0], c.acc[0])


def _sf2p_item(pool, case, n):
    """sf2p (two ciphertexts per workgroup, from 512) at B = 513: the whole batch equals sf2, rows 0, 256 and 512
    equal the oracle (test_gpu_modulus_edges.test_sf_two_digits_largest_c)."""
    c = pool.get(case, n)
    op, ctx, Bp = c.op, c.ctx, 513
    assert ctx.knobs()["sf2p"] != 0
    rs = np.random.default_rng(513 + n)
    amod = 2 * op.N
    a = rs.integers(0, amod, (Bp, n), dtype=np.uint64)
    acc = rs.integers(0, op.Q, (Bp, 2, op.N), dtype=np.uint64)
    idx = [0, 256, 512]
    acc[idx] = c.acc[:3]
    pair = _run(c, F("sf2p", duo=0), a, amod, acc)
    one = _run(c, F("sf2<2>", duo=0, sf2p=0), a, amod, acc)
    want = c.orc.eval_acc(a[idx], amod, acc[idx])
    print(f"{case} n = {n}: form sf2p at B = {Bp}: {int(np.count_nonzero(pair != one))} words differ from sf2, "
          f"{int(np.count_nonzero(pair[idx] != want))} from the oracle on ciphertexts {idx}")
    assert np.array_equal(pair, one)
    assert np.array_equal(pair[idx], want)
    RAN.setdefault((case, "sf2p"), set()).add(n)


def _compose_item(pool, case, n, k, capfd):
    """(b): n rounds = (n - k) rounds over the tail slice after k rounds over the head slice."""
    whole = pool.get(case, n)
    forms = [whole.spec["forms"][0]]
    if whole.spec.get("also"):
        forms += [f for f in whole.spec["forms"] if f["variant"] == whole.spec["also"]]
    Q = int(whole.op.Q)
    for what, a, amod, acc in whole.calls:
        (hb, ha), (tb, ta) = ld.split_rounds(n, whole.bsk, a, k)
        zero = lambda cp, op: np.zeros(cp.ksk_words(), dtype=np.uint64)  # noqa: E731
        head = pool.get(case, k, lambda cp, op: (hb, zero(cp, op)), f" (rounds 0..{k - 1} of {n})")
        tail = pool.get(case, n - k, lambda cp, op: (tb, zero(cp, op)), f" (rounds {k}..{n - 1} of {n})")
        for form in forms:
            want = _run(whole, form, a, amod, acc, capfd)
            got = ld.compose(lambda *x: _run(head, form, *x, capfd), lambda *x: _run(tail, form, *x, capfd), ha, ta,
                             amod, acc, Q)
            bad = int(np.count_nonzero(got != want))
            print(f"{case} n = {n} = {k} + {n - k}: form {form['label']}, {what}: {bad} of {got.size} words differ")
            assert bad == 0, (case, n, k, form["label"], what)
        assert not np.array_equal(want[0], ld.transpose0(acc, Q)[0])


def _e2e_item(pool, case, n, capfd):
    """(c): whole ops through the real key switch against the oracle, under the three key-switch settings."""
    from test_gpu_keyswitch_edges import KS_LINE

    c = pool.get(case, n)
    op, ctx, orc = c.op, c.ctx, c.orc
    rs = np.random.default_rng(31 * n + len(case))
    q = int(op.q)
    c1, c2 = (rs.integers(0, q, (ld.B, n + 1), dtype=np.uint64) for _ in range(2))
    c1[3, :n], c1[4, :n] = 0, q - 1
    big = rs.integers(0, QIN, (ld.B, n + 1), dtype=np.uint64)
    lut = cube_lut(q)
    ops = {  # name -> (device, oracle, fewest key switches)
        "NAND": (lambda: ctx.EvalBinGate("NAND", c1, c2), lambda: orc.eval_bin_gate("NAND", c1, c2), 1),
        "XOR": (lambda: ctx.EvalBinGate("XOR", c1, c2), lambda: orc.eval_bin_gate("XOR", c1, c2), 3),
        "FUNC": (lambda: ctx.EvalFunc(c1, lut), lambda: orc.eval_func(c1, lut), 2),
        "SIGN": (lambda: ctx.EvalSign(big, QIN), lambda: orc.eval_sign(big, QIN), 2),
    }
    t0 = ctx.info().duo_timeouts
    for name in c.spec["e2e"]:
        dev, ref, fewest = ops[name]
        want = ref()
        assert want.shape == (ld.B, n + 1)
        for ks, knobs in (("default", {}), ("gather", dict(ks_tiled_min=0)), ("tiled", dict(ks_tiled_min=1))):
            _stderr(capfd)
            with ctx.knobs_set(trace=1, **knobs):
                got = dev()
            lines = KS_LINE.findall(_stderr(capfd))
            bad = int(np.count_nonzero(got != want))
            print(f"{case} n = {n}: {name}, key switch {ks}: {bad} of {got.size} words differ from the oracle, "
                  f"{len(lines)} tiled launches")
            assert bad == 0, (case, n, name, ks)
            if ks == "gather":
                assert lines == [], (case, n, name, lines)
            elif ks == "tiled":
                assert len(lines) >= fewest, (case, n, name, lines)
        RAN.setdefault((case, name), set()).add(n)
    assert ctx.info().duo_timeouts == t0 == 0


def _items():
    out = []
    for fam in FAMILIES:
        for case, spec in CASES.items():
            if spec["family"] != fam:
                continue
            out += [(fam, "oracle", case, (n,)) for n in SWEEP[fam]]
            if case == "logq23":
                out += [(fam, "sf2p", case, (n,)) for n in SF2P_N]
            out += [(fam, "compose", case, nk) for nk in ld.COMPOSE]
            out += [(fam, "e2e", case, (n,)) for n in SWEEP[fam]]
    return out


ITEMS = _items()


@pytest.mark.parametrize("family,kind,case,at", ITEMS, indirect=["family"],
                         ids=[f"{f}-{c}-{k}-" + "-".join(f"{x}" for x in at) for f, k, c, at in ITEMS])
def test_lwe_dimension(family, capfd, kind, case, at):
    t0 = time.perf_counter()
    try:
        if kind == "oracle":
            _oracle_item(family, case, at[0], capfd)
        elif kind == "sf2p":
            _sf2p_item(family, case, at[0])
        elif kind == "compose":
            _compose_item(family, case, at[0], at[1], capfd)
        else:
            _e2e_item(family, case, at[0], capfd)
    finally:
        SECONDS[family.name] = SECONDS.get(family.name, 0.0) + time.perf_counter() - t0


# ---------------------------------------------------------------------------------------------------------------
# the key switch alone
# ---------------------------------------------------------------------------------------------------------------
KS_NAMES = ("u16-packed", "u32-bound", "split-b3")  # STD128 (u16 keys, packed sums), STD192 (u32), logQ = 12 (records)
KS_CASES = km.small_cases(KS_NAMES)


@pytest.mark.parametrize("name,n", KS_CASES, ids=[f"{a}-n{b}" for a, b in KS_CASES])
def test_key_switch_alone_at_small_n(oracle, capfd, name, n):
    """tfhe_mkm_switch_device at n = 1, 2, 7, 8, 9: n_pad (8 u16, 4 u32 or 2 u64 words per 16-byte piece) is smaller
    than one column tile, so every piece past it is a clamped one.  A random and an all-maximal KSK; the four edge rows
    and random rows of ks_model.make_ext; B = 1 (each of the first five rows alone) and 257; output moduli q and qKS;
    ks_split 1, 2 and the default.  Whole batch against the oracle and the gather, first six rows against the model."""
    import torch
    from test_gpu_keyswitch_edges import Edge, _check

    t0 = time.perf_counter()
    spec = km.CONTEXTS[name]
    for fill in ("random", "max"):
        e = Edge(oracle, name, n, fill)
        try:
            assert e.cp.n == n and e.ctx.info().ksk_device_bytes > 0
            for first, B in [(0, 257)] + [(r, 1) for r in range(5)]:
                for fmod in (int(e.op.q), int(e.op.qKS)):
                    gather, lines = e.run(capfd, first, B, fmod, ks_tiled_min=0)
                    assert lines == [], (name, n, "the gather printed a [ks] line", lines)
                    _check(e, gather, first, B, fmod, "gather")
                    for split in (1, 2, e.default_split):
                        out, lines = e.run(capfd, first, B, fmod, ks_tiled_min=1, ks_split=split)
                        what = f"tiled ks_split = {split}"
                        _check(e, out, first, B, fmod, what)
                        assert torch.equal(out, gather), (name, n, fill, B, fmod, what, "differs from the gather")
                        assert len(lines) == 1, (name, n, what, lines)
                        gotB, kb, sums, pk, _, _, _, nsplit = lines[0]
                        packed = bool(spec.get("pk"))
                        assert (gotB, kb, sums, pk) == (B, spec["kb"], spec["sums"][0 if packed else 1], int(packed))
                        assert nsplit == 1 if split == 1 else nsplit <= 2 if split == 2 else nsplit >= 1, lines[0]
        finally:
            e.close()
    SECONDS["key switch"] = SECONDS.get("key switch", 0.0) + time.perf_counter() - t0


# ---------------------------------------------------------------------------------------------------------------
# keys generated on the device
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SF2P_N)
@pytest.mark.parametrize("name", ["TOY", "STD128"])
def test_device_keygen_at_small_n(oracle, name, n):
    """tfhe_keygen_device / tfhe_setup_keygen at n = 1, 2, 9 equal the oracle's keygen under the rules of
    tests/test_gpu_keygen.py::test_keys_equal_oracle, and one NAND batch through the generated context equals the
    oracle on the same keys."""
    import tfhe_amd
    from phases import lowered_params
    from test_gpu_keygen import SEED, gauss_diffs

    t0 = time.perf_counter()
    cp, op = lowered_params(oracle, name, n)
    rng = oracle.Rng(SEED)
    sk_w, bsk_w, ksk_w = oracle.keygen(op, rng)
    sk, bsk, ksk = tfhe_amd.keygen(cp, SEED)
    assert tfhe_amd.keygen.seed_after == rng.s
    assert sk.shape == (n,) and np.array_equal(sk, sk_w)
    k_got, k_want = ksk.reshape(-1, n + 1), ksk_w.reshape(-1, n + 1)
    assert np.array_equal(k_got[:, :n], k_want[:, :n]), "KSK A words"
    b_got, b_want = bsk.reshape(-1, 2, cp.N), bsk_w.reshape(-1, 2, cp.N)
    assert np.array_equal(b_got[:, 0], b_want[:, 0]), "BSK a polynomials"
    gauss_diffs(k_got[:, n], k_want[:, n], cp.qKS, f"{name} n = {n} KSK B")
    gauss_diffs(b_got[:, 1], b_want[:, 1], cp.Q, f"{name} n = {n} BSK b")
    A, sk2 = tfhe_amd.BinFHEContextHIP.from_keygen(cp, SEED)
    orc = oracle.Oracle(op, bsk, ksk)  # the device's own keys: one +-1 Gaussian word would not matter here
    try:
        assert A.seed_after == rng.s and np.array_equal(sk2, sk_w)
        assert A.info().br_kernel == (1 if name == "STD128" else 0)
        erng = oracle.Rng(77 + n)
        m1, m2 = [0, 0, 1, 1, 1], [0, 1, 0, 1, 1]
        c1 = np.stack([oracle.encrypt(op, erng, sk_w, m, 4, op.q) for m in m1])
        c2 = np.stack([oracle.encrypt(op, erng, sk_w, m, 4, op.q) for m in m2])
        got = A.EvalBinGate("NAND", c1, c2)
        assert got.shape == (5, n + 1)
        assert np.array_equal(got, orc.eval_bin_gate("NAND", c1, c2))
    finally:
        A.GPUClean()
        orc.close()
    SECONDS["keygen"] = SECONDS.get("keygen", 0.0) + time.perf_counter() - t0


def test_every_form_ran_at_every_n(request):
    """Every form of every case met the oracle at every n of the sweep, sf2p at its three, every end-to-end op at
    every n; one line of seconds per family.  Reads what the items above recorded, so it is defined last and relies
    on pytest's definition order within one process; cases that a partial selection (-k, one node id) left
    incomplete are printed and not judged."""
    chosen = [it.callspec.params for it in request.session.items
              if it.module is request.module and it.originalname == "test_lwe_dimension"]
    for case, spec in CASES.items():
        mine = [p for p in chosen if p["case"] == case]
        complete = len(mine) == sum(1 for i in ITEMS if i[2] == case)
        labels = [f["label"] for f in spec["forms"]] + list(spec["e2e"])
        for label in labels:
            ran = sorted(RAN.get((case, label), ()))
            print(f"[lwe-dimension] {case}: {label}: n = {ran}" + ("" if complete else " (partial selection)"))
            if complete:
                assert tuple(ran) == SWEEP[spec["family"]], (case, label, ran)
        if case == "logq23" and complete:
            assert tuple(sorted(RAN.get((case, "sf2p"), ()))) == SF2P_N
    for fam, s in SECONDS.items():
        print(f"[lwe-dimension] {fam}: {s:.1f} s")
    print(f"[lwe-dimension] all: {sum(SECONDS.values()):.1f} s")
