"""GPU: the gadget digits' boundaries swept through every blind rotation.

Every round of every blind rotation starts by cutting each accumulator coefficient into signed gadget digits, the
one step whose result jumps at particular values of the accumulator, and each kernel family restates the
reference's carry loop in its own closed form: fast4 a signed bit-field extract of acc + K_l, f64w a floor of an
fma followed by f - B floor(f / B + 1/2) with the WRAP vote for the residual, the special-form kernels sf_digit,
the generic kernels their own u32 and u64 extraction.  A digit sits on its tie with probability 1 / B per
coefficient and round: random accumulators at B = 2^18 .. 2^27 never meet one.

Here the accumulators are tiled from digits.boundary_values (every tie, carry ripple, first residual and end of
the centred range of the case's digit shape, in every residue of the coefficient index mod 8), and synthetic round
keys carry them into the later rounds.  Every case of test_gpu_lwe_dimension.CASES at n = 3, B = 5, both a-moduli,
every launch form (test_gpu_lwe_dimension._run), under four recipes, one context each:

  first             random keys in every round: round 0 decomposes the list under real keys.  Oracle.
  identity          IDENTITY in every round: every round decomposes the rotated and negated list; on STD128Q the
                    WRAP correction runs in consecutive rounds of both parities.  digits.identity_model and oracle.
  zero-carried      ZERO, ZERO, random: the last round decomposes the list in the representation the update leaves.
                    Oracle, and the kernel's own 1-round context over the last round's rows on the same accumulators.
  identity-carried  IDENTITY, IDENTITY, random: the same after two rounds that moved every coefficient.  Oracle; the
                    model counts the list values that enter the last round (all of rows 0 .. B - 2 where the list
                    reconstructs).

All comparisons are bit for bit.  One family's contexts are alive at a time; the last test asserts that every form
of every case ran under every recipe and prints the seconds per family.
"""
import time

import numpy as np
import pytest

import digits as dg
import lwe_dim as ld
from test_gpu_lwe_dimension import CASES, FAMILIES, F, Pool, _run

pytestmark = pytest.mark.gpu

N = dg.N_ROUNDS
SF2P_CASE = "logq23"
RECIPES_OF = {fam: dg.RECIPES for fam in FAMILIES}

RAN = {}      # (case, form label) -> the recipes it ran under
SECONDS = {}  # family -> seconds in its items


@pytest.fixture(scope="module")
def family(request, oracle):
    pool = Pool(oracle, request.param)
    yield pool
    pool.close()


def _seed(case, recipe):
    return 50000 + 100 * list(CASES).index(case) + dg.RECIPES.index(recipe)


def _calls(case):
    return lambda op: dg.inputs(op, seed=list(CASES).index(case))[1]


def _context(pool, case, recipe):
    """The case's context under the recipe's keys with the tile accumulators and rotations as its calls."""
    c = pool.get(case, N, dg.recipe_keys(pool.oracle, recipe, _seed(case, recipe)), f" ({recipe})", _calls(case))
    rounds = c.bsk.reshape(N, -1)
    assert rounds[N - 1].any() and (recipe == "first" or np.count_nonzero(rounds[0]) in (0, c.op.dG2))
    return c


def _count(got, want, who, what):
    bad = int(np.count_nonzero(got != want))
    print(f"{who}: {bad} of {got.size} words differ from {what}")
    return bad


def _item(pool, case, recipe, capfd):
    c = _context(pool, case, recipe)
    sh = dg.shape(c.op)
    Q = sh[0]
    values, _ = dg.boundary_values(*sh)
    exact = dg.reconstructs(values, *sh)
    t0 = c.ctx.info().duo_timeouts
    refs = []  # per call: [(name, words)] beside the oracle
    for i, (what, a, amod, acc) in enumerate(c.calls):
        assert a.all() and dg.list_share(acc, values) == 1.0
        refs.append([])
        if recipe == "identity":
            refs[i].append(("the integer model", dg.identity_model(a, amod, acc, *sh)))
            assert not np.array_equal(refs[i][0][1], ld.transpose0(acc, Q))
        if recipe == "identity-carried":
            last = dg.identity_states(a, amod, acc, *sh, rounds=N - 1)[-1]
            share = dg.list_share(last, values)
            print(f"{case} ({recipe}), {what}: {int(round(share * last[:-1].size))} of {last[:-1].size} words of rows "
                  f"0 .. {ld.B - 2} enter the last round as list values" + ("" if exact else " (no exact list)"))
            assert share == 1.0 or not exact
    tail = None
    if recipe == "zero-carried":
        tb = ld.split_rounds(N, c.bsk, c.calls[0][1], N - 1)[1][0]
        ksk = lambda cp, op: np.zeros(cp.ksk_words(), dtype=np.uint64)  # noqa: E731
        tail = pool.get(case, 1, lambda cp, op: (tb, ksk(cp, op)), f" (round {N - 1} of {recipe})", lambda op: [])
    for form in c.spec["forms"]:
        for i, (what, a, amod, acc) in enumerate(c.calls):
            who = f"{case} ({recipe}): form {form['label']}, {what}"
            got = _run(c, form, a, amod, acc, capfd)
            bad = _count(got, c.want(i), who, "the oracle")
            for name, words in refs[i]:
                bad += _count(got, words, who, name)
            if tail is not None:  # two ZERO rounds leave the accumulator's value: the last round alone
                alone = _run(tail, form, np.ascontiguousarray(a[:, N - 1:]), amod, acc, capfd)
                bad += _count(got, alone, who, "the kernel's own 1-round context")
            assert bad == 0, (case, recipe, form["label"], what)
        RAN.setdefault((case, form["label"]), set()).add(recipe)
    assert c.ctx.info().duo_timeouts == t0 == 0
    assert tail is None or tail.ctx.info().duo_timeouts == 0
    if case == SF2P_CASE:
        _sf2p(c, recipe)


def _sf2p(c, recipe):
    """sf2p (two ciphertexts per workgroup, from 512) at B = 513 with the tile rows at ciphertexts 0, 256 and 512:
    the whole batch equals sf2, those rows equal the oracle (test_gpu_lwe_dimension._sf2p_item)."""
    op, Bp, idx = c.op, 513, [0, 256, 512]
    assert c.ctx.knobs()["sf2p"] != 0
    rs = np.random.default_rng(513)
    amod = 2 * op.N
    a = rs.integers(1, amod, (Bp, N), dtype=np.uint64)
    acc = rs.integers(0, op.Q, (Bp, 2, op.N), dtype=np.uint64)
    a[idx] = c.calls[-1][1][:3]
    acc[idx] = c.calls[-1][3][:3]
    assert c.calls[-1][2] == amod
    pair = _run(c, F("sf2p", duo=0), a, amod, acc)
    one = _run(c, F("sf2<2>", duo=0, sf2p=0), a, amod, acc)
    who = f"{c.case} ({recipe}): form sf2p at B = {Bp}"
    bad = _count(pair, one, who, "sf2") + _count(pair[idx], c.orc.eval_acc(a[idx], amod, acc[idx]), who,
                                                 f"the oracle on ciphertexts {idx}")
    assert bad == 0, (c.case, recipe)
    RAN.setdefault((c.case, "sf2p"), set()).add(recipe)


ITEMS = [(fam, case, recipe) for fam in FAMILIES for case, spec in CASES.items() if spec["family"] == fam
         for recipe in RECIPES_OF[fam]]


@pytest.mark.parametrize("family,case,recipe", ITEMS, indirect=["family"], ids=["-".join(i) for i in ITEMS])
def test_digit_boundaries(family, capfd, case, recipe):
    t0 = time.perf_counter()
    try:
        _item(family, case, recipe, capfd)
    finally:
        SECONDS[family.name] = SECONDS.get(family.name, 0.0) + time.perf_counter() - t0


def test_every_form_ran_under_every_recipe(request):
    """Every form of every case met its references under every recipe, sf2p once per recipe; one line of seconds
    per family.  Reads what the items above recorded, so it is defined last and relies on pytest's definition order
    within one process; cases that a partial selection (-k, one node id) left incomplete are printed and not judged."""
    chosen = [it.callspec.params for it in request.session.items
              if it.module is request.module and it.originalname == "test_digit_boundaries"]
    for case, spec in CASES.items():
        want = RECIPES_OF[spec["family"]]
        complete = sum(1 for p in chosen if p["case"] == case) == len(want)
        for label in [f["label"] for f in spec["forms"]] + (["sf2p"] if case == SF2P_CASE else []):
            ran = RAN.get((case, label), set())
            print(f"[digit-boundaries] {case}: {label}: {[r for r in dg.RECIPES if r in ran]}"
                  + ("" if complete else " (partial selection)"))
            if complete:
                assert ran == set(want), (case, label, ran)
    for fam, s in SECONDS.items():
        print(f"[digit-boundaries] {fam}: {s:.1f} s")
    print(f"[digit-boundaries] all: {sum(SECONDS.values()):.1f} s")
