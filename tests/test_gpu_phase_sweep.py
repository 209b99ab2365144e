"""GPU: every input phase through each op's test-vector builder.

The test vector of a bootstrap is built on the device in three places -- k_build_testvector (the vector API, with the
k_lwe_op glue around it), k_circuit_prep and k_fcircuit_prep -- and which entry a ciphertext selects depends on its
phase alone.  Three contexts at n = 32 with valid keys (tests/phases.py: G STD128 on fast4, F logQ = 12 arbFunc and
S logQ = 23 on sf) take ciphertexts of chosen phase, all of [0, q) where the op's modulus is q, through the public
API.  Every sweep gets two checks (_check):

  (a) the plain model of tests/phases.py on the GPU's output, decrypted with numpy, at every phase outside the
      windows of half-width W (phases.W, measured by tests/test_phase_model_cpu.py) around the op's boundaries;
  (b) bit-equality with the CPU oracle on every phase inside a window, the three fixed rows of with_phase and a
      stride through the rest.

So every phase is checked against at least one reference that is not the code under test; each sweep prints the
counts and asserts that the two sets cover it.
"""
from types import SimpleNamespace

import numpy as np
import pytest

import circuit_nets as cnets
import fcircuit_nets as fnets
import phases as ph

pytestmark = pytest.mark.gpu

BASES = {"G": ph.BASE_G, "F": ph.BASE_F, "S": ph.BASE_S}


@pytest.fixture(scope="module")
def contexts(oracle):
    made = {}

    def get(name):
        if name not in made:
            orc, ctx, s = ph.sweep_context(oracle, BASES[name])
            made[name] = SimpleNamespace(name=name, orc=orc, ctx=ctx, s=s, p=orc.p)
            print(f"context {name}: n = {orc.p.n}, N = {orc.p.N}, q = {orc.p.q}, br_kernel = {ctx.info().br_kernel}")
        c = made[name]
        assert c.ctx.info().br_kernel == ph.BR_KERNEL[name], name
        return c

    yield get
    timeouts = {k: c.ctx.info().duo_timeouts for k, c in made.items()}
    for c in made.values():
        c.ctx.GPUClean()
        c.orc.close()
    assert not any(timeouts.values()), timeouts


def _check(name, got, ok, excluded, oracle_rows, stride):
    """got[B, ...]: the GPU's result per row (the last three rows are with_phase's fixed ones); ok[B]: the model
    holds for row i; excluded[B]: row i is inside a window; oracle_rows(idx) -> the oracle's got[idx].  The windows
    may exclude at most 1/8 of the sweep's rows (the fixed rows aside) from the model check."""
    B = ok.size
    model_rows = np.flatnonzero(~excluded)  # the rows the model is asserted on
    sub = excluded.copy()
    sub[B - 3:] = True
    sub[::stride] = True
    idx = np.flatnonzero(sub)               # the rows compared with the oracle
    want = oracle_rows(idx)
    ex, of = int(excluded[:B - 3].sum()), B - 3
    bad = model_rows[~ok[model_rows]]
    differ = int(np.count_nonzero(np.any((got[idx] != want).reshape(idx.size, -1), axis=1)))
    covered = np.union1d(model_rows, idx).size
    print(f"{name}: {B} rows: model on {model_rows.size} ({bad.size} wrong), oracle on {idx.size} "
          f"({differ} differ), {covered} on either; windows exclude {ex} of {of} rows")
    assert ex * 8 <= of, (name, ex, of)
    assert covered == B and want.shape[0] == idx.size, (name, covered)  # every row met the model or the oracle
    assert bad.size == 0, (name, bad[:8])
    assert differ == 0, name
    return idx.size


def _none(B):
    return np.zeros(B, dtype=bool)


# ---------------------------------------------------------------------------------------------------------------
# the vector API: k_lwe_op + k_build_testvector
# ---------------------------------------------------------------------------------------------------------------
GATES = ["OR", "AND", "NOR", "NAND", "XOR_FAST", "XNOR_FAST", "XOR", "XNOR"]


def _gate_operands(rs, s, q):
    """x of random phase; y with x + y = t and z with x - z = t, t = 0 .. q - 1: the prepared ciphertext of a
    plain gate on (x, y) runs over every phase, that of a FAST gate on (x, z), 2 (x - z), over every even one."""
    t = np.arange(q)
    px = rs.integers(0, q, q)
    x, y, z = (ph.with_phase(rs, s, p, q) for p in (px, t - px, px - t))
    return x, y, z


@pytest.mark.parametrize("q", [1024, 512, 2048])
def test_gates_at_every_phase(contexts, q):
    """All eight gates on G at q = 1024 (factor 2N / q = 2), 512 (4) and 2048 (1)."""
    c = contexts("G")
    s, ctx, orc = c.s, c.ctx, c.orc
    assert (2 * c.p.N) % q == 0
    x, y, z = _gate_operands(np.random.default_rng(q), s, q)
    px = ph.phase_of(x, s, q)
    boots = 0
    for gate in GATES:
        fast = gate.endswith("_FAST")
        w = z if fast else y
        pw = ph.phase_of(w, s, q)
        swept = np.unique(ph.gate_phase(gate if gate in ph.GATE_K else "AND", px[:q], pw[:q], q))
        assert np.array_equal(swept, np.arange(0, q, 2 if fast else 1))
        got = ctx.EvalBinGate(gate, x, w, q=q)
        ok = ph.decrypt(got, s, 4, q) == ph.bin_gate_model(gate, px, pw, q)
        rows = _check(f"{gate} q = {q}", got, ok, _none(ok.size), lambda i: orc.eval_bin_gate(gate, x[i], w[i], q=q), 97)
        boots += rows * (3 if gate in ("XOR", "XNOR") else 1)
    print(f"gates q = {q}: {boots} oracle bootstraps")


def _table_neg(rs, q, rows=None):
    """Truly negacyclic (lut[i] == q - lut[i + q/2] as integers, so no entry is 0: checkInputFunction,
    binfhe-base-scheme.cpp:162-186), a random message 1 .. 7 of p = 8 at every index."""
    shape = (q // 2,) if rows is None else (rows, q // 2)
    h = rs.integers(1, 8, shape) * (q // 8)
    return np.concatenate([h, q - h], axis=-1).astype(np.uint64)


def _table_steps(rs, q, cls, rows=None):
    """A random message of p = 8 per interval of q / 8: periodic (second half = first; entry 0 is not q/2, which
    would also pass the negacyclic probe of entry 0) or arbitrary (entry q/2 is neither entry 0 nor q - entry 0)."""
    shape = (8,) if rows is None else (rows, 8)
    m = rs.integers(0, 8, shape)
    if cls == "periodic":
        m[..., 0] = rs.integers(0, 4, shape[:-1])
        m[..., 4:] = m[..., :4]
    else:
        m[..., 0] = rs.integers(1, 4, shape[:-1])  # 1 .. 3: q - entry is 7 .. 5
        m[..., 4] = 4
    return (np.repeat(m, q // 8, axis=-1) * (q // 8)).astype(np.uint64)


def _tables(rs, q, cls, rows=None):
    return _table_neg(rs, q, rows) if cls == "negacyclic" else _table_steps(rs, q, cls, rows)


CLASS_BOOTS = {"negacyclic": 1, "periodic": 2, "arbitrary": 2}


def _func_windows(cls, phi, q):
    if cls == "negacyclic":
        return _none(phi.size)
    return ph.dist(phi, ph.lut_boundaries(q), q) <= ph.W[cls]


@pytest.mark.parametrize("cls", ["negacyclic", "periodic", "arbitrary"])
def test_eval_func_at_every_phase(contexts, cls):
    """EvalFunc on F (q = N = 2048: negacyclic and periodic at factor 2, arbitrary at 2q = 2N, factor 1), all 2048
    phases: one table for the batch, then a different random table per row, the latter again under
    host_parts = 3 (the table offset ct * lut_stride crosses sub-batches)."""
    c = contexts("F")
    s, ctx, orc, q = c.s, c.ctx, c.orc, c.p.q
    assert q == c.p.N == 2048
    rs = np.random.default_rng(len(cls))
    ct = ph.with_phase(rs, s, np.arange(q), q)
    phi = ph.phase_of(ct, s, q)
    excluded = _func_windows(cls, phi, q)
    for form, lut in (("one table", _tables(rs, q, cls)), ("a table per row", _tables(rs, q, cls, ct.shape[0]))):
        got = ctx.EvalFunc(ct, lut)
        ok = ph.decrypt(got, s, 8, q) * (q // 8) == ph.lut_model(lut, phi, q)
        rows = _check(f"EvalFunc {cls}, {form}", got, ok, excluded,
                      lambda i: orc.eval_func(ct[i], lut[i] if lut.ndim == 2 else lut), 97 if cls == "negacyclic" else 131)
        print(f"EvalFunc {cls}, {form}: {rows * CLASS_BOOTS[cls]} oracle bootstraps")
    with ctx.knobs_set(host_parts=3):
        assert np.array_equal(ctx.EvalFunc(ct, lut), got)


def test_eval_func_short_table(contexts):
    """EvalFunc on G at q = 512: a table shorter than N (factor 4; the arbitrary class at 2q = 1024, factor 2, reads
    L[x % lut_len]).  Negacyclic: the model at all 512 phases.  Arbitrary: STD128's first-stage noise (31 of
    q/8 = 128 at q = 1024) is too large for a window within 1/8 of 512 phases, so the oracle at every phase."""
    c = contexts("G")
    s, ctx, orc, q = c.s, c.ctx, c.orc, 512
    rs = np.random.default_rng(512)
    ct = ph.with_phase(rs, s, np.arange(q), q)
    phi = ph.phase_of(ct, s, q)
    lut = _table_neg(rs, q)
    got = ctx.EvalFunc(ct, lut, q=q)
    ok = ph.decrypt(got, s, 8, q) * (q // 8) == ph.lut_model(lut, phi, q)
    _check("EvalFunc negacyclic q = 512", got, ok, _none(ok.size), lambda i: orc.eval_func(ct[i], lut, q=q), 17)
    lut = _table_steps(rs, q, "arbitrary")
    got = ctx.EvalFunc(ct, lut, q=q)
    want = orc.eval_func(ct, lut, q=q)
    print(f"EvalFunc arbitrary q = 512: oracle on all {ct.shape[0]} rows, {2 * ct.shape[0]} oracle bootstraps")
    assert np.array_equal(got, want)


def _s_phases(rs, Qin, q):
    """Offsets within +-(beta + 8 W) of 0 and of Qin / 2; within +-8 W of the half multiples of q next to them
    that the floors cross (phi + beta = q/2, q above each and q/2 below each: the first and the last period of
    either half); 64 random phases.  The neighbourhoods are four times the +-2 W that holds every window with
    room to spare, so that the windows (up to ten of 2 W rows with roundbits = 1) stay within 1/8 of the rows."""
    W = ph.W["floor"]
    wide = np.arange(-(ph.BETA + 8 * W), ph.BETA + 8 * W + 1)
    near = np.arange(-8 * W, 8 * W + 1)
    parts = [b + wide for b in (0, Qin // 2)]
    parts += [b + k * (q // 2) - ph.BETA + near for b in (0, Qin // 2) for k in (-1, 1, 2)]
    return np.concatenate(parts + [rs.integers(0, Qin, 64)]) % Qin


def _s_case(c, Qin, qf, seed):
    rs = np.random.default_rng(seed)
    ct = ph.with_phase(rs, c.s, _s_phases(rs, Qin, c.p.q), Qin)
    phi = ph.phase_of(ct, c.s, Qin)
    in_floor = ph.dist(phi, ph.floor_boundaries(phi, Qin, qf), Qin) <= ph.W["floor"]
    return ct, phi, in_floor


@pytest.mark.parametrize("Qin", [1 << 17, 1 << 23])
@pytest.mark.parametrize("roundbits", [0, 1])
def test_eval_floor_near_its_boundaries(contexts, Qin, roundbits):
    """EvalFloor on S (TV_HALF and TV_FLOOR2 at ctmod q = 4096, or 512 with roundbits = 1; fmod = Qin)."""
    c = contexts("S")
    s, ctx, orc, q = c.s, c.ctx, c.orc, c.p.q
    qf = q if roundbits == 0 else 2 * ph.BETA << roundbits
    ct, phi, excluded = _s_case(c, Qin, qf, Qin + roundbits)
    got = ctx.EvalFloor(ct, Qin, roundbits)
    ok = ph.decrypt(got, s, Qin // qf, Qin) == ph.floor_model(phi, Qin, qf)
    rows = _check(f"EvalFloor Qin = {Qin}, roundbits = {roundbits}", got, ok, excluded,
                  lambda i: orc.eval_floor(ct[i], Qin, roundbits), 113)
    print(f"EvalFloor: {2 * rows} oracle bootstraps")


def _floors(Qin, q):
    k = 0
    while Qin > q:
        Qin, k = Qin // q * 2 * ph.BETA, k + 1
    return k


@pytest.mark.parametrize("Qin", [1 << 17, 1 << 23])
def test_eval_sign_near_its_boundaries(contexts, Qin):
    """EvalSign on S: the floors, LWE_MODSWITCH between them, then TV_SIGN3 at the modulus they leave."""
    c = contexts("S")
    s, ctx, orc, q = c.s, c.ctx, c.orc, c.p.q
    ct, phi, _ = _s_case(c, Qin, q, Qin + 2)
    b = ph.sign_boundaries(Qin, q)
    excluded = ph.dist(phi, b, Qin) <= ph.W["sign"]
    got = ctx.EvalSign(ct, Qin)
    ok = ph.decrypt(got, s, 2, q) == ph.sign_model(phi, Qin)
    rows = _check(f"EvalSign Qin = {Qin}", got, ok, excluded, lambda i: orc.eval_sign(ct[i], Qin), 113)
    print(f"EvalSign: {rows * (2 * _floors(Qin, q) + 1)} oracle bootstraps")


@pytest.mark.parametrize("Qin", [1 << 17, 1 << 23])
def test_eval_decomp_near_its_boundaries(contexts, Qin):
    """EvalDecomp on S: digit 0 is the input mod q (no bootstrap: its model holds at every phase, window or not);
    the later digits come from the floors."""
    c = contexts("S")
    s, ctx, orc, q = c.s, c.ctx, c.orc, c.p.q
    ct, phi, excluded = _s_case(c, Qin, q, Qin + 3)
    got, moduli = ctx.EvalDecomp(ct, Qin)
    model = ph.decomp_model(phi, Qin, q)
    assert moduli == [m for _, _, m in model]
    dec = [ph.decrypt(got[:, j], s, p, m) for j, (_, p, m) in enumerate(model)]
    assert np.array_equal(dec[0], model[0][0])
    ok = np.all([d == want for d, (want, _, _) in zip(dec, model)], axis=0)

    def oracle_rows(i):
        want, mods = orc.eval_decomp(ct[i], Qin)
        assert mods == moduli
        return want

    rows = _check(f"EvalDecomp Qin = {Qin}", got, ok, excluded, oracle_rows, 113)
    print(f"EvalDecomp: {rows * 2 * _floors(Qin, q)} oracle bootstraps")


# ---------------------------------------------------------------------------------------------------------------
# circuits: k_circuit_prep, k_circuit_out
# ---------------------------------------------------------------------------------------------------------------
BOOTSTRAPPED = ["OR", "AND", "NOR", "NAND", "XOR_FAST", "XNOR_FAST"]
# inputs: x (a random phase r), y (t - r), z (r - t), w (t), t the instance: every first-level gate below sees a
# prepared phase that runs over all of [0, q) (every even phase for the FAST gates) as t does
X, Y, Z, T = range(4)
NX, NY, NZ, C0, C1 = range(4, 9)  # NOT x, NOT y, NOT z, CONST0, CONST1
# operand forms (in0, in1) per kind of gate: (x, y), (NOT x, y), (x, NOT y), (NOT x, NOT y), (0, y), (1, y), (x, constant)
FORMS = {False: [(X, Y), (NX, Z), (X, NZ), (NX, NY), (C0, T), (C1, T), (T, C1)],
         True: [(X, Z), (NX, Y), (X, NY), (NX, NZ), (C0, T), (C1, T), (T, C0)]}


def _sweep_netlist():
    """(gates, outputs, first): `first` lists (wire, op, in0, in1) of the first-level gates."""
    gates = [("NOT", X), ("NOT", Y), ("NOT", Z), ("CONST0",), ("CONST1",)]
    first = []
    for op in BOOTSTRAPPED:
        for a, b in FORMS[op.endswith("_FAST")]:
            first.append((4 + len(gates), op, a, b))
            gates.append((op, a, b))
    # second level: every op on first-level results (its own (x, y) gate and the next op's (NOT x, NOT y) gate), plain
    # and with either operand negated: the operands come from the wire store
    second = []
    for i, op in enumerate(BOOTSTRAPPED):
        u, v = first[7 * i][0], first[7 * ((i + 1) % 6) + 3][0]
        nu, nv = 4 + len(gates), 5 + len(gates)
        gates += [("NOT", u), ("NOT", v)]
        for a, b in ((u, v), (nu, v), (u, nv)):
            second.append(4 + len(gates))
            gates.append((op, a, b))
    for op in ("XOR", "XNOR"):
        second.append(4 + len(gates))
        gates.append((op, X, Y))
    nots = [4 + len(gates), 5 + len(gates)]
    gates += [("NOT", second[0]), ("NOT", C1)]
    outputs = [w for w, *_ in first] + second + nots + [C0, C1, NX, X]
    return gates, outputs, first


class _AsOracle:
    """The GPU's vector API behind the oracle's method name, for circuit_nets.oracle_netlist."""

    def __init__(self, ctx):
        self.ctx = ctx

    def eval_bin_gate(self, gate, a, b):
        return self.ctx.EvalBinGate(gate, a, b)


def test_circuit_at_every_phase(contexts):
    """One netlist on G, 1024 + 3 instances: equal to the vector API gate by gate at every instance, the model on
    the first level at every phase, the oracle composition on a stride of instances and the fixed rows."""
    import tfhe_amd

    c = contexts("G")
    s, ctx, orc, q = c.s, c.ctx, c.orc, c.p.q
    rs = np.random.default_rng(77)
    x, y, z = _gate_operands(rs, s, q)
    cts = np.stack([x, y, z, ph.with_phase(rs, s, np.arange(q), q)])
    gates, outputs, first = _sweep_netlist()
    circ = tfhe_amd.Circuit(4, gates, outputs)
    inf = circ.info()
    # level 1: the 42 first-level gates and the two ANDs each of XOR and XNOR
    assert circ.level_widths()[0] == len(first) + 4 and inf["bootstraps"] == len(first) + 18 + 6
    got = ctx.EvalCircuit(circ, cts)
    B = cts.shape[1]
    # the vector API, gate by gate on the same operands
    vector = int(np.count_nonzero(got != cnets.oracle_netlist(_AsOracle(ctx), 4, gates, outputs, cts, q)))
    # the model on the first level
    phi = {i: ph.phase_of(cts[i], s, q) for i in range(4)}
    phi.update({NX: ph.not_phase(phi[X], q), NY: ph.not_phase(phi[Y], q), NZ: ph.not_phase(phi[Z], q),
                C0: np.zeros(B, dtype=np.int64), C1: np.full(B, q // 4)})
    wrong = 0
    for k, (wire, op, a, b) in enumerate(first):
        swept = np.unique(ph.gate_phase(op, phi[a][:q], phi[b][:q], q))
        assert np.array_equal(swept, np.arange(0, q, 2 if op.endswith("_FAST") else 1)), (op, a, b)
        wrong += int(np.count_nonzero(ph.decrypt(got[k], s, 4, q) != ph.gate_model(op, ph.gate_phase(op, phi[a], phi[b], q), q)))
    idx = np.concatenate([np.arange(0, q, 341), np.arange(B - 3, B)])
    oracle = cnets.oracle_netlist(orc, 4, gates, outputs, cts[:, idx], q)
    differ = int(np.count_nonzero(got[:, idx] != oracle))
    print(f"circuit: {len(gates)} gates, {inf['bootstraps']} bootstraps x {B} instances: vector API at every instance "
          f"({vector} words differ), model on {len(first)} first-level gates x {B} phases ({wrong} wrong), oracle on "
          f"{idx.size} instances ({differ} words differ, {inf['bootstraps'] * idx.size} oracle bootstraps)")
    assert vector == 0
    assert wrong == 0
    assert differ == 0


# ---------------------------------------------------------------------------------------------------------------
# function circuits: k_fcircuit_prep, k_fcircuit_out
# ---------------------------------------------------------------------------------------------------------------
def _sweep_fnet(q, rs):
    """Inputs: x of phase t (the instance), y of a random phase r, z of phase t - r.  Wire 3 + g is node g."""
    # The two-stage nodes all read phase +-t, so their windows fall on the same 128 instances; the form 3 t + K,
    # whose neighbouring phases are far apart in t, feeds a negacyclic table (one bootstrap, no window).
    K = q - q // 8  # 3 t + K passes q for every t >= q / 24
    luts = np.stack([_table_neg(rs, q), _table_steps(rs, q, "periodic"), _table_steps(rs, q, "arbitrary"),
                     fnets.tables(q)["mod4"]])
    NEG, PER, ARB, MOD4 = range(4)
    nodes = [
        ("LUT", NEG, (0, 1)),                # 3: level 1, at q
        ("LUT", PER, (0, 1)),                # 4: levels 1, 2 at q
        ("LUT", ARB, (0, 1)),                # 5: levels 1, 2 at 2q, beside 3 and 4
        ("LIN", (0, q - 1)),                 # 6: phase -t
        ("LUT", ARB, (6, 1)),                # 7
        ("LUT", NEG, (0, 3), K),             # 8: phase 3 t + K, past q
        ("LIN", (1, 1), (2, 1)),             # 9: two inputs, phase t
        ("LUT", PER, (9, 1)),                # 10
        ("LUT", MOD4, (3, 1)),               # 11: a second-level table on a first-level slot
        ("LIN", (11, 1), (0, 2), q // 8),    # 12: a folded form over a slot and an input, an output
    ]
    outputs = [3, 4, 5, 7, 8, 10, 11, 12, 6]
    return 3, nodes, luts, outputs


def test_fcircuit_at_every_phase(contexts):
    """One FuncCircuit on F, 2048 + 3 instances: equal to EvalFunc and numpy linear algebra node by node at every
    instance, the model at every phase outside the windows, the oracle composition on the rest and a stride."""
    import tfhe_amd

    c = contexts("F")
    s, ctx, orc, q = c.s, c.ctx, c.orc, c.p.q
    rs = np.random.default_rng(99)
    t = np.arange(q)
    r = rs.integers(0, q, q)
    cts = np.stack([ph.with_phase(rs, s, p, q) for p in (t, r, t - r)])
    net = ni, nodes, luts, outputs = _sweep_fnet(q, rs)
    fc = tfhe_amd.FuncCircuit(ni, nodes, luts, outputs, q)
    assert fc.info()["bootstraps"] == 12
    got = ctx.EvalFuncCircuit(fc, cts)
    B = cts.shape[1]
    vector = int(np.count_nonzero(got != fnets.compose(ctx.EvalFunc, *net, q, cts)))
    # the model: phases are linear in the ciphertexts; a LUT node's output phase is its table entry (plus noise
    # far below q / 16, the distance of an entry from the next node's boundaries)
    px, py, pz = (ph.phase_of(cts[i], s, q) for i in range(3))
    assert np.array_equal(np.unique(px[:q]), t) and np.array_equal((py + pz) % q, px)
    K = q - q // 8
    w3 = ph.lut_model(luts[0], px, q)
    w11 = ph.lut_model(luts[3], w3, q)
    model = {3: (w3, px, "negacyclic"), 4: (ph.lut_model(luts[1], px, q), px, "periodic"),
             5: (ph.lut_model(luts[2], px, q), px, "arbitrary"), 7: (ph.lut_model(luts[2], -px % q, q), -px % q, "arbitrary"),
             8: (ph.lut_model(luts[0], (3 * px + K) % q, q), (3 * px + K) % q, "negacyclic"),
             10: (ph.lut_model(luts[1], (py + pz) % q, q), px, "periodic"),
             11: (w11, w3, "negacyclic")}  # no window: wire 3's entries are q / 16 from wire 11's boundaries
    excluded = _none(B)
    wrong = 0
    for k, wire in enumerate(outputs):
        if wire not in model:
            continue
        want, phi, cls = model[wire]
        ex = _func_windows(cls, phi, q)
        assert int(ex[:q].sum()) * 8 <= q
        excluded |= ex
        wrong += int(np.count_nonzero((ph.decrypt(got[k], s, 8, q) * (q // 8) != want) & ~ex))
    # the two linear outputs: exact phases (wire 12 carries wire 11's noise)
    wrong += int(np.count_nonzero(ph.phase_of(got[outputs.index(6)], s, q) != -px % q))
    wrong += int(np.count_nonzero(ph.lwe_error(got[outputs.index(12)], s, (w11 + 2 * px + q // 8) % q, q) >= q // 16))
    sub = excluded.copy()
    sub[B - 3:] = True
    sub[::293] = True
    idx = np.flatnonzero(sub)
    oracle = fnets.oracle_netlist(orc, *net, q, cts[:, idx])
    differ = int(np.count_nonzero(got[:, idx] != oracle))
    print(f"fcircuit: 12 bootstraps x {B} instances: EvalFunc node by node at every instance ({vector} words differ), "
          f"model on 7 LUT nodes and 2 linear outputs ({wrong} wrong outside the windows; {int(excluded.sum())} "
          f"instances in some window), oracle on {idx.size} instances ({differ} words differ, {12 * idx.size} oracle "
          f"bootstraps)")
    assert np.union1d(np.flatnonzero(~excluded), idx).size == B  # every instance met the model or the oracle
    assert vector == 0
    assert wrong == 0
    assert differ == 0
