"""The plain models of tests/phases.py against the CPU oracle alone, and the windows the GPU sweeps use.

Reduced sweeps (n = 32 contexts, keys from or_keygen seed phases.SEED; about 14,000 oracle bootstraps):
  G (STD128)            AND (q1 > q2) and NAND (q1 < q2), all 1024 sum phases, and XOR over 128 operand pairs
  F (logQ = 12 arbFunc) one table of each class over p = 8 messages, all 2048 phases
  S (logQ = 23)         EvalSign and EvalFloor at Qin = 2^17: +-48 around each boundary (four each), and 176
                        random phases

Asserted: the single-bootstrap ops (gates, negacyclic table) follow the model at every phase, no window; the
two-stage ops follow it at every phase outside a window of half-width W = phases.window(d_max) around each
boundary, where d_max, the largest distance from a boundary at which the oracle departs from the model, is
measured here over the sweep (printed; a sample maximum of noise) and the window from it must be the committed
phases.W; and no window excludes more than 1/8 of the rows of a sweep.
"""
import numpy as np
import pytest

import phases as ph

pytestmark = pytest.mark.slow


def _ctx(oracle, base):
    import tfhe_amd

    tfhe_amd.build()  # sweep_context finishes the parameters through the C-ABI
    orc, _, s = ph.sweep_context(oracle, base, gpu=False)
    return orc, s


def _sweep(rs, s, phis, mod):
    ct = ph.with_phase(rs, s, phis, mod)
    return ct, ph.phase_of(ct, s, mod)


def _measure(name, ok, d):
    """d_max over the failures `~ok` and the window from it; the model holds at every row outside the window, and
    the window excludes at most 1/8 of the sweep's rows (the three fixed rows aside)."""
    d_max = int(d[~ok].max()) if (~ok).any() else 0
    W = ph.window(d_max)
    excluded, rows = int((d[:-3] <= W).sum()), ok.size - 3
    print(f"{name}: {int((~ok).sum())} of {ok.size} rows depart from the model, d_max = {d_max}, W = {W}; "
          f"the window excludes {excluded} of {rows} rows")
    assert W == ph.W[name], (name, d_max)
    assert ok[d > W].all()
    assert excluded * 8 <= rows, (name, excluded, rows)
    return W


def test_gates_follow_the_range_rule_at_every_phase(oracle):
    orc, s = _ctx(oracle, ph.BASE_G)
    q = orc.p.q
    rs = np.random.default_rng(1)
    phi1 = rs.integers(0, q, q)
    worst = 0
    for gate in ("AND", "NAND"):
        c1, p1 = _sweep(rs, s, phi1, q)
        c2, p2 = _sweep(rs, s, (np.arange(q) - phi1) % q, q)
        assert np.array_equal(np.unique(ph.gate_phase(gate, p1[:q], p2[:q], q)), np.arange(q))
        out = orc.eval_bin_gate(gate, c1, c2)
        want = ph.gate_model(gate, ph.gate_phase(gate, p1, p2, q), q)
        assert np.array_equal(ph.decrypt(out, s, 4, q), want), gate
        worst = max(worst, int(ph.lwe_error(out, s, want * (q // 4), q).max()))
    print(f"gates: largest output error {worst} of q/8 = {q // 8}")
    assert worst < q // 16  # so XOR's OR, reading the sum of two AND outputs, stays q/8 - 2 worst from its range's ends
    c1, p1 = _sweep(rs, s, np.arange(0, q, 8), q)
    c2, p2 = _sweep(rs, s, rs.integers(0, q, q // 8), q)
    assert np.array_equal(ph.decrypt(orc.eval_bin_gate("XOR", c1, c2), s, 4, q), ph.xor_model("XOR", p1, p2, q))
    orc.close()


def test_tables_of_each_class(oracle):
    import fcircuit_nets as nets

    orc, s = _ctx(oracle, ph.BASE_F)
    q = orc.p.q
    assert q == orc.p.N == 2048
    rs = np.random.default_rng(2)
    t = nets.tables(q)
    ct, phi = _sweep(rs, s, np.arange(q), q)
    d = ph.dist(phi, ph.lut_boundaries(q), q)
    for name, table in (("negacyclic", t["neg1"]), ("periodic", t["mod4"]), ("arbitrary", t["cube"])):
        want = ph.lut_model(table, phi, q)
        out = orc.eval_func(ct, table)
        ok = ph.decrypt(out, s, 8, q) * (q // 8) == want
        if name == "negacyclic":  # one bootstrap: exact at every phase
            assert ok.all()
            print(f"negacyclic: largest output error {int(ph.lwe_error(out, s, want, q).max())}")
            continue
        W = _measure(name, ok, d)
        assert int((d[:q] <= W).sum()) == 8 * 2 * W
    orc.close()


def test_sign_and_floor_at_2_17(oracle):
    orc, s = _ctx(oracle, ph.BASE_S)
    q, Qin = orc.p.q, 1 << 17
    assert q == 4096
    rs = np.random.default_rng(3)
    near = np.arange(-48, 48)
    b_sign = ph.sign_boundaries(Qin, q)
    ct, phi = _sweep(rs, s, np.concatenate([b + near for b in b_sign] + [rs.integers(0, Qin, 176)]), Qin)
    ok = ph.decrypt(orc.eval_sign(ct, Qin), s, 2, q) == ph.sign_model(phi, Qin)
    _measure("sign", ok, ph.dist(phi, b_sign, Qin))
    # EvalFloor: boundaries at phi + beta = 0 mod q / 2; one of each kind, and both ends of the modulus
    b_floor = [(k * (q // 2) - ph.BETA) % Qin for k in (0, 1, 2, 2 * Qin // q - 1)]
    ct, phi = _sweep(rs, s, np.concatenate([b + near for b in b_floor] + [rs.integers(0, Qin, 176)]), Qin)
    out = orc.eval_floor(ct, Qin, 0)
    ok = ph.decrypt(out, s, Qin // q, Qin) == ph.floor_model(phi, Qin, q)
    _measure("floor", ok, ph.dist(phi, ph.floor_boundaries(phi, Qin, q), Qin))
    orc.close()
