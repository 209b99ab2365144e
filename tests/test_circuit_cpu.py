"""CPU: the netlist compiler of tfhe_circuit (tfhe-gpu_amd/csrc/circuit.cpp) -- lowering (XOR / XNOR into three
bootstraps, NOT into negate flags, constants into operand kinds, nothing else simplified), ASAP levels, slot
renumbering -- checked through the lowered plan's clear-bit evaluation against the netlist's own truth tables.
No GPU."""
import ctypes as C
import itertools

import numpy as np
import pytest

import circuit_nets as nets


@pytest.fixture(scope="module")
def tfhe():
    import tfhe_amd

    tfhe_amd.build()
    return tfhe_amd


def all_assignments(num_inputs):
    """Every input assignment as instances: [num_inputs, 2^num_inputs]."""
    return np.array(list(itertools.product((0, 1), repeat=num_inputs)), dtype=np.uint8).T.reshape(num_inputs, -1)


def expected_bootstraps(gates):
    plain = sum(1 for g in gates if nets.OPS[g[0]] <= 5)
    triple = sum(1 for g in gates if g[0] in ("XOR", "XNOR"))
    return plain + 3 * triple


def test_counts_of_the_all_ops_netlist(tfhe):
    assert {g[0] for g in nets.ALL_OPS} == set(nets.OPS)  # all eleven ops
    c = tfhe.Circuit(nets.ALL_OPS_INPUTS, nets.ALL_OPS, nets.ALL_OPS_OUTPUTS)
    info, widths = c.info(), c.level_widths()
    assert info == dict(num_inputs=4, num_outputs=7, num_gates=15, bootstraps=14, levels=9, widest_level=3)
    assert widths == nets.ALL_OPS_WIDTHS
    assert info["bootstraps"] == expected_bootstraps(nets.ALL_OPS) == sum(widths)
    bits = all_assignments(4)
    assert np.array_equal(c.eval_plain(bits), nets.eval_netlist(4, nets.ALL_OPS, nets.ALL_OPS_OUTPUTS, bits))
    # one instance, given flat
    one = c.eval_plain(bits[:, 5])
    assert one.shape == (7,) and np.array_equal(one, c.eval_plain(bits)[:, 5])


def test_counts_of_the_mixed_netlist(tfhe):
    c = tfhe.Circuit(nets.MIXED_INPUTS, nets.MIXED, nets.MIXED_OUTPUTS)
    assert c.level_widths() == nets.MIXED_WIDTHS
    assert c.info()["bootstraps"] == 12 == expected_bootstraps(nets.MIXED)
    bits = all_assignments(4)
    assert np.array_equal(c.eval_plain(bits), nets.eval_netlist(4, nets.MIXED, nets.MIXED_OUTPUTS, bits))


def random_netlist(rs):
    ni = int(rs.integers(1, 7))
    ng = int(rs.integers(1, 41))
    names = list(nets.OPS)
    gates = []
    for g in range(ng):
        op = names[int(rs.integers(0, len(names)))]
        gates.append((op, int(rs.integers(0, ni + g)), int(rs.integers(0, ni + g))))
    outputs = [int(w) for w in rs.integers(0, ni + ng, int(rs.integers(1, 6)))]
    return ni, gates, outputs


@pytest.mark.parametrize("seed", range(50))
def test_lowered_plan_equals_the_netlist(tfhe, seed):
    ni, gates, outputs = random_netlist(np.random.default_rng(1000 + seed))
    c = tfhe.Circuit(ni, gates, outputs)
    info, widths = c.info(), c.level_widths()
    assert info["bootstraps"] == expected_bootstraps(gates) == sum(widths)
    assert info["levels"] == len(widths) and info["widest_level"] == max(widths, default=0)
    assert all(w > 0 for w in widths)
    bits = all_assignments(ni)
    assert np.array_equal(c.eval_plain(bits), nets.eval_netlist(ni, gates, outputs, bits))


def test_four_bit_ripple_carry_adder(tfhe):
    ni, gates, outputs = nets.ripple_adder(4)
    c = tfhe.Circuit(ni, gates, outputs)
    # bit 0: level 1; the carry into bit i >= 1 arrives at level 2i - 1, its sum bit and AND at 2i, its carry at 2i + 1
    assert c.info()["levels"] == 7
    assert c.info()["bootstraps"] == 2 + 5 * 3
    a, b = np.meshgrid(np.arange(16), np.arange(16), indexing="ij")
    a, b = a.ravel(), b.ravel()
    bits = np.stack([(a >> i) & 1 for i in range(4)] + [(b >> i) & 1 for i in range(4)]).astype(np.uint8)
    out = c.eval_plain(bits)
    assert out.shape == (5, 256)
    assert np.array_equal(sum(out[i].astype(np.int64) << i for i in range(5)), a + b)
    # the exact XOR costs three bootstraps on two levels each
    cx = tfhe.Circuit(*nets.ripple_adder(4, xor="XOR"))
    assert cx.info()["bootstraps"] == 10 + 3 * 7
    assert np.array_equal(cx.eval_plain(bits), out)


def compile_raw(tfhe, num_inputs, gates, outputs, null_gates=False, num_gates=None):
    L = tfhe.lib()
    arr = (tfhe.capi.CircuitGate * max(1, len(gates)))(*gates)
    outs = (C.c_uint32 * max(1, len(outputs)))(*outputs)
    h = C.c_void_p()
    st = L.tfhe_circuit_compile(C.byref(h), num_inputs, None if null_gates else C.cast(arr, C.c_void_p),
                                len(gates) if num_gates is None else num_gates, C.cast(outs, C.c_void_p), len(outputs))
    msg = L.tfhe_last_error().decode()
    if st == 0:
        L.tfhe_circuit_free(h)
    return st, msg, h.value


@pytest.mark.parametrize("what,num_inputs,gates,outputs,kw,names", [
    ("forward reference", 2, [(1, 0, 1), (0, 2, 4)], [3], {}, "gate 1"),
    ("reads itself", 2, [(1, 0, 2)], [2], {}, "gate 0"),
    ("wire out of range", 2, [(1, 0, 1), (8, 77, 0)], [3], {}, "gate 1"),
    ("op 11", 2, [(1, 0, 1), (11, 0, 1)], [2], {}, "gate 1"),
    ("zero outputs", 2, [(1, 0, 1)], [], {}, "output"),
    ("output out of range", 2, [(1, 0, 1)], [3], {}, "output 0"),
    ("null gate pointer", 2, [], [0], dict(null_gates=True, num_gates=3), "null"),
])
def test_compile_errors(tfhe, what, num_inputs, gates, outputs, kw, names):
    st, msg, h = compile_raw(tfhe, num_inputs, gates, outputs, **kw)
    assert st == 1, what  # TFHE_ERR_INVALID_ARGUMENT
    assert names in msg, (what, msg)
    assert h is None  # no handle on failure


def test_ignored_operands_and_no_gates(tfhe):
    # in1 of NOT and both operands of a constant are ignored, whatever they hold
    st, _, _ = compile_raw(tfhe, 1, [(8, 0, 12345), (9, 999, 999), (10, 7, 7)], [1, 2, 3])
    assert st == 0
    # a circuit without gates: outputs name inputs
    c = tfhe.Circuit(2, [], [1, 0, 1])
    assert c.info() == dict(num_inputs=2, num_outputs=3, num_gates=0, bootstraps=0, levels=0, widest_level=0)
    assert c.level_widths() == []
    assert np.array_equal(c.eval_plain(np.array([[0, 1], [1, 1]], dtype=np.uint8)), [[1, 1], [0, 1], [1, 1]])
    with pytest.raises(tfhe.TfheError) as e:
        tfhe.Circuit(2, [("AND", 0, 5)], [2])
    assert e.value.status == 1 and "gate 0" in str(e.value)
