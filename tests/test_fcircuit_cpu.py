"""CPU: the netlist compiler of tfhe_fcircuit (tfhe-gpu_amd/csrc/fcircuit.cpp) -- validation, classification of
the tables by the reference's rule, folding of the linear forms, lowering of LUT nodes to one or two bootstrap
records, levels -- checked through the lowered plan's clear-value evaluation against a ten-line model of the
netlist (fcircuit_nets.eval_model).  No GPU."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import fcircuit_nets as nets

Q = 2048
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tfhe():
    import tfhe_amd

    tfhe_amd.build()
    return tfhe_amd


def all_messages(num_inputs, q):
    """Every assignment of multiples of interval to the inputs, as instances: [num_inputs, 8^num_inputs]."""
    grid = np.array(list(itertools.product(range(nets.P), repeat=num_inputs)), dtype=np.uint64).T
    return np.ascontiguousarray(grid.reshape(num_inputs, -1) * np.uint64(q // nets.P))


def test_classification_of_the_tables(tfhe):
    t = nets.tables(Q)
    for name in nets.TABLE_NAMES:
        c = tfhe.FuncCircuit(1, [("LUT", 0, (0, 1))], t[name][None, :], [1], Q)
        info = c.info()
        got = (info["negacyclic"], info["periodic"], info["arbitrary"]).index(1)
        assert got == nets.TABLE_CLASS[name], name
        assert info["bootstraps"] == (1 if got == nets.NEGACYCLIC else 2)
        assert c.level_widths() == ([1] if got == nets.NEGACYCLIC else [1, 1])


def test_counts_of_the_all_classes_netlist(tfhe):
    ni, nodes, luts, outputs = nets.all_classes(Q)
    c = tfhe.FuncCircuit(ni, nodes, luts, outputs, Q)
    assert c.info() == dict(num_inputs=3, num_outputs=9, num_nodes=10, bootstraps=12, levels=5, widest_level=3,
                            num_luts=5, negacyclic=1, periodic=1, arbitrary=3, q=Q)
    assert c.level_widths() == [3, 3, 3, 2, 1] == nets.ALL_CLASSES_WIDTHS
    assert nets.ALL_CLASSES_BOOTSTRAPS == 12
    vals = all_messages(ni, Q)
    assert np.array_equal(c.eval_plain(vals), nets.eval_model(ni, nodes, luts, outputs, Q, vals))
    one = c.eval_plain(vals[:, 77])  # one instance, given flat
    assert one.shape == (9,) and np.array_equal(one, c.eval_plain(vals)[:, 77])


def test_three_digit_adder(tfhe):
    ni, nodes, luts, outputs = nets.adder(3, Q)
    c = tfhe.FuncCircuit(ni, nodes, luts, outputs, Q)
    info = c.info()
    assert sum(1 for n in nodes if n[0] == "LUT") == 6 and info["bootstraps"] == 12
    # digit d: both first stages at level 2d + 1, both second stages (the carry among them) at 2d + 2
    assert c.level_widths() == [2] * 6
    interval = Q // nets.P
    digits = np.array(list(itertools.product(range(4), repeat=6)), dtype=np.uint64).T  # every pair of 3-digit numbers
    out = c.eval_plain(digits * np.uint64(interval))
    assert np.array_equal(out, nets.eval_model(ni, nodes, luts, outputs, Q, digits * np.uint64(interval)))
    x = sum(digits[d].astype(np.int64) << (2 * d) for d in range(3))
    y = sum(digits[3 + d].astype(np.int64) << (2 * d) for d in range(3))
    got = sum((out[d] // np.uint64(interval)).astype(np.int64) << (2 * d) for d in range(4))
    assert np.array_equal(got, x + y)
    # and on every multiple of interval, not only on digits
    vals = all_messages(ni, Q)
    assert np.array_equal(c.eval_plain(vals), nets.eval_model(ni, nodes, luts, outputs, Q, vals))


def random_table(rs, q, cls):
    h = q // 2
    if cls == nets.NEGACYCLIC:  # lut[i] == q - lut[h + i]: no zero entry
        first = rs.integers(1, q, h, dtype=np.uint64)
        return np.concatenate([first, np.uint64(q) - first])
    if cls == nets.PERIODIC:
        first = rs.integers(0, q, h, dtype=np.uint64)
        return np.concatenate([first, first])
    t = rs.integers(0, q, q, dtype=np.uint64)
    t[0], t[h] = 1, 2  # neither rule's first test holds
    return t


def random_netlist(rs, q):
    ni = int(rs.integers(1, 5))
    ng = int(rs.integers(1, 13))
    classes = [nets.NEGACYCLIC, nets.PERIODIC, nets.ARBITRARY] + [int(c) for c in rs.integers(0, 3, int(rs.integers(0, 3)))]
    luts = np.stack([random_table(rs, q, c) for c in classes])
    nodes = []
    for g in range(ng):
        terms = [(int(rs.integers(0, ni + g)), int(rs.integers(-5, 6)))]
        if rs.integers(0, 2):
            terms.append((int(rs.integers(0, ni + g)), int(rs.integers(-2 ** 31, 2 ** 31))))
        k = int(rs.integers(0, q)) if rs.integers(0, 2) else 0
        if rs.integers(0, 3) == 0:
            nodes.append(("LIN", *terms, k))
        else:
            nodes.append(("LUT", int(rs.integers(0, len(classes))), *terms, k))
    outputs = [int(w) for w in rs.integers(0, ni + ng, int(rs.integers(1, 6)))]
    return ni, nodes, luts, outputs, classes


@pytest.mark.parametrize("seed", range(30))
def test_lowered_plan_equals_the_model(tfhe, seed):
    q = 64
    rs = np.random.default_rng(3000 + seed)
    ni, nodes, luts, outputs, classes = random_netlist(rs, q)
    c = tfhe.FuncCircuit(ni, nodes, luts, outputs, q)
    info, widths = c.info(), c.level_widths()
    assert [info["negacyclic"], info["periodic"], info["arbitrary"]] == [classes.count(k) for k in range(3)]
    boots = sum(1 if classes[n[1]] == nets.NEGACYCLIC else 2 for n in nodes if n[0] == "LUT")
    assert info["bootstraps"] == boots == sum(widths)
    assert info["levels"] == len(widths) and info["widest_level"] == max(widths, default=0)
    assert all(w > 0 for w in widths)
    vals = rs.integers(0, q, (ni, 40), dtype=np.uint64)
    assert np.array_equal(c.eval_plain(vals), nets.eval_model(ni, nodes, luts, outputs, q, vals))


def compile_raw(tfhe, num_inputs, rows, q, luts, outputs, null=None, num_nodes=None):
    L = tfhe.lib()
    arr = (tfhe.capi.FuncNode * max(1, len(rows)))(*rows)
    outs = (C.c_uint32 * max(1, len(outputs)))(*outputs)
    tab = np.ascontiguousarray(luts, dtype=np.uint64)
    h = C.c_void_p()
    st = L.tfhe_fcircuit_compile(None if null == "out" else C.byref(h), num_inputs,
                                 None if null == "nodes" else C.cast(arr, C.c_void_p),
                                 len(rows) if num_nodes is None else num_nodes, q,
                                 None if null == "luts" else C.c_void_p(tab.ctypes.data), tab.shape[0],
                                 None if null == "outputs" else C.cast(outs, C.c_void_p), len(outputs))
    msg = L.tfhe_last_error().decode()
    if st == 0:
        L.tfhe_fcircuit_free(h)
    return st, msg, h.value


GOOD = np.tile(np.arange(64, dtype=np.uint64), (2, 1))  # two tables of q = 64 entries below q
BIG = GOOD.copy()
BIG[1, 9] = 64


# rows: (op, in0, in1, c0, c1, lut, k)
@pytest.mark.parametrize("what,num_inputs,rows,q,luts,outputs,kw,names", [
    ("unknown op", 2, [(1, 0, 0, 1, 0, 0, 0), (2, 0, 1, 1, 1, 0, 0)], 64, GOOD, [2], {}, "node 1"),
    ("forward reference", 2, [(0, 0, 1, 1, 1, 0, 0), (1, 2, 4, 1, 1, 0, 0)], 64, GOOD, [3], {}, "node 1"),
    ("reads itself", 2, [(0, 2, 0, 1, 0, 0, 0)], 64, GOOD, [2], {}, "node 0"),
    ("wire out of range", 2, [(0, 0, 1, 1, 1, 0, 0), (0, 77, 0, 1, 0, 0, 0)], 64, GOOD, [3], {}, "node 1"),
    ("second wire out of range", 2, [(0, 0, 77, 1, -1, 0, 0)], 64, GOOD, [2], {}, "node 0"),
    ("table index out of range", 2, [(0, 0, 1, 1, 1, 0, 0), (1, 0, 0, 1, 0, 2, 0)], 64, GOOD, [2], {}, "node 1"),
    ("table entry >= q", 2, [(1, 0, 0, 1, 0, 0, 0)], 64, BIG, [2], {}, "table 1"),
    ("k >= q", 2, [(0, 0, 0, 1, 0, 0, 0), (0, 0, 0, 1, 0, 0, 0), (0, 0, 0, 1, 0, 0, 64)], 64, GOOD, [2], {}, "node 2"),
    ("q not a power of two", 2, [(0, 0, 0, 1, 0, 0, 0)], 48, GOOD[:, :48], [2], {}, "q = 48"),
    ("q below 8", 2, [(0, 0, 0, 1, 0, 0, 0)], 4, GOOD[:, :4], [2], {}, "q = 4"),
    ("zero outputs", 2, [(0, 0, 0, 1, 0, 0, 0)], 64, GOOD, [], {}, "output"),
    ("output out of range", 2, [(0, 0, 0, 1, 0, 0, 0)], 64, GOOD, [3], {}, "output 0"),
    ("null node pointer", 2, [], 64, GOOD, [0], dict(null="nodes", num_nodes=3), "null"),
    ("null table pointer", 2, [(0, 0, 0, 1, 0, 0, 0)], 64, GOOD, [0], dict(null="luts"), "null"),
    ("null output array", 2, [(0, 0, 0, 1, 0, 0, 0)], 64, GOOD, [0], dict(null="outputs"), "null"),
    ("null handle pointer", 2, [(0, 0, 0, 1, 0, 0, 0)], 64, GOOD, [0], dict(null="out"), "null"),
])
def test_compile_errors(tfhe, what, num_inputs, rows, q, luts, outputs, kw, names):
    st, msg, h = compile_raw(tfhe, num_inputs, rows, q, luts, outputs, **kw)
    assert st == 1, what  # TFHE_ERR_INVALID_ARGUMENT
    assert names in msg, (what, msg)
    assert h is None  # no handle on failure


def test_ignored_operands_and_no_nodes(tfhe):
    # c1 == 0: in1 is ignored, whatever it holds; the table index of a LIN node likewise
    st, msg, _ = compile_raw(tfhe, 1, [(0, 0, 12345, 3, 0, 99, 5)], 64, GOOD, [1])
    assert st == 0, msg
    # a circuit without nodes or tables: outputs name inputs
    c = tfhe.FuncCircuit(2, [], np.zeros((0, 16), dtype=np.uint64), [1, 0, 1], 16)
    assert c.info() == dict(num_inputs=2, num_outputs=3, num_nodes=0, bootstraps=0, levels=0, widest_level=0,
                            num_luts=0, negacyclic=0, periodic=0, arbitrary=0, q=16)
    assert c.level_widths() == []
    assert np.array_equal(c.eval_plain(np.array([[3, 1], [7, 15]], dtype=np.uint64)), [[7, 15], [3, 1], [7, 15]])
    # node tuples: a bare wire is coefficient 1; the second term and k are optional
    a = tfhe.FuncCircuit(2, [("LIN", 0, (1, -1), 3), ("LIN", (2, 2)), ("LIN", (3, 1), 9)], np.zeros((0, 16)), [2, 3, 4], 16)
    assert np.array_equal(a.eval_plain(np.array([5, 9], dtype=np.uint64)), [15, 14, 7])
    with pytest.raises(tfhe.TfheError) as e:
        tfhe.FuncCircuit(2, [("LIN", (0, 1), (5, 1))], np.zeros((0, 16)), [2], 16)
    assert e.value.status == 1 and "node 0" in str(e.value)


def test_a_freed_circuit_is_refused(tfhe):
    ni, nodes, luts, outputs = nets.adder(1, 64)
    c = tfhe.FuncCircuit(ni, nodes, luts, outputs, 64)
    assert c.info()["bootstraps"] == 4
    c.free()
    for use in (c.info, c.level_widths, lambda: c.eval_plain(np.zeros(2, dtype=np.uint64)), c.free):
        with pytest.raises(tfhe.TfheError) as e:
            use()
        assert e.value.status == 1 and "freed" in str(e.value)
    L = tfhe.lib()
    assert L.tfhe_fcircuit_free(None) == 0  # as tfhe_circuit_free
    assert L.tfhe_fcircuit_get_info(None, None) == 1


def test_host_code_under_the_sanitizers(tfhe, tmp_path):
    """The compiler and a stand-alone driver (tests/fcircuit_driver.cpp: both netlists above, eval_plain, every
    compile error, free, double free) built with AddressSanitizer and UBSan and run on the CPU."""
    exe = str(tmp_path / "fcircuit_driver")
    csrc = os.path.join(ROOT, "tfhe-gpu_amd", "csrc")
    hipcc = os.path.join(os.environ.get("ROCM", "/opt/rocm"), "bin", "hipcc")
    # host code only: the sanitizers are host-side options (-Xarch_host), nothing is compiled for or run on a GPU
    subprocess.run([hipcc, "-x", "c++", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                    os.path.join(ROOT, "tests", "fcircuit_driver.cpp"), os.path.join(csrc, "fcircuit.cpp"),
                    "-pthread", "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "fcircuit driver ok" in r.stdout, r.stdout + r.stderr
