"""Netlists of the function-circuit tests (tfhe_amd.FuncCircuit), their tables, the ten-line clear model and the
oracle composition: the CPU oracle called node by node in netlist order -- numpy modular arithmetic for the
linear forms (k on b only), orc.eval_func(ct, table) for the LUT nodes.

Tables are over p = 8 messages, interval = q / 8: entry i holds f(i // interval) * interval mod q.

A note on the table `m < 4 ? m : -(m - 4)`: it is negacyclic as a function, but the reference's checkInputFunction
(binfhe-base-scheme.cpp:162-186) tests lut[0] == q - lut[q/2], which no table with f(0) = 0 can meet (an entry is
below q, so -0 is stored as 0, not as q).  EvalFunc therefore runs it as an arbitrary table, and so does the
circuit, which must equal EvalFunc bit for bit.  TABLES keeps it ("negm") and adds "neg1", m < 4 ? m + 1 :
-(m - 3), which has no zero entry and is negacyclic under the rule, so every class is present."""
import numpy as np

from helpers import cube_lut

P = 8
NEGACYCLIC, PERIODIC, ARBITRARY = 0, 1, 2


def table(f, q):
    interval = q // P
    return np.array([(f(i // interval) * interval) % q for i in range(q)], dtype=np.uint64)


def tables(q):
    """name -> table, in the index order of TABLE_NAMES."""
    return {"cube": cube_lut(q, P),
            "mod4": table(lambda m: m % 4, q),
            "negm": table(lambda m: m if m < 4 else -(m - 4), q),
            "div4": table(lambda m: m // 4, q),
            "neg1": table(lambda m: m + 1 if m < 4 else -(m - 3), q)}


TABLE_NAMES = ["cube", "mod4", "negm", "div4", "neg1"]
TABLE_CLASS = dict(cube=ARBITRARY, mod4=PERIODIC, negm=ARBITRARY, div4=ARBITRARY, neg1=NEGACYCLIC)
CUBE, MOD4, NEGM, DIV4, NEG1 = range(5)


def all_classes(q):
    """(num_inputs, nodes, luts, outputs): wires 0-2 are inputs, node g is wire 3 + g."""
    interval = q // P
    nodes = [
        ("LIN", (0, 1), (1, 1)),                 # 3: two terms
        ("LIN", (3, 2), (2, -1), interval),      # 4: a LIN of a LIN, a coefficient 2, a negative one, k != 0
        ("LUT", NEG1, (3, 1)),                   # 5: negacyclic             level 1
        ("LUT", MOD4, (4, 1)),                   # 6: periodic               levels 1, 2
        ("LUT", CUBE, (0, 1), (2, 1)),           # 7: arbitrary              levels 1, 2
        ("LUT", MOD4, (5, 1), (6, 1)),           # 8: the same table again, reads two LUT nodes: levels 3, 4
        ("LUT", DIV4, (5, 1)),                   # 9: arbitrary on a negacyclic node: levels 2, 3 (first stage beside 6's and 7's second)
        ("LUT", NEGM, (7, 1)),                   # 10: reads a slot written at 2q: levels 3, 4
        ("LIN", (9, 1), (0, -3)),                # 11: a LIN over a LUT node and an input
        ("LUT", NEG1, (11, 1), (8, 2), 2 * interval),  # 12: level 5
    ]
    outputs = [1, 4, 11, 5, 6, 7, 12, 10, 8]  # an input, two LIN nodes, LUT nodes of all three classes
    return 3, nodes, np.stack([tables(q)[t] for t in TABLE_NAMES]), outputs


ALL_CLASSES_WIDTHS = [3, 3, 3, 2, 1]
ALL_CLASSES_BOOTSTRAPS = 12  # nodes 5 and 12 one each, the other five LUT nodes two each


def adder(digits, q):
    """Base-4 adder over p = 8: inputs x_0 .. x_{d-1}, y_0 .. y_{d-1}; per digit s = x + y (+ carry),
    digit = mod4(s), carry = div4(s).  Outputs: the digits, then the last carry.  2 * digits LUT nodes,
    4 * digits bootstraps (mod4 is periodic, div4 arbitrary)."""
    t = tables(q)
    nodes, outputs, carry = [], [], None
    wire = 2 * digits
    for d in range(digits):
        nodes.append(("LIN", (d, 1), (digits + d, 1)))
        s = wire
        wire += 1
        if carry is not None:
            nodes.append(("LIN", (s, 1), (carry, 1)))
            s = wire
            wire += 1
        nodes.append(("LUT", 0, (s, 1)))
        nodes.append(("LUT", 1, (s, 1)))
        outputs.append(wire)
        carry = wire + 1
        wire += 2
    return 2 * digits, nodes, np.stack([t["mod4"], t["div4"]]), outputs + [carry]


def fields(node):
    """(op name, in0, in1, c0, c1, lut, k) of a node tuple."""
    from tfhe_amd.fcircuit import node_row

    code, in0, in1, c0, c1, lut, k = node_row(node)
    return ("LIN", "LUT")[code], in0, in1, c0, c1, lut, k


def eval_model(num_inputs, nodes, luts, outputs, q, values):
    """The clear model: LIN -> (c0 x + c1 y + k) mod q, LUT -> table[v].  values[num_inputs, instances]."""
    w = [np.asarray(v, dtype=np.int64) for v in values]
    for node in nodes:
        op, in0, in1, c0, c1, lut, k = fields(node)
        v = (c0 * w[in0] + (c1 * w[in1] if c1 else 0) + k) % q
        w.append(v if op == "LIN" else np.asarray(luts[lut], dtype=np.int64)[v])
    return np.stack([w[o] for o in outputs]).astype(np.uint64)


def node_value(eval_func, node, luts, q, x, y):
    """One node on ciphertext rows x (and y, if it has a second term), int64 [instances, n+1]: the linear form
    mod q (k on b only), then eval_func(ct, table) if it is a LUT node."""
    op, _, _, c0, c1, lut, k = fields(node)
    v = c0 * x + (c1 * y if c1 else 0)
    v[:, -1] += k
    v %= q
    if op == "LUT":
        v = eval_func(np.ascontiguousarray(v.astype(np.uint64)), np.ascontiguousarray(luts[lut])).astype(np.int64)
    return v


def compose(eval_func, num_inputs, nodes, luts, outputs, q, cts):
    """cts[num_inputs, instances, n+1] -> [num_outputs, instances, n+1]: the netlist node by node in order with any
    EvalFunc -- the GPU's vector API included -- for the LUT nodes, one call after the other."""
    w = [np.asarray(c, dtype=np.int64) for c in cts]
    for node in nodes:
        _, in0, in1, _, c1, _, _ = fields(node)
        w.append(node_value(eval_func, node, luts, q, w[in0], w[in1] if c1 else None))
    return np.stack([w[o] for o in outputs]).astype(np.uint64)


def oracle_netlist(orc, num_inputs, nodes, luts, outputs, q, cts):
    """cts[num_inputs, instances, n+1] -> [num_outputs, instances, n+1]: the oracle composed node by node.

    The oracle spreads a call over at most `instances` threads, so nodes that do not depend on each other run on a
    small thread pool (its calls release the GIL and share only read-only keys).  Nodes are submitted in netlist
    order and wait only for earlier ones, so the oldest unfinished node can always run."""
    from concurrent.futures import ThreadPoolExecutor

    def run(node, x, y):
        return node_value(orc.eval_func, node, luts, q, x.result(), y.result() if y is not None else None)

    with ThreadPoolExecutor(4) as pool:
        w = [pool.submit(np.asarray, c, np.int64) for c in cts]
        for node in nodes:
            _, in0, in1, _, c1, _, _ = fields(node)
            w.append(pool.submit(run, node, w[in0], w[in1] if c1 else None))
        return np.stack([w[o].result() for o in outputs]).astype(np.uint64)
