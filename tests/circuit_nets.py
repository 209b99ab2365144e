"""Netlists shared by tests/test_circuit_cpu.py and tests/test_gpu_circuit.py, a direct evaluation of the
*unlowered* netlist on clear bits, and the gate-by-gate composition of the CPU oracle that every device
result must equal bit for bit."""
import numpy as np

OPS = {"OR": 0, "AND": 1, "NOR": 2, "NAND": 3, "XOR_FAST": 4, "XNOR_FAST": 5, "XOR": 6, "XNOR": 7, "NOT": 8,
       "CONST0": 9, "CONST1": 10}
NAMES = {v: k for k, v in OPS.items()}
TRUTH = {"OR": lambda x, y: x | y, "AND": lambda x, y: x & y, "NOR": lambda x, y: 1 ^ (x | y),
         "NAND": lambda x, y: 1 ^ (x & y), "XOR_FAST": lambda x, y: x ^ y, "XNOR_FAST": lambda x, y: 1 ^ x ^ y,
         "XOR": lambda x, y: x ^ y, "XNOR": lambda x, y: 1 ^ x ^ y}

# Every op; fan-out (wires 4, 5, 6, 11); a NOT of a NOT (wire 7); a NOT of a constant (wire 12); a gate over two
# constants (wire 17: bootstrapped, never folded); gates reading a negated wire (8, 9); wire 4 (level 1) read again at
# level 7 by wire 16; outputs: an input (0), negated gates (16: XNOR, 6: NOT of wire 4), a constant (12).
ALL_OPS_INPUTS = 4
ALL_OPS = [
    ("AND", 0, 1),         # 4   level 1
    ("OR", 2, 3),          # 5   level 1
    ("NOT", 4),            # 6
    ("NOT", 6),            # 7   = wire 4
    ("NAND", 7, 5),        # 8   level 2
    ("NOR", 6, 2),         # 9   level 2
    ("XOR", 8, 9),         # 10  levels 3 (two ANDs), 4 (OR)
    ("CONST0",),           # 11
    ("NOT", 11),           # 12  = CONST1
    ("CONST1",),           # 13
    ("XOR_FAST", 10, 12),  # 14  level 5
    ("XNOR_FAST", 1, 14),  # 15  level 6
    ("XNOR", 4, 15),       # 16  levels 7, 8
    ("AND", 13, 11),       # 17  level 1
    ("OR", 17, 16),        # 18  level 9
]
ALL_OPS_OUTPUTS = [0, 16, 18, 12, 6, 10, 9]
ALL_OPS_WIDTHS = [3, 2, 2, 1, 1, 1, 2, 1, 1]  # 8 plain gates + 3 * 2 (XOR, XNOR) = 14 bootstraps

# Twelve bootstraps in levels of 4, 2, 1, 4 and 1, the wide levels mixing gate types: a gate with a constant
# operand (wire 8), FAST gates whose operands come in the opposite order of their slots (9, 12), the same pair in
# both operand orders (15, 16), a negated operand (11), and a negated gate and a constant among the outputs.
MIXED_INPUTS = 4
MIXED = [
    ("NAND", 0, 1),        # 4   level 1
    ("NOR", 2, 3),         # 5   level 1
    ("XOR_FAST", 0, 1),    # 6   level 1
    ("CONST1",),           # 7
    ("AND", 2, 7),         # 8   level 1
    ("XNOR_FAST", 5, 4),   # 9   level 2
    ("NOT", 6),            # 10
    ("OR", 10, 8),         # 11  level 2
    ("XOR_FAST", 11, 9),   # 12  level 3
    ("AND", 12, 0),        # 13  level 4
    ("OR", 12, 1),         # 14  level 4
    ("XOR_FAST", 2, 12),   # 15  level 4
    ("XOR_FAST", 12, 2),   # 16  level 4
    ("NAND", 15, 16),      # 17  level 5
]
MIXED_OUTPUTS = [17, 13, 14, 9, 10, 7]
MIXED_WIDTHS = [4, 2, 1, 4, 1]


def ripple_adder(bits, xor="XOR_FAST"):
    """a + b, both `bits` wide: inputs a_0.. (wires 0 .. bits-1), b_0.. ; outputs the bits+1 sum bits.
    Depth 2 bits - 1: the carry of bit i >= 1 is OR(AND(a_i, b_i), AND(a_i ^ b_i, carry))."""
    gates, outs = [], []
    w = 2 * bits

    def add(op, x, y):
        nonlocal w
        gates.append((op, x, y))
        w += 1
        return w - 1

    carry = None
    for i in range(bits):
        a, b = i, bits + i
        p = add(xor, a, b)
        g = add("AND", a, b)
        if carry is None:
            outs.append(p)
            carry = g
        else:
            outs.append(add(xor, p, carry))
            carry = add("OR", g, add("AND", p, carry))
    outs.append(carry)
    return 2 * bits, gates, outs


def eval_netlist(num_inputs, gates, outputs, bits):
    """The unlowered netlist on clear bits: bits[num_inputs, instances] -> [len(outputs), instances]."""
    wires = [np.asarray(b, dtype=np.uint8) for b in bits]
    inst = wires[0].shape if wires else ()
    for g in gates:
        op = g[0] if isinstance(g[0], str) else NAMES[g[0]]
        if op == "CONST0" or op == "CONST1":
            wires.append(np.full(inst, int(op == "CONST1"), dtype=np.uint8))
        elif op == "NOT":
            wires.append(1 ^ wires[g[1]])
        else:
            wires.append(TRUTH[op](wires[g[1]], wires[g[2]]))
    return np.stack([wires[o] for o in outputs])


def lwe_not(ct, q):
    """EvalNOT (binfhe-base-scheme.cpp:147-159): a -> -a, b -> q/4 - b, mod q."""
    ct = np.asarray(ct, dtype=np.uint64)
    out = (np.uint64(q) - ct) % np.uint64(q)
    out[..., -1] = (np.uint64(q + q // 4) - ct[..., -1]) % np.uint64(q)
    return out


def lwe_const(value, shape, q):
    """NoiselessEmbedding (lwe-pke.cpp:326-338): a = 0, b = value * (q >> 2)."""
    out = np.zeros(shape, dtype=np.uint64)
    out[..., -1] = value * (q >> 2)
    return out


def oracle_netlist(orc, num_inputs, gates, outputs, cts, q):
    """The oracle composed gate by gate in netlist order: cts[num_inputs, instances, n+1] ->
    [len(outputs), instances, n+1]."""
    wires = [np.ascontiguousarray(c) for c in cts]
    shape = cts.shape[1:]
    for g in gates:
        op = g[0] if isinstance(g[0], str) else NAMES[g[0]]
        if op == "CONST0" or op == "CONST1":
            wires.append(lwe_const(int(op == "CONST1"), shape, q))
        elif op == "NOT":
            wires.append(lwe_not(wires[g[1]], q))
        else:
            wires.append(orc.eval_bin_gate(op, wires[g[1]], wires[g[2]]))
    return np.stack([wires[o] for o in outputs])
