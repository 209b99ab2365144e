#!/usr/bin/env python3
"""A 32-bit ripple-carry adder (XOR_FAST, AND, OR: 157 gates on 63 levels) on one MI355X, STD128, at
instances = 1, 16, 64 and 256 independent input sets:

  (a) circuit   one tfhe_eval_circuit_device call: every level is one mixed batch (one preparation launch that
                gathers the operands by wire index, then blind rotation / extraction / key switch once);
  (b) baseline  what the gate entry point alone offers: per level and per gate type, torch index_select gathers of
                both operands, one EvalBinGateDevice call, and an index_copy_ scatter of the results.

Both run on one stream and are timed with device events over enough calls for a window of about half a second, after
a warm-up call of every shape, alternating (a) and (b) twice; the best window of each is reported.  The outputs of
(a) and (b) are compared.  The share of (a) spent in the preparation and output kernels comes from the engine's own
event pairs around those launches (the trace knob), in one extra call outside the timed windows.

    python3 tools/circuit_bench.py [--bits 32] [--instances 1,16,64,256] [--window 0.5]

One JSON line.
"""
import argparse
import json
import os
import re
import socket
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tfhe-gpu_amd")]


def ripple_adder(bits):
    """inputs a_0.. (wires 0 .. bits-1), b_0..; outputs the bits + 1 sum bits"""
    gates, outs = [], []
    carry = None
    for i in range(bits):
        a, b = i, bits + i
        base = 2 * bits + len(gates)
        gates += [("XOR_FAST", a, b), ("AND", a, b)]
        p, g = base, base + 1
        if carry is None:
            outs.append(p)
            carry = g
        else:
            gates += [("XOR_FAST", p, carry), ("AND", p, carry), ("OR", g, base + 3)]
            outs.append(base + 2)
            carry = base + 4
    outs.append(carry)
    return 2 * bits, gates, outs


def levels_by_type(num_inputs, gates):
    """ASAP levels of a netlist of plain gates: [level][gate type] -> (wire, in0, in1) lists"""
    level = [0] * num_inputs
    plan = []
    for g, (op, x, y) in enumerate(gates):
        lv = 1 + max(level[x], level[y])
        level.append(lv)
        while len(plan) < lv:
            plan.append({})
        plan[lv - 1].setdefault(op, []).append((num_inputs + g, x, y))
    return plan


def capture_stderr(fn):
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        return tmp.read().decode(errors="replace")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bits", type=int, default=32)
    ap.add_argument("--instances", default="1,16,64,256")
    ap.add_argument("--window", type=float, default=0.5, help="seconds of work per timed window")
    args = ap.parse_args()

    import torch

    import tfhe_amd
    from bench import synthetic_keys

    assert torch.cuda.is_available(), "circuit_bench needs a GPU"
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    sp = stream.cuda_stream
    sync = lambda: torch.cuda.synchronize(dev)

    p = tfhe_amd.params_from_set("STD128")
    bsk, ksk = synthetic_keys(p)
    ctx = tfhe_amd.BinFHEContextHIP(p).GPUSetup(bsk, ksk)
    del bsk, ksk
    ni, gates, outs = ripple_adder(args.bits)
    circ = tfhe_amd.Circuit(ni, gates, outs)
    info = circ.info()
    assert info["bootstraps"] == len(gates)
    plan = levels_by_type(ni, gates)
    w = p.n + 1
    gen = torch.Generator(device=dev)
    gen.manual_seed(17)

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(reps):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / reps  # ms per call

    rows = []
    for inst in [int(x) for x in args.instances.split(",")]:
        d_in = torch.randint(0, int(p.q), (ni, inst, w), dtype=torch.int64, device=dev, generator=gen)
        d_out = torch.zeros((len(outs), inst, w), dtype=torch.int64, device=dev)
        wires = torch.zeros((ni + len(gates), inst, w), dtype=torch.int64, device=dev)
        wires[:ni] = d_in
        idx = [{op: tuple(torch.tensor(col, dtype=torch.int64, device=dev) for col in zip(*rows_))
                for op, rows_ in lv.items()} for lv in plan]
        out_idx = torch.tensor(outs, dtype=torch.int64, device=dev)

        def circuit():
            ctx.EvalCircuitDevice(circ, inst, d_in.data_ptr(), d_out.data_ptr(), stream=sp)

        def baseline():
            for lv in idx:
                for op, (dst, i0, i1) in lv.items():
                    x = wires.index_select(0, i0)
                    y = wires.index_select(0, i1)
                    o = torch.empty_like(x)
                    ctx.EvalBinGateDevice(op, x.shape[0] * inst, x.data_ptr(), y.data_ptr(), o.data_ptr(), stream=sp)
                    wires.index_copy_(0, dst, o)

        circuit()
        baseline()
        sync()
        equal = bool(torch.equal(d_out, wires.index_select(0, out_idx)))
        ta = tb = None
        for _ in range(2):  # alternate, keep the best window of each
            ra = max(3, int(args.window * 1e3 / timed(circuit, 1)) + 1)
            t = timed(circuit, ra)
            ta = t if ta is None else min(ta, t)
            rb = max(3, int(args.window * 1e3 / timed(baseline, 1)) + 1)
            t = timed(baseline, rb)
            tb = t if tb is None else min(tb, t)
        with ctx.knobs_set(trace=1):
            log = capture_stderr(lambda: (circuit(), sync()))
        m = re.search(r"in ([0-9.]+) ms; (\d+) prep launches ([0-9.]+) ms, output ([0-9.]+) ms", log)
        share = round((float(m.group(3)) + float(m.group(4))) / float(m.group(1)), 4) if m else None
        n = len(gates) * inst
        rows.append({"instances": inst, "circuit_ms": round(ta, 3), "circuit_gates_per_s": round(n / ta * 1e3, 1),
                     "baseline_ms": round(tb, 3), "baseline_gates_per_s": round(n / tb * 1e3, 1),
                     "circuit_over_baseline": round(tb / ta, 3), "prep_and_output_share_of_circuit": share,
                     "prep_launches": int(m.group(2)) if m else None, "outputs_equal": equal})
        print(f"[circuit_bench] {rows[-1]}", file=sys.stderr, flush=True)
    try:
        clock_mhz = torch.cuda.clock_rate()
    except Exception:
        clock_mhz = None
    print(json.dumps({"what": f"{args.bits}-bit ripple-carry adder (XOR_FAST / AND / OR), STD128, device-resident: "
                              "one EvalCircuitDevice call vs per-level per-type index_select + EvalBinGateDevice + scatter",
                      "gates": len(gates), "levels": info["levels"], "widest_level": info["widest_level"],
                      "box": socket.gethostname(), "device": torch.cuda.get_device_name(0), "clock_mhz": clock_mhz,
                      "rows": rows}), flush=True)
    ctx.GPUClean()


if __name__ == "__main__":
    main()
