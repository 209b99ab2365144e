#!/usr/bin/env python3
"""A 16-digit base-4 adder over Z_8 digits (per digit s = x + y + carry, digit = mod4(s), carry = div4(s): 32 LUT
nodes, 64 bootstraps on 32 levels) on one MI355X, the C3 context (logQ = 12 arbFunc, N = q = 2048), at
instances = 1, 16, 64 and 256 independent input sets:

  (a) circuit   one tfhe_eval_fcircuit_device call: every level is one mixed batch -- a periodic and an arbitrary
                record side by side, one preparation launch, one blind rotation at a-modulus 2N, one extraction,
                two key switches (q and 2q);
  (b) baseline  what the EvalFunc entry point alone offers: x + y for all digits in one torch operation, then per
                digit the carry added with torch arithmetic and one EvalFuncDevice call per table.

Both run on one stream and are timed with device events over enough calls for a window of about half a second, after
a warm-up call of every shape, alternating (a) and (b) three times; the best window of each and the spread of the
windows (max / min - 1) are reported.  The outputs of (a) and (b) are asserted equal.  The share of (a) spent in the
preparation and output kernels comes from the engine's own event pairs around those launches (the trace knob), in one
extra call outside the timed windows.

    python3 tools/fcircuit_bench.py [--digits 16] [--instances 1,16,64,256] [--window 0.5]

One JSON line.
"""
import argparse
import json
import os
import re
import socket
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tfhe-gpu_amd"), os.path.join(ROOT, "tools")]

P = 8


def table(f, q):
    return np.array([(f(i // (q // P)) * (q // P)) % q for i in range(q)], dtype=np.uint64)


def adder(digits):
    """inputs x_0 .. (wires 0 .. digits-1), y_0 ..; tables 0 = mod4, 1 = div4; outputs the digits, then the last carry"""
    nodes, outs, carry = [], [], None
    wire = 2 * digits
    for d in range(digits):
        nodes.append(("LIN", (d, 1), (digits + d, 1)))
        s, wire = wire, wire + 1
        if carry is not None:
            nodes.append(("LIN", (s, 1), (carry, 1)))
            s, wire = wire, wire + 1
        nodes += [("LUT", 0, (s, 1)), ("LUT", 1, (s, 1))]
        outs.append(wire)
        carry = wire + 1
        wire += 2
    return 2 * digits, nodes, outs + [carry]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--digits", type=int, default=16)
    ap.add_argument("--instances", default="1,16,64,256")
    ap.add_argument("--window", type=float, default=0.5, help="seconds of work per timed window")
    args = ap.parse_args()

    import torch

    import tfhe_amd
    from bench import synthetic_keys
    from circuit_bench import capture_stderr

    assert torch.cuda.is_available(), "fcircuit_bench needs a GPU"
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    sp = stream.cuda_stream
    sync = lambda: torch.cuda.synchronize(dev)

    p = tfhe_amd.params_from_logq("STD128", True, 12, 0, 0, 1)
    q, w, D = int(p.q), p.n + 1, args.digits
    bsk, ksk = synthetic_keys(p)
    ctx = tfhe_amd.BinFHEContextHIP(p).GPUSetup(bsk, ksk)
    del bsk, ksk
    luts = np.stack([table(lambda m: m % 4, q), table(lambda m: m // 4, q)])
    ni, nodes, outs = adder(D)
    fc = tfhe_amd.FuncCircuit(ni, nodes, luts, outs, q)
    info = fc.info()
    assert info["bootstraps"] == 4 * D and (info["periodic"], info["arbitrary"]) == (1, 1)
    d_luts = torch.from_numpy(luts.astype(np.int64)).to(dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(18)

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
        d_in = torch.randint(0, q, (ni, inst, w), dtype=torch.int64, device=dev, generator=gen)
        d_out = torch.zeros((D + 1, inst, w), dtype=torch.int64, device=dev)
        b_out = torch.zeros_like(d_out)

        def circuit():
            ctx.EvalFuncCircuitDevice(fc, inst, d_in.data_ptr(), d_out.data_ptr(), stream=sp)

        def baseline():
            s = torch.remainder(d_in[:D] + d_in[D:], q)
            carry = None
            for d in range(D):
                v = s[d] if carry is None else torch.remainder(s[d] + carry, q)
                ctx.EvalFuncDevice(inst, v.data_ptr(), d_luts[0].data_ptr(), b_out[d].data_ptr(), q=q, stream=sp)
                carry = b_out[D] if d == D - 1 else torch.empty_like(v)
                ctx.EvalFuncDevice(inst, v.data_ptr(), d_luts[1].data_ptr(), carry.data_ptr(), q=q, stream=sp)

        circuit()
        baseline()
        sync()
        assert torch.equal(d_out, b_out), "the circuit and the per-node EvalFuncDevice composition differ"
        wa, wb = [], []
        for _ in range(3):  # alternate the legs
            ra = max(3, int(args.window * 1e3 / timed(circuit, 1)) + 1)
            wa.append(timed(circuit, ra))
            rb = max(3, int(args.window * 1e3 / timed(baseline, 1)) + 1)
            wb.append(timed(baseline, rb))
        ta, tb = min(wa), min(wb)
        with ctx.knobs_set(trace=1):
            log = capture_stderr(lambda: (circuit(), sync()))
        m = re.search(r"in ([0-9.]+) ms; (\d+) prep launches ([0-9.]+) ms, output ([0-9.]+) ms", log)
        share = round((float(m.group(3)) + float(m.group(4))) / float(m.group(1)), 4) if m else None
        n = info["bootstraps"] * inst
        rows.append({"instances": inst, "circuit_ms": round(ta, 3), "circuit_bootstraps_per_s": round(n / ta * 1e3, 1),
                     "baseline_ms": round(tb, 3), "baseline_bootstraps_per_s": round(n / tb * 1e3, 1),
                     "circuit_over_baseline": round(tb / ta, 3),
                     "circuit_spread": round(max(wa) / min(wa) - 1, 4), "baseline_spread": round(max(wb) / min(wb) - 1, 4),
                     "prep_and_output_share_of_circuit": share, "prep_launches": int(m.group(2)) if m else None,
                     "outputs_equal": True})
        print(f"[fcircuit_bench] {rows[-1]}", file=sys.stderr, flush=True)
    try:
        clock_mhz = torch.cuda.clock_rate()
    except Exception:
        clock_mhz = None
    print(json.dumps({"what": f"{D}-digit base-4 adder over Z_8 digits (mod4 periodic, div4 arbitrary), logQ = 12 arbFunc "
                              "context, device-resident: one EvalFuncCircuitDevice call vs per-digit torch arithmetic + "
                              "one EvalFuncDevice call per table",
                      "lut_nodes": 2 * D, "bootstraps": info["bootstraps"], "levels": info["levels"],
                      "widest_level": info["widest_level"], "box": socket.gethostname(),
                      "device": torch.cuda.get_device_name(0), "clock_mhz": clock_mhz, "rows": rows}), flush=True)
    ctx.GPUClean()


if __name__ == "__main__":
    main()
