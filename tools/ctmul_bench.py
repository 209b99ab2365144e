#!/usr/bin/env python3
"""The product of two encrypted tensors on one MI355X, device-resident buffers, timed with device events around whole
calls.

Shapes a user would run: a 16 x 16 x 16 matrix product over 4 instances (16,384 products, 32,768 look-ups per call)
and 8,192 elementwise products (16,384 look-ups) -- on STD128 and on the logQ = 12 arbFunc context, each at its own
ciphertext modulus q, with the negacyclic product tables (one bootstrap per look-up).

  (a) layer        tfhe_eval_ct_matmul_device, against
  (b) composition  what a user had to write before: torch broadcast adds into the 2 P flat rows, one
                   EvalFuncTablesDevice over them (inner = P: the sums take table 0, the differences table 1), a
                   subtract and a torch sum over k.  The sides alternate, three windows each; the median and the
                   spread (max / min - 1) of each side are reported.  The two outputs are asserted equal, word for word.
  (c) func         EvalFuncTablesDevice alone on the same 2 P batch: what the layer spends in its bootstraps; the
                   layer's share outside them is (a - c) / a.

    python3 tools/ctmul_bench.py [--window 0.3]

One JSON line (profiles/ctmul/ctmul_bench.json).
"""
import argparse
import json
import os
import socket
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tfhe-gpu_amd"), os.path.join(ROOT, "tools")]

SHAPES = [("matmul-4x16x16x16", 4, (16, 16, 16)), ("elementwise-8192", 8192, (1, 1, 1))]
P_MSG = 16  # the product tables' plaintext modulus (timing does not depend on it)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3, help="seconds of work per timed window")
    args = ap.parse_args()

    import torch

    import tfhe_amd
    from bench import synthetic_keys

    assert torch.cuda.is_available(), "ctmul_bench needs a GPU"
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    sp = stream.cuda_stream
    sync = lambda: torch.cuda.synchronize(dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(11)

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(reps):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / reps  # ms per call

    def alternating(fns):
        """three windows per side, the sides taking turns; the warm-up call sizes the windows"""
        reps = [max(1, int(args.window * 1e3 / timed(fn, 1))) for fn in fns]
        out = [[] for _ in fns]
        for _ in range(3):
            for k, fn in enumerate(fns):
                out[k].append(timed(fn, reps[k]))
        return out

    def stats(ws, digits=3):
        return round(statistics.median(ws), digits), [round(x, digits) for x in ws], round(max(ws) / min(ws) - 1, 4)

    rows = []
    for cname, p in (("STD128", tfhe_amd.params_from_set("STD128")),
                     ("logQ=12 arbFunc", tfhe_amd.params_from_logq("STD128", True, 12, 0, 0, 1))):
        bsk, ksk = synthetic_keys(p)
        ctx = tfhe_amd.BinFHEContextHIP(p).GPUSetup(bsk, ksk)
        del bsk, ksk
        q, w = int(p.q), p.n + 1
        d_l = torch.from_numpy(tfhe_amd.product_tables(q, P_MSG, negacyclic=True).view(np.int64)).to(dev)
        for sname, inst, (R, K, Cn) in SHAPES:
            desc = tfhe_amd.CtMatMul(R, K, Cn)
            P = inst * R * K * Cn
            d_x = torch.randint(0, q, (inst, R, K, w), dtype=torch.int64, device=dev, generator=gen)
            d_y = torch.randint(0, q, (inst, K, Cn, w), dtype=torch.int64, device=dev, generator=gen)
            d_out = torch.empty((inst, R, Cn, w), dtype=torch.int64, device=dev)
            d_z = torch.randint(0, q, (2 * P, w), dtype=torch.int64, device=dev, generator=gen)
            d_f = torch.empty_like(d_z)
            kept = {}

            def layer():
                ctx.EvalCtMatMulDevice(desc, inst, d_x.data_ptr(), d_y.data_ptr(), d_l.data_ptr(), d_out.data_ptr(), q=q,
                                       stream=sp)

            def composition():
                a = d_x[:, :, None]                    # [inst, R, 1, K, w]
                b = d_y.transpose(1, 2)[:, None]       # [inst, 1, C, K, w]
                z = torch.stack(((a + b) & (q - 1), (a - b) & (q - 1))).reshape(2 * P, w)
                f = torch.empty_like(z)
                ctx.EvalFuncTablesDevice(2 * P, z.data_ptr(), d_l.data_ptr(), 2, f.data_ptr(), inner=P, q=q, stream=sp)
                f = f.reshape(2, inst, R, Cn, K, w)
                kept["out"] = (f[0] - f[1]).sum(dim=3) & (q - 1)
                kept["extra_bytes"] = 8 * (2 * z.numel() + f.numel() // 2)  # the stacked halves, z, f, f0 - f1

            def func():
                ctx.EvalFuncTablesDevice(2 * P, d_z.data_ptr(), d_l.data_ptr(), 2, d_f.data_ptr(), inner=P, q=q, stream=sp)

            wl, wc, wf = alternating([layer, composition, func])
            layer()
            composition()
            sync()
            assert torch.equal(d_out, kept["out"]), "layer != composition"
            (tl, rl, sl), (tc, rc, sc), (tf, rf, sf) = stats(wl), stats(wc), stats(wf)
            row = {"context": cname, "shape": sname, "instances": inst, "rows": R, "inner": K, "cols": Cn, "n": p.n,
                   "q": q, "products": P, "lookups": 2 * P, "layer_ms": tl, "layer_windows_ms": rl, "layer_spread": sl,
                   "composition_ms": tc, "composition_windows_ms": rc, "composition_spread": sc,
                   "composition_over_layer": round(tc / tl, 4), "composition_extra_bytes": kept["extra_bytes"],
                   "layer_extra_bytes": 8 * w * 4 * P,  # the flat rows z | f of the dense store
                   "input_bytes": (d_x.numel() + d_y.numel()) * 8, "outputs_equal": True,
                   "func_ms": tf, "func_windows_ms": rf, "func_spread": sf,
                   "outside_func_share": round((tl - tf) / tl, 5)}
            rows.append(row)
            print(f"[ctmul_bench] {row}", file=sys.stderr, flush=True)
            kept.clear()
        ctx.GPUClean()
    try:
        clock_mhz = torch.cuda.clock_rate()
    except Exception:
        clock_mhz = None
    print(json.dumps({"what": "the product of two encrypted tensors (tfhe_eval_ct_matmul_device, negacyclic product "
                              "tables) against torch adds + EvalFuncTablesDevice + a torch sum, and "
                              "EvalFuncTablesDevice alone on the same 2 P batch (event-timed, alternating windows)",
                      "box": socket.gethostname(), "device": torch.cuda.get_device_name(0), "clock_mhz": clock_mhz,
                      "rows": rows}), flush=True)


if __name__ == "__main__":
    main()
