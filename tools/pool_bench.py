#!/usr/bin/env python3
"""The pooling layer on one MI355X, device-resident buffers, timed with device events around whole calls.

Shapes: LeNet's two 2 x 2 max pools over 16 instances -- pool1: 6 planes of 28 x 28; pool2: 16 planes of 10 x 10 -- on
STD128 and on the logQ = 12 arbFunc context, each at its own ciphertext modulus q.

  (1) layer        tfhe_eval_pool2d_device with the negacyclic max table, against
  (2) composition  what a user had to write before: per round a torch gather of both operands, a subtract,
                   EvalFuncDevice, and an add.  The two sides alternate, three windows each; the median and the spread
                   (max / min - 1) of each side are reported, with the bytes of the buffers the composition allocates.
                   The two outputs are asserted equal, word for word.
  (3) func         EvalFuncDevice alone on the layer's two round batches: what the layer spends in its bootstraps;
                   the layer's share outside them is 1 - func / layer.
  (4) arbitrary    the layer with the default (arbitrary-class) max table: two bootstraps per pair.

    python3 tools/pool_bench.py [--window 0.3]

One JSON line (profiles/pool/pool_bench.json).
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

SHAPES = [("lenet-pool1", dict(c=6, h=28, w=28, kh=2, kw=2, stride_h=2, stride_w=2, pad_h=0, pad_w=0)),
          ("lenet-pool2", dict(c=16, h=10, w=10, kh=2, kw=2, stride_h=2, stride_w=2, pad_h=0, pad_w=0))]
INSTANCES = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3, help="seconds of work per timed window")
    args = ap.parse_args()

    import torch

    import tfhe_amd
    from bench import synthetic_keys

    assert torch.cuda.is_available(), "pool_bench needs a GPU"
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    sp = stream.cuda_stream
    sync = lambda: torch.cuda.synchronize(dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(9)

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
        d_neg = torch.from_numpy(tfhe_amd.max_table(q, True).view(np.int64)).to(dev)
        d_arb = torch.from_numpy(tfhe_amd.max_table(q).view(np.int64)).to(dev)
        for sname, fields in SHAPES:
            desc = tfhe_amd.Pool2d(**fields)
            oh, ow, rounds, pairs = tfhe_amd.pool2d_shape(desc)
            inst = INSTANCES
            # values below q/4: the differences stay inside the negacyclic table's range (timing does not depend on it)
            d_ct = torch.randint(0, q // 4, (inst, desc.c, desc.h, desc.w, w), dtype=torch.int64, device=dev, generator=gen)
            d_out = torch.empty((inst, desc.c, oh, ow, w), dtype=torch.int64, device=dev)
            batches = [inst * desc.c * oh * ow * 2, inst * desc.c * oh * ow]  # the pairs of the two rounds
            d_z = torch.randint(0, q, (batches[0], w), dtype=torch.int64, device=dev, generator=gen)
            d_f = torch.empty_like(d_z)
            kept = {}

            def layer(table=d_neg):
                ctx.EvalPool2dDevice(desc, inst, d_ct.data_ptr(), table.data_ptr(), d_out.data_ptr(), q=q, stream=sp)

            def pair(a, b, extra):
                z = (a - b) & (q - 1)
                f = torch.empty_like(z)
                ctx.EvalFuncDevice(z.numel() // w, z.data_ptr(), d_neg.data_ptr(), f.data_ptr(), q=q, stream=sp)
                r = (f + b) & (q - 1)
                extra.append(8 * (a.numel() + b.numel() + z.numel() + f.numel() + r.numel()))
                return r

            def composition():
                extra = []
                x = d_ct.reshape(inst, desc.c, oh, 2, ow, 2, w)
                a = torch.stack((x[:, :, :, 0, :, 0], x[:, :, :, 1, :, 0])).contiguous()  # taps 0 and 2
                b = torch.stack((x[:, :, :, 0, :, 1], x[:, :, :, 1, :, 1])).contiguous()  # taps 1 and 3
                r = pair(a, b, extra)
                kept["out"] = pair(r[0], r[1], extra)
                kept["extra_bytes"] = sum(extra)

            def func():
                for B in batches:
                    ctx.EvalFuncDevice(B, d_z.data_ptr(), d_neg.data_ptr(), d_f.data_ptr(), q=q, stream=sp)

            wl, wc, wf = alternating([layer, composition, func])
            layer()
            composition()
            sync()
            assert torch.equal(d_out, kept["out"]), "layer != composition"
            (wa,) = alternating([lambda: layer(d_arb)])
            (tl, rl, sl), (tc, rc, sc), (tf, rf, sf), (ta, ra, sa) = stats(wl), stats(wc), stats(wf), stats(wa)
            row = {"context": cname, "shape": sname, "instances": inst, "n": p.n, "q": q, "rounds": rounds,
                   "pairs": pairs * desc.c * inst, "layer_ms": tl, "layer_windows_ms": rl, "layer_spread": sl,
                   "composition_ms": tc, "composition_windows_ms": rc, "composition_spread": sc,
                   "composition_over_layer": round(tc / tl, 4), "composition_extra_bytes": kept["extra_bytes"],
                   "layer_extra_bytes": 8 * w * (2 * batches[0] + batches[0]),  # flat rows z | f, and the slot store
                   "input_bytes": d_ct.numel() * 8, "outputs_equal": True,
                   "func_ms": tf, "func_windows_ms": rf, "func_spread": sf, "outside_func_share": round(1 - tf / tl, 5),
                   "arbitrary_layer_ms": ta, "arbitrary_windows_ms": ra, "arbitrary_spread": sa,
                   "arbitrary_over_negacyclic": round(ta / tl, 4)}
            rows.append(row)
            print(f"[pool_bench] {row}", file=sys.stderr, flush=True)
            kept.clear()
        ctx.GPUClean()
    try:
        clock_mhz = torch.cuda.clock_rate()
    except Exception:
        clock_mhz = None
    print(json.dumps({"what": "the pooling layer (tfhe_eval_pool2d_device, negacyclic max table) against the per-round "
                              "torch gather + subtract + EvalFuncDevice + add, EvalFuncDevice alone on the same "
                              "batches, and the arbitrary-class table (event-timed, alternating windows)",
                      "box": socket.gethostname(), "device": torch.cuda.get_device_name(0), "clock_mhz": clock_mhz,
                      "rows": rows}), flush=True)


if __name__ == "__main__":
    main()
