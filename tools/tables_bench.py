#!/usr/bin/env python3
"""The layers with one table per channel on one MI355X, device-resident buffers, timed with device events around whole
calls.

Shapes: 16 instances of LeNet's first convolution (1 x 32 x 32 -> 6 planes of 28 x 28 by a 5 x 5 window) and of its
84-column dense layer (K = 120), on STD128 and on the logQ = 12 arbFunc context, each at its own ciphertext modulus q.

  (i)   tabled       the layer with one table per channel, all of one class (negacyclic, every table different)
  (ii)  shared       the same layer with one shared table (the path the tabled one must not be slower than)
  (iii) composition  what a user had to write before: the linear part, then per channel a torch gather of the channel's
                     results, EvalFuncDevice with the channel's table, and a scatter.  Its output is asserted equal to
                     (i)'s, word for word.
  (iv)  mixed        (i) with the three classes cycling over the channels

The sides alternate, three windows each; the median and the spread (max / min - 1) of each are reported, with the
ratios (i) / (ii) and (iii) / (i).

    python3 tools/tables_bench.py [--window 0.3]

One JSON line (profiles/tables/tables_bench.json).
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

INSTANCES = 16
CONV = dict(c_in=1, h=32, w=32, c_out=6, kh=5, kw=5, stride_h=1, stride_w=1, pad_h=0, pad_w=0, groups=1)
DENSE = dict(K=120, cols=84)


def tables(q, channels, mixed):
    """[channels, q]: every table different; negacyclic throughout, or the three classes cycling over the channels"""
    h, x = q // 2, np.arange(q, dtype=np.int64)
    out = []
    for c in range(channels):
        k = 3 + 2 * c
        neg = np.where(x < h, 1 + (k * x) % (q - 1), q - 1 - (k * (x - h)) % (q - 1))
        per = (x * k) % h
        arb = (x * x * x * k + c) % q
        out.append([neg, per, arb][c % 3] if mixed else neg)
    return np.stack(out).astype(np.uint64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3, help="seconds of work per timed window")
    args = ap.parse_args()

    import torch

    import tfhe_amd
    from bench import synthetic_keys

    assert torch.cuda.is_available(), "tables_bench needs a GPU"
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
        q, w, inst = int(p.q), p.n + 1, INSTANCES
        for sname in ("lenet-conv1", "lenet-fc2"):
            if sname == "lenet-conv1":
                desc = tfhe_amd.Conv2d(**CONV)
                oh, ow, K = tfhe_amd.conv2d_shape(desc)
                channels, per_channel = desc.c_out, oh * ow
                d_ct = torch.randint(0, q, (inst, desc.c_in, desc.h, desc.w, w), dtype=torch.int64, device=dev, generator=gen)
                d_wt = torch.randint(-8, 8, (channels, desc.c_in, desc.kh, desc.kw), dtype=torch.int64, device=dev, generator=gen)

                def layer(d_l, T, out):
                    ctx.EvalConv2dDevice(desc, inst, d_ct.data_ptr(), d_wt.data_ptr(), d_l.data_ptr(), out.data_ptr(), q=q,
                                         stream=sp, num_luts=T)

                def linear(out):
                    ctx.CiphertextConv2dDevice(desc, inst, d_ct.data_ptr(), d_wt.data_ptr(), q, out.data_ptr(), stream=sp)
            else:
                K, channels, per_channel = DENSE["K"], DENSE["cols"], 1
                d_ct = torch.randint(0, q, (inst, K, w), dtype=torch.int64, device=dev, generator=gen)
                d_wt = torch.randint(-8, 8, (K, channels), dtype=torch.int64, device=dev, generator=gen)

                def layer(d_l, T, out):
                    ctx.EvalDenseDevice(inst, K, d_ct.data_ptr(), channels, d_wt.data_ptr(), d_l.data_ptr(), out.data_ptr(),
                                        q=q, stream=sp, num_luts=T)

                def linear(out):
                    ctx.CiphertextMulMatrixDevice(inst, K, d_ct.data_ptr(), channels, d_wt.data_ptr(), q, out.data_ptr(),
                                                  stream=sp)
            one, mix = tables(q, channels, False), tables(q, channels, True)
            classes = tfhe_amd.lut_classes(mix, q).tolist()
            assert tfhe_amd.lut_classes(one, q).tolist() == [0] * channels and sorted(set(classes)) == [0, 1, 2]
            d_one, d_mix = (torch.from_numpy(t.view(np.int64)).to(dev) for t in (one, mix))
            shape = (inst, channels, per_channel, w)
            d_out, d_sh, d_z, d_comp = (torch.empty(shape, dtype=torch.int64, device=dev) for _ in range(4))

            def tabled():
                layer(d_one, channels, d_out)

            def shared():
                layer(d_one[0], 1, d_sh)

            def composition():
                linear(d_z)
                for c in range(channels):
                    rows_c = d_z[:, c].contiguous()  # the gather
                    res = torch.empty_like(rows_c)
                    ctx.EvalFuncDevice(inst * per_channel, rows_c.data_ptr(), d_one[c].data_ptr(), res.data_ptr(), q=q,
                                       stream=sp)
                    d_comp[:, c] = res  # the scatter

            def mixed():
                layer(d_mix, channels, d_out)

            wt, ws, wc, wm = alternating([tabled, shared, composition, mixed])
            tabled()
            composition()
            sync()
            assert torch.equal(d_out, d_comp), "tabled layer != per-channel composition"
            (tt, rt, st), (ts, rs, ss), (tc, rc, sc), (tm, rm, sm) = stats(wt), stats(ws), stats(wc), stats(wm)
            _, per, boots = tfhe_amd.lut_tables_info(mix, q, per_channel, inst * channels * per_channel)
            row = {"context": cname, "shape": sname, "instances": inst, "n": p.n, "q": q, "channels": channels,
                   "results": inst * channels * per_channel,
                   "tabled_ms": tt, "tabled_windows_ms": rt, "tabled_spread": st,
                   "shared_ms": ts, "shared_windows_ms": rs, "shared_spread": ss,
                   "tabled_over_shared": round(tt / ts, 4),
                   "composition_ms": tc, "composition_windows_ms": rc, "composition_spread": sc,
                   "composition_over_tabled": round(tc / tt, 4), "outputs_equal": True,
                   "mixed_ms": tm, "mixed_windows_ms": rm, "mixed_spread": sm, "mixed_per_class": list(per),
                   "mixed_bootstraps": boots, "mixed_over_tabled": round(tm / tt, 4)}
            rows.append(row)
            print(f"[tables_bench] {row}", file=sys.stderr, flush=True)
        ctx.GPUClean()
    try:
        clock_mhz = torch.cuda.clock_rate()
    except Exception:
        clock_mhz = None
    print(json.dumps({"what": "the convolution and dense layers with one table per channel (all negacyclic) against the "
                              "same layers with one shared table, the per-channel gather + EvalFuncDevice + scatter, "
                              "and the three classes mixed over the channels (event-timed, alternating windows)",
                      "box": socket.gethostname(), "device": torch.cuda.get_device_name(0), "clock_mhz": clock_mhz,
                      "rows": rows}), flush=True)


if __name__ == "__main__":
    main()
