#!/usr/bin/env python3
"""Conv2d on ciphertexts and the convolution layer on one MI355X, device-resident buffers, timed with device events.

Shapes: LeNet's two convolutions over 16 instances -- conv1: 1 -> 6 planes, 5 x 5 on 28 x 28 with padding 2; conv2:
6 -> 16 planes, 5 x 5 on 14 x 14 without padding -- on STD128 and on the logQ = 12 arbFunc context, each at its own
ciphertext modulus q.

  (1) product   tfhe_ciphertext_conv2d_device (the gather inside the kernel) against the composition a user had to
                write before: a torch gather into an im2col buffer [instances oh ow][K][n+1], CiphertextMulMatrixDevice,
                and a permute to plane-major order.  The two sides alternate, three windows each; the median and the
                spread (max / min - 1) of each side are reported, with the bytes of the im2col buffer the composition
                needs.  The two outputs are asserted equal.
  (2) layer     tfhe_eval_conv2d_device (a negacyclic table) on the same shapes: the total and the product's share.

    python3 tools/conv_bench.py [--window 0.3] [--skip-layer]

One JSON line (profiles/conv/conv_bench.json).
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

SHAPES = [("lenet-conv1", dict(c_in=1, h=28, w=28, c_out=6, kh=5, kw=5, stride_h=1, stride_w=1, pad_h=2, pad_w=2, groups=1)),
          ("lenet-conv2", dict(c_in=6, h=14, w=14, c_out=16, kh=5, kw=5, stride_h=1, stride_w=1, pad_h=0, pad_w=0, groups=1))]
INSTANCES = 16


def negacyclic_lut(q):
    h = q // 2
    return np.array([1 + (3 * x) % (q - 1) if x < h else q - 1 - (3 * (x - h)) % (q - 1) for x in range(q)], dtype=np.uint64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3, help="seconds of work per timed window")
    ap.add_argument("--skip-layer", action="store_true")
    args = ap.parse_args()

    import torch

    import tfhe_amd
    from bench import synthetic_keys

    assert torch.cuda.is_available(), "conv_bench needs a GPU"
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    sp = stream.cuda_stream
    sync = lambda: torch.cuda.synchronize(dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(8)

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(reps):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / reps  # ms per call

    def alternating(fns, floor=3):
        """three windows per side, the sides taking turns"""
        for fn in fns:
            fn()
        sync()
        reps = [max(floor, int(args.window * 1e3 / timed(fn, 1)) + 1) for fn in fns]
        out = [[] for _ in fns]
        for _ in range(3):
            for k, fn in enumerate(fns):
                out[k].append(timed(fn, reps[k]))
        return out

    def stats(ws, digits=4):
        return round(statistics.median(ws), digits), [round(x, digits) for x in ws], round(max(ws) / min(ws) - 1, 4)

    product, layer = [], []
    for cname, p in (("STD128", tfhe_amd.params_from_set("STD128")),
                     ("logQ=12 arbFunc", tfhe_amd.params_from_logq("STD128", True, 12, 0, 0, 1))):
        bsk, ksk = synthetic_keys(p)
        ctx = tfhe_amd.BinFHEContextHIP(p).GPUSetup(bsk, ksk)
        del bsk, ksk
        q, w = int(p.q), p.n + 1
        for sname, fields in SHAPES:
            desc = tfhe_amd.Conv2d(**fields)
            oh, ow, K = tfhe_amd.conv2d_shape(desc)
            npos, inst = oh * ow, INSTANCES
            d_ct = torch.randint(0, q, (inst, desc.c_in, desc.h, desc.w, w), dtype=torch.int64, device=dev, generator=gen)
            d_w = torch.randint(-8, 8, (desc.c_out, desc.c_in, desc.kh, desc.kw), dtype=torch.int64, device=dev, generator=gen)
            d_b = torch.randint(0, q, (desc.c_out,), dtype=torch.int64, device=dev, generator=gen)
            d_out = torch.empty((inst, desc.c_out, oh, ow, w), dtype=torch.int64, device=dev)
            d_mat = d_w.reshape(desc.c_out, K).t().contiguous()  # the composition's [K][cols]: prepared once, not timed
            d_z = torch.empty((inst * npos, desc.c_out, w), dtype=torch.int64, device=dev)
            kept = {}

            def gathered():
                ctx.CiphertextConv2dDevice(desc, inst, d_ct.data_ptr(), d_w.data_ptr(), q, d_out.data_ptr(),
                                           d_bias=d_b.data_ptr(), stream=sp)

            def composition():
                xp = torch.nn.functional.pad(d_ct, (0, 0, desc.pad_w, desc.pad_w, desc.pad_h, desc.pad_h))
                win = xp.unfold(2, desc.kh, desc.stride_h).unfold(3, desc.kw, desc.stride_w)
                cols = win.permute(0, 2, 3, 1, 5, 6, 4).reshape(inst * npos, K, w).contiguous()  # the im2col buffer
                ctx.CiphertextMulMatrixDevice(inst * npos, K, cols.data_ptr(), desc.c_out, d_mat.data_ptr(), q,
                                              d_z.data_ptr(), d_bias=d_b.data_ptr(), stream=sp)
                kept["out"] = d_z.reshape(inst, npos, desc.c_out, w).permute(0, 2, 1, 3).contiguous()
                kept["im2col_bytes"] = cols.numel() * 8

            wg, wc = alternating([gathered, composition])
            sync()
            assert torch.equal(d_out.reshape(inst, desc.c_out, npos, w), kept["out"]), "gathered product != composition"
            (tg, rg, sg), (tc, rc, sc) = stats(wg), stats(wc)
            row = {"context": cname, "shape": sname, "instances": inst, "n": p.n, "modulus": q, "K": K,
                   "results": inst * desc.c_out * npos, "gathered_ms": tg, "gathered_windows_ms": rg,
                   "gathered_spread": sg, "composition_ms": tc, "composition_windows_ms": rc, "composition_spread": sc,
                   "composition_over_gathered": round(tc / tg, 2), "im2col_bytes": kept["im2col_bytes"],
                   "gathered_extra_bytes": 0, "input_bytes": d_ct.numel() * 8, "outputs_equal": True}
            product.append(row)
            print(f"[conv_bench] {row}", file=sys.stderr, flush=True)
            kept.clear()
            if not args.skip_layer:
                d_l = torch.from_numpy(negacyclic_lut(q).view(np.int64)).to(dev)
                d_y = torch.empty_like(d_out)

                def conv_layer():
                    ctx.EvalConv2dDevice(desc, inst, d_ct.data_ptr(), d_w.data_ptr(), d_l.data_ptr(), d_y.data_ptr(),
                                         d_bias=d_b.data_ptr(), q=q, stream=sp)

                (wl,) = alternating([conv_layer], floor=1)
                tl, rl, sl = stats(wl, 3)
                row = {"context": cname, "shape": sname, "instances": inst, "bootstraps": inst * desc.c_out * npos,
                       "layer_ms": tl, "layer_windows_ms": rl, "layer_spread": sl, "product_ms": tg,
                       "product_share": round(tg / tl, 5)}
                layer.append(row)
                print(f"[conv_bench] {row}", file=sys.stderr, flush=True)
        ctx.GPUClean()
    try:
        clock_mhz = torch.cuda.clock_rate()
    except Exception:
        clock_mhz = None
    kt, ctile, threads, positions = tfhe_amd.conv2d_tiles()
    print(json.dumps({"what": "Conv2d on ciphertexts with the gather in the kernel against im2col + "
                              "CiphertextMulMatrixDevice + permute (event-timed, alternating windows), and the "
                              "convolution layer on top of it",
                      "tiles": {"kt": kt, "ct": ctile, "threads": threads, "positions": positions},
                      "box": socket.gethostname(), "device": torch.cuda.get_device_name(0), "clock_mhz": clock_mhz,
                      "product": product, "layer": layer}), flush=True)


if __name__ == "__main__":
    main()
