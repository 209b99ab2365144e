#!/usr/bin/env python3
"""The tiled matrix product and the dense layer on one MI355X, device-resident buffers, timed with device events.

  (1) product   tfhe_ciphertext_mul_matrix_device at examples/GEMM.cpp's shape (K = cols = 1024) on the logQ = 12
                arbFunc context (n = 1305), instances = 1 and 8, at moduli 2^35 (qKS: the M64 instance), 2^12 (M32)
                and 2^54 - 77823 (GEN).  Three windows per row; the median and the spread (max / min - 1) are
                reported.  --parent FILE adds the first-draft kernel's times: a JSON object
                {"<modulus>": [ms, ms, ms]} of k_ct_mul_matrix's kernel time (rocprofv3 --kernel-trace of the parent
                commit's tools/mm_bench.py), with the ratio parent / new.
  (2) layer     tfhe_eval_dense_device at K = cols = 256, instances = 16 (4096 results, a negacyclic table: 4096
                bootstraps) on the logQ = 12 arbFunc context and on STD128: the total, the matrix product's share
                (the same product timed alone), and the same work through host arrays (16 x CiphertextMulMatrix, the
                bias added in numpy, one EvalFunc; wall clock).  The two outputs are asserted equal.

    python3 tools/dense_bench.py [--window 0.3] [--parent FILE] [--skip-layer] [--product-runs RUN.json ...]

One JSON line (profiles/dense/dense_bench.json).
"""
import argparse
import json
import os
import socket
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tfhe-gpu_amd"), os.path.join(ROOT, "tools")]

MODULI = [("2^35", 1 << 35, "M64"), ("2^12", 1 << 12, "M32"), ("2^54-77823", (1 << 54) - 77823, "GEN")]


def negacyclic_lut(q):
    h = q // 2
    return np.array([1 + (3 * x) % (q - 1) if x < h else q - 1 - (3 * (x - h)) % (q - 1) for x in range(q)], dtype=np.uint64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3, help="seconds of work per timed window")
    ap.add_argument("--parent", default=None, help="JSON file of the parent kernel's times per modulus")
    ap.add_argument("--skip-layer", action="store_true")
    ap.add_argument("--product-runs", nargs="*", default=[],
                    help="outputs of earlier --skip-layer runs (the repetitions alternated with the parent's): the "
                         "product rows become the median over those runs instead of being timed again")
    args = ap.parse_args()

    import torch

    import tfhe_amd
    from bench import synthetic_keys

    assert torch.cuda.is_available(), "dense_bench needs a GPU"
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

    def windows(fn):
        fn()
        sync()
        out = []
        for _ in range(3):
            reps = max(3, int(args.window * 1e3 / timed(fn, 1)) + 1)
            out.append(timed(fn, reps))
        return out

    def context(p):
        bsk, ksk = synthetic_keys(p)
        return tfhe_amd.BinFHEContextHIP(p).GPUSetup(bsk, ksk)

    parent = json.load(open(args.parent)) if args.parent else {}
    kt, ctile, threads = tfhe_amd.mm_tiles()
    arb = tfhe_amd.params_from_logq("STD128", True, 12, 0, 0, 1)
    ctx = context(arb)
    w = arb.n + 1
    K = cols = 1024
    product = []
    earlier = [json.loads(open(f).read().strip().splitlines()[-1])["product"] for f in args.product_runs]
    for name, mod, inst_name in MODULI:
        d_m = torch.randint(0, 64, (K, cols), dtype=torch.int64, device=dev, generator=gen)  # GEMM.cpp's entries
        for inst in (1, 8):
            if earlier:  # one figure per earlier run: its median window
                ws = [r["ms"] for run in earlier for r in run if r["modulus"] == name and r["instances"] == inst]
                assert len(ws) == len(earlier), (name, inst)
            else:
                d_ct = torch.randint(0, mod, (inst, K, w), dtype=torch.int64, device=dev, generator=gen)
                d_out = torch.empty((inst, cols, w), dtype=torch.int64, device=dev)
                ws = windows(lambda: ctx.CiphertextMulMatrixDevice(inst, K, d_ct.data_ptr(), cols, d_m.data_ptr(), mod,
                                                                   d_out.data_ptr(), stream=sp))
                del d_ct, d_out
            row = {"modulus": name, "kernel_instance": inst_name, "instances": inst, "K": K, "cols": cols, "n": arb.n,
                   "ms": round(statistics.median(ws), 4), ("runs_ms" if earlier else "windows_ms"): [round(x, 4) for x in ws],
                   "spread": round(max(ws) / min(ws) - 1, 4)}
            if inst == 1 and str(mod) in parent:
                pm = parent[str(mod)]
                row["parent_kernel_ms"] = round(statistics.median(pm), 4)
                row["parent_runs_ms"] = [round(x, 4) for x in pm]
                row["parent_spread"] = round(max(pm) / min(pm) - 1, 4)
                row["parent_over_new"] = round(row["parent_kernel_ms"] / row["ms"], 2)
            product.append(row)
            print(f"[dense_bench] {row}", file=sys.stderr, flush=True)

    layer = []
    if not args.skip_layer:
        for cname, p in (("logQ=12 arbFunc", arb), ("STD128", tfhe_amd.params_from_set("STD128"))):
            if p is not arb:
                ctx.GPUClean()
                ctx = context(p)
            q, w, K, cols, inst = int(p.q), p.n + 1, 256, 256, 16
            rs = np.random.default_rng(9)
            ct = rs.integers(0, q, (inst, K, w), dtype=np.uint64)
            mat = rs.integers(-8, 8, (K, cols), dtype=np.int64)
            bias = rs.integers(0, q, cols, dtype=np.uint64)
            lut = negacyclic_lut(q)
            d_ct, d_m, d_b, d_l = (torch.from_numpy(a.view(np.int64)).to(dev) for a in (ct, mat, bias, lut))
            d_out = torch.empty((inst, cols, w), dtype=torch.int64, device=dev)
            d_z = torch.empty_like(d_out)
            dense = lambda: ctx.EvalDenseDevice(inst, K, d_ct.data_ptr(), cols, d_m.data_ptr(), d_l.data_ptr(),
                                                d_out.data_ptr(), d_bias=d_b.data_ptr(), q=q, stream=sp)
            prod = lambda: ctx.CiphertextMulMatrixDevice(inst, K, d_ct.data_ptr(), cols, d_m.data_ptr(), q,
                                                         d_z.data_ptr(), d_bias=d_b.data_ptr(), stream=sp)
            wd, wp = windows(dense), windows(prod)

            def host():
                z = np.stack([ctx.CiphertextMulMatrix(x, mat, q) for x in ct])
                z[:, :, -1] = (z[:, :, -1] + bias[None, :]) % np.uint64(q)
                return ctx.EvalFunc(z.reshape(-1, w), lut, q).reshape(z.shape)

            want = host()
            wh = []
            for _ in range(3):
                t = time.perf_counter()
                host()
                wh.append((time.perf_counter() - t) * 1e3)
            sync()
            assert np.array_equal(d_out.cpu().numpy().view(np.uint64), want), "device layer != host-array composition"
            td, tp, th = statistics.median(wd), statistics.median(wp), statistics.median(wh)
            row = {"context": cname, "instances": inst, "K": K, "cols": cols, "bootstraps": inst * cols,
                   "dense_ms": round(td, 3), "dense_spread": round(max(wd) / min(wd) - 1, 4),
                   "product_ms": round(tp, 4), "product_share": round(tp / td, 4),
                   "host_arrays_ms": round(th, 2), "host_arrays_spread": round(max(wh) / min(wh) - 1, 4),
                   "host_over_device": round(th / td, 2), "outputs_equal": True}
            layer.append(row)
            print(f"[dense_bench] {row}", file=sys.stderr, flush=True)
    try:
        clock_mhz = torch.cuda.clock_rate()
    except Exception:
        clock_mhz = None
    print(json.dumps({"what": "tiled CiphertextMulMatrix (device-resident, event-timed) and the dense layer "
                              "EvalFunc(W^T x + b) on top of it",
                      "tiles": {"kt": kt, "ct": ctile, "threads": threads}, "box": socket.gethostname(),
                      "device": torch.cuda.get_device_name(0), "clock_mhz": clock_mhz, "product": product,
                      "layer": layer}), flush=True)
    ctx.GPUClean()


if __name__ == "__main__":
    main()
