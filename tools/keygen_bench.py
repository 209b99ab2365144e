#!/usr/bin/env python3
"""From a seed to a context that has answered one call, on one MI355X, for the C2 context (STD128) and the C3
context (logQ = 12 arbFunc):

  (a) device  tfhe_setup_keygen (BinFHEContextHIP.from_keygen): the keys are generated straight into the key arena;
  (b) host    the only route before it: the CPU oracle's or_keygen (OpenMP, the box's 16 threads), then tfhe_setup
              (host NTT of every BSK polynomial, range check and repack of the KSK, PCIe upload).

Each leg is wall clock (time.perf_counter) from the seed to the return of one host-array call on the new context
(C2: EvalBinGate NAND on 4 ciphertexts; C3: EvalFunc of the cube table on 8), which ends in a device synchronise;
the context is released outside the window.  Both legs produce the same keys (tests/test_gpu_keygen.py), and the
first call's outputs are asserted equal.  A prologue runs leg (a) once per context (warm-up of every kernel; the
process's peak host memory is read after each: it must not grow with the key size), then the legs alternate three
times; the best time of each and the spread of the three (max / min - 1) are reported.

Kernel figures come from one extra tfhe_setup_keygen with TFHE_TRACE set (device events around the two row
kernels, outside the timed windows): the KSK kernel's written bytes over its time against the box's write rate
(hipMemset-style fill of 4 GiB through torch, best of five, device events), and the BSK kernel's time per row.
Device memory: what each leg's context holds after setup (free memory before - after); neither leg allocates
device scratch that grows with the keys, so this is also its peak.

    python3 tools/keygen_bench.py [--reps 3]

One JSON line.
"""
import argparse
import json
import os
import re
import resource
import socket
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tfhe-gpu_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"),
                os.path.join(ROOT, "tools")]

SEED = 7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()

    import torch

    import pyoracle
    import tfhe_amd
    from circuit_bench import capture_stderr
    from helpers import cube_lut

    assert torch.cuda.is_available(), "keygen_bench needs a GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    pyoracle.build()
    threads = int(os.environ.get("OMP_NUM_THREADS", "16"))

    contexts = {
        "C2 STD128": (tfhe_amd.params_from_set("STD128"), pyoracle.params_from_set("STD128"), "gate"),
        "C3 logQ12 arbFunc": (tfhe_amd.params_from_logq("STD128", True, 12, 0, 0, 1),
                              pyoracle.params_from_logq("STD128", True, 12, 0, 0, 1), "func"),
    }

    def first_call(cc, sk, kind):
        p = cc.params
        if kind == "gate":
            c1 = cc.Encrypt(sk, [0, 0, 1, 1], p=4, seed=100)
            c2 = cc.Encrypt(sk, [0, 1, 0, 1], p=4, seed=101)
            out = cc.EvalBinGate("NAND", c1, c2)
            assert cc.Decrypt(sk, out, p=4) == [1, 1, 1, 0]
        else:
            out = cc.EvalFunc(cc.Encrypt(sk, list(range(8)), p=8, seed=100), cube_lut(int(p.q)))
            assert cc.Decrypt(sk, out, p=8) == [m ** 3 % 8 for m in range(8)]
        return out

    def free_bytes():
        torch.cuda.synchronize(dev)
        return torch.cuda.mem_get_info(dev)[0]

    def leg_device(cp, kind):
        before = free_bytes()
        t0 = time.perf_counter()
        cc, sk = tfhe_amd.BinFHEContextHIP.from_keygen(cp, SEED)
        t1 = time.perf_counter()
        held = before - torch.cuda.mem_get_info(dev)[0]
        t1b = time.perf_counter()
        out = first_call(cc, sk, kind)
        t2 = time.perf_counter()
        cc.GPUClean()
        return dict(total_s=t2 - t0 - (t1b - t1), setup_keygen_s=t1 - t0, first_call_s=t2 - t1b, device_bytes=held), out

    def leg_host(cp, op, kind):
        before = free_bytes()
        t0 = time.perf_counter()
        sk, bsk, ksk = pyoracle.keygen(op, pyoracle.Rng(SEED))
        t1 = time.perf_counter()
        cc = tfhe_amd.BinFHEContextHIP(cp).GPUSetup(bsk, ksk)
        t2 = time.perf_counter()
        held = before - torch.cuda.mem_get_info(dev)[0]
        t2b = time.perf_counter()
        out = first_call(cc, sk, kind)
        t3 = time.perf_counter()
        cc.GPUClean()
        del bsk, ksk
        return dict(total_s=t3 - t0 - (t2b - t2), or_keygen_s=t1 - t0, tfhe_setup_s=t2 - t1, first_call_s=t3 - t2b,
                    device_bytes=held), out

    # the box's write rate: a 4 GiB fill, device events
    fill = torch.empty(1 << 32, dtype=torch.uint8, device=dev)
    fill.zero_()
    rates = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fill.zero_()
        e1.record()
        e1.synchronize()
        rates.append(fill.numel() / (e0.elapsed_time(e1) * 1e-3))
    del fill
    torch.cuda.empty_cache()
    fill_rate = max(rates)

    # prologue: HIP and every keygen kernel warm; host peak after each context's device leg
    toy, sk = tfhe_amd.BinFHEContextHIP.from_keygen(tfhe_amd.params_from_set("TOY"), SEED)
    toy.GPUClean()
    rss = {}
    for name, (cp, op, kind) in contexts.items():
        leg_device(cp, kind)
        rss[name] = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss * 1024

    rows = []
    for name, (cp, op, kind) in contexts.items():
        A, B = [], []
        for _ in range(args.reps):  # alternate the legs
            a, out_a = leg_device(cp, kind)
            b, out_b = leg_host(cp, op, kind)
            assert np.array_equal(out_a, out_b), "the two legs' first calls differ"
            A.append(a)
            B.append(b)
            print(f"[keygen_bench] {name}: device {a} host {b}", file=sys.stderr, flush=True)
        best_a, best_b = min(A, key=lambda r: r["total_s"]), min(B, key=lambda r: r["total_s"])
        spread = lambda rs: round(max(r["total_s"] for r in rs) / min(r["total_s"] for r in rs) - 1, 4)
        os.environ["TFHE_TRACE"] = "1"
        try:
            log = capture_stderr(lambda: tfhe_amd.BinFHEContextHIP.from_keygen(cp, SEED)[0].GPUClean())
        finally:
            del os.environ["TFHE_TRACE"]
        m = re.search(r"keygen: ksk ([0-9.]+) ms, (\d+) rows, (\d+) bytes; bsk ([0-9.]+) ms, (\d+) rows, (\d+) bytes", log)
        assert m, log
        ksk_ms, ksk_rows, ksk_bytes, bsk_ms, bsk_rows, bsk_bytes = (float(m.group(1)), int(m.group(2)), int(m.group(3)),
                                                                    float(m.group(4)), int(m.group(5)), int(m.group(6)))
        rnd = lambda r: {k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()}
        rows.append({
            "context": name, "n": cp.n, "N": cp.N, "bsk_coeff_bytes": cp.bsk_words() * 8, "ksk_coeff_bytes": cp.ksk_words() * 8,
            "device_best": rnd(best_a), "device_spread": spread(A), "host_best": rnd(best_b), "host_spread": spread(B),
            "host_over_device": round(best_b["total_s"] / best_a["total_s"], 2),
            "ksk_kernel_ms": ksk_ms, "ksk_rows": ksk_rows, "ksk_arena_bytes": ksk_bytes,
            "ksk_write_GBps": round(ksk_bytes / ksk_ms / 1e6, 1),
            "ksk_share_of_fill_rate": round(ksk_bytes / (ksk_ms * 1e-3) / fill_rate, 4),
            "bsk_kernel_ms": bsk_ms, "bsk_rows": bsk_rows, "bsk_arena_bytes": bsk_bytes,
            "bsk_us_per_row": round(bsk_ms * 1e3 / bsk_rows, 3),
            "host_peak_rss_bytes_after_device_leg": rss[name], "outputs_equal": True})
    print(json.dumps({"what": "seed -> context that answered one call: tfhe_setup_keygen (device) vs or_keygen + tfhe_setup "
                              "(host), wall clock, legs alternated, best of reps and spread (max / min - 1)",
                      "reps": args.reps, "oracle_threads": threads, "fill_rate_GBps": round(fill_rate / 1e9, 1),
                      "box": socket.gethostname(), "device": torch.cuda.get_device_name(0), "rows": rows}), flush=True)


if __name__ == "__main__":
    main()
