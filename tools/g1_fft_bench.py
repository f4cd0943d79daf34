#!/usr/bin/env python3
"""Timing of the G1 transform (svdw_g1_fft, inverse: g_to_lagrange) on the
device, one JSON line, also written to profiles/g1_fft_bench.json.

For each k of --sizes the input is svdw_srs_setup's g for halo2-base's default
secret, so the result can be compared with the setup's own g_lagrange (`same`)
and is checked with svdw_check_lagrange. For each window of --windows (0: the
planned one; the option "g1_window_bits"):

  ms            one svdw_g1_fft call; HIP events on torch's stream, median of
                --reps and the spread (the first call, which sizes the scratch,
                is the warm-up and is reported as first_ms);
  kernels_ms    the profiled split of one call (a run of its own);
  muls_per_s    the result's `multiplications` over the time of k_g1_table and
                k_g1_mul, and over the whole call;
  group_ops_per_s
                per multiplication c W doublings, W adds (every digit counted,
                though a zero digit, one in 2^c, adds nothing) and 2^(c-1) - 1
                table adds; per butterfly 2 adds; over the whole call;
  add_rate      svdw_commit_add_probe's register-resident mixed adds per second
                on the same device, the yardstick tools/commit_bench.py uses.

    python tools/g1_fft_bench.py [--out FILE] [--sizes 16,20] [--windows 0,3,4]
"""
import argparse
import ctypes as ct
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DISTINCT = 4096
A0, D = 0x1234567, (1 << 251) + 0x89abcdef
RHO = 0x123456789abcdef0fedcba9876543211


def median(xs):
    return sorted(xs)[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="16,20")
    ap.add_argument("--windows", default="0")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "g1_fft_bench.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        print("g1_fft_bench: no HIP device", file=sys.stderr)
        return 1
    import halo2_svd041_amd as hs
    from commit_cases import point_bytes, progression
    from halo2_svd041_amd import srs
    L = hs.zk.lib()
    dev = torch.device("cuda", 0)
    rec = {"reps": a.reps, "sizes": {}}
    s = srs.default_secret()

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    with hs.Context(device=0, precision_bits=32, lookup_bits=8) as ctx:
        distinct = torch.from_numpy(np.frombuffer(point_bytes(progression(DISTINCT, A0, D), "montgomery"),
                                                  dtype=np.uint8).reshape(DISTINCT, 64).copy()).to(dev)
        threads, adds = 1 << 19, 256
        sec = ct.c_double()
        rates = []
        for i in range(a.reps + 1):
            hs.zk.check(L.svdw_commit_add_probe(ctx._h, distinct.data_ptr(), DISTINCT, threads, adds, ct.byref(sec)))
            if i:
                rates.append(threads * adds / sec.value)
        rec["add_rate_per_s"] = round(median(rates))
        rec["add_rate_spread_per_s"] = round(max(rates) - min(rates))
        for k in [int(x) for x in a.sizes.split(",")]:
            n = 1 << k
            g, gl, _ = ctx.srs_setup(k, s)
            out = torch.empty((n, 64), dtype=torch.uint8, device=dev)
            per_window = {}
            for wb in [int(x) for x in a.windows.split(",")]:
                ctx.set_option("g1_window_bits", wb)
                res = {}

                def call():
                    res.update(ctx.g1_fft(g, k, inverse=True, out=out)[1])

                first = event_ms(call)
                ts = [event_ms(call) for _ in range(a.reps)]
                ctx.profile(True, "k_g1")
                call()
                kern = {p["name"].split("@")[0]: round(p["total_ms"], 3) for p in ctx.profile_collect()}
                ctx.profile(False)
                ctx.set_option("g1_window_bits", 0)
                c, W, muls = res["window_bits"], res["windows"], res["multiplications"]
                ops = muls * (c * W + W + (1 << (c - 1)) - 1) + 2 * (k - 1) * (n // 2) + n
                mul_ms = kern.get("k_g1_mul", 0.0) + kern.get("k_g1_table", 0.0)
                per_window[str(wb)] = {
                    "ms": round(median(ts), 3), "spread_ms": round(max(ts) - min(ts), 3), "first_ms": round(first, 3),
                    "window_bits": c, "windows": W, "multiplications": muls, "kernels_ms": kern,
                    "muls_per_s": round(muls / (mul_ms * 1e-3)) if mul_ms else None,
                    "muls_per_s_whole_call": round(muls / (median(ts) * 1e-3)),
                    "group_ops": ops, "group_ops_per_s_whole_call": round(ops / (median(ts) * 1e-3)),
                    "same": bool(torch.equal(out, gl)), "check": ctx.check_lagrange(g, out, k, RHO)}
            rec["sizes"][str(k)] = per_window
            del g, gl, out
            torch.cuda.empty_cache()
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
