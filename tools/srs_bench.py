#!/usr/bin/env python3
"""Timing of the SRS setup (svdw_srs_setup) on the device, one JSON line, also
written to profiles/srs_bench.json.

For each k of --sizes, with halo2-base's default secret and both arrays:

  ms            one svdw_srs_setup call (the table is cached: the first call,
                which builds it, is the warm-up and is reported as first_ms);
                HIP events on torch's stream, median of --reps and the spread;
  g_only_ms, lagrange_only_ms
                the same call for one array alone (the other left out): their
                sum against ms is what multiplying both columns in one launch
                is worth;
  kernels_ms    the profiled split of one call (a run of its own);
  adds_per_s    2 x 2^k x W mixed adds over the time of k_fb_mul: every digit
                counted, though a zero digit (one in 2^c) adds nothing, and the
                kernel's share of inversion and conversion left in;
  add_rate      svdw_commit_add_probe's register-resident mixed adds per second
                on the same device, the yardstick tools/commit_bench.py uses.

    python tools/srs_bench.py [--out FILE] [--sizes 20,22]
"""
import argparse
import ctypes as ct
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DISTINCT = 4096
A0, D = 0x1234567, (1 << 251) + 0x89abcdef


def median(xs):
    return sorted(xs)[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", default="20,22")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "srs_bench.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        print("srs_bench: no HIP device", file=sys.stderr)
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
            g = torch.empty((n, 64), dtype=torch.uint8, device=dev)
            gl = torch.empty((n, 64), dtype=torch.uint8, device=dev)
            res = {}

            def call():
                res.update(ctx.srs_setup(k, s, g=g, g_lagrange=gl)[2])

            first = event_ms(call)
            ts = [event_ms(call) for _ in range(a.reps)]
            alone = {}                                          # either array alone: two launches of half the outputs
            for tag, kw in (("g_only_ms", {"g": g, "g_lagrange": None}),
                            ("lagrange_only_ms", {"g": None, "g_lagrange": gl})):
                one = [event_ms(lambda: ctx.srs_setup(k, s, **kw)) for _ in range(a.reps + 1)][1:]
                alone[tag] = round(median(one), 3)
            ctx.profile(True, "k_")
            call()
            kern = {p["name"].split("@")[0]: round(p["total_ms"], 3) for p in ctx.profile_collect()}
            ctx.profile(False)
            chk = ctx.check_srs(g, gl, k, s, 0x123456789abcdef0fedcba9876543211) if k <= 20 else None
            fb = kern.get("k_fb_mul", 0.0)
            rec["sizes"][str(k)] = {
                "ms": round(median(ts), 3), "spread_ms": round(max(ts) - min(ts), 3), "first_ms": round(first, 3),
                **alone,
                "window_bits": res["window_bits"], "windows": res["windows"], "chunks": res["chunks"],
                "kernels_ms": kern, "mixed_adds": 2 * n * res["windows"],
                "adds_per_s": round(2 * n * res["windows"] / (fb * 1e-3)) if fb else None,
                "adds_per_s_whole_call": round(2 * n * res["windows"] / (median(ts) * 1e-3)), "check": chk}
            del g, gl
            torch.cuda.empty_cache()
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
