#!/usr/bin/env python3
"""Timing of the commitments (svdw_commit) on the device, one JSON line, also
written to profiles/commit_bench.json.

At k = 16 and k = 20, for 1 and 8 columns:

  full_width    253 random bits per cell;
  witness       the first advice columns of a 128 x 128 SVD witness laid out at
                that k (range-checked cells, long zero runs);
  windows       the full-width case at window_bits c - 1, c, c + 1 around
                svdw_commit_plan's c (option "commit_window_bits"), the figures
                the plan's table is corrected by;
  kernels       the profiled split of one full-width call;
  add_rate      a register-resident loop of mixed adds alone
                (svdw_commit_add_probe), adds per second;
  bound_share   (sorted adds + reduction adds) / add_rate over the measured time,
                the adds counted from the result: columns x windows x (rows +
                2 x 2^(window_bits - 1)). Reduction adds are full adds (14
                products against the probe's 10), so the bound flatters them.

The bases are 4096 distinct points [a0 + i d] G tiled to 2^k (building 2^20
distinct ones on the host would take a minute); repeated bases are ordinary
inputs. HIP events on torch's stream around the calls, one warm-up, then the
median of --reps and the spread.

    python tools/commit_bench.py [--out FILE] [--sizes 16,20]
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="16,20")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "commit_bench.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        print("commit_bench: no HIP device", file=sys.stderr)
        return 1
    import halo2_svd041_amd as hs
    from commit_cases import point_bytes, progression
    L = hs.zk.lib()
    dev = torch.device("cuda", 0)
    distinct = torch.from_numpy(np.frombuffer(point_bytes(progression(DISTINCT, A0, D), "montgomery"),
                                              dtype=np.uint8).reshape(DISTINCT, 64).copy()).to(dev)
    rec = {"reps": a.reps, "distinct_bases": DISTINCT, "sizes": {}}

    def events(fn, reps):
        ts = []
        for i in range(reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if i:
                ts.append(e0.elapsed_time(e1))
        return round(median(ts), 3), round(max(ts) - min(ts), 3)

    with hs.Context(device=0, precision_bits=32, lookup_bits=8) as ctx:
        # the add rate: 2^19 threads, 256 adds each, after one warm-up launch
        threads, adds = 1 << 19, 256
        sec = ct.c_double()
        rates = []
        for i in range(a.reps + 1):
            hs.zk.check(L.svdw_commit_add_probe(ctx._h, distinct.data_ptr(), DISTINCT, threads, adds, ct.byref(sec)))
            if i:
                rates.append(threads * adds / sec.value)
        rate = median(rates)
        rec["add_rate_per_s"] = round(rate)
        rec["add_rate_spread_per_s"] = round(max(rates) - min(rates))

        rs = np.random.RandomState(7)
        m = rs.uniform(-10, 10, size=(128, 128))
        m = m / np.linalg.norm(m, ord=2) * rs.uniform(1, 100)
        u, d, v = np.linalg.svd(m)
        hs.svd_witness(ctx, m, u, v, d, 0x1d5e7a8046f1e2d3c4b5a69788796a5b4c3d2e1f0a1b2c3d4e5f607182)

        for k in [int(s) for s in a.sizes.split(",")]:
            rows = 1 << k
            bases = distinct.repeat(max(rows // DISTINCT, 1), 1)[:rows].contiguous()
            g = torch.Generator(device=dev)
            g.manual_seed(k)
            full = torch.randint(0, 256, (8, rows, 32), dtype=torch.uint8, device=dev, generator=g)
            full[:, :, 31] &= 0x1F                              # 253 random bits: below r
            r = {}
            plan_c, _ = hs.commit_plan(k)

            def bound_ms(res):
                adds_ = res["columns"] * res["windows"] * (res["rows"] + 2 * (1 << (res["window_bits"] - 1)))
                return adds_ / rate * 1e3

            def timed(tag, cols):
                out = torch.empty((cols.shape[0], 64), dtype=torch.uint8, device=dev)
                res = ctx.commit(cols, bases, k, out=out)[1]
                ms, spread = events(lambda: ctx.commit(cols, bases, k, out=out), a.reps)
                r[tag] = {"ms": ms, "spread_ms": spread, "window_bits": res["window_bits"], "windows": res["windows"],
                          "zero_scalars": res["zero_scalars"], "bound_ms": round(bound_ms(res), 3),
                          "bound_share": round(bound_ms(res) / ms, 3)}
                return out

            for n in (1, 8):
                timed(f"full_width_{n}", full[:n])
            try:
                ctx.physical_layout(k, 20)
                adv = ctx.assign_columns(0)[0]
                for n in (1, 8):
                    if adv.shape[0] >= n:
                        timed(f"witness_{n}", adv[:n].contiguous())
                r["witness_columns"] = int(adv.shape[0])
                del adv
            except hs.SvdwError as e:                           # the witness does not fit this k
                r["witness_error"] = str(e)
            for c in sorted({max(2, plan_c - 1), plan_c, min(16, plan_c + 1)}):
                ctx.set_option("commit_window_bits", c)
                for n in (1, 8):
                    timed(f"window_{c}_cols_{n}", full[:n])
            ctx.set_option("commit_window_bits", 0)
            ctx.profile(True, "k_commit")
            out = ctx.commit(full, bases, k)[0]
            r["kernels_full_width_8_ms"] = {s["name"].split("@")[0]: round(s["total_ms"], 3)
                                            for s in ctx.profile_collect()}
            ctx.profile(False)
            if k <= 16:
                r["check"] = ctx.check_commit(full, bases, out, k)
            rec["sizes"][str(k)] = r
            del full, bases
            torch.cuda.empty_cache()
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
