#!/usr/bin/env python3
"""Timing of the SHPLONK opening calls (svdw_open_quotient, svdw_open_linearise)
on the device, one JSON line, also written to profiles/open_bench.json.

At k = 16 and k = 20, the five rotation sets of the circuit shape ({0,1,2,3},
{0}, {0,1,usable}, {0,1}, {0,-1} at a point x) over 17 columns of random cells:

  open_quotient, open_linearise   each whole call;
  commit_2        svdw_commit of the two outputs h1 and h2 in one call (what
                  follows the opening in a proof);
  eval            svdw_eval_polynomial of the same 17 columns at the |T| points;
  of_commit, of_eval   both opening calls over those;
  bytes_bound_ms  what the calls must move at the memset rate DESIGN.md records
                  (6.5 TB/s): (ncols + passes) 2^k 32 B read plus the writes of
                  the passes, and its share of the measured time;
  kernels         the profiled split of one call of each.

HIP events on torch's stream around the calls, one warm-up, then the median of
--reps and the spread, all in one session and process.

    python tools/open_bench.py [--out FILE] [--sizes 16,20]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DISTINCT = 4096
A0, D = 0x1234567, (1 << 251) + 0x89abcdef
NCOLS = 17
MEMSET_BPS = 6.5e12


def median(xs):
    return sorted(xs)[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="16,20")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "open_bench.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        print("open_bench: no HIP device", file=sys.stderr)
        return 1
    import halo2_svd041_amd as hs
    from commit_cases import point_bytes, progression
    from open_cases import U, V, X_POINT, Y, circuit_sets
    dev = torch.device("cuda", 0)
    distinct = torch.from_numpy(np.frombuffer(point_bytes(progression(DISTINCT, A0, D), "montgomery"),
                                              dtype=np.uint8).reshape(DISTINCT, 64).copy()).to(dev)
    rec = {"reps": a.reps, "columns": NCOLS, "memset_bytes_per_s": MEMSET_BPS, "sizes": {}}

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
        for k in [int(s) for s in a.sizes.split(",")]:
            rows = 1 << k
            _, sets = circuit_sets(k, 6, X_POINT)
            set_of = [0] * 4 + [1] * 7 + [2] * 2 + [3] * 2 + [4] * 2      # 17 columns over the five sets
            assert len(set_of) == NCOLS
            points = sorted({p for s in sets for p in s})
            bases = distinct.repeat(max(rows // DISTINCT, 1), 1)[:rows].contiguous()
            g = torch.Generator(device=dev)
            g.manual_seed(k)
            cols = torch.randint(0, 256, (NCOLS, rows, 32), dtype=torch.uint8, device=dev, generator=g)
            cols[:, :, 31] &= 0x1F                              # 253 random bits: below p
            h1 = torch.empty((1, rows, 32), dtype=torch.uint8, device=dev)
            h2 = torch.empty((1, rows, 32), dtype=torch.uint8, device=dev)
            pts2 = torch.empty((2, 64), dtype=torch.uint8, device=dev)
            res = ctx.open_quotient(cols, set_of, sets, Y, V, k, out=h1)[1]
            passes = res["passes"]
            r = {"sets": res["sets"], "points": res["points"], "passes": passes}
            calls = {
                "open_quotient": lambda: ctx.open_quotient(cols, set_of, sets, Y, V, k, out=h1),
                "open_linearise": lambda: ctx.open_linearise(cols, set_of, sets, Y, V, U, h1, k, out=h2),
                "commit_2": lambda: ctx.commit([h1, h2], bases, k, out=pts2),
                "eval": lambda: ctx.eval_polynomial(cols, k, points),
            }
            for name, fn in calls.items():
                ms, spread = events(fn, a.reps)
                r[name] = {"ms": ms, "spread_ms": spread}
            both = r["open_quotient"]["ms"] + r["open_linearise"]["ms"]
            r["opening_ms"] = round(both, 3)
            r["of_commit"] = round(both / r["commit_2"]["ms"], 3)
            r["of_eval"] = round(both / r["eval"]["ms"], 3)
            # the quotient reads every column once and each pass's input, and writes each pass's
            # output and the folds; the linearisation reads the columns and h1 and divides once
            moved = {"open_quotient": (NCOLS + passes) * rows * 32 + (passes + res["sets"]) * rows * 32,
                     "open_linearise": (NCOLS + 1 + 1) * rows * 32 + 2 * rows * 32}
            for name, b in moved.items():
                bound = b / MEMSET_BPS * 1e3
                r[name]["bytes"] = b
                r[name]["bytes_bound_ms"] = round(bound, 4)
                r[name]["bytes_bound_share"] = round(bound / r[name]["ms"], 3)
            ctx.profile(True, "k_open")
            calls["open_quotient"]()
            r["kernels_open_quotient_ms"] = {s["name"].split("@")[0]: round(s["total_ms"], 3)
                                             for s in ctx.profile_collect()}
            calls["open_linearise"]()
            r["kernels_open_linearise_ms"] = {s["name"].split("@")[0]: round(s["total_ms"], 3)
                                              for s in ctx.profile_collect()}
            ctx.profile(False)
            if k <= 16:
                chk = ctx.check_open(cols, set_of, sets, Y, V, U, h1, h2, X_POINT + 1, k)
                r["check"] = {f: chk[f] for f in ("identity1_failures", "identity2_failures", "h1_top_nonzero",
                                                  "h2_top_nonzero")}
            rec["sizes"][str(k)] = r
            del cols, bases, h1, h2
            torch.cuda.empty_cache()
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
