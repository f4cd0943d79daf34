#!/usr/bin/env python3
"""Timing of the quotient polynomial (svdw_quotient) on the extended domain, one
JSON line, also written to profiles/quotient_time.json.

Shapes: k = 20 and 22 with extended_k = k + 2 (E = 4), chunk_len 2, the column
counts of the 1024^2 P = 63 LB = 19 witness's physical layout at that k
(svdw_physical_layout, minimum_rows 20; both phases' advice columns gated, the
lookup columns of phase 0, the permutation over all of them):

    k = 20   230 gates, 279 permutation columns in 140 sets, 49 lookups
    k = 22    58 gates,  71 permutation columns in  36 sets, 13 lookups

Columns of random cells below p, each family in its own tensor; as in a prover,
the permutation's columns are the advice and lookup columns themselves and the
lookups share one table column. A size runs only if its buffers fit the
device's free memory. At each size and in both forms:

  call_ms      the whole svdw_quotient call between two HIP events on torch's
               stream (one warm-up, then the median of --reps; spread = max - min);
  kernel_ms    k_quotient alone, from the engine's profile of one more call;
  muls_per_row the kernel's own count (quotient.hpp's table);
  ms_per_mul   kernel ms per (multiplication x 2^26 rows);
  yardstick    the same figure of k_lp_write from --lookup-json
               (tools/lookup_product_time.py's record of the same session), whose
               kernel runs the same mont_mul: the yardstick, not the code under
               test; ratio = ms_per_mul / yardstick.

    python tools/quotient_time.py [--out FILE] [--lookup-json FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P_MOD = 21888242871839275222246405745257275088548364400416034343698204186575808495617
SHIFT = 0x2b3f9c1d5e7a8046f1e2d3c4b5a69788796a5b4c3d2e1f0a1b2c3d4e5f607182 % P_MOD
BETA, GAMMA, Y = 0x1234567890abcdef1234567890abcdef, P_MOD - (1 << 200), P_MOD - 0x0fedcba987654321
EXT, CHUNK, UNUSABLE = 2, 2, 6
# k -> (gated advice columns, lookup columns) of the 1024^2 P = 63 witness
SHAPES = {20: (230, 49), 22: (58, 13)}
LOOKUP_MULS = {"k_lp_write": 10.5}                           # per row (lookup_product.hip's header)


def median(xs):
    return sorted(xs)[len(xs) // 2]


def muls_per_row(ng, np_, nsets, nl, canonical):
    """quotient.hpp's quotient_muls."""
    m = ng * (5 if canonical else 3) + nl * (22 if canonical else 16) + 1
    if np_:
        m += 2 + (6 if canonical else 5) + 2 * (nsets - 1) + 2 * nsets + np_ * (6 if canonical else 4)
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quotient_time.json"))
    ap.add_argument("--lookup-json", default=os.path.join(ROOT, "profiles", "lookup_product_time.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        print("quotient_time: no HIP device", file=sys.stderr)
        return 1
    import halo2_svd041_amd as hs
    dev = torch.device("cuda", 0)
    free = torch.cuda.mem_get_info(dev)[0]
    rec = {"reps": a.reps, "chunk_len": CHUNK, "unusable_rows": UNUSABLE, "free_GB": round(free / 1e9, 1),
           "sizes": {}}
    yard = {}
    if a.lookup_json and os.path.exists(a.lookup_json):
        lk = json.loads(open(a.lookup_json).read().splitlines()[0])
        per = lk["columns"] * ((1 << lk["k"]) - lk["unusable_rows"]) / 2 ** 26
        for form in ("canonical", "montgomery"):
            kern = {n.split("@")[0]: ms for n, ms in lk.get(f"kernels_{form}_ms", {}).items()}
            if "k_lp_write" in kern:
                yard[form] = round(kern["k_lp_write"] / (LOOKUP_MULS["k_lp_write"] * per), 3)
        rec["yardstick_source"] = os.path.basename(a.lookup_json)
        rec["yardstick_ms_per_mul"] = yard

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
        for k, (ng, nl) in SHAPES.items():
            ke, rows = k + EXT, 1 << (k + EXT)
            np_ = ng + nl
            nsets = -(-np_ // CHUNK)
            # advice, selectors, sigma, Z of the sets; A, A', S', Z of the lookups and the table; h; the l columns
            # and the transform's buffer that builds them
            ncols = 2 * ng + np_ + nsets + 4 * nl + 1 + 1 + 6
            need = ncols * rows * 32 + (2 << 30)
            r = {"gates": ng, "permutation_columns": np_, "sets": nsets, "lookups": nl, "extended_k": ke,
                 "need_GB": round(need / 1e9, 1)}
            if need > free:
                r["skipped"] = "does not fit the free memory"
                rec["sizes"][str(k)] = r
                continue
            g = torch.Generator(device=dev)
            g.manual_seed(k)

            def cells(n):
                t = torch.randint(0, 256, (n, rows, 32), dtype=torch.uint8, device=dev, generator=g)
                t[:, :, 31] &= 0x1F                          # 253 random bits: below p in either form
                return t

            advice, lookup_input = cells(ng), cells(nl)
            table = cells(1)
            fams = dict(advice=advice, selectors=cells(ng), perm_columns=[advice, lookup_input], sigma=cells(np_),
                        perm_z=cells(nsets), lookup_input=lookup_input, lookup_table=[table] * nl,
                        permuted_input=cells(nl), permuted_table=cells(nl), lookup_z=cells(nl))
            out = torch.empty((1, rows, 32), dtype=torch.uint8, device=dev)
            per = rows / 2 ** 26
            for form in ("canonical", "montgomery"):
                call = lambda: ctx.quotient(k, ke, SHIFT, BETA, GAMMA, Y, chunk_len=CHUNK,   # noqa: E731
                                            unusable_rows=UNUSABLE, form=form, out=out, **fams)
                r[f"call_{form}_ms"], r[f"call_{form}_spread_ms"] = events(call, a.reps)
                ctx.profile(True, "k_quotient")
                res = call()[1]
                kern = {s["name"].split("@")[0]: round(s["total_ms"], 3) for s in ctx.profile_collect()}
                ctx.profile(False)
                muls = muls_per_row(ng, np_, nsets, nl, form == "canonical")
                r[f"kernel_{form}_ms"] = kern.get("k_quotient")
                r[f"muls_per_row_{form}"] = muls
                r[f"ms_per_mul_{form}"] = round(kern["k_quotient"] / (muls * per), 3)
                if form in yard:
                    r[f"ratio_to_yardstick_{form}"] = round(r[f"ms_per_mul_{form}"] / yard[form], 3)
                r["result"] = res
            del fams, advice, lookup_input, table, out
            torch.cuda.empty_cache()
            rec["sizes"][str(k)] = r
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
