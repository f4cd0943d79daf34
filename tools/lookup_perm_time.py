#!/usr/bin/env python3
"""Lookup-argument timing at a BASELINE size (default 1024^2, P=63, LB=19, k=24,
phase 0, all lookup columns read from the stream), one JSON line, also written
to profiles/lookup_perm_time.json:

  multiplicities   svdw_lookup_multiplicities;
  permute          svdw_lookup_permute in the canonical and the Montgomery form;
  check            svdw_check_lookup_argument on both results;
  d2d              a hipMemcpyDtoD that moves the bytes a perfect permute moves
                   (each column read once, two columns written: 3 x ncols x 2^k
                   x 32 B, i.e. a copy of half that many bytes), same process;
  kernels          the per-kernel split of one profiled permute and check;
  skew             per column, the share of the usable rows equal to 0, to
                   2^LB - 1, and in the fullest other bin.

HIP events on torch's stream around the calls (the engine's streams are ordered
with it on both sides; the calls also wait on the host), one warm-up, then the
median of --reps.

    python tools/lookup_perm_time.py [--size 1024] [--k 24] [--out FILE]
"""
import argparse
import ctypes as ct
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def median(xs):
    return sorted(xs)[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--precision", type=int, default=63)
    ap.add_argument("--lookup-bits", type=int, default=19)
    ap.add_argument("--k", type=int, default=24)
    ap.add_argument("--unusable-rows", type=int, default=6)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lookup_perm_time.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    from bench import gen_input
    import torch
    if not torch.cuda.is_available():
        print("lookup_perm_time: no HIP device", file=sys.stderr)
        return 1
    import halo2_svd041_amd as hs
    hip = ct.CDLL("libamdhip64.so")
    hip.hipMemcpyDtoDAsync.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_size_t, ct.c_void_p]
    dev = torch.device("cuda", 0)
    N = M = a.size
    P, LB, k, un = a.precision, a.lookup_bits, a.k, a.unusable_rows
    m, u, d, v = gen_input(N, M, 0)
    rec = {"N": N, "M": M, "P": P, "LB": LB, "k": k, "unusable_rows": un, "reps": a.reps}

    def events(fn, reps=a.reps):
        """median ms of fn() between two events on torch's stream (one warm-up)"""
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
        return median(ts)

    with hs.Context(device=0, precision_bits=P, lookup_bits=LB) as ctx:
        hs.svd_witness(ctx, m, u, v, d, 0x1234567)
        ctx.sync()
        pp = ctx.physical_layout(k, 20)
        ncols, rows = pp["num_lookup_advice"][0], 1 << k
        usable = rows - un
        col_bytes = ncols * rows * 32
        rec.update(lookup_cells=ctx.lookup_len(0), columns=ncols, ideal_GB=round(3 * col_bytes / 1e9, 3))
        out = (torch.empty((ncols, rows, 32), dtype=torch.uint8, device=dev),
               torch.empty((ncols, rows, 32), dtype=torch.uint8, device=dev))

        mult = ctx.lookup_multiplicities(0, un)
        top = (1 << LB) - 1
        rest = mult[:, 1:top].max(dim=1).values
        rec["skew"] = [{"zero": round(int(mult[c, 0]) / usable, 4), "top": round(int(mult[c, top]) / usable, 4),
                        "max_other_bin": round(int(rest[c]) / usable, 6),
                        "distinct": int((mult[c] > 0).sum())} for c in range(ncols)]
        del mult, rest
        rec["multiplicities_ms"] = round(events(lambda: ctx.lookup_multiplicities(0, un)), 3)
        for form in ("canonical", "montgomery"):
            rec[f"permute_{form}_ms"] = round(events(lambda: ctx.lookup_permute(0, un, form, out=out)), 3)
            r = ctx.lookup_permute(0, un, form, out=out)[2]
            rec[f"check_{form}_ms"] = round(events(lambda: ctx.check_lookup_argument(0, out[0], out[1], un, form)), 3)
            chk = ctx.check_lookup_argument(0, out[0], out[1], un, form)
            rec[f"check_{form}_failures"] = sum(x for n, x in chk.items() if n.endswith("failures"))
        rec["out_of_table"], rec["distinct"] = r["out_of_table"], r["distinct"]

        # the floor: a device copy that reads 1.5 and writes 1.5 column sets
        half = col_bytes * 3 // 2
        src = torch.empty(half, dtype=torch.uint8, device=dev)
        dst = torch.empty(half, dtype=torch.uint8, device=dev)
        src.zero_()
        stream = torch.cuda.current_stream(dev).cuda_stream

        def d2d():
            if hip.hipMemcpyDtoDAsync(dst.data_ptr(), src.data_ptr(), half, stream) != 0:
                raise RuntimeError("hipMemcpyDtoDAsync failed")

        rec["d2d_ms"] = round(events(d2d), 3)
        rec["d2d_GBps"] = round(2 * half / rec["d2d_ms"] / 1e6, 1)
        for form in ("canonical", "montgomery"):
            rec[f"permute_{form}_over_d2d"] = round(rec[f"permute_{form}_ms"] / rec["d2d_ms"], 2)
        del src, dst

        ctx.profile(True, "k_lk")
        ctx.lookup_permute(0, un, "montgomery", out=out)
        ctx.check_lookup_argument(0, out[0], out[1], un, "montgomery")
        rec["kernels_montgomery_ms"] = {s["name"]: round(s["total_ms"], 3) for s in ctx.profile_collect()}
        ctx.profile(False)
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
