#!/usr/bin/env python3
"""Lookup grand-product timing at a BASELINE size (default 1024^2, P=63, LB=19,
k=24, phase 0, all lookup columns read from the stream), one JSON line, also
written to profiles/lookup_product_time.json:

  product          svdw_lookup_product in the canonical and the Montgomery form
                   (A', S' from svdw_lookup_permute in the same form);
  check            svdw_check_lookup_product on both results;
  permute          svdw_lookup_permute, same process, for the ratio;
  d2d              a hipMemcpyDtoD of the bytes the product has to move (three
                   columns read, one written per column: 4 x ncols x 2^k x 32 B,
                   i.e. a copy of half that many bytes), same process;
  kernels          the per-kernel split of one profiled product and check in
                   each form.

HIP events on torch's stream around the calls (the engine's streams are ordered
with it on both sides; the calls also wait on the host), one warm-up, then the
median of --reps.

    python tools/lookup_product_time.py [--size 1024] [--k 24] [--out FILE]
"""
import argparse
import ctypes as ct
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P_MOD = 21888242871839275222246405745257275088548364400416034343698204186575808495617
BETA, GAMMA = 0x1234567890abcdef1234567890abcdef, P_MOD - (1 << 200)


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lookup_product_time.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    from bench import gen_input
    import torch
    if not torch.cuda.is_available():
        print("lookup_product_time: no HIP device", file=sys.stderr)
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
        col_bytes = ncols * rows * 32
        rec.update(lookup_cells=ctx.lookup_len(0), columns=ncols, ideal_GB=round(4 * col_bytes / 1e9, 3))
        out = (torch.empty((ncols, rows, 32), dtype=torch.uint8, device=dev),
               torch.empty((ncols, rows, 32), dtype=torch.uint8, device=dev))
        z = torch.empty((ncols, rows, 32), dtype=torch.uint8, device=dev)

        for form in ("canonical", "montgomery"):
            rec[f"permute_{form}_ms"] = round(events(lambda: ctx.lookup_permute(0, un, form, out=out)), 3)
            rec[f"product_{form}_ms"] = round(
                events(lambda: ctx.lookup_product(0, out[0], out[1], BETA, GAMMA, un, form, out=z)), 3)
            r = ctx.lookup_product(0, out[0], out[1], BETA, GAMMA, un, form, out=z)[1]
            rec[f"product_{form}_result"] = r
            rec[f"check_{form}_ms"] = round(
                events(lambda: ctx.check_lookup_product(0, out[0], out[1], z, BETA, GAMMA, un, form)), 3)
            chk = ctx.check_lookup_product(0, out[0], out[1], z, BETA, GAMMA, un, form)
            rec[f"check_{form}_failures"] = sum(x for n, x in chk.items() if n.endswith("failures"))
            ctx.profile(True, "k_lp")
            ctx.lookup_product(0, out[0], out[1], BETA, GAMMA, un, form, out=z)
            ctx.check_lookup_product(0, out[0], out[1], z, BETA, GAMMA, un, form)
            rec[f"kernels_{form}_ms"] = {s["name"]: round(s["total_ms"], 3) for s in ctx.profile_collect()}
            ctx.profile(False)

        # the floor: a device copy that reads 2 and writes 2 column sets
        half = col_bytes * 2
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
            rec[f"product_{form}_over_d2d"] = round(rec[f"product_{form}_ms"] / rec["d2d_ms"], 2)
            rec[f"product_{form}_over_permute"] = round(rec[f"product_{form}_ms"] / rec[f"permute_{form}_ms"], 2)
        del src, dst
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
