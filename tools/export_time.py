#!/usr/bin/env python3
"""Read-out timing at a BASELINE size (default 1024^2, P=63, LB=19), one JSON line:

  export_mont     svdw_export_cells of all four streams in the Montgomery form,
                  next to a hipMemcpyDtoD of the same bytes in the same process
                  (the floor: one read and one write of every cell);
  assign_columns  svdw_assign_columns_form(MONTGOMERY) and svdw_assign_columns,
                  both phases at 2^k rows;
  dequantize_m    svdw_dequantize_mat of m into device memory;
  values_u        ZkMatrix.values() of u (host copy).

HIP events on torch's stream around the queued calls (the engine's streams are
ordered with it on both sides), a host clock around the calls that wait; one
warm-up, then the median of --reps. --root imports the package from another
checkout (the parent commit's build: it reports what that build has);
--baseline embeds such a run's line as "parent".

    python tools/export_time.py [--size 1024] [--k 24] [--root DIR] [--baseline FILE]
"""
import argparse
import ctypes as ct
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def median(xs):
    return sorted(xs)[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--precision", type=int, default=63)
    ap.add_argument("--lookup-bits", type=int, default=19)
    ap.add_argument("--k", type=int, default=24)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--baseline", default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    from bench import gen_input
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    if not torch.cuda.is_available():
        print("export_time: no HIP device", file=sys.stderr)
        return 1
    import halo2_svd041_amd as hs
    from halo2_svd041_amd import _lib
    from halo2_svd041_amd._lib import Mat
    from halo2_svd041_amd.zk import _after_torch, _before_torch
    L = _lib.lib()
    new = hasattr(L, "svdw_export_cells")
    hip = ct.CDLL("libamdhip64.so")
    hip.hipMemcpyDtoDAsync.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_size_t, ct.c_void_p]
    dev = torch.device("cuda", 0)
    N = M = a.size
    P = a.precision
    m, u, d, v = gen_input(N, M, 0)
    rec = {"N": N, "M": M, "P": P, "LB": a.lookup_bits, "k": a.k, "reps": a.reps,
           "build": "this" if new else "parent"}

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

    def wall(fn, reps=a.reps):
        ts = []
        for i in range(reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i:
                ts.append((time.perf_counter() - t0) * 1e3)
        return median(ts)

    with hs.Context(device=0, precision_bits=P, lookup_bits=a.lookup_bits) as ctx:
        cnt = hs.svd_witness(ctx, m, u, v, d, 0x1234567)
        ctx.sync()
        streams = [(ph, lk, (ctx.lookup_len if lk else ctx.advice_len)(ph)) for ph in (0, 1) for lk in (0, 1)]
        cells = sum(n for _, _, n in streams)
        rec["cells"] = cells
        rec["GB"] = round(cells * 32 / 1e9, 3)
        stream = torch.cuda.current_stream(dev).cuda_stream
        if new:
            dst = torch.empty((max(n for _, _, n in streams), 32), dtype=torch.uint8, device=dev)

            def export(form):
                _after_torch(ctx)
                for ph, lk, n in streams:
                    hs.zk.check(L.svdw_export_cells(ctx.handle, ph, lk, 0, n, form, dst.data_ptr()))
                _before_torch(ctx)

            def d2d():
                for ph, lk, n in streams:
                    src = (ctx.lookup_device_ptr if lk else ctx.advice_device_ptr)(ph)
                    if n and hip.hipMemcpyDtoDAsync(dst.data_ptr(), src, n * 32, stream) != 0:
                        raise RuntimeError("hipMemcpyDtoDAsync failed")

            t_m, t_c, t_f = events(lambda: export(1)), events(lambda: export(0)), events(d2d)
            rec["export_mont_ms"] = round(t_m, 3)
            rec["export_canonical_ms"] = round(t_c, 3)
            rec["d2d_ms"] = round(t_f, 3)
            rec["export_mont_GBps"] = round(cells * 64 / t_m / 1e6, 1)      # read + write
            rec["d2d_GBps"] = round(cells * 64 / t_f / 1e6, 1)
            rec["export_mont_over_d2d"] = round(t_m / t_f, 2)
            del dst
            zm = hs.ZkMatrix(ctx, Mat(0, N, M, 0, M, 1))
            out = torch.empty((N, M), dtype=torch.float64, device=dev)

            def deq():
                _after_torch(ctx)
                hs.zk.check(L.svdw_dequantize_mat(ctx.handle, ct.byref(zm.mat), out.data_ptr(), 1))
                _before_torch(ctx)

            rec["dequantize_m_ms"] = round(events(deq, 20), 4)
            rec["dequantize_m_max_err"] = float((out.cpu() - torch.as_tensor(m)).abs().max())
        # physical columns (the calls wait: host clock), tensors allocated once
        pp = ctx.physical_layout(a.k, 20)
        rows = 1 << a.k
        bufs = []
        for ph in (0, 1):
            nc, nl = pp["columns_used"][ph], pp["num_lookup_advice"][ph]
            bufs.append((torch.empty((nc, rows, 32), dtype=torch.uint8, device=dev),
                         torch.empty((nc, rows), dtype=torch.uint8, device=dev),
                         torch.empty((max(nl, 1), rows, 32), dtype=torch.uint8, device=dev), nl))
        rec["columns"] = [pp["columns_used"][0] + pp["num_lookup_advice"][0],
                          pp["columns_used"][1] + pp["num_lookup_advice"][1]]

        def assign(form):
            for ph, (adv, sel, lk, nl) in enumerate(bufs):
                args = (adv.data_ptr(), sel.data_ptr(), lk.data_ptr() if nl else None)
                if form is None:
                    hs.zk.check(L.svdw_assign_columns(ctx.handle, ph, *args))
                else:
                    hs.zk.check(L.svdw_assign_columns_form(ctx.handle, ph, form, *args))

        rec["assign_columns_ms"] = round(wall(lambda: assign(None), 3), 2)
        if new:
            rec["assign_columns_mont_ms"] = round(wall(lambda: assign(1), 3), 2)
        del bufs
        # u was loaded right after m (svd_witness: ZkMatrix::new of m, u, v, then d)
        zu = hs.ZkMatrix(ctx, Mat(0, N, N, N * M, N, 1))
        rec["values_u_ms"] = round(wall(zu.values, 2), 2)
        rec["advice0"] = cnt["advice0"]
    if a.baseline:
        with open(a.baseline) as fh:
            rec["parent"] = json.loads(fh.read().strip().splitlines()[-1])
    print(json.dumps(rec), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
