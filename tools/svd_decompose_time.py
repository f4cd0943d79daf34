#!/usr/bin/env python3
"""Timing of the decomposition (svdw_svd_decompose) on recipe matrices, one
JSON line, also written to profiles/svd_decompose_time.json.

Shapes 256^2, 512^2, 1024^2 and 2048 x 1024, panels b = 4 and 8, device
tensors in and out. Per (shape, b):

  ms, spread_ms      HIP events on torch's stream around the call, one warm-up,
                     then the median of --reps and max - min;
  sweeps, rotations, converged, off   the call's info;
  kernels_ms         the per-kernel split of one profiled call, and launches;
  R1, R2, R3, d_error  max|u d - m v^T|, max|u u^T - I|, max|v v^T - I| and
                     max|d - d_numpy| / d_0 in numpy f64 (--residuals-upto rows).

Per shape, for scale: np.linalg.svd on this box's CPU with the thread count it
ran with, torch.linalg.svd on the device if it runs, and the witness step
(svd_witness at P = 63 from the device factors, host clock around call and
sync, median of --witness-reps).

  skipped_share      info.skipped_pairs / info.pairs: the share of panel pairs
                     whose solve made no rotation, so that their apply blocks
                     return before touching the columns. No launch is left
                     out: the solve runs inside k_svd_rotate.

    python tools/svd_decompose_time.py [--out FILE] [--shapes 256x256,1024x1024]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = "256x256,512x512,1024x1024,2048x1024"


def median(xs):
    return sorted(xs)[len(xs) // 2]


def recipe(N, M, seed):
    """input-creator.py:23-29 with a seeded RandomState."""
    import numpy as np
    rs = np.random.RandomState(seed)
    m = rs.uniform(-10, 10, size=(N, M))
    return m / np.linalg.norm(m, ord=2) * rs.uniform(1, 100)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--witness-reps", type=int, default=3)
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--panels", default="4,8")
    ap.add_argument("--residuals-upto", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "svd_decompose_time.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        print("svd_decompose_time: no HIP device", file=sys.stderr)
        return 1
    import halo2_svd041_amd as hs
    dev = torch.device("cuda", 0)
    rec = {"reps": a.reps, "witness_reps": a.witness_reps,
           "cpu_threads": int(os.environ.get("OMP_NUM_THREADS", "0")) or torch.get_num_threads(), "shapes": {}}

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

    with hs.Context(device=0, precision_bits=63, lookup_bits=19) as ctx:
        for shape in a.shapes.split(","):
            N, M = (int(x) for x in shape.split("x"))
            m = recipe(N, M, N + M)
            tm = torch.from_numpy(m).to(dev)
            r = {}
            t0 = time.perf_counter()
            d_ref = np.linalg.svd(m)[1]
            r["numpy_svd_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            try:
                r["torch_svd_ms"], r["torch_svd_spread_ms"] = events(lambda: torch.linalg.svd(tm), 2)
            except Exception as e:   # noqa: BLE001
                r["torch_svd_error"] = str(e)[:200]
            last = None
            for b in (int(x) for x in a.panels.split(",")):
                out = {}

                def call():
                    out["r"] = hs.svd_decompose(ctx, tm, device=True, panel=b)
                q = {}
                q["ms"], q["spread_ms"] = events(call, a.reps)
                tu, td, tv, info = out["r"]
                q.update(info)
                q["skipped_share"] = round(info["skipped_pairs"] / max(info["pairs"], 1), 4)
                ctx.profile(True, "k_svd")
                call()
                stats = ctx.profile_collect()
                ctx.profile(False)
                q["kernels_ms"] = {s["name"].split("@")[0]: round(s["total_ms"], 3) for s in stats}
                q["launches"] = {s["name"].split("@")[0]: s["launches"] for s in stats}
                if max(N, M) <= a.residuals_upto:
                    u, d, v = tu.cpu().numpy(), td.cpu().numpy(), tv.cpu().numpy()
                    k = min(N, M)
                    ud = np.zeros((N, M))
                    ud[:, :k] = u[:, :k] * d[None, :k]
                    q["R1"] = float(np.max(np.abs(ud - m @ v.T)))
                    q["R2"] = float(np.max(np.abs(u @ u.T - np.eye(N))))
                    q["R3"] = float(np.max(np.abs(v @ v.T - np.eye(M))))
                    q["d_error"] = float(np.max(np.abs(d - d_ref)) / d_ref[0])
                r[f"b{b}"] = q
                last = (tu, td, tv)
            tu, td, tv = last
            # the witness call returns with its work queued on the engine's own streams: host clock around
            # call and sync, one warm-up
            ws = []
            for i in range(a.witness_reps + 1):
                ctx.sync()
                t0 = time.perf_counter()
                hs.svd_witness(ctx, tm, tu, tv, td, 7)
                ctx.sync()
                if i:
                    ws.append((time.perf_counter() - t0) * 1e3)
            r["witness_ms"], r["witness_spread_ms"] = round(median(ws), 3), round(max(ws) - min(ws), 3)
            chk = ctx.check_gates()
            r["witness_failures"] = chk["gate_failures"] + chk["copy_failures"] + chk["lookup_failures"]
            rec["shapes"][shape] = r
            print(shape, json.dumps(r), file=sys.stderr, flush=True)
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
