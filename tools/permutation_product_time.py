#!/usr/bin/env python3
"""Permutation grand-product timing on the advice columns of both phases of an
SVD witness, one JSON line, also written to profiles/permutation_product_time.json.

The size is the largest of 1024^2 P=63 k=24 and 512^2 P=32 k=22 whose columns,
sigma and Z fit the device's free memory together (recorded as "size"). Sigma is
made on the device: the usable cells sorted by value (four stable sorts, one per
64-bit word), each run of equal values linked into a cycle, then
svdw_permutation_values; it is honest by construction, so final_not_one == 0
doubles as a full-size check of the product.

  product          svdw_permutation_product with chunk_len 2 and 3 in the
                   canonical and the Montgomery form;
  check            svdw_check_permutation_product on each result;
  d2d              a hipMemcpyDtoD of the bytes the product has to move (columns
                   and sigma read, Z written: a copy of half of them), same
                   process;
  kernels          the per-kernel split of one profiled product and check;
  ms_per_mul       kernel ms per (multiplication x 2^26 rows), with the
                   multiplications per row of a set that permutation_product.hip
                   states; and the same figure of the lookup product's kernels
                   from --lookup-json (tools/lookup_product_time.py's record of
                   the same session), whose kernels run the same mont_mul.

HIP events on torch's stream around the calls, one warm-up, then the median of
--reps.

    python tools/permutation_product_time.py [--out FILE] [--lookup-json FILE]
"""
import argparse
import ctypes as ct
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P_MOD = 21888242871839275222246405745257275088548364400416034343698204186575808495617
BETA, GAMMA = 0x1234567890abcdef1234567890abcdef, P_MOD - (1 << 200)
SIZES = [(1024, 63, 24), (512, 32, 22)]
LB, MIN_ROWS = 19, 20
# multiplications per row of a set of m columns (permutation_product.hip's header)
MULS = {"k_pp_tiles": lambda m: 4 * m + 1 + 2 + 12 / 16, "k_pp_write": lambda m: 4 * m + 1 + 4 + 18 / 4,
        "k_pp_check": lambda m: 4 * m + 1 + 3}
LOOKUP_MULS = {"k_lp_tiles": 4.75, "k_lp_write": 10.5, "k_lp_check": 4.0}


def median(xs):
    return sorted(xs)[len(xs) // 2]


def value_sorted_mapping(torch, cols, usable):
    """[n, rows] int64 col << 32 | row: every run of equal cells among the rows
    < usable linked into one cycle, the identity elsewhere."""
    n, rows = cols.shape[0], cols.shape[1]
    dev = cols.device
    cell = torch.arange(n, device=dev)[:, None] << 32 | torch.arange(rows, device=dev)[None, :]
    words = cols.view(torch.int64)[:, :usable, :].reshape(-1, 4)
    order = torch.arange(words.shape[0], device=dev)
    for w in range(4):                                       # least significant sort first, each stable
        order = order[torch.sort(words[order, w], stable=True).indices]
    sw = words[order]
    at = cell[:, :usable].reshape(-1)[order]
    start = torch.ones(at.numel(), dtype=torch.bool, device=dev)
    start[1:] = (sw[1:] != sw[:-1]).any(dim=1)
    del sw, words
    i = torch.arange(at.numel(), device=dev)
    run_start = torch.cummax(torch.where(start, i, torch.zeros_like(i)), 0).values
    nxt = torch.where(torch.roll(start, -1), at[run_start], torch.roll(at, -1))
    mapping = cell.clone()
    mapping.view(-1)[(at >> 32) * rows + (at & 0xffffffff)] = nxt
    return mapping, int(start.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--unusable-rows", type=int, default=6)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "permutation_product_time.json"))
    ap.add_argument("--lookup-json", default=os.path.join(ROOT, "profiles", "lookup_product_time.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    from bench import gen_input
    import torch
    if not torch.cuda.is_available():
        print("permutation_product_time: no HIP device", file=sys.stderr)
        return 1
    import halo2_svd041_amd as hs
    hip = ct.CDLL("libamdhip64.so")
    hip.hipMemcpyDtoDAsync.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_size_t, ct.c_void_p]
    dev = torch.device("cuda", 0)
    un = a.unusable_rows
    free = torch.cuda.mem_get_info(dev)[0]
    rec = None
    for N, P, k in SIZES:
        m, u, d, v = gen_input(N, N, 0)
        with hs.Context(device=-1, precision_bits=P, lookup_bits=LB) as plan:
            hs.svd_witness(plan, m, u, v, d, 0x1234567)
            used = plan.physical_layout(k, MIN_ROWS)["columns_used"]
        ncols, rows = sum(used), 1 << k
        # columns, sigma, Z of chunk_len 2, and the sort's index and key tensors (8 x 8 B per cell)
        need = (2 * ncols + (ncols + 1) // 2) * rows * 32 + 64 * ncols * rows + (4 << 30)
        if need <= free:
            rec = {"size": f"{N}x{N} P={P} k={k}", "N": N, "P": P, "LB": LB, "k": k, "unusable_rows": un,
                   "reps": a.reps, "columns": ncols, "columns_per_phase": used,
                   "need_GB": round(need / 1e9, 1), "free_GB": round(free / 1e9, 1)}
            break
    if rec is None:
        print("permutation_product_time: no size fits the device", file=sys.stderr)
        return 1
    usable = rows - un

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
        assert ctx.physical_layout(k, MIN_ROWS)["columns_used"] == used
        cols = torch.cat([ctx.assign_columns(ph)[0] for ph in (0, 1)])
        mapping, runs = value_sorted_mapping(torch, cols, usable)
        rec.update(distinct_values=runs, cells=ncols * usable)
        torch.cuda.empty_cache()
        for form in ("canonical", "montgomery"):
            if form == "montgomery":
                del cols
                cols = torch.cat([ctx.assign_columns(ph, form=form)[0] for ph in (0, 1)])
            sigma, bad = ctx.permutation_values(k, mapping, form=form)
            assert bad == 0
            rec[f"values_{form}_ms"] = round(events(lambda: ctx.permutation_values(k, mapping, form=form)), 3)
            for chunk in (2, 3):
                nsets = -(-ncols // chunk)
                sets = [min(chunk, ncols - s * chunk) for s in range(nsets)]
                z = torch.empty((nsets, rows, 32), dtype=torch.uint8, device=dev)
                args = (BETA, GAMMA, chunk, k, un, form)
                tag = f"{form}_c{chunk}"
                rec[f"product_{tag}_ms"] = round(events(lambda: ctx.permutation_product(cols, sigma, *args, out=z)), 3)
                rec[f"product_{tag}_result"] = ctx.permutation_product(cols, sigma, *args, out=z)[1]
                rec[f"check_{tag}_ms"] = round(
                    events(lambda: ctx.check_permutation_product(cols, sigma, z, *args)), 3)
                chk = ctx.check_permutation_product(cols, sigma, z, *args)
                rec[f"check_{tag}_failures"] = sum(x for n, x in chk.items() if n.endswith("failures"))
                ctx.profile(True, "k_pp")
                ctx.permutation_product(cols, sigma, *args, out=z)
                ctx.check_permutation_product(cols, sigma, z, *args)
                kern = {s["name"].split("@")[0]: round(s["total_ms"], 3) for s in ctx.profile_collect()}
                ctx.profile(False)
                rec[f"kernels_{tag}_ms"] = kern
                rec[f"ms_per_mul_{tag}"] = {
                    n: round(kern[n] / (sum(f(mm) for mm in sets) * usable / 2 ** 26), 3)
                    for n, f in MULS.items() if n in kern}
                # the floor: a device copy of the bytes read plus the bytes written
                half = (2 * ncols + nsets) * rows * 32 // 2
                src = torch.empty(half, dtype=torch.uint8, device=dev)
                dst = torch.empty(half, dtype=torch.uint8, device=dev)
                src.zero_()
                stream = torch.cuda.current_stream(dev).cuda_stream

                def d2d():
                    if hip.hipMemcpyDtoDAsync(dst.data_ptr(), src.data_ptr(), half, stream) != 0:
                        raise RuntimeError("hipMemcpyDtoDAsync failed")

                rec[f"d2d_{tag}_ms"] = round(events(d2d), 3)
                rec[f"product_{tag}_over_d2d"] = round(rec[f"product_{tag}_ms"] / rec[f"d2d_{tag}_ms"], 2)
                del src, dst, z
            del sigma
    if a.lookup_json and os.path.exists(a.lookup_json):
        lk = json.loads(open(a.lookup_json).read().splitlines()[0])
        per = lk["columns"] * ((1 << lk["k"]) - lk["unusable_rows"]) / 2 ** 26
        for form in ("canonical", "montgomery"):
            kern = {n.split("@")[0]: ms for n, ms in lk.get(f"kernels_{form}_ms", {}).items()}
            rec[f"lookup_ms_per_mul_{form}"] = {n: round(kern[n] / (mul * per), 3)
                                                for n, mul in LOOKUP_MULS.items() if n in kern}
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
