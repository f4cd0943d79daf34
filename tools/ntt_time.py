#!/usr/bin/env python3
"""Timing of the domain transforms (svdw_ntt, svdw_check_ntt) on 8 columns of
full-width cells, one JSON line, also written to profiles/ntt_time.json.

Sizes k = 20, 22, 24, each only if its buffers fit the device's free memory
(the largest that ran is recorded as "size"). At each size:

  forward, inverse   svdw_ntt without a shift, canonical and Montgomery;
  extended           coeff_to_extended k -> k + 2 with a full-width shift;
  check              svdw_check_ntt with log_samples = 10 on the forward result
                     (--check-reps runs: it evaluates 2^10 points per column);
  kernels            the per-kernel split of one profiled forward, inverse,
                     extension and check;
  d2d                a hipMemcpyDtoD of the bytes one pass moves (the columns
                     read, the columns written: a copy of one of them);
  ms_per_mul         kernel ms per (multiplication x 2^26 elements), with the
                     multiplications per element and pass that ntt.hip's header
                     states; and the same figure of the grand-product kernels
                     from --lookup-json (tools/lookup_product_time.py's or
                     tools/permutation_product_time.py's record of the same
                     session), whose kernels run the same mont_mul: they are the
                     yardstick, not the code under test.

HIP events on torch's stream around the calls, one warm-up, then the median of
--reps.

    python tools/ntt_time.py [--out FILE] [--lookup-json FILE]
"""
import argparse
import ctypes as ct
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P_MOD = 21888242871839275222246405745257275088548364400416034343698204186575808495617
SHIFT = 0x2b3f9c1d5e7a8046f1e2d3c4b5a69788796a5b4c3d2e1f0a1b2c3d4e5f607182 % P_MOD
NCOLS, SIZES, EXT, LOG_SAMPLES = 8, (20, 22, 24), 2, 10
LOOKUP_MULS = {"k_lp_write": 10.5}                           # per row (lookup_product.hip's header)


def median(xs):
    return sorted(xs)[len(xs) // 2]


def pass_muls(k, passes, bits, k_in=None, inverse=False, shifted=False):
    """Multiplications per output element of each pass (ntt.hip's header)."""
    k_in = k if k_in is None else k_in
    out = []
    for i in range(passes):
        m = (bits[i] - 1) / 2 + (2 if i + 1 < passes else 0)
        if i == 0 and shifted and not inverse:
            m += 2 / (1 << (k - k_in))                       # the loaded cells only
        if i + 1 == passes and inverse:
            m += 2 if shifted else 1
        out.append(m)
    return out


def eval_muls(n):
    run = min(256, max(1, n // 256))
    return 1 + (8 + 2 * max(1, (n - 1).bit_length()) + 1) / run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--check-reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ntt_time.json"))
    ap.add_argument("--lookup-json", default=os.path.join(ROOT, "profiles", "lookup_product_time.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        print("ntt_time: no HIP device", file=sys.stderr)
        return 1
    import halo2_svd041_amd as hs
    L = hs.zk.lib()
    hip = ct.CDLL("libamdhip64.so")
    hip.hipMemcpyDtoDAsync.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_size_t, ct.c_void_p]
    dev = torch.device("cuda", 0)
    free = torch.cuda.mem_get_info(dev)[0]
    rec = {"columns": NCOLS, "reps": a.reps, "check_reps": a.check_reps, "log_samples": LOG_SAMPLES,
           "free_GB": round(free / 1e9, 1), "sizes": {}}

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
        for k in SIZES:
            rows, ke = 1 << k, k + EXT
            col_bytes = NCOLS * rows * 32
            # in, out, the engine's buffer between passes; the extension's out and buffer
            need = 3 * col_bytes + 2 * (col_bytes << EXT) + (2 << 30)
            if need > free or ke > 28:
                continue
            r = {"need_GB": round(need / 1e9, 1)}
            g = torch.Generator(device=dev)
            g.manual_seed(k)
            cols = torch.randint(0, 256, (NCOLS, rows, 32), dtype=torch.uint8, device=dev, generator=g)
            cols[:, :, 31] &= 0x1F                            # 253 random bits: below p in either form
            out = torch.empty_like(cols)
            passes = L.svdw_ntt_passes(k)
            bits = [k // passes + (1 if i < k % passes else 0) for i in range(passes)]
            r.update(passes=passes, radix_bits=bits)
            per = NCOLS * rows / 2 ** 26

            def kernels(fn):
                ctx.profile(True, "k_ntt")
                fn()
                kern = {s["name"].split("@")[0]: round(s["total_ms"], 3) for s in ctx.profile_collect()}
                ctx.profile(False)
                return kern

            def per_mul(kern, muls, elems):
                return {f"k_ntt_pass{i + 1}": round(kern[f"k_ntt_pass{i + 1}"] / (m * elems), 3)
                        for i, m in enumerate(muls) if f"k_ntt_pass{i + 1}" in kern}

            for form in ("canonical", "montgomery"):
                for inverse in (False, True):
                    tag = f"{'inverse' if inverse else 'forward'}_{form}"
                    call = lambda: ctx.ntt(cols, k, inverse=inverse, form=form, out=out)   # noqa: E731
                    r[f"{tag}_ms"], r[f"{tag}_spread_ms"] = events(call, a.reps)
                    kern = kernels(call)
                    r[f"kernels_{tag}_ms"] = kern
                    r[f"ms_per_mul_{tag}"] = per_mul(kern, pass_muls(k, passes, bits, inverse=inverse), per)
            form = "canonical"
            ctx.ntt(cols, k, form=form, out=out)
            chk = lambda: ctx.check_ntt(cols, out, k, form=form, log_samples=LOG_SAMPLES, seed=k)   # noqa: E731
            r["check_ms"], r["check_spread_ms"] = events(chk, a.check_reps)
            r["check_result"] = chk()
            kern = kernels(chk)
            r["kernels_check_ms"] = kern
            r["ms_per_mul_check"] = {"k_ntt_eval": round(
                kern["k_ntt_eval"] / (eval_muls(rows) * per * (1 << LOG_SAMPLES)), 3)}
            # a device copy of the bytes one pass moves
            stream = torch.cuda.current_stream(dev).cuda_stream

            def d2d():
                if hip.hipMemcpyDtoDAsync(out.data_ptr(), cols.data_ptr(), col_bytes, stream) != 0:
                    raise RuntimeError("hipMemcpyDtoDAsync failed")

            r["d2d_ms"], r["d2d_spread_ms"] = events(d2d, a.reps)
            r["forward_canonical_over_d2d"] = round(r["forward_canonical_ms"] / r["d2d_ms"], 2)
            del out
            ext = torch.empty((NCOLS, 1 << ke, 32), dtype=torch.uint8, device=dev)
            pe = L.svdw_ntt_passes(ke)
            be = [ke // pe + (1 if i < ke % pe else 0) for i in range(pe)]
            call = lambda: ctx.coeff_to_extended(cols, k, ke, SHIFT, form=form, out=ext)   # noqa: E731
            r["extended_ms"], r["extended_spread_ms"] = events(call, a.reps)
            kern = kernels(call)
            r["kernels_extended_ms"] = kern
            r["ms_per_mul_extended"] = per_mul(kern, pass_muls(ke, pe, be, k_in=k, shifted=True), per * (1 << EXT))
            r["extended_check"] = ctx.check_ntt(cols, ext, ke, k_in=k, shift=SHIFT, form=form, log_samples=6, seed=1)
            del ext, cols
            torch.cuda.empty_cache()
            rec["sizes"][str(k)] = r
            rec["size"] = f"{NCOLS} columns k={k}"
    if "size" not in rec:
        print("ntt_time: no size fits the device", file=sys.stderr)
        return 1
    if a.lookup_json and os.path.exists(a.lookup_json):
        lk = json.loads(open(a.lookup_json).read().splitlines()[0])
        rec["yardstick_source"] = os.path.basename(a.lookup_json)
        for key, val in lk.items():                         # either tool's record: its own ms_per_mul figures
            if key.startswith(("ms_per_mul_", "lookup_ms_per_mul_")):
                rec.setdefault("yardstick_ms_per_mul", {})[key] = val
        if "yardstick_ms_per_mul" not in rec and "kernels_canonical_ms" in lk:
            per = lk["columns"] * ((1 << lk["k"]) - lk["unusable_rows"]) / 2 ** 26
            for form in ("canonical", "montgomery"):
                kern = {n.split("@")[0]: ms for n, ms in lk.get(f"kernels_{form}_ms", {}).items()}
                rec.setdefault("yardstick_ms_per_mul", {})[f"lookup_ms_per_mul_{form}"] = {
                    n: round(kern[n] / (mul * per), 3) for n, mul in LOOKUP_MULS.items() if n in kern}
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
