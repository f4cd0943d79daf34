"""Which product kernels a call runs, pinned to a recording.

The value tests (test_exact_edges_gpu.py, test_parity_gpu.py) compare cells: a
change that sent a product to the Montgomery GEMM would pass them all and only
be slow. A call's route is what the context's profiler saw of the product
kernels: (name, launches, bytes, ops) per kernel name (with its stream tag) in
order of first appearance, over the names beginning with k_gemm, k_to_residues,
k_to_digits or k_residues. All four are integers (the byte and operation counts
fit a double exactly), compared with ==.

tests/golden/gemm_routes.json holds the routes recorded on an MI355X at the
commit before gemm.cpp / gemm.hip were split off (record() run against that
build). The tests never re-record; a case missing from the fixture fails.

Cases: the smallest shapes at which each branch of the product's host code
exists. Route A / B of tests/exact_cases.py (the one-call recipe / the modular
calls) on either side of the digit capacities and of the K gate, a symmetric
product through the modular API, and svd_witness at 136 x 130 (both dimensions
cross a 128 tile with a partial tile; the shard row boundary at 68 is not
tile-aligned) unsharded, pipelined, with residues from the cells, with
host-known bits and as rank 1 of 2.
"""
import json
import os

import numpy as np
import pytest

import exact_cases as ec
from conftest import gamma_for, gen_svd_input

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_routes.json")
PREFIXES = ("k_gemm", "k_to_residues", "k_to_digits", "k_residues")
BY_ID = {c[0]: c for c in ec.cases()}

LADDER = "ladder-n19-tight-a49-b96-k1"
CRT0 = (("gemm_crt", 0),)
# (case id, route, options, gemm impl, exact case)
EXACT = [
    ("A-dev", "A-dev", (), None, LADDER),
    ("A-host", "A-host", (), None, LADDER),
    ("A-kern1", "A-dev", (("gemm_kern", 1),), None, "ladder-n37-tight-a128-b128-k512"),      # K >= 512: persistent
    ("A-digits-le70", "A-dev", CRT0, None, "digits-a39-o70-k7"),
    ("A-digits-gt70", "A-dev", CRT0, None, "digits-a62-o71-k64"),
    ("B-narrow", "B", (), None, "ladder-n01-tight-a2-b3-k2"),
    ("B-128", "B", (), None, "ladder-n36-tight-a128-b128-k256"),
    ("B-mfma-5", "B", CRT0, "mfma", "digits-byte7f-a8-b7-k64"),                             # 5 x 5 planes
    ("B-mfma-8", "B", CRT0, "mfma", "digits-a7-o39-k64"),                                   # 5 x 8
    ("B-mfma-9", "B", CRT0, "mfma", "digits-a38-o63-k64"),                                  # 5 x 9
    ("B-mfma-gt70", "B", CRT0, "mfma", "digits-a62-o71-k64"),
    ("B-valu", "B", CRT0, "valu", "digits-b39-o70-k7"),                                     # 9 x 8 on v_dot4
    ("A-kgate-8192", "A-dev", (), None, "kgate-k8192-a7-b8"),
    ("A-kgate-8193", "A-dev", (), None, "kgate-k8193-a70-b33"),
    ("B-kgate-8192", "B", (), None, "kgate-k8192-a7-b8"),
    ("B-kgate-8193", "B", (), None, "kgate-k8193-a70-b33"),
]
SYM = [("sym-default", ()), ("sym-digits", CRT0)]
# (case id, options, gemm impl, shard, calls)
SVD = [
    ("svd-default-twice", (), None, None, 2),                  # the second call is the pipelined one
    ("svd-res_f64-0", (("res_f64", 0),), None, None, 1),       # a_from_b
    ("svd-valu", (), "valu", None, 1),                         # host-known bits
    ("svd-shard", (), None, (1, 2), 1),                        # the row block in the batch
    ("svd-shard-res_f64-0", (("res_f64", 0),), None, (1, 2), 1),   # bbuf = digC and b_ready
]
SVD_N, SVD_M, SVD_P = 136, 130, 32
# every product kernel name (stream tag dropped) must occur in the fixture; the
# last three: any host-chosen DA x DB on the matrix cores and on v_dot4, any symmetric digit variant
NAMES = ["k_to_residues", "k_residues_f64", "k_gemm_crt", "k_gemm_crt:s", "k_gemm_crt:multi", "k_to_digits_mf",
         "k_gemm_mfma:rt", "k_to_digits", "k_gemm_mont"]
PATTERNS = [r"k_gemm_mfma:\d+x\d+s?", r"k_gemm_dot4:\d+x\d+s?", r"k_gemm_(mfma|dot4):(\d+x\d+|rt)s"]


def _context(factory, P, opts, impl, shard=None):
    ctx = factory(P)
    for name, val in opts:
        ctx.set_option(name, val)
    if impl:
        ctx.set_gemm_impl(impl)
    if shard:
        ctx.set_shard(*shard)
    return ctx


def _route(ctx, call):
    ctx.profile(True)
    call()
    out = []
    for r in ctx.profile_collect():
        if r["name"].startswith(PREFIXES):
            assert float(r["bytes"]).is_integer() and float(r["ops"]).is_integer(), r
            out.append([r["name"], int(r["launches"]), int(r["bytes"]), int(r["ops"])])
    ctx.profile(False)
    return out


def _exact(factory, route, opts, impl, cid):
    import halo2_svd041_amd as hs
    import torch
    _, P, N, K, M, a, b = BY_ID[cid]
    ctx = _context(factory, P, opts, impl)
    g = gamma_for(7)
    if route == "A-dev":
        ta, tb = (torch.tensor(x, dtype=torch.float64, device="cuda:0") for x in (a, b))
        return _route(ctx, lambda: hs.verify_mul_witness(ctx, ta, tb, g))
    if route == "A-host":
        return _route(ctx, lambda: hs.verify_mul_witness(ctx, a, b, g))

    def modular():
        za, zb = hs.ZkMatrix.new(ctx, a), hs.ZkMatrix.new(ctx, b)
        hs.ZkMatrix.verify_mul(ctx, za, zb, hs.honest_prover_mat_mul(ctx, za, zb), g)
    return _route(ctx, modular)


def _sym(factory, opts):
    import halo2_svd041_amd as hs
    ctx = _context(factory, 32, opts, None)
    a = np.random.RandomState(5).uniform(-8, 8, size=(136, 70))

    def product():
        za = hs.ZkMatrix.new(ctx, a)
        hs.honest_prover_mat_mul(ctx, za, za.transpose_matrix())
    return _route(ctx, product)


def _svd(factory, opts, impl, shard, calls):
    import halo2_svd041_amd as hs
    import torch
    ctx = _context(factory, SVD_P, opts, impl, shard)
    m, u, d, v = gen_svd_input(SVD_N, SVD_M, seed=3)
    dev = [torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device="cuda:0") for x in (m, u, v, d)]

    def witness():
        for _ in range(calls):
            hs.svd_witness(ctx, *dev, gamma_for(3))
    return _route(ctx, witness)


CASES = {}
for _id, *_args in EXACT:
    CASES[_id] = (_exact, _args)
for _id, *_args in SYM:
    CASES[_id] = (_sym, _args)
for _id, *_args in SVD:
    CASES[_id] = (_svd, _args)


def record(factory) -> dict:
    """Every case's route on the library in use (for the fixture; no test calls it)."""
    return {cid: fn(factory, *args) for cid, (fn, args) in CASES.items()}


def _golden() -> dict:
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", list(CASES))
def test_route_is_the_recorded_one(gpu_ctx_factory, cid):
    golden = _golden()
    assert cid in golden, f"{cid}: no recorded route in {FIXTURE}"
    fn, args = CASES[cid]
    got = fn(gpu_ctx_factory, *args)
    print(cid, got)
    assert got == golden[cid]


def test_fixture_covers_every_product_kernel():
    import re
    golden = _golden()
    assert set(golden) == set(CASES)
    seen = {r[0].split("@")[0] for route in golden.values() for r in route}
    for name in NAMES:
        assert name in seen, f"{name} occurs in no recorded route: {sorted(seen)}"
    for pat in PATTERNS:
        assert any(re.fullmatch(pat, s) for s in seen), f"{pat} matches no recorded name: {sorted(seen)}"
