"""The exact-arithmetic edge cases (tests/exact_cases.py) on the GPU, bit-exact.

Every case's whole phase-0 and phase-1 advice streams are compared cell for
cell with the C oracle's verify_mul recipe (corc.verify_mul_witness, pinned
against Python integer sums in tests/test_exact_edges_cpu.py), and the counts
are checked. The cases sit on the bit widths where the exact-integer kernels
switch code path: the CRT GEMM's modulus count, the residue words, the digit
planes, the row scans' small-operand words, the K <= 8192 gate and the
bit-length fold over quantize blocks.

Route A is the one-call recipe (verify_mul_witness): device inputs (fused
quantize + bit-length fold, residues from the f64 inputs, GEMM and scans sized
from device words), host inputs (residues from the cells), the persistent
CRT GEMM (gemm_kern 1) for the ladder / K-gate cases with K >= 257, and, for
the digit-plane cases, gemm_crt 0 (digit planes chosen on the device).
Route B is the modular API (ZkMatrix.new x 2, honest_prover_mat_mul,
ZkMatrix.verify_mul) with host-known bounds: (i) default options, (ii) the
digit GEMM on matrix cores, (iii) the digit GEMM on v_dot4; the digit routes
fall back to the Montgomery GEMM above 70 bits.

One context per (route, option set, precision), reset between cases, and the
cases run in the generator's order (wide and narrow interleaved), so state a
wide case leaves behind would show in the narrow case after it.
"""
import numpy as np
import pytest

import corc
import exact_cases as ec
from conftest import gamma_for

pytestmark = pytest.mark.gpu

CASES = ec.cases()
IDS = [c[0] for c in CASES]
BY_ID = {c[0]: c for c in CASES}
_ref = {}


def _reference(cid):
    """(gamma, advice0, advice1) of the C oracle, computed once per case."""
    if cid not in _ref:
        _, P, N, K, M, a, b = BY_ID[cid]
        g = gamma_for(1000 + IDS.index(cid))
        c0, c1 = corc.verify_mul_witness(a, b, P, g)
        c0.setflags(write=False)
        c1.setflags(write=False)
        _ref[cid] = (g, c0, c1)
    return _ref[cid]


@pytest.fixture(scope="module")
def edge_ctx(gpu_ctx_factory):
    """Context of a (route, options, P) key, created on first use and shared by
    every case of that key."""
    ctxs = {}

    def get(route, P, opts=(), impl=None):
        key = (route, P, opts, impl)
        if key not in ctxs:
            ctx = gpu_ctx_factory(P)
            for name, val in opts:
                ctx.set_option(name, val)
            if impl:
                ctx.set_gemm_impl(impl)
            ctxs[key] = ctx
        return ctxs[key]
    return get


def _compare(ctx, cid, counts=None):
    _, c0, c1 = _reference(cid)
    if counts is not None:
        assert counts == {"advice0": c0.shape[0], "advice1": c1.shape[0], "lookup0": 0, "lookup1": 0}
    assert ctx.advice_len(0) == c0.shape[0] and ctx.advice_len(1) == c1.shape[0]
    assert ctx.lookup_len(0) == 0 and ctx.lookup_len(1) == 0
    _, P, N, K, M, _, _ = BY_ID[cid]
    cs0 = N * K + K * M
    for name, got, want in (("advice0", ctx.advice(0), c0), ("advice1", ctx.advice(1), c1)):
        bad = np.nonzero(np.any(got != want, axis=1))[0]
        where = ""
        if bad.size and name == "advice0":
            where = f" (loads end at {cs0}; c_s cells (i, j): {[divmod(int(x) - cs0, M) for x in bad[:8] if x >= cs0]})"
        assert bad.size == 0, f"{cid} {name}: {bad.size} of {want.shape[0]} cells differ, first at {bad[:8]}{where}"


def _route_a(ctx, cid, device):
    import halo2_svd041_amd as hs
    _, P, N, K, M, a, b = BY_ID[cid]
    g = _reference(cid)[0]
    try:
        if device:
            import torch
            ta, tb = (torch.tensor(x, dtype=torch.float64, device="cuda:0") for x in (a, b))
            counts = hs.verify_mul_witness(ctx, ta, tb, g)
        else:
            counts = hs.verify_mul_witness(ctx, a, b, g)
        _compare(ctx, cid, counts)
    finally:
        ctx.reset()


def _route_b(ctx, cid):
    import halo2_svd041_amd as hs
    _, P, N, K, M, a, b = BY_ID[cid]
    g = _reference(cid)[0]
    try:
        za, zb = hs.ZkMatrix.new(ctx, a), hs.ZkMatrix.new(ctx, b)
        cs = hs.honest_prover_mat_mul(ctx, za, zb)
        hs.ZkMatrix.verify_mul(ctx, za, zb, cs, g)
        _compare(ctx, cid)
    finally:
        ctx.reset()


ROUTES = ec.routes(CASES)


@pytest.mark.parametrize("cid", IDS)
def test_recipe_device_inputs(edge_ctx, cid):
    """Route A, device inputs: k_quantize_multi + fold, k_residues_f64, CRT GEMM
    and combine, scans sized from the device bit-length words."""
    _route_a(edge_ctx("A-dev", BY_ID[cid][1]), cid, device=True)


@pytest.mark.parametrize("cid", IDS)
def test_recipe_host_inputs(edge_ctx, cid):
    """Route A, host inputs: the residue planes come from the quantized cells."""
    _route_a(edge_ctx("A-host", BY_ID[cid][1]), cid, device=False)


@pytest.mark.parametrize("cid", ROUTES["A gemm_kern 1"])
def test_recipe_persistent_gemm(edge_ctx, cid):
    """Route A with the persistent CRT GEMM (gemm_kern 1), K >= 257."""
    _route_a(edge_ctx("A-kern1", BY_ID[cid][1], (("gemm_kern", 1),)), cid, device=True)


@pytest.mark.parametrize("cid", ROUTES["A gemm_crt 0"])
def test_recipe_device_digit_gemm(edge_ctx, cid):
    """Route A with gemm_crt 0, device inputs: the digit planes are chosen on the
    device from the bit-length words (the modular routes below choose them on
    the host), the Montgomery GEMM takes over above 70 bits."""
    _route_a(edge_ctx("A-digits", BY_ID[cid][1], (("gemm_crt", 0),)), cid, device=True)


@pytest.mark.parametrize("cid", IDS)
def test_modular_default(edge_ctx, cid):
    """Route B (i): the modular calls with default options (CRT GEMM fed by
    host-known bit bounds, scans with host-known widths)."""
    _route_b(edge_ctx("B-crt", BY_ID[cid][1]), cid)


@pytest.mark.parametrize("cid", ROUTES["B gemm_crt 0 mfma"])
def test_modular_digit_gemm_mfma(edge_ctx, cid):
    """Route B (ii): gemm_crt 0 on matrix cores: 5 / 8 / 9 digit planes, the
    Montgomery GEMM above 70 bits."""
    _route_b(edge_ctx("B-mfma", BY_ID[cid][1], (("gemm_crt", 0),), "mfma"), cid)


@pytest.mark.parametrize("cid", ROUTES["B gemm_crt 0 valu"])
def test_modular_digit_gemm_valu(edge_ctx, cid):
    """Route B (iii): gemm_crt 0 on v_dot4."""
    _route_b(edge_ctx("B-valu", BY_ID[cid][1], (("gemm_crt", 0),), "valu"), cid)
