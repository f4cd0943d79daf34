"""svdw_svd_decompose on the device against the circuit's own tolerances, LAPACK's
singular values and the plain numpy restatement (svd_decompose_cases), and end
to end: the witness made from the device factors passes the device checker and
equals the C oracle's witness of those same factors.

Every shared input runs with host arrays; the rectangular shapes, 17x17 and the
special matrices also run with device tensors. A run is made once per
(input, kind of memory) and shared by the tests.
"""
import ctypes as ct

import numpy as np
import pytest

import corc
from conftest import gamma_for
from svd_decompose_cases import CASES, CASE_IDS, EPS, RECTANGULAR, d_error, recipe, residuals, restated

pytestmark = pytest.mark.gpu

DEVICE_TOO = RECTANGULAR | {"17x17", "zero4", "rank1_5x4", "ones4x6", "3I5", "orth12", "graded13", "64x64_b4_i2"}
RUNS = [(n, False) for n in CASE_IDS] + [(n, True) for n in CASE_IDS if n in DEVICE_TOO]
RECIPE_IDS = [c[0] for c in CASES if c[5]]


@pytest.fixture(scope="module")
def ctxs():
    from conftest import have_gpu
    if not have_gpu():
        pytest.skip("no HIP device")
    import halo2_svd041_amd as hs
    made = {63: hs.Context(device=0, precision_bits=63, lookup_bits=19),
            32: hs.Context(device=0, precision_bits=32, lookup_bits=19)}
    yield made
    for c in made.values():
        c.close()


_runs = {}


def run(ctxs, name, device):
    """(u, d, v, info) of case `name` as numpy arrays, and the device tensors (m, u, d, v) when device."""
    import torch
    import halo2_svd041_amd as hs
    if (name, device) not in _runs:
        _, m, b, inner, _, _ = CASES[CASE_IDS.index(name)]
        if device:
            tm = torch.from_numpy(m).to("cuda:0")
            tu, td, tv, info = hs.svd_decompose(ctxs[63], tm, device=True, panel=b, inner=inner)
            assert tu.is_cuda and td.is_cuda and tv.is_cuda
            _runs[(name, device)] = (tu.cpu().numpy(), td.cpu().numpy(), tv.cpu().numpy(), info, (tm, tu, td, tv))
        else:
            u, d, v, info = hs.svd_decompose(ctxs[63], m, panel=b, inner=inner)
            _runs[(name, device)] = (u, d, v, info, None)
    return _runs[(name, device)]


@pytest.mark.parametrize("name,device", RUNS, ids=[f"{n}-{'device' if dv else 'host'}" for n, dv in RUNS])
def test_factors(ctxs, name, device):
    import halo2_svd041_amd as hs
    _, m, b, inner, completed, _ = CASES[CASE_IDS.index(name)]
    u, d, v, info, _ = run(ctxs, name, device)
    N, M = m.shape
    # 1. properties that need no tolerance
    assert info["converged"] == 1, info
    assert u.shape == (N, N) and v.shape == (M, M) and d.shape == (min(N, M),)
    assert np.all(np.isfinite(u)) and np.all(np.isfinite(v)) and np.all(np.isfinite(d))
    assert np.all(d >= 0) and np.all(np.diff(d) <= 0)
    assert info["completed"] == completed, info
    ref = np.linalg.svd(m, compute_uv=False)
    assert completed == int(np.sum(ref <= max(N, M) * EPS * ref[0]))
    # 2. the circuit's tolerances with a factor 10 to spare
    es, eu = hs.err_calc(63, max(N, M), 100.0, 1e-10, 1e-10)
    r1, r2, r3 = residuals(m, u, d, v)
    # 3. the singular values against LAPACK, beside the restatement's
    dev_err, cpu_err = d_error(m, d), d_error(m, restated(name)[1])
    print(f"{name} {'device' if device else 'host'}: {info} R1 {r1:.3e} R2 {r2:.3e} R3 {r3:.3e} "
          f"d error {dev_err:.3e} (restatement {cpu_err:.3e}, {restated(name)[3]['sweeps']} sweeps)")
    assert r1 <= es / 10 and r2 <= eu / 10 and r3 <= eu / 10, (r1, r2, r3, es, eu)
    assert dev_err <= 4 * cpu_err, (dev_err, cpu_err)


def test_zero_matrix_gives_identities(ctxs):
    for device in (False, True):
        u, d, v, info, _ = run(ctxs, "zero4", device)
        assert np.array_equal(u, np.eye(4)) and np.array_equal(v, np.eye(4)) and np.array_equal(d, np.zeros(4))
        assert info["rotations"] == 0 and info["sweeps"] == 1


def _witness_cells(ctx):
    return ctx.advice(0), ctx.lookups(0), ctx.advice(1)


@pytest.mark.parametrize("name", RECIPE_IDS)
def test_witness_from_device_factors(ctxs, name):
    """4. svd_witness(on_device) of the device factors passes the device checker at P = 63 and 32 and is the
    C oracle's witness of the same factors byte for byte."""
    import torch
    import halo2_svd041_amd as hs
    _, m, b, inner, _, _ = CASES[CASE_IDS.index(name)]
    tm = torch.from_numpy(m).to("cuda:0")
    tu, td, tv, info = hs.svd_decompose(ctxs[63], tm, device=True, panel=b, inner=inner)
    u, d, v = tu.cpu().numpy(), td.cpu().numpy(), tv.cpu().numpy()
    for P in (63, 32):
        ctx, g = ctxs[P], gamma_for(P)
        hs.svd_witness(ctx, tm, tu, tv, td, g)
        chk = ctx.check_gates()
        assert chk["gates_checked"] > 0 and chk["copies_checked"] > 0
        assert chk["gate_failures"] == 0 and chk["copy_failures"] == 0 and chk["lookup_failures"] == 0, chk
        a0, l0, a1 = corc.svd_witness(m, u, v, d, P, 19, g)
        g0, gl, g1 = _witness_cells(ctx)
        assert np.array_equal(g0, a0) and np.array_equal(gl, l0) and np.array_equal(g1, a1)


def test_matrix_wrong_still_fails(ctxs):
    """input-creator.py:46-49: m[i][j] += 1e-7 after the decomposition of the unperturbed m fails copies at P = 63."""
    import halo2_svd041_amd as hs
    m = recipe(6, 6, 11)
    u, d, v, info = hs.svd_decompose(ctxs[63], m)
    hs.svd_witness(ctxs[63], m, u, v, d, 3)
    chk = ctxs[63].check_gates()
    assert chk["gate_failures"] == 0 and chk["copy_failures"] == 0 and chk["lookup_failures"] == 0, chk
    wrong = m.copy()
    wrong[2][3] += 1e-7
    hs.svd_witness(ctxs[63], wrong, u, v, d, 3)
    assert ctxs[63].check_gates()["copy_failures"] > 0


@pytest.mark.parametrize("name,panel", [("17x17", 8), ("70x33", 8), ("96x130", 8), ("33x70", 4), ("33x70", 1)])
def test_two_calls_give_the_same_bytes(ctxs, name, panel):
    import halo2_svd041_amd as hs
    m = CASES[CASE_IDS.index(name)][1]
    first = hs.svd_decompose(ctxs[63], m, panel=panel)
    second = hs.svd_decompose(ctxs[63], m, panel=panel)
    for x, y in zip(first[:3], second[:3]):
        assert x.tobytes() == y.tobytes()
    assert first[3] == second[3]
    N, M = m.shape
    es, eu = hs.err_calc(63, max(N, M), 100.0, 1e-10, 1e-10)
    r1, r2, r3 = residuals(m, *first[:3])
    assert first[3]["converged"] == 1 and r1 <= es / 10 and r2 <= eu / 10 and r3 <= eu / 10


def test_errors(ctxs):
    import torch
    import halo2_svd041_amd as hs
    from halo2_svd041_amd import _lib
    L = _lib.lib()
    ctx = ctxs[63]
    for bad in (np.nan, np.inf, -np.inf):
        for shape in ((5, 7), (7, 5)):
            m = recipe(*shape, 9)
            m[3, 4] = bad
            N, M = shape
            u, d, v = np.full((N, N), 7.0), np.full(min(N, M), 7.0), np.full((M, M), 7.0)
            rc = L.svdw_svd_decompose(ctx.handle, m.ctypes.data, N, M, 0, None, u.ctypes.data, d.ctypes.data,
                                      v.ctypes.data, None)
            assert rc == -1 and b"finite" in L.svdw_last_error()
            assert np.all(u == 7.0) and np.all(d == 7.0) and np.all(v == 7.0)
    tm = torch.from_numpy(recipe(5, 7, 9)).to("cuda:0")
    tm[1, 1] = float("nan")
    tu, td, tv = (torch.full(s, 7.0, dtype=torch.float64, device="cuda:0") for s in ((5, 5), (5,), (7, 7)))
    torch.cuda.synchronize()
    rc = L.svdw_svd_decompose(ctx.handle, tm.data_ptr(), 5, 7, 1, None, tu.data_ptr(), td.data_ptr(), tv.data_ptr(),
                              None)
    assert rc == -1 and b"finite" in L.svdw_last_error()
    assert bool((tu == 7.0).all()) and bool((td == 7.0).all()) and bool((tv == 7.0).all())
    with pytest.raises(hs.SvdwError) as e:
        hs.svd_decompose(ctx, recipe(5, 7, 9), panel=3)
    assert e.value.code == -2
    buf = torch.zeros(200, dtype=torch.float64, device="cuda:0")
    good = torch.from_numpy(recipe(5, 7, 9)).to("cuda:0")
    torch.cuda.synchronize()
    p = buf.data_ptr()
    info = _lib.SvdInfo()
    # v starts inside u; d inside v; u on m itself
    for up, dp, vp in ((p, p + 8 * 100, p + 8 * 24), (p, p + 8 * 30, p + 8 * 25), (good.data_ptr(), p, p + 8 * 8)):
        rc = L.svdw_svd_decompose(ctx.handle, good.data_ptr(), 5, 7, 1, None, up, dp, vp, ct.byref(info))
        assert rc == -1 and b"overlap" in L.svdw_last_error()
    # side by side is fine
    rc = L.svdw_svd_decompose(ctx.handle, good.data_ptr(), 5, 7, 1, None, p, p + 8 * 25, p + 8 * 30, ct.byref(info))
    assert rc == 0 and info.converged == 1
    # not converged within max_sweeps: SVDW_OK, converged = 0, the factors of the last sweep
    u, d, v, inf1 = hs.svd_decompose(ctx, recipe(33, 70, 203), max_sweeps=1)
    assert inf1["converged"] == 0 and inf1["sweeps"] == 1 and inf1["rotations"] > 0
    assert np.all(np.isfinite(u)) and np.all(np.isfinite(v)) and np.all(np.diff(d) <= 0)


@pytest.mark.parametrize("kind,N,M", [("zero", 320, 320), ("rank1", 320, 320), ("rank1", 300, 200), ("rank1", 200, 300)])
def test_completion_of_many_columns_is_quick(ctxs, kind, N, M):
    """Rank deficiency at a few hundred rows: R or R - 1 columns made by completion. With the search for a unit
    vector carried on from column to column a column costs 2 passes x 2 R flops per vector held and try,
    2 R^3 = 7e7 flops in all at R = 320 when every first try is taken: well under 0.1 s of host time. A search
    restarted at the first unit vector for every column costs R^4 / 3 and took 6.5 s at R = 256. The bound of 2 s
    on the whole call (a few sweeps on the device besides) separates the two."""
    import time
    import halo2_svd041_amd as hs
    rs = np.random.RandomState(N + M)
    m = np.zeros((N, M)) if kind == "zero" else np.outer(rs.uniform(-1, 1, N), rs.uniform(-1, 1, M)) * 3.0
    R = min(N, M)
    hs.svd_decompose(ctxs[63], np.eye(2))                      # (the library is loaded and warm)
    t0 = time.perf_counter()
    u, d, v, info = hs.svd_decompose(ctxs[63], m)
    took = time.perf_counter() - t0
    print(f"{kind} {N}x{M}: {info} {took:.3f} s")
    assert info["converged"] == 1 and info["completed"] == (R if kind == "zero" else R - 1), info
    es, eu = hs.err_calc(63, max(N, M), 100.0, 1e-10, 1e-10)
    r1, r2, r3 = residuals(m, u, d, v)
    assert r1 <= es / 10 and r2 <= eu / 10 and r3 <= eu / 10, (r1, r2, r3)
    assert np.all(d >= 0) and np.all(np.diff(d) <= 0)
    if kind == "zero":
        assert np.array_equal(u, np.eye(N)) and np.array_equal(v, np.eye(M))
    assert took <= 2.0, took


def test_pairs_are_counted(ctxs):
    """info.pairs = sweeps (P - 1) P / 2; skipped_pairs counts those whose solve made no rotation: every pair of
    the last sweep of a converged call at the least, and exactly the restatement's count where the two made the
    same rotations."""
    for name in ("17x17", "33x70", "zero4", "3I5"):
        _, m, b, inner, _, _ = CASES[CASE_IDS.index(name)]
        info = run(ctxs, name, False)[3]
        P = -(-max(m.shape) // 8)
        P += P & 1
        per_sweep = (P - 1) * (P // 2)
        assert info["pairs"] == info["sweeps"] * per_sweep
        assert per_sweep <= info["skipped_pairs"] <= info["pairs"]
        if info["rotations"] == 0:
            assert info["skipped_pairs"] == info["pairs"]
