"""The restatement of svdw_svd_decompose (svd_decompose_cases.restate) on its
own, without a GPU: it shows that the shared inputs stay inside the caps the
GPU test imposes, and checks the binding's argument errors on a planning
context.

Sweeps the restatement needs on the shared inputs (default panel 8, inner 2
unless the case says otherwise): 1 for 1x1, the zero matrix and 3 I_5; 2 for
1x5, 5x1, rank 1, all ones and the orthogonal 12x12; 3 for 2x3; 5 for 16x16;
6 for 17x17 and the graded 13x13; 10 for 33x70, 70x33 and 64x64 at b = 4, 8;
11 for 64x64 at b = 1 and for 96x130; 12 for 130x96, the most. The tests
assert <= 20, half the default cap of 40.
"""
import ctypes as ct

import numpy as np
import pytest

import pyoracle as po
import halo2_svd041_amd as hs
from halo2_svd041_amd import _lib
from svd_decompose_cases import CASES, CASE_IDS, EPS, recipe, residuals, restate, restated


@pytest.mark.parametrize("name", CASE_IDS)
def test_restatement_converges_and_factors(name):
    _, m, b, inner, completed, _ = CASES[CASE_IDS.index(name)]
    u, d, v, info = restated(name)
    N, M = m.shape
    assert info["converged"] == 1 and info["sweeps"] <= 20, info
    assert info["completed"] == completed
    assert u.shape == (N, N) and v.shape == (M, M) and d.shape == (min(N, M),)
    assert np.all(np.isfinite(u)) and np.all(np.isfinite(v)) and np.all(np.isfinite(d))
    assert np.all(d >= 0) and np.all(np.diff(d) <= 0)
    ref = np.linalg.svd(m, compute_uv=False)
    assert completed == int(np.sum(ref <= max(N, M) * EPS * ref[0]))
    es, eu = hs.err_calc(63, max(N, M), 100.0, 1e-10, 1e-10)
    r1, r2, r3 = residuals(m, u, d, v)
    assert r1 <= es / 10 and r2 <= eu / 10 and r3 <= eu / 10, (r1, r2, r3)


def test_completion_cost_grows_with_the_cube():
    """complete() carries its search on from column to column: on an empty 200 x 200 factor every first try is
    taken (200 tries for 200 columns) and the result is the identity."""
    import svd_decompose_cases as sc
    Q = np.zeros((200, 200))
    sc.complete(Q, list(range(200)))
    assert np.array_equal(Q, np.eye(200))
    rs = np.random.RandomState(1)
    q0 = rs.standard_normal(60)
    Q = np.zeros((60, 60))
    Q[:, 0] = q0 / np.linalg.norm(q0)
    sc.complete(Q, list(range(1, 60)))
    assert np.max(np.abs(Q.T @ Q - np.eye(60))) <= 1e-14


def test_zero_matrix_gives_identities():
    u, d, v, info = restated("zero4")
    assert np.array_equal(u, np.eye(4)) and np.array_equal(v, np.eye(4)) and np.array_equal(d, np.zeros(4))


@pytest.mark.parametrize("N,M", [(1, 1), (1, 5), (5, 1), (2, 3), (6, 5), (5, 8), (7, 7), (12, 12)])
@pytest.mark.parametrize("P", [32, 63])
def test_restated_factors_satisfy_the_circuit(N, M, P):
    m = recipe(N, M, 100 + N + M)
    u, d, v, info = restate(m)
    assert info["converged"] == 1 and info["completed"] == 0
    w = po.svd_witness(m.tolist(), u.tolist(), v.tolist(), d.tolist(), P, 19, gamma=7)
    assert po.check_constraints(w.ctx0, 19) == []
    assert po.check_constraints(w.ctx1, 19) == []


def test_argument_errors_on_a_planning_context():
    L = _lib.lib()
    ctx = hs.Context(device=-1, precision_bits=63, lookup_bits=19)
    m, u, d, v = np.ones((3, 4)), np.empty((3, 3)), np.empty(3), np.empty((4, 4))
    info = _lib.SvdInfo()

    def call(mm, N, M, uu, dd, vv, opts=None, handle=None):
        p = [x.ctypes.data if x is not None else None for x in (mm, uu, dd, vv)]
        return L.svdw_svd_decompose(ctx.handle if handle is None else handle, p[0], N, M, 0, opts, p[1], p[2], p[3],
                                    ct.byref(info))
    try:
        assert call(m, 0, 4, u, d, v) == -1 and call(m, 3, 0, u, d, v) == -1
        assert b"empty" in L.svdw_last_error()
        for args in ((None, 3, 4, u, d, v), (m, 3, 4, None, d, v), (m, 3, 4, u, None, v), (m, 3, 4, u, d, None)):
            assert call(*args) == -1
            assert b"null" in L.svdw_last_error()
        big = np.empty(64)
        assert call(m, 3, 4, m[:, :3], d, v) == -1                       # u inside m
        assert b"overlaps m" in L.svdw_last_error()
        assert call(m, 3, 4, big[:9], big[8:11], v) == -1                # d starts on u's last element
        assert b"overlap each other" in L.svdw_last_error()
        assert call(m, 3, 4, big[:9], big[9:12], big[12:28]) == -1       # adjacent is no overlap: refused as dry
        assert b"device context" in L.svdw_last_error()
        assert call(m, 3, 4, u, d, v, ct.byref(_lib.SvdOpts(3, 0, 0))) == -2
        assert b"panel" in L.svdw_last_error()
        for ok in (0, 1, 4, 8):                                          # then the planning context is refused
            assert call(m, 3, 4, u, d, v, ct.byref(_lib.SvdOpts(ok, 0, 0))) == -1
            assert b"device context" in L.svdw_last_error()
        with pytest.raises(hs.SvdwError) as e:
            hs.svd_decompose(ctx, m)
        assert e.value.code == -1
        with pytest.raises(hs.SvdwError) as e:
            hs.svd_decompose(ctx, m, panel=3)
        assert e.value.code == -2
    finally:
        ctx.close()
    assert L.svdw_abi_version() == 2
