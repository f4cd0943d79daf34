"""The opening calls without a device: the oracle (open_cases.py) pinned against
the definitions it restates, shplonk_queries against hand-written tables, and
the argument checks of the C ABI in the documented order as far as a planning
context reaches."""
import ctypes as ct

import pytest

import halo2_svd041_amd as hs
from halo2_svd041_amd import _lib
from halo2_svd041_amd.zk import shplonk_queries
from open_cases import (P_MOD, T_POINT, U, V, X_POINT, Y, circuit_sets, constant, divide, divide_by_set, divide_closed,
                        fold, folded, horner, identity1, identity2, interpolate, kernel_constant, omega, open_g,
                        open_h1, open_h2, poly_mul, poly_sub, rand_poly, remainders, set_weights, union, vanishing)

ENTRIES = ("svdw_open_quotient", "svdw_open_linearise", "svdw_check_open", "svdw_linear_combination")


def _instance(k: int = 5, unusable: int = 6, seed: int = 1):
    set_of, sets = circuit_sets(k, unusable, X_POINT)
    return [rand_poly(1 << k, seed + j) for j in range(len(set_of))], set_of, sets


# ------------------------------------------------------------ oracle pins
def test_successive_division_is_the_quotient_of_f_minus_r():
    polys, set_of, sets = _instance()
    for f, S, r in zip(folded(polys, set_of, len(sets), Y), sets, remainders(polys, set_of, sets, Y)):
        q = divide_by_set(f, S)
        assert all(c == 0 for c in q[len(f) - len(S):]) and any(q)
        assert poly_mul(q[:len(f) - len(S)], vanishing(S)) == poly_sub(f, r)   # F - r = Q Z_S, exactly
        assert all(horner(r, s) == horner(f, s) for s in S) and len(r) == len(S)


@pytest.mark.parametrize("s", [0, 1, P_MOD - 1, X_POINT])
def test_division_closed_form(s):
    a = rand_poly(37, 3)
    q, rem = divide(a, s)
    assert q == divide_closed(a, s) and q[-1] == 0
    assert rem == horner(a, s)
    assert poly_sub(poly_mul(q[:-1], [-s % P_MOD, 1]), a) == [-rem % P_MOD] + [0] * 36


@pytest.mark.parametrize("k", [3, 5])
def test_h1_times_z_t_is_the_folded_numerator(k):
    polys, set_of, sets = _instance(k, 3)
    T = union(sets)
    assert len(T) == 6 and len(sets) == 5                  # x, x w, x w^2, x w^3, x w^usable, x w^-1
    h1 = open_h1(polys, set_of, sets, Y, V)
    F, R = folded(polys, set_of, len(sets), Y), remainders(polys, set_of, sets, Y)
    num = [0]
    for f, S, r in zip(F, sets, R):
        term = poly_mul(vanishing([t for t in T if t not in S]), poly_sub(f, r))
        num = poly_sub([c * V % P_MOD for c in num], [-c % P_MOD for c in term])
    assert poly_sub(poly_mul(h1, vanishing(T)), num) == [0] * (len(h1) + len(T))
    lhs, rhs = identity1(polys, set_of, sets, Y, V, h1, T_POINT)
    assert lhs == rhs != 0


def test_g_at_u_is_the_constant():
    polys, set_of, sets = _instance()
    h1 = open_h1(polys, set_of, sets, Y, V)
    h2, rem = open_h2(polys, set_of, sets, Y, V, U, h1)
    assert rem == constant(polys, set_of, sets, Y, V, U) != 0
    assert rem == horner(open_g(polys, set_of, sets, Y, V, U, h1), U) and h2[-1] == 0
    assert set_weights(sets, U)[0] == 1
    lhs, rhs = identity2(polys, set_of, sets, Y, V, U, h1, h2, T_POINT)
    assert lhs == rhs != 0
    # a tampered h1 moves the remainder off the constant, a tampered h2 breaks identity 2 alone
    bad = list(h1)
    bad[3] = (bad[3] + 1) % P_MOD
    assert open_h2(polys, set_of, sets, Y, V, U, bad)[1] != rem
    lhs, rhs = identity1(polys, set_of, sets, Y, V, bad, T_POINT)
    assert lhs != rhs
    bad2 = list(h2)
    bad2[0] = (bad2[0] + 1) % P_MOD
    lhs, rhs = identity2(polys, set_of, sets, Y, V, U, h1, bad2, T_POINT)
    assert lhs != rhs


def test_interpolation_and_fold():
    pts = [3, 5, 11, X_POINT]
    p = rand_poly(4, 9)
    assert interpolate(pts, [horner(p, s) for s in pts]) == p
    a, b, c = rand_poly(4, 1), rand_poly(4, 2), rand_poly(4, 3)
    assert fold([a, b, c], Y) == [(x * Y * Y + y_ * Y + z) % P_MOD for x, y_, z in zip(a, b, c)]


def test_kernel_constants():
    tile = kernel_constant("kOpenTile")
    assert tile == 1 << kernel_constant("kOpenLogTile") and kernel_constant("kOpenCarryCap") >= 1


# ------------------------------------------------------------ shplonk_queries
def _points(k, x, rots):
    w = omega(k)
    return [x * pow(w, r, P_MOD) % P_MOD for r in rots]


def test_shplonk_queries_every_family():
    k, unusable, x = 5, 6, X_POINT
    set_of, sets = shplonk_queries(k, unusable, n_gate=2, n_perm=5, chunk_len=2, n_lookup=1, x=x)
    # advice x2, selectors x2, sigma x5, A, table, perm_z x3 (last {0, 1}), lookup_z, A', S', h
    assert set_of == [0, 0] + [1, 1] + [1] * 5 + [1] + [1] + [2, 2, 3] + [3] + [4] + [1] + [1]
    assert sets == [_points(k, x, r) for r in ((0, 1, 2, 3), (0,), (0, 1, 26), (0, 1), (0, 31))]
    assert hs.permutation_constants(k)[1] == omega(k)


def test_shplonk_queries_with_empty_families():
    k, x = 4, 7
    # no permutation: no {0, 1, usable}; the lookup Z opens {0, 1}
    set_of, sets = shplonk_queries(k, 3, n_gate=1, n_perm=0, chunk_len=0, n_lookup=2, x=x)
    assert set_of == [0] + [1] + [1, 1] + [1, 1] + [2, 2] + [3, 3] + [1, 1] + [1]
    assert sets == [_points(k, x, r) for r in ((0, 1, 2, 3), (0,), (0, 1), (0, 15))]
    # no gates and no lookups, one permutation set: {0} first, then {0, 1}
    set_of, sets = shplonk_queries(k, 3, n_gate=0, n_perm=2, chunk_len=3, n_lookup=0, x=x)
    assert set_of == [0, 0] + [1] + [0]
    assert sets == [_points(k, x, r) for r in ((0,), (0, 1))]
    # nothing but h
    assert shplonk_queries(k, 3, 0, 0, 0, 0, x) == ([0], [[x]])
    # gates only
    set_of, sets = shplonk_queries(k, 3, 3, 0, 0, 0, x)
    assert set_of == [0, 0, 0, 1, 1, 1, 1] and [len(s) for s in sets] == [4, 1]
    with pytest.raises(hs.SvdwError):
        shplonk_queries(k, 0, 1, 0, 0, 0, x)
    with pytest.raises(hs.SvdwError):
        shplonk_queries(k, 3, 1, 2, 0, 0, x)
    with pytest.raises(hs.SvdwError):
        shplonk_queries(k, 3, 1, 0, 0, 0, P_MOD)


# ------------------------------------------------------------ the ABI
def test_binding_declares_the_entries():
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
    assert ct.sizeof(_lib.OpenResult) == 56 and ct.sizeof(_lib.OpenCheck) == 5 * 32 + 6 * 8
    assert _lib.lib().svdw_abi_version() == 2


def _words(x: int):
    return (ct.c_uint64 * 4)(*[(x >> (64 * i)) & ((1 << 64) - 1) for i in range(4)])


def _call_all(ctx, k=4, form=0, ncols=2, set_of=(0, 1), sets=((3, 5), (7,)), npoints=None, nsets=None, y=Y, v=V, u=U,
              t=T_POINT):
    """The three opening entries with one argument list; null columns and outputs
    (they are looked at last)."""
    L = _lib.lib()
    nsets = len(sets) if nsets is None else nsets
    so = (ct.c_uint32 * max(len(set_of), 1))(*set_of)
    npts = (ct.c_uint32 * max(len(sets), 1))(*(npoints or [len(s) for s in sets]))
    pts = (ct.c_uint64 * max(32 * len(sets), 1))()
    for i, s in enumerate(sets):
        for q, x in enumerate(s[:8]):
            pts[32 * i + 4 * q:32 * i + 4 * q + 4] = list(_words(x))
    r, c = _lib.OpenResult(), _lib.OpenCheck()
    common = (ctx._h, k, form, None, ncols, so, pts, npts, nsets, _words(y), _words(v))
    return [L.svdw_open_quotient(*common, None, ct.byref(r)),
            L.svdw_open_linearise(*common, _words(u), None, None, ct.byref(r)),
            L.svdw_check_open(*common, _words(u), None, None, _words(t), None, ct.byref(c))]


def test_argument_checks_come_in_the_documented_order():
    """Each call breaks one rule and every rule after it that a planning context
    reaches; the code and the message are those of the first rule broken."""
    err = lambda: _lib.lib().svdw_last_error().decode()
    EINVAL, ERANGE = -1, -2
    with hs.Context(device=-1, precision_bits=32, lookup_bits=8) as ctx:
        # 1. form
        assert _call_all(ctx, k=29, form=7, y=P_MOD) == [EINVAL] * 3
        assert "form" in err()
        # 2. the challenges, then the points, duplicates, set_of, an empty set, u in T
        assert _call_all(ctx, k=29, y=P_MOD, sets=((3, 3), (P_MOD,))) == [EINVAL] * 3
        assert ">= p" in err() and "point" not in err()
        assert _call_all(ctx, k=29, v=P_MOD + 1) == [EINVAL] * 3
        assert _call_all(ctx, k=29, u=P_MOD)[1:] == [EINVAL] * 2
        assert _call_all(ctx, k=29, t=P_MOD)[2] == EINVAL
        assert _call_all(ctx, k=29, sets=((3, 3), (P_MOD,)), set_of=(0, 2)) == [EINVAL] * 3
        assert "a point >= p" in err()
        assert _call_all(ctx, k=29, sets=((3, 5, 3), (7,)), set_of=(0, 2)) == [EINVAL] * 3
        assert "equal points" in err()
        assert _call_all(ctx, k=29, set_of=(0, 2), sets=((3, 5), (7,), (9,)), nsets=2) == [EINVAL] * 3
        assert "set_of" in err()
        assert _call_all(ctx, k=29, set_of=(0, 0), u=5) == [EINVAL] * 3
        assert "without a polynomial" in err()
        assert _call_all(ctx, k=29, u=7)[1:] == [EINVAL] * 2
        assert "u is one of the points" in err()
        assert _call_all(ctx, k=29, u=7)[0] == ERANGE      # the first call takes no u
        # 3. k outside 1..28
        for k in (0, 29):
            assert _call_all(ctx, k=k, ncols=70000, set_of=(0, 1) * 35000) == [ERANGE] * 3
            assert "k must be" in err()
        # 4. a planning context, with and without columns
        assert _call_all(ctx, ncols=70000, set_of=(0, 1) * 35000) == [EINVAL] * 3
        assert "device context" in err()
        assert _call_all(ctx, ncols=0, set_of=(), sets=(), nsets=0) == [EINVAL] * 3
        assert "device context" in err()
        # a null result comes before everything
        L = _lib.lib()
        assert L.svdw_open_quotient(ctx._h, 29, 7, None, 1, None, None, None, 0, None, None, None, None) == EINVAL
        # svdw_linear_combination: form, a scalar >= p, k, the planning context
        sc = (ct.c_uint64 * 8)(*list(_words(P_MOD)), *list(_words(1)))
        assert L.svdw_linear_combination(ctx._h, 29, 7, None, 2, sc, None) == EINVAL
        assert "form" in err()
        assert L.svdw_linear_combination(ctx._h, 29, 1, None, 2, sc, None) == EINVAL
        assert "scalar >= p" in err()
        ok = (ct.c_uint64 * 8)(*list(_words(P_MOD - 1)), *list(_words(1)))
        assert L.svdw_linear_combination(ctx._h, 29, 1, None, 2, ok, None) == ERANGE
        assert "k must be" in err()
        assert L.svdw_linear_combination(ctx._h, 28, 1, None, 2, ok, None) == EINVAL
        assert "device context" in err()
        assert L.svdw_linear_combination(ctx._h, 28, 1, None, 0, None, None) == EINVAL
        assert "device context" in err()
