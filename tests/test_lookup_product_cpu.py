"""Lookup grand product without a GPU: the literal restatement
(lookup_product_cases.py) closes (Z[usable] == 1, zeros above) on the restated
permuted columns of the synthetic columns and of the oracle's 4x4 witness, does
not close on a tampered S', and shows inv0 for a challenge that meets a table
value; the two C entries exist, keep the ABI version, and reject a planning
context, unusable_rows == 0, a challenge >= p and a missing physical layout."""
import ctypes as ct

import pytest

import halo2_svd041_amd as hs
import pyoracle as po
from halo2_svd041_amd import _lib
from halo2_svd041_amd._lib import LookupProductCheck, LookupProductResult
from conftest import gamma_for, gen_svd_input
from lookup_perm_cases import (MINIMUM_ROWS, WITNESS_CASES, lookup_columns, permute_expression_pair,
                               synthetic_columns, table_column)
from lookup_product_cases import CHALLENGES, P_MOD, grand_product, recurrence_holds

ENTRIES = ("svdw_lookup_product", "svdw_check_lookup_product")
SETS = [(8, 9, 20), (3, 4, 2), (3, 4, 1)]


def _witness_columns():
    N, M, P, LB, k, ncells, ncols = WITNESS_CASES[0]
    m, u, d, v = gen_svd_input(N, M, seed=N + M + P)
    w = po.svd_witness(m.tolist(), u.tolist(), v.tolist(), d.tolist(), P, LB, gamma=gamma_for(1))
    cols = lookup_columns([int(x) for x in w.ctx0.lookups], k)
    assert len(cols) == ncols
    return {f"witness{c}": col for c, col in enumerate(cols)}, LB, k


def _column_sets():
    """(name, columns, LB, k, unusable) of every set the restatement runs on."""
    out = [(f"LB{LB}-k{k}-u{un}", synthetic_columns(LB, k, un), LB, k, un) for LB, k, un in SETS]
    cols, LB, k = _witness_columns()
    return out + [("witness-u6", cols, LB, k, 6)]


@pytest.fixture(scope="module")
def column_sets():
    sets = []
    for name, cols, LB, k, un in _column_sets():
        rows = 1 << k
        T = table_column(LB, rows)
        perm = {n: permute_expression_pair(c, T, rows - un) for n, c in cols.items()}
        sets.append((name, cols, perm, T, rows, rows - un))
    return sets


@pytest.mark.parametrize("beta,gamma", CHALLENGES, ids=["plain", "top_bits"])
def test_restatement_closes_on_honest_columns(column_sets, beta, gamma):
    for name, cols, perm, T, rows, usable in column_sets:
        for n, A in cols.items():
            Ap, Sp = perm[n]
            Z, zeros = grand_product(A, T, Ap, Sp, beta, gamma, usable, rows)
            assert Z[0] == 1 and Z[usable] == 1 and zeros == 0, (name, n)
            assert not any(Z[usable + 1:]), (name, n)
            assert recurrence_holds(A, T, Ap, Sp, Z, beta, gamma, usable, rows) == [], (name, n)


def test_restatement_does_not_close_on_a_tampered_table_column(column_sets):
    beta, gamma = CHALLENGES[0]
    for name, cols, perm, T, rows, usable in column_sets:
        for n, A in cols.items():
            Ap, Sp = perm[n]
            Sp = list(Sp)
            Sp[usable // 2] = (Sp[usable // 2] + 1) % 8
            Z, zeros = grand_product(A, T, Ap, Sp, beta, gamma, usable, rows)
            assert Z[usable] not in (0, 1) and zeros == 0, (name, n)
            # the recurrence still holds row by row: only the boundary row tells
            assert recurrence_holds(A, T, Ap, Sp, Z, beta, gamma, usable, rows) == [], (name, n)


def test_restatement_inv0_zeroes_the_rows_after_a_zero_denominator(column_sets):
    """gamma = p - 3 and 3 is in every table: S' holds one 3 per column."""
    beta, gamma = CHALLENGES[0][0], P_MOD - 3
    for name, cols, perm, T, rows, usable in column_sets:
        for n, A in cols.items():
            Ap, Sp = perm[n]
            assert Sp.count(3) == 1, (name, n)
            r0 = Sp.index(3)
            Z, zeros = grand_product(A, T, Ap, Sp, beta, gamma, usable, rows)
            assert zeros == 1, (name, n)
            assert not any(Z[r0 + 1:]), (name, n)
            # T[3] + gamma is zero too: Z is already zero from row 4 on
            assert all(Z[:min(r0, 3) + 1]), (name, n)


def test_symbols_and_abi_version():
    L = _lib.lib()
    for name in ENTRIES:
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES
    assert L.svdw_abi_version() == 2


def _words(x):
    return (ct.c_uint64 * 4)(*[(x >> (64 * i)) & (2 ** 64 - 1) for i in range(4)])


def _call_both(ctx, ncols=1, unusable=6, beta=CHALLENGES[0][0], gamma=CHALLENGES[0][1]):
    """Return codes of the two entries on ctx (null device pointers: the
    argument checks come first)."""
    L = _lib.lib()
    r, c = LookupProductResult(), LookupProductCheck()
    b, g = _words(beta), _words(gamma)
    return [L.svdw_lookup_product(ctx._h, 0, unusable, 0, None, ncols, None, None, b, g, None, ct.byref(r)),
            L.svdw_check_lookup_product(ctx._h, 0, unusable, 0, None, ncols, None, None, b, g, None, ct.byref(c))]


def test_planning_context_and_bad_arguments_are_rejected():
    N, M, P, LB, k, _, ncols = WITNESS_CASES[0]
    m, u, d, v = gen_svd_input(N, M, seed=N + M + P)
    with hs.Context(device=-1, precision_bits=P, lookup_bits=LB) as ctx:
        hs.svd_witness(ctx, m, u, v, d, gamma_for(1))
        assert _call_both(ctx, ncols) == [-1, -1]           # before svdw_physical_layout
        p = ctx.physical_layout(k, MINIMUM_ROWS)
        assert p["num_lookup_advice"][0] == ncols
        assert _call_both(ctx, ncols) == [-1, -1]           # SVDW_EINVAL after it too
        assert "device context" in _lib.lib().svdw_last_error().decode()
        assert _call_both(ctx, ncols, unusable=0) == [-2, -2]
        assert "unusable_rows" in _lib.lib().svdw_last_error().decode()
        for beta, gamma in ((P_MOD, 5), (5, P_MOD), (2 ** 256 - 1, 5)):
            assert _call_both(ctx, ncols, beta=beta, gamma=gamma) == [-1, -1]
            assert ">= p" in _lib.lib().svdw_last_error().decode()
        for call in (lambda b, g: ctx.lookup_product(0, None, None, b, g),
                     lambda b, g: ctx.check_lookup_product(0, None, None, None, b, g)):
            for beta, gamma in ((P_MOD, 5), (5, -1)):
                with pytest.raises(hs.SvdwError) as e:
                    call(beta, gamma)
                assert e.value.code == -1


def test_python_calls_need_a_layout():
    with hs.Context(device=-1, precision_bits=32, lookup_bits=8) as ctx:
        with pytest.raises(RuntimeError):
            ctx.lookup_product(0, None, None, 1, 2)
        with pytest.raises(RuntimeError):
            ctx.check_lookup_product(0, None, None, None, 1, 2)
