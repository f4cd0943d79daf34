"""Lookup argument without a GPU: the literal restatement of halo2's
permute_expression_pair (lookup_perm_cases.py) satisfies the argument's own
adjacency and multiset conditions on the synthetic columns and on the oracle's
lookup columns of a 4x4 witness, and the three C entries exist, keep the ABI
version and reject a planning context and a missing physical layout."""
import ctypes as ct

import pytest

import halo2_svd041_amd as hs
import pyoracle as po
from halo2_svd041_amd import _lib
from halo2_svd041_amd._lib import LookupCheck, LookupResult
from conftest import gamma_for, gen_svd_input
from lookup_perm_cases import (MINIMUM_ROWS, WITNESS_CASES, argument_holds, lookup_columns,
                               permute_expression_pair, synthetic_columns, table_column)

ENTRIES = ("svdw_lookup_multiplicities", "svdw_lookup_permute", "svdw_check_lookup_argument")


@pytest.mark.parametrize("LB,k,unusable", [(8, 9, 20), (8, 10, 20), (3, 4, 2)])
def test_restatement_satisfies_the_argument_on_synthetic_columns(LB, k, unusable):
    rows = 1 << k
    usable = rows - unusable
    table = table_column(LB, rows)
    for name, col in synthetic_columns(LB, k, unusable).items():
        a, s = permute_expression_pair(col, table, usable)
        argument_holds(col, table, a, s, usable)
        assert a == sorted(col[:usable]), name


def test_restatement_hands_leftovers_out_in_descending_row_order():
    """usable = 8, LB = 2: A' = [0 0 0 1 1 3 3 3]; table {0 x5, 1, 2, 3}; the
    leftovers 0 0 0 0 2 ascending go to the repeated rows 7 6 4 2 1."""
    a, s = permute_expression_pair([3, 0, 1, 3, 0, 1, 0, 3], table_column(2, 8), 8)
    assert a == [0, 0, 0, 1, 1, 3, 3, 3]
    assert s == [0, 2, 0, 1, 0, 3, 0, 0]


def test_restatement_rejects_a_value_outside_the_table():
    with pytest.raises(ValueError):
        permute_expression_pair([0, 1, 4, 0, 0, 0, 0, 0], table_column(2, 8), 8)


@pytest.mark.parametrize("unusable", [6, 20])
def test_restatement_satisfies_the_argument_on_a_witness(unusable):
    N, M, P, LB, k, ncells, ncols = WITNESS_CASES[0]
    m, u, d, v = gen_svd_input(N, M, seed=N + M + P)
    w = po.svd_witness(m.tolist(), u.tolist(), v.tolist(), d.tolist(), P, LB, gamma=gamma_for(1))
    vals = [int(x) for x in w.ctx0.lookups]
    assert len(vals) == ncells
    cols = lookup_columns(vals, k)
    assert len(cols) == ncols
    assert cols == [c + [0] * ((1 << k) - len(c))
                    for c in po.physical_layout(w.ctx0, k, MINIMUM_ROWS).lookup_columns]
    assert len(vals) - (ncols - 1) * ((1 << k) - MINIMUM_ROWS) == 403
    assert 0 not in vals[(ncols - 1) * ((1 << k) - MINIMUM_ROWS):]
    rows = 1 << k
    table = table_column(LB, rows)
    for col in cols:
        a, s = permute_expression_pair(col, table, rows - unusable)
        argument_holds(col, table, a, s, rows - unusable)


def test_symbols_and_abi_version():
    L = _lib.lib()
    for name in ENTRIES:
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES
    assert L.svdw_abi_version() == 2


def _call_all(ctx, ncols=1):
    """Return codes of the three entries on ctx (null device pointers: the
    argument checks come first)."""
    L = _lib.lib()
    r, c = LookupResult(), LookupCheck()
    return [L.svdw_lookup_multiplicities(ctx._h, 0, 6, None, ncols, None),
            L.svdw_lookup_permute(ctx._h, 0, 6, 0, None, ncols, None, None, ct.byref(r)),
            L.svdw_check_lookup_argument(ctx._h, 0, 6, 0, None, ncols, None, None, ct.byref(c))]


def test_planning_context_is_rejected():
    N, M, P, LB, k, _, ncols = WITNESS_CASES[0]
    m, u, d, v = gen_svd_input(N, M, seed=N + M + P)
    with hs.Context(device=-1, precision_bits=P, lookup_bits=LB) as ctx:
        hs.svd_witness(ctx, m, u, v, d, gamma_for(1))
        assert _call_all(ctx, ncols) == [-1, -1, -1]        # before svdw_physical_layout
        p = ctx.physical_layout(k, MINIMUM_ROWS)
        assert p["num_lookup_advice"][0] == ncols
        assert _call_all(ctx, ncols) == [-1, -1, -1]        # SVDW_EINVAL after it too
        assert "device context" in _lib.lib().svdw_last_error().decode()


def test_python_calls_need_a_layout():
    with hs.Context(device=-1, precision_bits=32, lookup_bits=8) as ctx:
        with pytest.raises(RuntimeError):
            ctx.lookup_multiplicities(0)
        with pytest.raises(RuntimeError):
            ctx.lookup_permute(0)
