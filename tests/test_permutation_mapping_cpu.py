"""Sigma from the copy constraints without a GPU: the host restatement of the
rule (cycle_cases.py) against halo2's serial Assembly restated in
permutation_cases.py (the same classes, another order inside a cycle), its
independence of the edges' order, and the argument checks of
svdw_permutation_cycles / svdw_check_permutation_mapping as far as a planning
context reaches."""
import ctypes as ct

import numpy as np
import pytest

import halo2_svd041_amd as hs
from halo2_svd041_amd import _lib
from cycle_cases import (K, UNUSABLE, canonical_mapping, classes, cycles_of, chain_case, hub_case,
                         small_classes_case, summary)
from permutation_cases import Assembly, mapping_entries


def _random_edges(rs, ncols, k, unusable, n):
    usable = (1 << k) - unusable
    c = rs.randint(0, ncols, size=(n, 2)).astype(np.int64)
    r = rs.randint(0, usable, size=(n, 2)).astype(np.int64)
    return c << 32 | r


@pytest.mark.parametrize("ncols,k,unusable,n,seed", [(3, 4, 2, 12, 0), (4, 5, 6, 40, 1), (2, 6, 3, 90, 2),
                                                     (5, 5, 1, 200, 3)])
def test_classes_are_those_of_the_serial_merge(ncols, k, unusable, n, seed):
    """The cycles of canonical_mapping hold the cells of the cycles of halo2's
    Assembly::copy run over the same edges in order; each ascends with exactly
    one descent, from its largest cell back to its smallest."""
    rs = np.random.RandomState(seed)
    e = _random_edges(rs, ncols, k, unusable, n)
    asm = Assembly(ncols, 1 << k)
    for a, b in e.tolist():
        asm.copy((a >> 32, a & 0xFFFFFFFF), (b >> 32, b & 0xFFFFFFFF))
    got = canonical_mapping(e, ncols, k, unusable)
    mine = cycles_of(got)
    serial = cycles_of(mapping_entries(asm.mapping))
    assert sorted(sorted(c) for c in mine) == sorted(sorted(c) for c in serial) == classes(e, ncols, k, unusable)
    assert len(mine) >= 1
    for cyc in mine:
        assert cyc == sorted(cyc) and len(cyc) >= 2
        nxt = cyc[1:] + cyc[:1]
        assert sum(b < a for a, b in zip(cyc, nxt)) == 1
    rows = 1 << k
    pad = got[:, rows - unusable:]
    assert np.array_equal(pad, (np.arange(ncols)[:, None] << 32) | np.arange(rows - unusable, rows)[None, :])


@pytest.mark.parametrize("case", [chain_case, hub_case, small_classes_case])
def test_mapping_ignores_order_and_repetition(case):
    e, ncols = case()
    rs = np.random.RandomState(9)
    want = canonical_mapping(e, ncols, K, UNUSABLE)
    assert np.array_equal(canonical_mapping(e[::-1], ncols, K, UNUSABLE), want)
    assert np.array_equal(canonical_mapping(e[rs.permutation(e.shape[0])][:, ::-1], ncols, K, UNUSABLE), want)
    assert np.array_equal(canonical_mapping(np.concatenate([e, e[::3], e]), ncols, K, UNUSABLE), want)
    assert summary(e, ncols, K, UNUSABLE)["linked_cells"] == int((want != canonical_mapping(e[:0], ncols, K,
                                                                                              UNUSABLE)).sum())


@pytest.mark.parametrize("fn,res", [("svdw_permutation_cycles", _lib.PermutationCyclesResult),
                                    ("svdw_check_permutation_mapping", _lib.PermutationMappingCheck)])
def test_argument_checks_on_a_planning_context(fn, res):
    """In the header's order: null ctx or result (SVDW_EINVAL), k outside 1..28
    (SVDW_ERANGE), unusable_rows >= 2^k (SVDW_ERANGE), then the planning context
    itself (SVDW_EINVAL), whatever the later arguments are."""
    L = _lib.lib()
    f = getattr(L, fn)
    r = res()
    with hs.Context(device=-1, precision_bits=32, lookup_bits=8) as ctx:
        h = ctx.handle
        assert f(None, 10, 6, 3, None, 0, None, ct.byref(r)) == -1
        assert f(h, 10, 6, 3, None, 0, None, None) == -1
        for k in (0, 29, 64):
            assert f(h, k, 1 << 30, 1 << 20, None, 5, None, ct.byref(r)) == -2, k
            assert b"k must be in [1, 28]" in L.svdw_last_error()
        for k, unusable in ((1, 2), (10, 1024), (28, 1 << 28), (3, 0xFFFFFFFF)):
            assert f(h, k, unusable, 1 << 20, None, 5, None, ct.byref(r)) == -2, (k, unusable)
            assert b"unusable_rows" in L.svdw_last_error()
        assert f(h, 10, 6, 1 << 20, None, 5, None, ct.byref(r)) == -1
        assert b"needs a device context" in L.svdw_last_error()
        assert f(h, 10, 6, 0, None, 0, None, ct.byref(r)) == -1


W_K, W_MIN_ROWS, W_LB = 10, 20, 8


@pytest.mark.parametrize("N,M,P,prefix", [(5, 3, 63, 0), (6, 6, 42, 0), (6, 6, 42, 1)])
def test_edge_counts_on_a_planning_context(N, M, P, prefix):
    """svdw_permutation_edges without a list: copies + constants + breaks (+ 2
    with the rlc prefix) of svdw_equalities / svdw_break_points, split as the
    host rebuild of the list splits them."""
    from conftest import gamma_for, gen_svd_input
    from cycle_cases import witness_edges
    m, u, d, v = gen_svd_input(N, M, seed=N + M + P)
    with hs.Context(device=-1, precision_bits=P, lookup_bits=W_LB) as ctx:
        L = _lib.lib()
        lay = _lib.PermutationLayout()
        if prefix:
            ctx.set_option("rlc_prefix", 1)
        hs.svd_witness(ctx, m, u, v, d, gamma_for(W_K))
        assert L.svdw_permutation_edges(ctx.handle, None, 0, ct.byref(lay)) == -1      # no layout yet
        assert b"svdw_physical_layout" in L.svdw_last_error()
        phys = ctx.physical_layout(W_K, W_MIN_ROWS)
        got = ctx.permutation_layout()
        eqs = [ctx.equalities(ph) for ph in (0, 1)]
        breaks = sum(len(ctx.break_points(ph)) for ph in (0, 1))
        copies, consts = sum(len(e[0]) for e in eqs), sum(len(e[1]) for e in eqs)
        assert breaks >= 1 and copies > 100 and consts > 10
        assert got["edges"] == copies + consts + breaks + 2 * prefix
        assert got["constants"] == phys["constants"] and got["fixed"] == phys["num_fixed"] == 1
        assert got["advice"] == phys["columns_used"] and got["external"] == 1
        want_edges, want, _ = witness_edges(ctx, phys)
        assert got == want and want_edges.shape == (got["edges"], 2)
        # what a planning context refuses
        assert L.svdw_permutation_edges(ctx.handle, None, 0, None) == -1
        assert L.svdw_permutation_edges(ctx.handle, 4096, 1 << 30, ct.byref(lay)) == -1
        assert b"device context" in L.svdw_last_error()
        assert L.svdw_assign_fixed(ctx.handle, 7, None) == -1
        assert b"form" in L.svdw_last_error()
        assert L.svdw_assign_fixed(ctx.handle, 0, None) == -1
        assert b"device context" in L.svdw_last_error()
