"""The assigned-witness calls (csrc/circuit.cpp) stage in the same scratch as the
prover calls (csrc/prover.cpp): the two families in turn on one context."""
from __future__ import annotations

import pytest

from conftest import gamma_for, gen_svd_input

# A 6 x 6 witness at P = 42 with physical_layout(k = 9, minimum_rows = 19). At
# k = 8 this witness needs 42 advice columns where num_advice is 41
# (svdw_assign_columns refuses), and no 2^lookup_bits table (lookup_bits >= 8)
# fits the 2^8 - 6 usable rows svdw_lookup_permute has there; k = 9 is the
# smallest k at which all eight calls run.
N, P, LB, K, MIN_ROWS, UNUSABLE = 6, 42, 8, 9, 19, 6


def _same(got, want):
    import torch
    if isinstance(want, (tuple, list)):
        return len(got) == len(want) and all(_same(g, w) for g, w in zip(got, want))
    return torch.equal(got, want) if torch.is_tensor(want) else got == want


@pytest.mark.gpu
def test_circuit_and_prover_calls_share_one_context(gpu_ctx_factory):
    """check_gates, assign_columns, lookup_permute, check_equalities on the
    physical columns, permutation_edges, assign_fixed, check_physical and
    check_gates again on one context: every result dict and output tensor equals,
    byte for byte, what the same call returns on a fresh context that ran only
    that call's prerequisites, and the second check_gates equals the first."""
    import halo2_svd041_amd as hs
    m, u, d, v = gen_svd_input(N, N, seed=66)

    def fresh(layout=True):
        c = gpu_ctx_factory(P, LB)
        hs.svd_witness(c, m, u, v, d, gamma_for(K))
        if layout:
            c.physical_layout(K, MIN_ROWS)
        return c

    ctx = fresh()
    gates = ctx.check_gates()
    cols = [ctx.assign_columns(ph) for ph in (0, 1)]
    permuted = ctx.lookup_permute(0, UNUSABLE)
    adv = [c[0] for c in cols]
    eq = [ctx.check_equalities(ph, adv[0], adv[1]) for ph in (0, 1)]
    edges = ctx.permutation_edges()
    fixed = ctx.assign_fixed()
    phys = [ctx.check_physical(ph, cols[ph][0], cols[ph][1]) for ph in (0, 1)]
    gates2 = ctx.check_gates()

    assert gates2 == gates
    assert gates["gates_checked"] and gates["copies_checked"] and gates["lookups_checked"]
    assert gates["gate_failures"] == gates["copy_failures"] == gates["lookup_failures"] == 0
    assert _same(gates, fresh(layout=False).check_gates())
    want_cols = [fresh().assign_columns(ph) for ph in (0, 1)]
    assert _same(cols, want_cols)
    assert permuted[2]["out_of_table"] == 0 and permuted[2]["columns"] == len(cols[0][2]) > 0
    assert _same(permuted, fresh().lookup_permute(0, UNUSABLE))
    want_adv = [c[0] for c in want_cols]
    for ph in (0, 1):
        assert eq[ph]["copies_checked"] and eq[ph]["consts_checked"]
        assert eq[ph]["copy_failures"] == eq[ph]["const_failures"] == 0
        assert _same(eq[ph], fresh().check_equalities(ph, want_adv[0], want_adv[1]))
        assert phys[ph]["gates_checked"] and phys[ph]["gate_failures"] == phys[ph]["copy_failures"] == 0
        assert _same(phys[ph], fresh().check_physical(ph, want_cols[ph][0], want_cols[ph][1]))
    other = fresh()
    assert edges[1]["edges"] == len(edges[0]) > 0 and _same(edges, other.permutation_edges())
    assert fixed.any() and _same(fixed, other.assign_fixed())
