"""svdw_lookup_product / svdw_check_lookup_product on the device against the
literal restatement of halo2's lookup grand product (lookup_product_cases.py;
parity of the rule itself unpinned): witness lookup columns and the
degenerate synthetic columns byte for byte in both forms and with both pairs of
challenges, columns of several tiles, inv0 on zero denominators, the checker
against tampered columns, and one mid-size run checked by the device checker
alone. A' and S' come from svdw_lookup_permute in the same form."""
import numpy as np
import pytest

from conftest import gamma_for, gen_svd_input
from lookup_perm_cases import (MINIMUM_ROWS, WITNESS_CASES, cell_values, cells, lookup_columns,
                               permute_expression_pair, synthetic_columns, table_column)
from lookup_product_cases import CHALLENGES, P_MOD, grand_product, recurrence_holds

pytestmark = pytest.mark.gpu

SENTINEL = 0xAB
FORMS = ("canonical", "montgomery")
_witnesses = {}


def _witness(gpu_ctx_factory, case):
    """(ctx, layout, lookup columns as value lists) of a witness case, made once."""
    if case not in _witnesses:
        import halo2_svd041_amd as hs
        N, M, P, LB, k, ncells, ncols = case
        m, u, d, v = gen_svd_input(N, M, seed=N + M + P)
        ctx = gpu_ctx_factory(P, LB)
        hs.svd_witness(ctx, m, u, v, d, gamma_for(1))
        p = ctx.physical_layout(k, MINIMUM_ROWS)
        vals = cell_values(ctx.lookups(0).view(np.uint8))
        assert len(vals) == ncells and p["num_lookup_advice"] == [ncols, 0]
        _witnesses[case] = (ctx, p, lookup_columns(vals, k))
    return _witnesses[case]


def _synthetic_ctx(gpu_ctx_factory, LB, k):
    """A context without a witness: the columns come in through columns=."""
    ctx = gpu_ctx_factory(32, LB)
    ctx.physical_layout(k, MINIMUM_ROWS)
    return ctx


def _restated(cols, LB, k, unusable, beta, gamma):
    """Per column (Z as [2^k, 32] u8 canonical cells, zero denominators, Z[usable],
    rows that break the recurrence), with A', S' of the restated permute."""
    rows = 1 << k
    usable = rows - unusable
    T = table_column(LB, rows)
    out = []
    for col in cols:
        a, s = permute_expression_pair(col, T, usable)
        z, zeros = grand_product(col, T, a, s, beta, gamma, usable, rows)
        broken = len(recurrence_holds(col, T, a, s, z, beta, gamma, usable, rows))
        out.append((cells(z, rows), zeros, z[usable], broken))
    return out


def _canonical(t, form):
    """[n, rows, 32] u8 device tensor in `form` -> canonical numpy cells (svdw_fr_convert)."""
    import halo2_svd041_amd as hs
    a = t.cpu().numpy()
    if form == "montgomery" and a.size:
        a = hs.fr_convert(a.view("<u8").reshape(-1, 4), "montgomery", "canonical").view(np.uint8).reshape(a.shape)
    return a


def _device_columns(cols, rows):
    import torch
    return torch.from_numpy(np.stack([cells(c, rows) for c in cols])).cuda()


def _prefilled(n, rows):
    import torch
    return torch.full((n, rows, 32), SENTINEL, dtype=torch.uint8, device="cuda")


def _clean(ncols, k, unusable):
    rows = 1 << k
    return {"recurrence_checked": ncols * (rows - unusable), "recurrence_failures": 0,
            "boundary_checked": 2 * ncols, "boundary_failures": 0,
            "padding_checked": ncols * (unusable - 1), "padding_failures": 0}


def _run(ctx, cols, LB, k, unusable, pairs, columns, honest=True):
    """The product of `cols` (value lists; `columns`: a list of the columns=
    arguments that must all give the same Z) in both forms against the
    restatement, for each (beta, gamma) of `pairs`."""
    import torch
    rows, ncols = 1 << k, len(cols)
    for beta, gamma in pairs:
        want = _restated(cols, LB, k, unusable, beta, gamma)
        zeros = sum(w[1] for w in want)
        not_one = sum(w[2] != 1 for w in want)
        broken = sum(w[3] for w in want)
        if honest:
            assert zeros == 0 and not_one == 0 and broken == 0
        for form in FORMS:
            first = None
            for dev in columns:
                a, s, r = ctx.lookup_permute(0, unusable, form, columns=dev)
                assert r["out_of_table"] == 0
                z, res = ctx.lookup_product(0, a, s, beta, gamma, unusable, form, columns=dev,
                                            out=_prefilled(ncols, rows))
                assert res == {"columns": ncols, "usable_rows": rows - unusable, "zero_denominators": zeros,
                               "final_not_one": not_one}, (form, res)
                if first is None:
                    first = z
                    cz = _canonical(z, form)
                    for c in range(ncols):
                        assert np.array_equal(cz[c], want[c][0]), (form, c, hex(beta), hex(gamma))
                else:
                    assert torch.equal(z, first)
                chk = ctx.check_lookup_product(0, a, s, z, beta, gamma, unusable, form, columns=dev)
                # Z[usable] == 0 is legal; a zero denominator breaks the recurrence in
                # its row unless Z or the numerator is zero there too
                assert chk == dict(_clean(ncols, k, unusable), recurrence_failures=broken), (form, chk)


@pytest.mark.parametrize("unusable", [6, 20])
@pytest.mark.parametrize("case", WITNESS_CASES, ids=lambda c: f"{c[0]}x{c[1]}-P{c[2]}-LB{c[3]}-k{c[4]}")
def test_witness_columns_match_restatement(gpu_ctx_factory, case, unusable):
    N, M, P, LB, k, ncells, ncols = case
    ctx, p, cols = _witness(gpu_ctx_factory, case)
    lk = ctx.assign_columns(0)[2]
    assert lk.shape == (ncols, 1 << k, 32)
    _run(ctx, cols, LB, k, unusable, CHALLENGES, [None, lk])


def test_synthetic_columns(gpu_ctx_factory):
    """LB = 8, k = 9, unusable_rows = minimum_rows: one run, all zeros, no zero at
    all, every value once, only the two hot bins, uniform."""
    LB, k = 8, 9
    ctx = _synthetic_ctx(gpu_ctx_factory, LB, k)
    cols = list(synthetic_columns(LB, k, MINIMUM_ROWS).values())
    _run(ctx, cols, LB, k, MINIMUM_ROWS, CHALLENGES, [_device_columns(cols, 1 << k)])


@pytest.mark.parametrize("unusable,pair", [(6, 0), (1, 1)])
def test_columns_of_several_tiles(gpu_ctx_factory, unusable, pair):
    """k = 13: eight tiles of 1024 rows per column, so the carries cross tiles in
    both directions; unusable_rows = 1: Z[usable] is the last row, none is padding.
    Not the full cross product: the restatement takes over a second per column
    here, so unusable_rows = 6 runs with the plain pair of challenges only and
    unusable_rows = 1 with the top-bits pair only."""
    LB, k = 8, 13
    ctx = _synthetic_ctx(gpu_ctx_factory, LB, k)
    c = synthetic_columns(LB, k, unusable)
    cols = [c["uniform"], c["hot_bins"]]
    _run(ctx, cols, LB, k, unusable, [CHALLENGES[pair]], [_device_columns(cols, 1 << k)])


def test_inv0_on_zero_denominators(gpu_ctx_factory):
    """gamma = p - 3: S' + gamma is zero in the one row of each column that holds
    the table's 3. beta = p - 5: A' + beta is zero in every row of the column of
    fives, in a few rows of others. Z is zero from the row after the first such
    row on, as batch_invert leaves a zero zero."""
    LB, k, unusable = 8, 9, MINIMUM_ROWS
    ctx = _synthetic_ctx(gpu_ctx_factory, LB, k)
    named = synthetic_columns(LB, k, unusable)
    cols = list(named.values())
    assert list(named)[0] == "same_nonzero" and cols[0][0] == 5
    dev = [_device_columns(cols, 1 << k)]
    g3 = (CHALLENGES[0][0], P_MOD - 3)
    want = _restated(cols, LB, k, unusable, *g3)
    assert [w[1] for w in want] == [1] * len(cols) and all(w[2] != 1 for w in want)
    _run(ctx, cols, LB, k, unusable, [g3], dev, honest=False)
    b5 = (P_MOD - 5, CHALLENGES[0][1])
    want = _restated(cols, LB, k, unusable, *b5)
    assert want[0][1] == (1 << k) - unusable and want[1][1] == 0 and want[1][2] == 1
    _run(ctx, cols, LB, k, unusable, [b5], dev, honest=False)


@pytest.mark.parametrize("form", FORMS)
def test_checker_catches_tampering(gpu_ctx_factory, form):
    LB, k, unusable = 8, 10, MINIMUM_ROWS
    ctx = _synthetic_ctx(gpu_ctx_factory, LB, k)
    c = synthetic_columns(LB, k, unusable)
    cols = [c["uniform"], c["no_zero"]]
    rows = 1 << k
    usable = rows - unusable
    dev = _device_columns(cols, rows)
    beta, gamma = CHALLENGES[1]
    a, s, r = ctx.lookup_permute(0, unusable, form, columns=dev)
    z, res = ctx.lookup_product(0, a, s, beta, gamma, unusable, form, columns=dev)
    assert res["final_not_one"] == 0 and res["zero_denominators"] == 0
    assert ctx.check_lookup_product(0, a, s, z, beta, gamma, unusable, form, columns=dev) == _clean(2, k, unusable)
    # cells are bytes: a tensor of the same shape and another dtype is refused
    import torch
    import halo2_svd041_amd as hs
    for bad in ((a.view(torch.int8), s, z), (a, s.view(torch.int8), z), (a, s, z.view(torch.int8))):
        with pytest.raises(hs.SvdwError):
            ctx.check_lookup_product(0, bad[0], bad[1], bad[2], beta, gamma, unusable, form, columns=dev)
        with pytest.raises(hs.SvdwError):
            ctx.lookup_product(0, bad[0], bad[1], beta, gamma, unusable, form, columns=dev, out=bad[2])
    # one S' cell changed: that column's product no longer closes; its Z obeys
    # the recurrence row by row, only Z[usable] tells
    s2 = s.clone()
    s2[1, 300, 0] ^= 1
    z2, res = ctx.lookup_product(0, a, s2, beta, gamma, unusable, form, columns=dev)
    assert res["final_not_one"] == 1 and res["zero_denominators"] == 0
    chk = ctx.check_lookup_product(0, a, s2, z2, beta, gamma, unusable, form, columns=dev)
    assert chk == dict(_clean(2, k, unusable), boundary_failures=1), chk
    # the honest Z against the tampered S': the row of the changed cell
    chk = ctx.check_lookup_product(0, a, s2, z, beta, gamma, unusable, form, columns=dev)
    assert chk == dict(_clean(2, k, unusable), recurrence_failures=1), chk
    # one Z cell in the middle changed: the rows r - 1 and r, no others
    row = 517
    z3 = z.clone()
    z3[0, row, 0] ^= 1
    chk = ctx.check_lookup_product(0, a, s, z3, beta, gamma, unusable, form, columns=dev)
    assert chk == dict(_clean(2, k, unusable), recurrence_failures=2), chk
    T = table_column(LB, rows)
    ca, cs, cz = (cell_values(_canonical(t, form)[0]) for t in (a, s, z3))
    assert recurrence_holds(cols[0], T, ca, cs, cz, beta, gamma, usable, rows) == [row - 1, row]
    # Z[0] != 1
    z4 = z.clone()
    z4[1, 0, 31] ^= 1
    chk = ctx.check_lookup_product(0, a, s, z4, beta, gamma, unusable, form, columns=dev)
    assert chk == dict(_clean(2, k, unusable), recurrence_failures=1, boundary_failures=1), chk
    # a non-zero cell above usable
    z5 = z.clone()
    z5[0, rows - 1, 0] = 1
    chk = ctx.check_lookup_product(0, a, s, z5, beta, gamma, unusable, form, columns=dev)
    assert chk == dict(_clean(2, k, unusable), padding_failures=1), chk


def test_mid_size_run_checks_clean(gpu_ctx_factory):
    """48 x 48, P = 63, LB = 12 at k = 13, the smallest k whose usable rows hold
    the 2^LB table: a few dozen lookup columns of eight tiles, no host loop."""
    import halo2_svd041_amd as hs
    N, P, LB = 48, 63, 12
    k = LB + 1
    m, u, d, v = gen_svd_input(N, N, seed=N + N + P)
    ctx = gpu_ctx_factory(P, LB)
    hs.svd_witness(ctx, m, u, v, d, gamma_for(N))
    p = ctx.physical_layout(k, MINIMUM_ROWS)
    ncols = p["num_lookup_advice"][0]
    assert ncols >= 2
    beta, gamma = CHALLENGES[1]
    for form in FORMS:
        a, s, r = ctx.lookup_permute(0, 6, form)
        assert r["out_of_table"] == 0
        z, res = ctx.lookup_product(0, a, s, beta, gamma, 6, form)
        assert res == {"columns": ncols, "usable_rows": (1 << k) - 6, "zero_denominators": 0, "final_not_one": 0}
        assert ctx.check_lookup_product(0, a, s, z, beta, gamma, 6, form) == _clean(ncols, k, 6)


def test_runs_of_tiles_per_carry_thread(gpu_ctx_factory):
    """k = 21, LB = 8: 2048 tiles per column, so each of k_lp_carry's 256 threads
    multiplies, prefixes and suffixes a run of eight tile products, and
    k_lp_check's grid of 4096 blocks strides twice over the 2^21 rows. Two
    columns made on the device (uniform; half zeros and 255s), both forms,
    checked by the device checker alone: a wrong carry breaks the recurrence at
    a tile seam and Z[usable]. Then one S' cell changed in a high tile: that
    column no longer closes and its Z still obeys the recurrence; the rows up to
    the cell keep their bytes although the suffix products below it and the
    inverse all change, the rows above it do not."""
    import torch
    LB, k, unusable = 8, 21, 6
    rows = 1 << k
    usable = rows - unusable
    ctx = _synthetic_ctx(gpu_ctx_factory, LB, k)
    g = torch.Generator(device="cuda").manual_seed(821)
    vals = torch.randint(0, 1 << LB, (2, rows), generator=g, device="cuda")
    hot = torch.randint(0, 4, (rows,), generator=g, device="cuda")
    vals[1] = torch.where(hot == 0, 0, torch.where(hot == 1, 255, vals[1]))
    vals[:, usable:] = 0
    dev = torch.zeros((2, rows, 32), dtype=torch.uint8, device="cuda")
    dev[:, :, 0] = vals.to(torch.uint8)
    assert (rows // 1024) // 256 == 8 and rows > 4096 * 256
    clean = _clean(2, k, unusable)
    for form, (beta, gamma) in [(f, c) for f in FORMS for c in CHALLENGES]:
        a, s, r = ctx.lookup_permute(0, unusable, form, columns=dev)
        assert r["out_of_table"] == 0
        z, res = ctx.lookup_product(0, a, s, beta, gamma, unusable, form, columns=dev, out=_prefilled(2, rows))
        assert res == {"columns": 2, "usable_rows": usable, "zero_denominators": 0, "final_not_one": 0}, (form, res)
        assert ctx.check_lookup_product(0, a, s, z, beta, gamma, unusable, form, columns=dev) == clean, form
        row = 1901 * 1024 + 77                               # tile 1901: run 237 of the carry, its sixth tile
        s2 = s.clone()
        s2[0, row, 0] ^= 1
        z2, res = ctx.lookup_product(0, a, s2, beta, gamma, unusable, form, columns=dev)
        assert res["final_not_one"] == 1 and res["zero_denominators"] == 0, (form, res)
        chk = ctx.check_lookup_product(0, a, s2, z2, beta, gamma, unusable, form, columns=dev)
        assert chk == dict(clean, boundary_failures=1), (form, chk)
        assert torch.equal(z2[1], z[1])
        assert torch.equal(z2[0, :row + 1], z[0, :row + 1])
        assert not bool((z2[0, row + 1:usable + 1] == z[0, row + 1:usable + 1]).all(dim=1).any())


def test_no_lookup_columns(gpu_ctx_factory):
    """Phase 1 of an SVD witness has no lookup cells: empty tensors, SVDW_OK."""
    case = WITNESS_CASES[0]
    ctx, p, cols = _witness(gpu_ctx_factory, case)
    rows = 1 << case[4]
    a, s, r = ctx.lookup_permute(1, 6)
    z, res = ctx.lookup_product(1, a, s, *CHALLENGES[0])
    assert z.shape == (0, rows, 32)
    assert res == {"columns": 0, "usable_rows": rows - 6, "zero_denominators": 0, "final_not_one": 0}
    assert set(ctx.check_lookup_product(1, a, s, z, *CHALLENGES[0]).values()) == {0}
