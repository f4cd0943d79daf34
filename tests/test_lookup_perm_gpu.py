"""svdw_lookup_permute / svdw_lookup_multiplicities / svdw_check_lookup_argument on
the device against the literal restatement of halo2's permute_expression_pair
(lookup_perm_cases.py; parity of the rule itself unpinned): witness
lookup columns and degenerate synthetic columns byte for byte in both forms,
cells outside the table, the checker against tampered columns, and one mid-size
run checked by the device checker alone."""
import numpy as np
import pytest

from conftest import gamma_for, gen_svd_input
from lookup_perm_cases import (MINIMUM_ROWS, WITNESS_CASES, cell_values, cells, lookup_columns,
                               permute_expression_pair, synthetic_columns, table_column)

pytestmark = pytest.mark.gpu

SENTINEL = 0xAB
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


def _expected(cols, LB, k, unusable):
    """Per column (A', S') of the restatement as [2^k, 32] u8 cells, and the distinct count."""
    rows = 1 << k
    table = table_column(LB, rows)
    out, distinct = [], 0
    for col in cols:
        a, s = permute_expression_pair(col, table, rows - unusable)
        out.append((cells(a, rows), cells(s, rows)))
        distinct += len(set(a))
    return out, distinct


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


def _bincount(cols, LB, usable):
    return np.stack([np.bincount(np.asarray(c[:usable], dtype=np.int64), minlength=1 << LB) for c in cols])


def _expect_clean(r, ncols, LB, k, unusable):
    rows = 1 << k
    assert r == {"adjacency_checked": ncols * (rows - unusable), "adjacency_failures": 0,
                 "multiset_checked": ncols * 2 * (1 << LB), "multiset_failures": 0,
                 "padding_checked": ncols * 2 * unusable, "padding_failures": 0}, r


@pytest.mark.parametrize("unusable", [6, 20])
@pytest.mark.parametrize("case", WITNESS_CASES, ids=lambda c: f"{c[0]}x{c[1]}-P{c[2]}-LB{c[3]}-k{c[4]}")
def test_witness_columns_match_restatement(gpu_ctx_factory, case, unusable):
    import torch
    N, M, P, LB, k, ncells, ncols = case
    ctx, p, cols = _witness(gpu_ctx_factory, case)
    rows = 1 << k
    if case == WITNESS_CASES[0]:                     # the last column: 403 cells, none of them zero
        assert ncells - (ncols - 1) * p["max_rows"] == 403 and 0 not in cols[-1][:403]
    want, distinct = _expected(cols, LB, k, unusable)
    lk = ctx.assign_columns(0)[2]
    assert lk.shape == (ncols, rows, 32)
    for form in ("canonical", "montgomery"):
        a, s, r = ctx.lookup_permute(0, unusable, form)
        assert r == {"columns": ncols, "usable_rows": rows - unusable, "out_of_table": 0, "distinct": distinct}
        ca, cs = _canonical(a, form), _canonical(s, form)
        for c in range(ncols):
            assert np.array_equal(ca[c], want[c][0]), (form, c)
            assert np.array_equal(cs[c], want[c][1]), (form, c)
        a2, s2, r2 = ctx.lookup_permute(0, unusable, form, columns=lk)
        assert r2 == r and torch.equal(a2, a) and torch.equal(s2, s)
        _expect_clean(ctx.check_lookup_argument(0, a, s, unusable, form), ncols, LB, k, unusable)
        _expect_clean(ctx.check_lookup_argument(0, a, s, unusable, form, columns=lk), ncols, LB, k, unusable)
    hist = _bincount(cols, LB, rows - unusable)
    assert np.array_equal(ctx.lookup_multiplicities(0, unusable).cpu().numpy(), hist)
    assert np.array_equal(ctx.lookup_multiplicities(0, unusable, columns=lk).cpu().numpy(), hist)
    # phase 1 has no lookup cells: empty tensors, nothing touched
    a, s, r = ctx.lookup_permute(1, unusable)
    assert a.shape == (0, rows, 32) and s.shape == (0, rows, 32)
    assert r == {"columns": 0, "usable_rows": rows - unusable, "out_of_table": 0, "distinct": 0}
    assert ctx.lookup_multiplicities(1, unusable).shape == (0, 1 << LB)
    assert set(ctx.check_lookup_argument(1, a, s, unusable).values()) == {0}


def _synthetic_ctx(gpu_ctx_factory, LB, k, minimum_rows):
    """A context without a witness: the columns come in through columns=."""
    ctx = gpu_ctx_factory(32, LB)
    ctx.physical_layout(k, minimum_rows)
    return ctx


def _run_columns(ctx, cols, LB, k, unusable):
    """Permute `cols` (value lists) in both forms against the restatement; returns (A', S') canonical."""
    rows = 1 << k
    dev = _device_columns(cols, rows)
    want, distinct = _expected(cols, LB, k, unusable)
    for form in ("canonical", "montgomery"):
        a, s, r = ctx.lookup_permute(0, unusable, form, columns=dev)
        assert r == {"columns": len(cols), "usable_rows": rows - unusable, "out_of_table": 0,
                     "distinct": distinct}
        ca, cs = _canonical(a, form), _canonical(s, form)
        for c in range(len(cols)):
            assert np.array_equal(ca[c], want[c][0]), (form, c)
            assert np.array_equal(cs[c], want[c][1]), (form, c)
        _expect_clean(ctx.check_lookup_argument(0, a, s, unusable, form, columns=dev), len(cols), LB, k, unusable)
    assert np.array_equal(ctx.lookup_multiplicities(0, unusable, columns=dev).cpu().numpy(),
                          _bincount(cols, LB, rows - unusable))
    return dev, a, s


@pytest.mark.parametrize("k", [9, 10])
def test_synthetic_columns(gpu_ctx_factory, k):
    """LB = 8, unusable_rows = minimum_rows: one run, all zeros, no zero at all,
    every value once (no absent value), only the two hot bins, uniform."""
    LB = 8
    ctx = _synthetic_ctx(gpu_ctx_factory, LB, k, MINIMUM_ROWS)
    cols = synthetic_columns(LB, k, MINIMUM_ROWS)
    assert 0 not in cols["no_zero"][:(1 << k) - MINIMUM_ROWS] and 0 not in cols["same_nonzero"][:1]
    _run_columns(ctx, list(cols.values()), LB, k, MINIMUM_ROWS)


def test_table_fills_the_usable_rows_or_does_not_fit(gpu_ctx_factory):
    """LB = k - 1 = 8 under a layout of 300 unusable rows at the most: 2^LB <=
    usable runs (usable == 2^LB leaves one table zero, or none), 2^LB > usable
    is SVDW_ERANGE, unusable_rows > minimum_rows SVDW_EINVAL."""
    import halo2_svd041_amd as hs
    LB, k = 8, 9
    ctx = _synthetic_ctx(gpu_ctx_factory, LB, k, 300)
    for unusable in (6, 256):
        c = synthetic_columns(LB, k, unusable, seed=unusable)
        _run_columns(ctx, [c["uniform"], c["no_zero"], c["each_once"]], LB, k, unusable)
    dev = _device_columns([[1] * 512], 512)
    for unusable, code in ((257, -2), (300, -2), (301, -1)):
        with pytest.raises(hs.SvdwError) as e:
            ctx.lookup_permute(0, unusable, columns=dev)
        assert e.value.code == code
        with pytest.raises(hs.SvdwError) as e:
            ctx.lookup_multiplicities(0, unusable, columns=dev)
        assert e.value.code == code
        with pytest.raises(hs.SvdwError) as e:
            ctx.check_lookup_argument(0, dev, dev, unusable, columns=dev)
        assert e.value.code == code


def test_many_scan_blocks(gpu_ctx_factory):
    """LB = 13, k = 14: eight tiles of bins per column in the scans, two columns
    (a skewed one: half zeros and top values; a sparse one: most values absent)."""
    LB, k, unusable = 13, 14, MINIMUM_ROWS
    ctx = _synthetic_ctx(gpu_ctx_factory, LB, k, MINIMUM_ROWS)
    rows, B = 1 << k, 1 << LB
    rs = np.random.RandomState(1314)
    usable = rows - unusable
    skew = np.where(rs.rand(usable) < 0.5, rs.choice([0, B - 1], size=usable), rs.randint(0, B, size=usable))
    sparse = rs.choice(rs.randint(1, B, size=300), size=usable)
    cols = [[int(x) for x in c] + [0] * unusable for c in (skew, sparse)]
    _run_columns(ctx, cols, LB, k, unusable)


def _prefilled(n, rows):
    import torch
    return (torch.full((n, rows, 32), SENTINEL, dtype=torch.uint8, device="cuda"),
            torch.full((n, rows, 32), SENTINEL, dtype=torch.uint8, device="cuda"))


@pytest.mark.parametrize("bad,count", [([(0, 17, 1 << 8)], 1), ([(1, 400, 1 << 224)], 1),
                                       ([(0, 0, 256), (1, 491, (1 << 8) + (1 << 64))], 2)],
                         ids=["two_pow_lb", "high_word", "two_cells"])
def test_cells_outside_the_table(gpu_ctx_factory, bad, count):
    """out_of_table counts the bad cells of usable rows and the outputs keep their bytes."""
    LB, k, unusable = 8, 9, MINIMUM_ROWS
    ctx = _synthetic_ctx(gpu_ctx_factory, LB, k, MINIMUM_ROWS)
    c = synthetic_columns(LB, k, unusable)
    cols = [list(c["uniform"]), list(c["hot_bins"])]
    for col, row, value in bad:
        cols[col][row] = value
    dev = _device_columns(cols, 1 << k)
    out = _prefilled(2, 1 << k)
    for form in ("canonical", "montgomery"):
        a, s, r = ctx.lookup_permute(0, unusable, form, columns=dev, out=out)
        assert r["out_of_table"] == count and r["columns"] == 2
        assert bool((a == SENTINEL).all()) and bool((s == SENTINEL).all())


def test_bad_cell_in_a_blinding_row_is_ignored(gpu_ctx_factory):
    LB, k, unusable = 8, 9, MINIMUM_ROWS
    ctx = _synthetic_ctx(gpu_ctx_factory, LB, k, MINIMUM_ROWS)
    col = list(synthetic_columns(LB, k, unusable)["uniform"])
    rows = 1 << k
    want, _ = _expected([col], LB, k, unusable)
    col[rows - unusable] = 1 << 200                  # the first row that is not usable
    col[rows - 1] = 1 << LB
    a, s, r = ctx.lookup_permute(0, unusable, columns=_device_columns([col], rows), out=_prefilled(1, rows))
    assert r["out_of_table"] == 0
    assert np.array_equal(a.cpu().numpy()[0], want[0][0]) and np.array_equal(s.cpu().numpy()[0], want[0][1])


def test_tampered_witness_column(gpu_ctx_factory):
    case = WITNESS_CASES[0]
    N, M, P, LB, k, ncells, ncols = case
    ctx, p, cols = _witness(gpu_ctx_factory, case)
    rows = 1 << k
    lk = ctx.assign_columns(0)[2].clone()
    lk[1, 100, 1] = 1                                # + 2^8 = 2^LB on an assigned cell
    a, s, r = ctx.lookup_permute(0, 6, columns=lk, out=_prefilled(ncols, rows))
    assert r["out_of_table"] == 1
    assert bool((a == SENTINEL).all()) and bool((s == SENTINEL).all())
    a, s, r = ctx.lookup_permute(0, 6)               # the context's own stream is untouched
    assert r["out_of_table"] == 0
    chk = ctx.check_lookup_argument(0, a, s, 6, columns=lk)   # A' no longer matches the tampered input
    assert chk["multiset_failures"] >= 2 and chk["adjacency_failures"] == 0


@pytest.mark.parametrize("form", ["canonical", "montgomery"])
def test_checker_catches_tampering(gpu_ctx_factory, form):
    LB, k, unusable = 8, 10, MINIMUM_ROWS
    ctx = _synthetic_ctx(gpu_ctx_factory, LB, k, MINIMUM_ROWS)
    col = synthetic_columns(LB, k, unusable)["uniform"]
    rows = 1 << k
    dev = _device_columns([col], rows)
    a, s, r = ctx.lookup_permute(0, unusable, form, columns=dev)
    _expect_clean(ctx.check_lookup_argument(0, a, s, unusable, form, columns=dev), 1, LB, k, unusable)
    av = sorted(col[:rows - unusable])
    heads = [r_ for r_ in range(1, rows - unusable) if av[r_] != av[r_ - 1]]
    i, j = heads[3], heads[40]                       # first rows of two runs: S' must equal A' there
    assert av[i] != av[j]
    # swapping two S' rows of different values: both rows break adjacency, the multisets hold
    s2 = s.clone()
    s2[0, i], s2[0, j] = s[0, j], s[0, i]
    chk = ctx.check_lookup_argument(0, a, s2, unusable, form, columns=dev)
    assert chk["adjacency_failures"] == 2 and chk["multiset_failures"] == 0 and chk["padding_failures"] == 0
    # one A' cell changed to another value of the table: two bins of its histogram move
    a2 = a.clone()
    a2[0, i] = a[0, j]
    chk = ctx.check_lookup_argument(0, a2, s, unusable, form, columns=dev)
    assert chk["multiset_failures"] == 2 and chk["padding_failures"] == 0
    # a non-zero cell in a blinding row
    s3 = s.clone()
    s3[0, rows - 1, 0] = 1
    chk = ctx.check_lookup_argument(0, a, s3, unusable, form, columns=dev)
    assert chk["padding_failures"] == 1 and chk["adjacency_failures"] == 0 and chk["multiset_failures"] == 0


def test_mid_size_run_checks_clean(gpu_ctx_factory):
    """256 x 256, P = 32, LB = 19, k = 21: 512 tiles of bins in the scans, no host reference."""
    import halo2_svd041_amd as hs
    N, P, LB, k = 256, 32, 19, 21
    m, u, d, v = gen_svd_input(N, N, seed=N + N + P)
    ctx = gpu_ctx_factory(P, LB)
    hs.svd_witness(ctx, m, u, v, d, gamma_for(N))
    p = ctx.physical_layout(k, MINIMUM_ROWS)
    ncols = p["num_lookup_advice"][0]
    assert ncols >= 1
    for form in ("canonical", "montgomery"):
        a, s, r = ctx.lookup_permute(0, 6, form)
        assert r["out_of_table"] == 0 and 1 <= r["distinct"] <= ncols << LB
        if ncols == 1:
            assert r["distinct"] <= 1 << LB
        _expect_clean(ctx.check_lookup_argument(0, a, s, 6, form), ncols, LB, k, 6)
    mult = ctx.lookup_multiplicities(0, 6)
    assert int(mult.sum()) == ncols * ((1 << k) - 6)
    assert int((mult > 0).sum()) == r["distinct"]
