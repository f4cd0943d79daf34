"""svdw_permutation_values / svdw_permutation_product /
svdw_check_permutation_product on the device against the literal restatement of
halo2's permutation grand products (permutation_cases.py; parity of the rule
itself unpinned): sigma cells against delta^c omega^r, the identity
sigma, synthetic columns with value-grouped cycles byte for byte in both forms
and with both pairs of challenges, columns of several tiles, the copy
constraints of SVD witnesses merged on the host, inv0 on a zero denominator,
the checker against tampered columns, and one run of 2^21 rows checked by the
device checker alone."""
import numpy as np
import pytest

from conftest import gamma_for, gen_svd_input
from lookup_perm_cases import cell_values
from permutation_cases import (CHALLENGES, DELTA, P_MOD, Assembly, cells_of, first_placement, grand_products,
                               identity_mapping, mapping_entries, omega, recurrence_holds, sigma_values,
                               value_cycles)

pytestmark = pytest.mark.gpu

SENTINEL = 0xAB
FORMS = ("canonical", "montgomery")


def _in_form(a: np.ndarray, form: str) -> np.ndarray:
    """Canonical numpy cells [..., 32] u8 -> cells in `form` (svdw_fr_convert)."""
    import halo2_svd041_amd as hs
    a = np.ascontiguousarray(a)
    if form == "montgomery" and a.size:
        a = hs.fr_convert(a.view("<u8").reshape(-1, 4), "canonical", "montgomery").view(np.uint8).reshape(a.shape)
    return a


def _canonical(t, form: str) -> np.ndarray:
    """Device cells in `form` -> canonical numpy cells."""
    import halo2_svd041_amd as hs
    a = t.cpu().numpy()
    if form == "montgomery" and a.size:
        a = hs.fr_convert(a.view("<u8").reshape(-1, 4), "montgomery", "canonical").view(np.uint8).reshape(a.shape)
    return a


def _device(cols, form: str):
    """Value lists -> [n, rows, 32] u8 device tensor in `form`."""
    import torch
    return torch.from_numpy(_in_form(np.stack([cells_of(c) for c in cols]), form)).cuda()


def _sigma(ctx, mapping, k: int, form: str):
    """The mapping's sigma columns, made on the device in `form`."""
    import torch
    s, bad = ctx.permutation_values(k, torch.from_numpy(mapping_entries(mapping)).cuda(), form=form)
    assert bad == 0
    return s


def _prefilled(n: int, rows: int):
    import torch
    return torch.full((n, rows, 32), SENTINEL, dtype=torch.uint8, device="cuda")


def _clean(nsets: int, k: int, unusable: int) -> dict:
    rows = 1 << k
    return {"recurrence_checked": nsets * (rows - unusable), "recurrence_failures": 0,
            "boundary_checked": nsets + 1, "boundary_failures": 0,
            "padding_checked": nsets * (unusable - 1), "padding_failures": 0}


def _columns(k: int, unusable: int, ncols: int, seed: int) -> list:
    """Columns drawn from 8 distinct small integers, column 1 of full 254-bit
    values; rows >= usable zero."""
    rows = 1 << k
    rs = np.random.RandomState(seed)
    cols = [[int(x) for x in rs.randint(0, 8, size=rows - unusable)] + [0] * unusable for _ in range(ncols)]
    if ncols > 1:
        cols[1] = [int.from_bytes(rs.bytes(32), "little") % P_MOD for _ in range(rows - unusable)] + [0] * unusable
    return cols


def _run(ctx, cols, mapping, k, unusable, chunk_len, pairs, honest=True, split=None):
    """The products of `cols` under `mapping` in both forms against the
    restatement for each (beta, gamma) of `pairs`, then the device checker.
    split: also pass columns and sigma as lists of tensors cut there."""
    import torch
    rows, ncols = 1 << k, len(cols)
    usable = rows - unusable
    nsets = -(-ncols // chunk_len)
    sig = sigma_values(mapping, k)
    for beta, gamma in pairs:
        Z, zeros = grand_products(cols, sig, beta, gamma, chunk_len, k, unusable)
        broken = sum(len(b) for b in recurrence_holds(cols, sig, Z, beta, gamma, chunk_len, k, unusable))
        if honest:                                          # the condition of the case, checked on the CPU first
            assert zeros == 0 and Z[-1][usable] == 1 and broken == 0
        want = np.stack([cells_of(z) for z in Z])
        for form in FORMS:
            dc, ds = _device(cols, form), _sigma(ctx, mapping, k, form)
            z, res = ctx.permutation_product(dc, ds, beta, gamma, chunk_len, k, unusable, form,
                                             out=_prefilled(nsets, rows))
            assert res == {"columns": ncols, "sets": nsets, "usable_rows": usable, "zero_denominators": zeros,
                           "final_not_one": int(Z[-1][usable] != 1)}, (form, res)
            got = _canonical(z, form)
            for s in range(nsets):
                assert np.array_equal(got[s], want[s]), (form, s, chunk_len, hex(beta))
            if split:
                z2, res2 = ctx.permutation_product([dc[:split], dc[split:]], [ds[:split], ds[split:]], beta, gamma,
                                                   chunk_len, k, unusable, form, out=_prefilled(nsets, rows))
                assert res2 == res and torch.equal(z2, z)
            chk = ctx.check_permutation_product(dc, ds, z, beta, gamma, chunk_len, k, unusable, form)
            assert chk == dict(_clean(nsets, k, unusable), recurrence_failures=broken), (form, chk)


# ------------------------------------------------------------ 1. sigma values
@pytest.mark.parametrize("k", [9, 13])
def test_sigma_values_match_delta_omega_powers(gpu_ctx_factory, k):
    """Every cell of the identity and of a shuffled mapping over 3 columns, in
    both forms; first_col > 0; an out-of-range entry is counted and zeroed."""
    import torch
    ctx = gpu_ctx_factory(32, 8)
    rows, ncols = 1 << k, 3
    rs = np.random.RandomState(k)
    ident = identity_mapping(ncols, rows)
    flat = [e for col in ident for e in col]
    flat = [flat[i] for i in rs.permutation(len(flat))]
    shuffled = [flat[c * rows:(c + 1) * rows] for c in range(ncols)]
    for form in FORMS:
        for mapping in (ident, shuffled):
            want = np.stack([cells_of(col) for col in sigma_values(mapping, k)])
            assert np.array_equal(_canonical(_sigma(ctx, mapping, k, form), form), want), form
        want = np.stack([cells_of(col) for col in sigma_values(ident, k)])
        s, bad = ctx.permutation_values(k, ncols=ncols, form=form)
        assert bad == 0 and np.array_equal(_canonical(s, form), want)
        s, bad = ctx.permutation_values(k, first_col=1, ncols=2, form=form)
        assert bad == 0 and np.array_equal(_canonical(s, form), want[1:])
        # identity columns past total_cols; then mapping entries one past either range
        s, bad = ctx.permutation_values(k, first_col=1, ncols=2, total_cols=2, form=form)
        got = _canonical(s, form)
        assert bad == rows and np.array_equal(got[0], want[1]) and not got[1].any()
        e = mapping_entries(shuffled)
        e[0, 5], e[2, rows - 1] = ncols << 32, (1 << 32) | rows
        s, bad = ctx.permutation_values(k, torch.from_numpy(e).cuda(), form=form)
        got = _canonical(s, form)
        want = np.stack([cells_of(col) for col in sigma_values(shuffled, k)])
        want[0, 5] = want[2, rows - 1] = 0
        assert bad == 2 and np.array_equal(got, want)


def test_sigma_values_across_the_table_seams(gpu_ctx_factory):
    """k = 21: omega^r is the product of two table entries, r = hi 2^11 + lo.
    4096 sampled rows of column 2, both sides of every one of the 1023 seams
    among them, against pow."""
    import torch
    ctx = gpu_ctx_factory(32, 8)
    k, h = 21, 11
    rows = 1 << k
    seams = [i << h for i in range(1, 1 << (k - h))]
    rs = np.random.RandomState(21)
    sample = sorted(set([0, rows - 1] + seams + [s - 1 for s in seams]
                        + [int(r) for r in rs.randint(0, rows, size=4096 - 2 * len(seams) - 2)]))
    assert 4000 < len(sample) <= 4096
    w, d2 = omega(k), DELTA * DELTA % P_MOD
    want = cells_of([d2 * pow(w, r, P_MOD) % P_MOD for r in sample])
    idx = torch.tensor(sample, device="cuda")
    for form in FORMS:
        s, bad = ctx.permutation_values(k, first_col=2, ncols=1, form=form)
        assert bad == 0 and np.array_equal(_canonical(s[0, idx], form), want), form


# ----------------------------------------------------------- 2. identity sigma
def test_identity_sigma_gives_ones(gpu_ctx_factory):
    """N == D in every row: every Z cell at rows <= usable is 1 in every set.
    A delta^j index that restarts per set or an omega^r off by a row shows."""
    ctx = gpu_ctx_factory(32, 8)
    k, unusable, ncols, chunk_len = 11, 6, 5, 2
    rows = 1 << k
    usable = rows - unusable
    cols = _columns(k, unusable, ncols, seed=2)
    one = cells_of([1] * (usable + 1) + [0] * (unusable - 1))
    for form in FORMS:
        dc = _device(cols, form)
        ds, bad = ctx.permutation_values(k, ncols=ncols, form=form)
        for beta, gamma in CHALLENGES:
            z, res = ctx.permutation_product(dc, ds, beta, gamma, chunk_len, k, unusable, form,
                                             out=_prefilled(3, rows))
            assert res == {"columns": ncols, "sets": 3, "usable_rows": usable, "zero_denominators": 0,
                           "final_not_one": 0}, (form, res)
            got = _canonical(z, form)
            assert all(np.array_equal(got[s], one) for s in range(3)), form
            assert ctx.check_permutation_product(dc, ds, z, beta, gamma, chunk_len, k, unusable,
                                                 form) == _clean(3, k, unusable)


# -------------------------------------------------------- 3. synthetic columns
@pytest.mark.parametrize("chunk_len", [1, 2, 3, 5, 7])
@pytest.mark.parametrize("k,unusable", [(9, 6), (10, 6), (11, 1024)])
def test_synthetic_columns_match_restatement(gpu_ctx_factory, k, unusable, chunk_len):
    """5 columns: one column per set, a short last set, one set. k = 9 is less
    than one tile; k = 11 with 1024 unusable rows puts Z[usable] exactly on a
    tile seam. Condition (checked in _run on the CPU): no zero denominator."""
    ctx = gpu_ctx_factory(32, 8)
    cols = _columns(k, unusable, 5, seed=k)
    mapping = value_cycles(cols, (1 << k) - unusable, seed=k + 1)
    _run(ctx, cols, mapping, k, unusable, chunk_len, CHALLENGES, split=2)


# ----------------------------------------------------------- 4. several tiles
@pytest.mark.parametrize("unusable,pair", [(6, 0), (1, 1)])
def test_columns_of_several_tiles(gpu_ctx_factory, unusable, pair):
    """k = 13: eight tiles per set, the carries cross tiles in both directions
    and the start crosses sets; unusable_rows = 1: Z[usable] is the last row.
    One pair of challenges each: the restatement takes seconds here."""
    ctx = gpu_ctx_factory(32, 8)
    k = 13
    cols = _columns(k, unusable, 3, seed=13)
    mapping = value_cycles(cols, (1 << k) - unusable, seed=14)
    _run(ctx, cols, mapping, k, unusable, 2, [CHALLENGES[pair]])


# ----------------------------------------------------- 5. real copy constraints
WITNESSES = [(5, 3, 63), (6, 6, 42)]
W_LB, W_K, W_MIN_ROWS, W_UNUSABLE = 8, 10, 20, 6


def _witness_mapping(ctx, ncols, rows):
    """Keygen's merge on the host over the break-cell duplicates and the copy
    records between advice cells (source phase 0 or 1). Records whose source is
    the external init_rand cell and constant records are left out: their other
    end lies in columns this argument does not hold here."""
    base = [0, ncols[0]]
    bps = [ctx.break_points(ph) for ph in (0, 1)]
    asm = Assembly(ncols[0] + ncols[1], rows)
    merged = 0
    for ph in (0, 1):
        for j, b in enumerate(bps[ph]):
            asm.copy((base[ph] + j, int(b)), (base[ph] + j + 1, 0))
            merged += 1
        for sp, s, d in ctx.equalities(ph)[0]:
            if int(sp) > 1:
                continue
            sc, sr = first_placement(bps[int(sp)], int(s))
            dc, dr = first_placement(bps[ph], int(d))
            asm.copy((base[int(sp)] + sc, sr), (base[ph] + dc, dr))
            merged += 1
    return asm.mapping, merged, sum(len(b) for b in bps)


@pytest.mark.parametrize("N,M,P", WITNESSES)
def test_witness_copy_constraints_close(gpu_ctx_factory, N, M, P):
    """Advice columns of both phases of an SVD witness, sigma from the host merge:
    Z equals the restatement and closes, the checker is clean. Then two rows of
    one advice column swapped: the last Z[usable] is not 1, the recurrence still
    holds, one boundary failure."""
    import torch
    import halo2_svd041_amd as hs
    m, u, d, v = gen_svd_input(N, M, seed=N + M + P)
    with hs.Context(device=-1, precision_bits=P, lookup_bits=W_LB) as plan:
        hs.svd_witness(plan, m, u, v, d, gamma_for(W_K))
        p = plan.physical_layout(W_K, W_MIN_ROWS)
        used = p["columns_used"]
        # the conditions of the case, on the planning context
        assert used == p["num_advice"] and 4 <= sum(used) <= 16
        assert len(plan.break_points(0)) + len(plan.break_points(1)) >= 1
    ctx = gpu_ctx_factory(P, W_LB)
    hs.svd_witness(ctx, m, u, v, d, gamma_for(W_K))
    assert ctx.physical_layout(W_K, W_MIN_ROWS)["columns_used"] == used
    rows, ncols = 1 << W_K, sum(used)
    usable = rows - W_UNUSABLE
    dev = {f: [ctx.assign_columns(ph, form=f)[0] for ph in (0, 1)] for f in FORMS}
    torch.cuda.synchronize()
    host = np.concatenate([t.cpu().numpy() for t in dev["canonical"]])
    cols = [cell_values(c) for c in host]
    mapping, merged, breaks = _witness_mapping(ctx, used, rows)
    assert breaks >= 1 and merged > 100
    for c in range(ncols):                                   # an honest sigma: cycles of equal values, rows < usable
        for r in range(rows):
            cc, rr = mapping[c][r]
            assert cols[cc][rr] == cols[c][r] and (r < usable or (cc, rr) == (c, r))
    sig = sigma_values(mapping, W_K)
    for chunk_len in (2, 3):
        nsets = -(-ncols // chunk_len)
        for beta, gamma in CHALLENGES:
            Z, zeros = grand_products(cols, sig, beta, gamma, chunk_len, W_K, W_UNUSABLE)
            assert zeros == 0 and Z[-1][usable] == 1 and Z[0][usable] != 1
            want = np.stack([cells_of(z) for z in Z])
            for form in FORMS:
                ds = _sigma(ctx, mapping, W_K, form)
                z, res = ctx.permutation_product(dev[form], ds, beta, gamma, chunk_len, W_K, W_UNUSABLE, form,
                                                 out=_prefilled(nsets, rows))
                assert res == {"columns": ncols, "sets": nsets, "usable_rows": usable, "zero_denominators": 0,
                               "final_not_one": 0}, (form, res)
                assert np.array_equal(_canonical(z, form), want), (form, chunk_len)
                assert ctx.check_permutation_product(dev[form], ds, z, beta, gamma, chunk_len, W_K, W_UNUSABLE,
                                                     form) == _clean(nsets, W_K, W_UNUSABLE)
    # rows 1 and 2 of the first advice column swapped; the condition: one of the
    # two cells sits in a cycle whose other cells now differ from it
    cols[0][1], cols[0][2] = cols[0][2], cols[0][1]
    assert any(cols[cc][rr] != cols[0][r] for r in (1, 2) for cc, rr in [mapping[0][r]])
    beta, gamma = CHALLENGES[0]
    Z, zeros = grand_products(cols, sig, beta, gamma, 2, W_K, W_UNUSABLE)
    assert zeros == 0 and Z[-1][usable] not in (0, 1)
    nsets = -(-ncols // 2)
    for form in FORMS:
        c0, c1 = dev[form]
        c0[0, [1, 2]] = c0[0, [2, 1]]
        ds = _sigma(ctx, mapping, W_K, form)
        z, res = ctx.permutation_product([c0, c1], ds, beta, gamma, 2, W_K, W_UNUSABLE, form)
        assert res["final_not_one"] == 1 and res["zero_denominators"] == 0, (form, res)
        assert np.array_equal(_canonical(z, form), np.stack([cells_of(x) for x in Z])), form
        chk = ctx.check_permutation_product([c0, c1], ds, z, beta, gamma, 2, W_K, W_UNUSABLE, form)
        assert chk == dict(_clean(nsets, W_K, W_UNUSABLE), boundary_failures=1), (form, chk)


# --------------------------------------------------------------------- 6. inv0
def test_inv0_on_a_zero_denominator(gpu_ctx_factory):
    """gamma = -(v + beta sigma) of cell (0, 200): D_0[200] is zero in set 0 of 2.
    Z is zero from row 201 on and throughout set 1, as batch_invert leaves a zero
    zero; the checker reports the rows the restatement's recurrence reports."""
    ctx = gpu_ctx_factory(32, 8)
    k, unusable, r0 = 9, 6, 200
    cols = _columns(k, unusable, 3, seed=6)
    mapping = value_cycles(cols, (1 << k) - unusable, seed=7)
    sig = sigma_values(mapping, k)
    beta = CHALLENGES[1][0]
    gamma = (-(cols[0][r0] + beta * sig[0][r0])) % P_MOD
    Z, zeros = grand_products(cols, sig, beta, gamma, 2, k, unusable)
    assert zeros == 1 and all(Z[0][:r0 + 1]) and not any(Z[0][r0 + 1:]) and not any(Z[1])
    assert recurrence_holds(cols, sig, Z, beta, gamma, 2, k, unusable) == [[r0], []]
    _run(ctx, cols, mapping, k, unusable, 2, [(beta, gamma)], honest=False)


# ---------------------------------------------------------------- 7. tampering
@pytest.mark.parametrize("form", FORMS)
def test_checker_catches_tampering(gpu_ctx_factory, form):
    import torch
    import halo2_svd041_amd as hs
    ctx = gpu_ctx_factory(32, 8)
    k, unusable, chunk_len = 10, 6, 2
    rows = 1 << k
    usable = rows - unusable
    cols = _columns(k, unusable, 4, seed=70)
    mapping = value_cycles(cols, usable, seed=71)
    sig = sigma_values(mapping, k)
    beta, gamma = CHALLENGES[1]
    Z, zeros = grand_products(cols, sig, beta, gamma, chunk_len, k, unusable)
    assert zeros == 0 and Z[-1][usable] == 1 and all(Z[0][:usable + 1]) and all(Z[1][:usable + 1])
    dc, ds = _device(cols, form), _sigma(ctx, mapping, k, form)
    args = (beta, gamma, chunk_len, k, unusable, form)
    clean = _clean(2, k, unusable)
    z, res = ctx.permutation_product(dc, ds, *args)
    assert res["final_not_one"] == 0 and res["zero_denominators"] == 0
    assert ctx.check_permutation_product(dc, ds, z, *args) == clean
    # cells are bytes: a tensor of the same shape and another dtype is refused
    for bad in ((dc.view(torch.int8), ds, z), (dc, ds.view(torch.int8), z), (dc, ds, z.view(torch.int8))):
        with pytest.raises(hs.SvdwError):
            ctx.check_permutation_product(bad[0], bad[1], bad[2], *args)
        with pytest.raises(hs.SvdwError):
            ctx.permutation_product(bad[0], bad[1], *args, out=bad[2])
    # one Z cell in the middle of set 0 changed: the rows r - 1 and r, no others
    row = 517
    z2 = z.clone()
    z2[0, row, 0] ^= 1
    chk = ctx.check_permutation_product(dc, ds, z2, *args)
    assert chk == dict(clean, recurrence_failures=2), chk
    cz = [cell_values(c) for c in _canonical(z2, form)]
    assert recurrence_holds(cols, sig, cz, beta, gamma, chunk_len, k, unusable) == [[row - 1, row], []]
    # one sigma cell changed, the honest Z: the row of the changed cell
    s2 = ds.clone()
    s2[3, 300, 0] ^= 1
    chk = ctx.check_permutation_product(dc, s2, z, *args)
    assert chk == dict(clean, recurrence_failures=1), chk
    # ... and its own Z obeys the recurrence; only the last Z[usable] tells
    z3, res = ctx.permutation_product(dc, s2, *args)
    assert res["final_not_one"] == 1 and res["zero_denominators"] == 0
    chk = ctx.check_permutation_product(dc, s2, z3, *args)
    assert chk == dict(clean, boundary_failures=1), chk
    assert torch.equal(z3[0], z[0]) and torch.equal(z3[1, :301], z[1, :301])
    # Z_1[0] != Z_0[usable]: the chain and row 0 of set 1
    z4 = z.clone()
    z4[1, 0, 0] ^= 1
    chk = ctx.check_permutation_product(dc, ds, z4, *args)
    assert chk == dict(clean, recurrence_failures=1, boundary_failures=1), chk
    # Z_0[0] != 1
    z5 = z.clone()
    z5[0, 0, 0] ^= 2
    chk = ctx.check_permutation_product(dc, ds, z5, *args)
    assert chk == dict(clean, recurrence_failures=1, boundary_failures=1), chk
    # a non-zero cell above usable
    z6 = z.clone()
    z6[1, rows - 1, 0] = 1
    chk = ctx.check_permutation_product(dc, ds, z6, *args)
    assert chk == dict(clean, padding_failures=1), chk


# ------------------------------------------------- 8. runs of tiles per thread
def test_runs_of_tiles_per_carry_thread(gpu_ctx_factory):
    """k = 21, 3 columns in 2 sets: 2048 tiles per set, so each of the carry
    kernels' 256 threads multiplies, prefixes and suffixes a run of eight tile
    products, and the checker's grid of 4096 blocks strides twice over the rows
    (its second omega^r comes from the step, not the table). Columns and sigma
    made on the device: values below 300, a stable sort of the usable cells by
    value, each run of equal values linked into a cycle. Checked by the device
    checker alone. Then one sigma cell changed in a high tile of set 0: the last
    Z[usable] is not 1; set 0 keeps its bytes up to that row, everything after
    and all of set 1 change.

    Condition, checked on the CPU first: no cell's denominator factor
    v + beta delta^c omega^r + gamma is zero, for no v < 300, c < 3 and no row."""
    import torch
    import halo2_svd041_amd as hs
    ctx = gpu_ctx_factory(32, 8)
    k, unusable, ncols, chunk_len, nvals = 21, 6, 3, 2, 300
    rows = 1 << k
    usable = rows - unusable
    assert (rows // 1024) // 256 == 8 and rows > 4096 * 256
    for beta, gamma in CHALLENGES:
        for c in range(ncols):
            bd = pow(beta * pow(DELTA, c, P_MOD), P_MOD - 2, P_MOD)
            assert all(pow((-gamma - v) * bd % P_MOD, rows, P_MOD) != 1 for v in range(nvals))
    g = torch.Generator(device="cuda").manual_seed(2100)
    vals = torch.randint(0, nvals, (ncols, rows), generator=g, device="cuda")
    vals[:, usable:] = 0
    # the usable cells in the order of their values; each run of equal values a cycle
    cell = (torch.arange(ncols, device="cuda")[:, None] << 32 | torch.arange(rows, device="cuda")[None, :])
    keys, order = torch.sort(vals[:, :usable].reshape(-1), stable=True)
    at = cell[:, :usable].reshape(-1)[order]                 # the cells, sorted
    n = at.numel()
    i = torch.arange(n, device="cuda")
    start = torch.ones(n, dtype=torch.bool, device="cuda")
    start[1:] = keys[1:] != keys[:-1]
    run_start = torch.cummax(torch.where(start, i, torch.zeros_like(i)), 0).values
    nxt = torch.roll(at, -1)
    last = torch.roll(start, -1)                             # the next cell starts a run: this one ends its own
    nxt = torch.where(last, at[run_start], nxt)
    mapping = cell.clone()
    flat = mapping.view(-1)
    flat[(at >> 32) * rows + (at & 0xffffffff)] = nxt
    table = cells_of(range(nvals))
    clean = _clean(2, k, unusable)
    row = 1901 * 1024 + 77                                   # tile 1901: run 237 of the carry, its sixth tile
    for form, (beta, gamma) in zip(FORMS, CHALLENGES):
        dc = torch.from_numpy(_in_form(table, form)).cuda()[vals]
        assert dc.shape == (ncols, rows, 32) and dc.is_contiguous()
        ds, bad = ctx.permutation_values(k, mapping, form=form)
        assert bad == 0
        args = (beta, gamma, chunk_len, k, unusable, form)
        z, res = ctx.permutation_product(dc, ds, *args, out=_prefilled(2, rows))
        assert res == {"columns": ncols, "sets": 2, "usable_rows": usable, "zero_denominators": 0,
                       "final_not_one": 0}, (form, res)
        assert ctx.check_permutation_product(dc, ds, z, *args) == clean, form
        s2 = ds.clone()
        s2[0, row, 0] ^= 1
        z2, res = ctx.permutation_product(dc, s2, *args)
        assert res["final_not_one"] == 1 and res["zero_denominators"] == 0, (form, res)
        chk = ctx.check_permutation_product(dc, s2, z2, *args)
        assert chk == dict(clean, boundary_failures=1), (form, chk)
        assert torch.equal(z2[0, :row + 1], z[0, :row + 1])
        assert not bool((z2[0, row + 1:usable + 1] == z[0, row + 1:usable + 1]).all(dim=1).any())
        assert not bool((z2[1, :usable + 1] == z[1, :usable + 1]).all(dim=1).any())


# ----------------------------------------------------------------- 9. no columns
def test_no_columns(gpu_ctx_factory):
    import torch
    ctx = gpu_ctx_factory(32, 8)
    empty = torch.empty((0, 512, 32), dtype=torch.uint8, device="cuda")
    for cols in (empty, []):
        z, res = ctx.permutation_product(cols, cols, *CHALLENGES[0], 2, k=9)
        assert z.shape == (0, 512, 32)
        assert res == {"columns": 0, "sets": 0, "usable_rows": 506, "zero_denominators": 0, "final_not_one": 0}
        assert set(ctx.check_permutation_product(cols, cols, z, *CHALLENGES[0], 2, k=9).values()) == {0}
    s, bad = ctx.permutation_values(9, ncols=0)
    assert s.shape == (0, 512, 32) and bad == 0
