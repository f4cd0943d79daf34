"""svdw_ntt / svdw_eval_polynomial / svdw_check_ntt on the device against the
literal restatement (ntt_cases.py; parity of the rule itself unpinned,
DESIGN.md): every size around one tile in full, coset extensions and their way
back, two passes in full, three passes on spikes in full and on dense columns by
round trip plus the device checker, the checker itself against tampering, a
wrong shift and a wrong scale, evaluation at points, and the columns and Z of an
SVD witness end to end. Outputs are prefilled with a sentinel byte; both forms
throughout; comparisons byte for byte after fr_convert."""
import ctypes as ct

import numpy as np
import pytest

from conftest import gamma_for, gen_svd_input
from lookup_perm_cases import cell_values
from ntt_cases import (P_MOD, WIDE_SHIFT, ZETA, horner, inv, ntt_forward, ntt_inverse, omega, sample_rows,
                       spikes_forward, spikes_inverse)

pytestmark = pytest.mark.gpu

SENTINEL = 0xAB
FORMS = ("canonical", "montgomery")


@pytest.fixture(scope="module")
def ctx(gpu_ctx_factory):
    return gpu_ctx_factory(32, 8)


def _cells(vals) -> np.ndarray:
    """[len(vals), 32] u8 canonical cells."""
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint8).reshape(-1, 32).copy()


def _in_form(a: np.ndarray, form: str) -> np.ndarray:
    import halo2_svd041_amd as hs
    a = np.ascontiguousarray(a)
    if form == "montgomery" and a.size:
        a = hs.fr_convert(a.view("<u8").reshape(-1, 4), "canonical", "montgomery").view(np.uint8).reshape(a.shape)
    return a


def _canonical(t, form: str) -> np.ndarray:
    import halo2_svd041_amd as hs
    a = t.cpu().numpy()
    if form == "montgomery" and a.size:
        a = hs.fr_convert(a.view("<u8").reshape(-1, 4), "montgomery", "canonical").view(np.uint8).reshape(a.shape)
    return a


def _device(cols, form: str):
    """Value lists -> [n, rows, 32] u8 device tensor in `form`."""
    import torch
    return torch.from_numpy(_in_form(np.stack([_cells(c) for c in cols]), form)).cuda()


def _prefilled(n: int, rows: int):
    import torch
    return torch.full((n, rows, 32), SENTINEL, dtype=torch.uint8, device="cuda")


def _wide(n: int, seed: int) -> list:
    rs = np.random.RandomState(seed)
    return [int.from_bytes(rs.bytes(32), "little") % P_MOD for _ in range(n)]


def _three_columns(k: int) -> list:
    """Full-width random; small values with 0 and p - 1 among them; one spike at the last row."""
    n = 1 << k
    small = [(5 * i + 3) % 11 for i in range(n)]
    small[0], small[-1] = 0, P_MOD - 1
    return [_wide(n, 40 + k), small, [0] * (n - 1) + [P_MOD - 2]]


def _result(ncols: int, k_in: int, k: int) -> dict:
    import halo2_svd041_amd as hs
    return {"columns": ncols, "passes": hs.zk.lib().svdw_ntt_passes(k), "rows_in": 1 << k_in, "rows_out": 1 << k}


# ------------------------------------------------- 1. small sizes, full compare
@pytest.mark.parametrize("k", range(1, 13))
def test_sizes_around_one_tile(ctx, k):
    cols = _three_columns(k)
    fwd = np.stack([_cells(ntt_forward(c, k, k)) for c in cols])
    bwd = np.stack([_cells(ntt_inverse(c, k)) for c in cols])
    for form in FORMS:
        d = _device(cols, form)
        split = [d[:2].contiguous(), d[2:].contiguous()]
        out, res = ctx.ntt(split, k, form=form, out=_prefilled(3, 1 << k))
        assert res == _result(3, k, k), (form, res)
        assert np.array_equal(_canonical(out, form), fwd), (form, "forward")
        out, res = ctx.ntt(split, k, inverse=True, form=form, out=_prefilled(3, 1 << k))
        assert res == _result(3, k, k), (form, res)
        assert np.array_equal(_canonical(out, form), bwd), (form, "inverse")
        assert np.array_equal(_canonical(ctx.coeff_to_lagrange(d, k, form)[0], form), fwd), form
        assert np.array_equal(_canonical(ctx.lagrange_to_coeff(d, k, form)[0], form), bwd), form


# ----------------------------------------------------------- 2. coset extension
@pytest.mark.parametrize("k_in", [3, 9, 10, 11])
def test_coset_extension_and_back(ctx, k_in):
    n_in = 1 << k_in
    cols = [_wide(n_in, 60 + k_in), [(3 * i) % 7 for i in range(n_in - 1)] + [P_MOD - 1]]
    for k in (k_in + 1, k_in + 2, k_in + 3):
        for shift in (ZETA, WIDE_SHIFT):
            want = np.stack([_cells(ntt_forward(c, k_in, k, shift)) for c in cols])
            back = np.stack([_cells(c + [0] * ((1 << k) - n_in)) for c in cols])
            for form in FORMS:
                d = _device(cols, form)
                ext, res = ctx.coeff_to_extended(d, k_in, k, shift, form=form, out=_prefilled(2, 1 << k))
                assert res == _result(2, k_in, k), (form, res)
                assert np.array_equal(_canonical(ext, form), want), (form, k, hex(shift))
                co, res = ctx.extended_to_coeff(ext, k, inv(shift), form=form, out=_prefilled(2, 1 << k))
                assert res == _result(2, k, k), (form, res)
                assert np.array_equal(_canonical(co, form), back), (form, k, hex(shift))


# ----------------------------------------------------------------- 3. two passes
def test_two_passes_in_full(ctx):
    import halo2_svd041_amd as hs
    k = 16
    assert hs.zk.lib().svdw_ntt_passes(k) == 2
    a = _wide(1 << k, 16)
    want = _cells(ntt_forward(a, k, k))[None]
    src = _cells(a)[None]
    for form in FORMS:
        d = _device([a], form)
        out, res = ctx.ntt(d, k, form=form, out=_prefilled(1, 1 << k))
        assert res == _result(1, k, k)
        assert np.array_equal(_canonical(out, form), want), form
        # the inverse of the restatement's output is the input
        back, _ = ctx.ntt(_device_cells(want, form), k, inverse=True, form=form, out=_prefilled(1, 1 << k))
        assert np.array_equal(_canonical(back, form), src), form
        # every row through the checker: more points than one of its launches takes
        every = {"rows_checked": 1 << k, "row_failures": 0}
        assert ctx.check_ntt(d, out, k, form=form, log_samples=k) == every
        out[0, 40000, 1] ^= 4
        assert ctx.check_ntt(d, out, k, form=form, log_samples=k) == dict(every, row_failures=1)


def _device_cells(a: np.ndarray, form: str):
    import torch
    return torch.from_numpy(_in_form(a, form)).cuda()


# --------------------------------------------------------------- 4. three passes
def _k3() -> int:
    import halo2_svd041_amd as hs
    k3 = min(k for k in range(1, 29) if hs.zk.lib().svdw_ntt_passes(k) == 3)
    assert k3 <= 23                      # a changed tile size must not silently drop the case
    return k3


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
def test_three_passes_sparse_in_full(ctx, inverse):
    import torch
    k3 = _k3()
    n = 1 << k3
    spikes = [(n - 1, P_MOD - 5), ((1 << (k3 // 2)) + 1, WIDE_SHIFT)]
    want = _cells((spikes_inverse if inverse else spikes_forward)(spikes, k3))[None]
    for form in FORMS:
        d = torch.zeros((1, n, 32), dtype=torch.uint8, device="cuda")
        for row, value in spikes:
            d[0, row] = torch.from_numpy(_in_form(_cells([value]), form)[0]).cuda()
        out, res = ctx.ntt(d, k3, inverse=inverse, form=form, out=_prefilled(1, n))
        assert res == _result(1, k3, k3)
        assert np.array_equal(_canonical(out, form), want), form


@pytest.fixture(scope="module")
def dense_k3():
    """Two columns of 2^K3 full-width cells (253 random bits each: below p in
    either form), made once."""
    import torch
    k3 = _k3()
    rs = np.random.RandomState(21)
    a = rs.randint(0, 256, size=(2, 1 << k3, 32), dtype=np.uint8)
    a[:, :, 31] &= 0x1F
    return k3, torch.from_numpy(a).cuda()


@pytest.mark.parametrize("form", FORMS)
def test_three_passes_dense_round_trip_and_checker(ctx, dense_k3, form):
    """Dense columns are compared on sampled rows only, by design: the round trip
    alone cannot see an indexing error mirrored in both directions, so the
    checker carries the case, and test_checker_* earn it that trust."""
    import torch
    k3, a = dense_k3
    n = 1 << k3
    clean = {"rows_checked": 2 * 1024, "row_failures": 0}
    fwd, res = ctx.ntt(a, k3, form=form, out=_prefilled(2, n))
    assert res == _result(2, k3, k3)
    assert ctx.check_ntt(a, fwd, k3, form=form, log_samples=10, seed=11) == clean
    back, _ = ctx.ntt(fwd, k3, inverse=True, form=form, out=_prefilled(2, n))
    assert torch.equal(back, a)
    assert ctx.check_ntt(fwd, back, k3, inverse=True, form=form, log_samples=10, seed=12) == clean
    # the other order, through the coset of a full-width shift
    co, _ = ctx.ntt(a, k3, inverse=True, shift=WIDE_SHIFT, form=form, out=_prefilled(2, n))
    assert ctx.check_ntt(a, co, k3, inverse=True, shift=WIDE_SHIFT, form=form, log_samples=10, seed=13) == clean
    ev, _ = ctx.ntt(co, k3, shift=inv(WIDE_SHIFT), form=form, out=_prefilled(2, n))
    assert torch.equal(ev, a)
    assert ctx.check_ntt(co, ev, k3, shift=inv(WIDE_SHIFT), form=form, log_samples=10, seed=14) == clean
    # one output cell at a row the rule samples: exactly one failure
    row = sample_rows(k3, 10, 11)[700]
    fwd[1, row, 3] ^= 0x40
    assert ctx.check_ntt(a, fwd, k3, form=form, log_samples=10, seed=11) == dict(clean, row_failures=1)


# ----------------------------------------------------------------- 5. the checker
@pytest.mark.parametrize("form", FORMS)
def test_checker_on_every_row(ctx, form):
    """k = 9, log_samples = 9: every row. A forward row compares one cell of out,
    so one tampered output cell is one failure; an inverse row evaluates the
    whole of out and compares one cell of the input, so there one tampered input
    cell is one failure and a tampered output cell (a coefficient) fails every
    row."""
    import torch
    k, n = 9, 512
    cols = _three_columns(k)
    d = _device(cols, form)
    every = {"rows_checked": 3 * n, "row_failures": 0}
    for shift in (None, WIDE_SHIFT):
        s = 1 if shift is None else shift
        fwd, _ = ctx.ntt(d, k, shift=shift, form=form)
        bwd, _ = ctx.ntt(d, k, inverse=True, shift=shift, form=form)
        assert ctx.check_ntt(d, fwd, k, shift=shift, form=form, log_samples=k) == every
        assert ctx.check_ntt(d, bwd, k, inverse=True, shift=shift, form=form, log_samples=k) == every
        # the restatement's outputs, uploaded from the host
        hf = _device([ntt_forward(c, k, k, s) for c in cols], form)
        hb = _device([ntt_inverse(c, k, s) for c in cols], form)
        assert ctx.check_ntt(d, hf, k, shift=shift, form=form, log_samples=k) == every
        assert ctx.check_ntt(d, hb, k, inverse=True, shift=shift, form=form, log_samples=k) == every
        # fewer samples: the stratified rows only
        assert ctx.check_ntt(d, fwd, k, shift=shift, form=form, log_samples=4, seed=5) == \
            {"rows_checked": 3 * 16, "row_failures": 0}
    fwd, _ = ctx.ntt(d, k, form=form)
    bwd, _ = ctx.ntt(d, k, inverse=True, form=form)
    # one tampered cell
    t = fwd.clone()
    t[1, 77, 0] ^= 1
    assert ctx.check_ntt(d, t, k, form=form, log_samples=k) == dict(every, row_failures=1)
    t = d.clone()
    t[2, 300, 5] ^= 1
    assert ctx.check_ntt(t, bwd, k, inverse=True, form=form, log_samples=k) == dict(every, row_failures=1)
    t = bwd.clone()
    t[0, 5, 0] ^= 1
    assert ctx.check_ntt(d, t, k, inverse=True, form=form, log_samples=k) == dict(every, row_failures=n)
    # sampled rows see a tampered cell only where the rule samples it
    rows = sample_rows(k, 4, 5)
    t = fwd.clone()
    t[0, rows[3], 9] ^= 2
    assert ctx.check_ntt(d, t, k, form=form, log_samples=4, seed=5)["row_failures"] == 1
    miss = next(j for j in range(n) if j not in rows)
    t = fwd.clone()
    t[0, miss, 9] ^= 2
    assert ctx.check_ntt(d, t, k, form=form, log_samples=4, seed=5)["row_failures"] == 0
    # a wrong shift: every row fails, but possibly row 0 (the random column's rows all do)
    sh, _ = ctx.ntt(d[:1].contiguous(), k, shift=ZETA, form=form)
    bad = ctx.check_ntt(d[:1].contiguous(), sh, k, shift=WIDE_SHIFT, form=form, log_samples=k)
    assert bad["rows_checked"] == n and bad["row_failures"] >= n - 1
    si, _ = ctx.ntt(d[:1].contiguous(), k, inverse=True, shift=ZETA, form=form)
    bad = ctx.check_ntt(d[:1].contiguous(), si, k, inverse=True, shift=WIDE_SHIFT, form=form, log_samples=k)
    assert bad["rows_checked"] == n and bad["row_failures"] >= n - 1
    # an inverse without its 2^-k: every row with a nonzero input fails
    scaled = [[x * n % P_MOD for x in ntt_inverse(c, k)] for c in cols]
    bad = ctx.check_ntt(d, _device(scaled, form), k, inverse=True, form=form, log_samples=k)
    assert bad == dict(every, row_failures=sum(1 for c in cols for x in c if x))
    assert torch.equal(d, _device(cols, form))               # the checker writes to neither side


# --------------------------------------------------------- 6. eval_polynomial
@pytest.mark.parametrize("k", [1, 5, 10, 13])
def test_eval_polynomial_matches_horner(ctx, k):
    n = 1 << k
    cols = [_wide(n, 80 + k), [(7 * i + 1) % 13 for i in range(n - 1)] + [P_MOD - 1]]
    points = [0, 1, P_MOD - 1, omega(k), WIDE_SHIFT]
    want = np.stack([_cells([horner(c, x) for x in points]) for c in cols])
    for form in FORMS:
        d = _device(cols, form)
        got = ctx.eval_polynomial(d, k, points, form)
        assert tuple(got.shape) == (2, len(points), 32)
        assert np.array_equal(_canonical(got, form), want), form
        got = ctx.eval_polynomial([d[1:].contiguous(), d[:1].contiguous()], k, points[3:], form)
        assert np.array_equal(_canonical(got, form), want[::-1, 3:]), form
        assert tuple(ctx.eval_polynomial(d, k, [], form).shape) == (2, 0, 32)
        assert tuple(ctx.eval_polynomial([], k, points, form).shape) == (0, len(points), 32)


def test_eval_polynomial_more_points_than_one_launch(ctx):
    """32768 points go into one launch: one more, on a polynomial of two
    coefficients, a + b x."""
    a, b = WIDE_SHIFT, P_MOD - 7
    points = [(x * x + 3) % P_MOD for x in range(32769)]
    points[-1] = P_MOD - 1
    got = _canonical(ctx.eval_polynomial(_device([[a, b]], "canonical"), 1, points), "canonical")
    assert np.array_equal(got[0], _cells([(a + b * x) % P_MOD for x in points]))


def test_eval_polynomial_writes_nothing_without_points_or_columns(ctx):
    import halo2_svd041_amd as hs
    L = hs.zk.lib()
    d = _device([_wide(32, 1)], "canonical")
    out = _prefilled(1, 4)
    ptrs = (ct.c_void_p * 1)(d.data_ptr())
    pts = (ct.c_uint64 * 4)(5, 0, 0, 0)
    assert L.svdw_eval_polynomial(ctx._h, 5, 0, ptrs, 1, pts, 0, out.data_ptr()) == 0
    assert L.svdw_eval_polynomial(ctx._h, 5, 0, ptrs, 0, pts, 1, out.data_ptr()) == 0
    ctx.sync()
    assert bool((out == SENTINEL).all())


# ------------------------------------------------------------------ 7. end to end
def test_witness_columns_to_coefficients(ctx):
    """The advice columns of a 4 x 4 SVD witness and the Z of their permutation
    argument: lagrange_to_coeff, then the polynomial at omega^r is the cell at
    row r, and the checker is clean on every row."""
    import torch
    import halo2_svd041_amd as hs
    K, MIN_ROWS, UNUSABLE = 10, 20, 6
    rows = 1 << K
    m, u, d, v = gen_svd_input(4, 4, seed=44)
    hs.svd_witness(ctx, m, u, v, d, gamma_for(K))
    used = ctx.physical_layout(K, MIN_ROWS)["columns_used"]
    assert sum(used) >= 1
    for form in FORMS:
        adv = [ctx.assign_columns(ph, form=form)[0] for ph in (0, 1)]
        adv = [t for t in adv if t.shape[0]]
        ncols = sum(t.shape[0] for t in adv)
        sigma, bad = ctx.permutation_values(K, ncols=ncols, form=form)
        z, res = ctx.permutation_product(adv, sigma, gamma_for(1), gamma_for(2), 2, K, UNUSABLE, form)
        assert bad == 0 and res["final_not_one"] == 0
        cols = adv + [z]
        total = ncols + z.shape[0]
        coeffs, res = ctx.lagrange_to_coeff(cols, K, form, out=_prefilled(total, rows))
        assert res == _result(total, K, K)
        lag = np.concatenate([_canonical(t, form) for t in cols])
        assert lag[:ncols].any() and lag[ncols:].any()
        rs = (0, 1, rows - UNUSABLE)
        got = _canonical(ctx.eval_polynomial(coeffs, K, [pow(omega(K), r, P_MOD) for r in rs], form), form)
        for i, r in enumerate(rs):
            assert np.array_equal(got[:, i], lag[:, r]), (form, r)
        assert ctx.check_ntt(cols, coeffs, K, inverse=True, form=form, log_samples=K) == \
            {"rows_checked": total * rows, "row_failures": 0}
        # and one column against the restatement
        assert np.array_equal(_canonical(coeffs[:1], form)[0], _cells(ntt_inverse(cell_values(lag[0]), K)))


# ------------------------------------------------------ 8. no columns, an overlap
def test_no_columns_and_overlap(ctx):
    import torch
    import halo2_svd041_amd as hs
    from halo2_svd041_amd._lib import NttCheck, NttResult
    L = hs.zk.lib()
    k = 9
    out = _prefilled(1, 1 << k)
    r, c = NttResult(), NttCheck()
    ptrs = (ct.c_void_p * 1)(out.data_ptr())
    assert L.svdw_ntt(ctx._h, k, k, 0, 0, None, ptrs, 0, out.data_ptr(), ct.byref(r)) == 0
    assert (r.columns, r.passes, r.rows_in, r.rows_out) == (0, 1, 1 << k, 1 << k)
    assert L.svdw_check_ntt(ctx._h, k, k, 0, 0, None, ptrs, 0, out.data_ptr(), 3, 0, ct.byref(c)) == 0
    assert (c.rows_checked, c.row_failures) == (0, 0)
    out0, res = ctx.ntt([], k)
    assert tuple(out0.shape) == (0, 1 << k, 32) and res["columns"] == 0
    ctx.sync()
    assert bool((out == SENTINEL).all())
    # out over an input column, whole or in part
    d = _device([_wide(1 << k, 2), _wide(1 << k, 3)], "canonical")
    before = d.clone()
    shifted = d.view(-1)[16 * 32:(16 + (1 << k)) * 32].view(1, 1 << k, 32)   # 16 rows into column 0
    for cols, dst in ((d, d), (d[:1], shifted), (d[1:], shifted)):
        for inverse in (False, True):
            with pytest.raises(hs.SvdwError) as e:
                ctx.ntt(cols, k, inverse=inverse, out=dst)
            assert e.value.code == -1 and "overlaps" in str(e.value)
    ctx.sync()
    assert torch.equal(d, before)
    # next to each other is no overlap
    out1, _ = ctx.ntt(d[:1], k, out=d[1:])
    assert torch.equal(d[:1], before[:1]) and not torch.equal(out1, before[1:])


# ------------------------------------- 9. the prover calls alternate on one context
def test_families_share_one_context(gpu_ctx_factory):
    """The prover calls stage in one scratch and share the context's omega
    tables: transforms, a permutation product, a commitment and a lookup
    permutation in turn on one context, each against its Python-integer
    restatement, and the first transform again, byte for byte as before."""
    import torch
    import halo2_svd041_amd as hs
    from commit_cases import R, msm, parse_srs, point_bytes
    from lookup_perm_cases import MINIMUM_ROWS, WITNESS_CASES, argument_holds, lookup_columns, table_column
    from permutation_cases import CHALLENGES, cells_of, grand_products, identity_mapping, sigma_values
    N, M, P, LB, K, ncells, nlk = WITNESS_CASES[0]
    ctx = gpu_ctx_factory(P, LB)
    # 1. forward transform of 2 random columns, k = 4
    a = [_wide(16, 91), _wide(16, 92)]
    da = _device(a, "canonical")
    want_a = np.stack([_cells(ntt_forward(c, 4, 4)) for c in a])
    first, res = ctx.ntt(da, 4, out=_prefilled(2, 16))
    assert res == _result(2, 4, 4)
    assert np.array_equal(first.cpu().numpy(), want_a)
    # 2. permutation product, k = 5: 3 columns in sets of 2, the identity sigma
    k, unusable = 5, 6
    beta, gamma = CHALLENGES[0]
    cols = [_wide(32 - unusable, 93 + j) + [0] * unusable for j in range(3)]
    sig = sigma_values(identity_mapping(3, 32), k)
    Z, zeros = grand_products(cols, sig, beta, gamma, 2, k, unusable)
    ds, bad = ctx.permutation_values(k, ncols=3)
    assert bad == 0 and np.array_equal(ds.cpu().numpy(), np.stack([cells_of(c) for c in sig]))
    z, res = ctx.permutation_product(_device(cols, "canonical"), ds, beta, gamma, 2, k, unusable,
                                     out=_prefilled(2, 32))
    assert zeros == 0 and res == {"columns": 3, "sets": 2, "usable_rows": 32 - unusable, "zero_denominators": 0,
                                  "final_not_one": 0}, res
    assert np.array_equal(z.cpu().numpy(), np.stack([cells_of(c) for c in Z]))
    # 3. forward coset transform, k_in = 4 to k = 11: two passes, through the buffer between them
    assert hs.zk.lib().svdw_ntt_passes(11) == 2
    ext, res = ctx.coeff_to_extended(da, 4, 11, WIDE_SHIFT, out=_prefilled(2, 1 << 11))
    assert res == _result(2, 4, 11)
    assert np.array_equal(ext.cpu().numpy(), np.stack([_cells(ntt_forward(c, 4, 11, WIDE_SHIFT)) for c in a]))
    # 4. commitment of one k = 4 column to the first 16 bases of the SRS
    g = parse_srs()[1][:16]
    assert all(0 < s < R for s in a[0])
    bases = torch.from_numpy(np.frombuffer(point_bytes(g, "montgomery"), dtype=np.uint8).reshape(-1, 64).copy()).cuda()
    pts, res = ctx.commit(da[:1].contiguous(), bases, 4)
    assert pts.cpu().numpy().tobytes() == point_bytes([msm(g, a[0])], "montgomery")
    assert (res["columns"], res["zero_scalars"], res["identity_bases"], res["identity_outputs"]) == (1, 0, 0, 0), res
    # 5. lookup permutation of a small witness's phase-0 lookups
    m, u, d, v = gen_svd_input(N, M, seed=N + M + P)
    hs.svd_witness(ctx, m, u, v, d, gamma_for(1))
    assert ctx.physical_layout(K, MINIMUM_ROWS)["num_lookup_advice"] == [nlk, 0]
    vals = cell_values(ctx.lookups(0).view(np.uint8))
    assert len(vals) == ncells
    rows = 1 << K
    pa, pt, res = ctx.lookup_permute(0, unusable)
    assert (res["columns"], res["usable_rows"], res["out_of_table"]) == (nlk, rows - unusable, 0), res
    pa, pt = pa.cpu().numpy(), pt.cpu().numpy()
    assert not pa[:, rows - unusable:].any() and not pt[:, rows - unusable:].any()
    for j, col in enumerate(lookup_columns(vals, K)):
        argument_holds(col, table_column(LB, rows), cell_values(pa[j, :rows - unusable]),
                       cell_values(pt[j, :rows - unusable]), rows - unusable)
    # 6. the first transform again
    again, res = ctx.ntt(da, 4, out=_prefilled(2, 16))
    assert res == _result(2, 4, 4)
    assert torch.equal(again, first) and np.array_equal(again.cpu().numpy(), want_a)
    assert ctx.check_ntt(da, again, 4, log_samples=4) == {"rows_checked": 32, "row_failures": 0}
