"""svdw_open_quotient / svdw_open_linearise / svdw_check_open /
svdw_linear_combination on the device against the integer oracle
(open_cases.py): the sizes around the tile and at the carry stage's second
round, the shapes of rotation sets, degenerate coefficients and points, the
chain through the checker with tampering, the linear combination and the
pieces of h, a witness end to end with the commitments of h1 and h2, and the
edge arguments. Outputs are prefilled with a sentinel byte; both cell forms;
comparisons byte for byte after conversion."""
import ctypes as ct

import numpy as np
import pytest

from commit_cases import msm, parse_srs, point_bytes
from conftest import gamma_for, gen_svd_input
from lookup_perm_cases import cell_values
from ntt_cases import ZETA, ntt_forward
from open_cases import (P_MOD, T_POINT, U, V, X_POINT, Y, circuit_sets, constant, evals, horner, identity1, identity2,
                        kernel_constant, linear_combination, omega, open_h1, open_h2, rand_poly, union)

pytestmark = pytest.mark.gpu

SENTINEL = 0xAB
FORMS = ("canonical", "montgomery")
LOG_TILE = kernel_constant("kOpenLogTile")
TILE, CARRY_CAP = kernel_constant("kOpenTile"), kernel_constant("kOpenCarryCap")
SECOND_ROUND_K = (TILE * CARRY_CAP).bit_length()           # the smallest k with more tiles than one round takes
assert SECOND_ROUND_K <= 18, "the second round of the carry stage lies beyond the sizes the suite runs"
assert TILE == 1 << LOG_TILE and (1 << SECOND_ROUND_K) // TILE > CARRY_CAP >= (1 << (SECOND_ROUND_K - 1)) // TILE


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


def _prefilled(rows: int):
    import torch
    return torch.full((1, rows, 32), SENTINEL, dtype=torch.uint8, device="cuda")


def _split(t):
    """A column tensor as a list of tensors, one column first."""
    return [t[:1].contiguous(), t[1:].contiguous()] if t.shape[0] > 1 else [t]


def _chain(ctx, polys, set_of, sets, k: int, split: bool = False, forms=FORMS):
    """open_quotient, then open_linearise on the device's own h1, in every form,
    byte for byte against the oracle; (h1, h2, constant) of the oracle."""
    n = 1 << k
    want1 = open_h1(polys, set_of, sets, Y, V)
    want2, rem = open_h2(polys, set_of, sets, Y, V, U, want1)
    top = min(len(s) for s in sets)                         # the degree of h1 is that of the smallest set's Q_i
    assert all(c == 0 for c in want1[n - min(top, n):]) and want2[-1] == 0
    res1 = {"columns": len(polys), "sets": len(sets), "points": len(union(sets)),
            "passes": sum(len(s) for s in sets), "rows": n, "remainder": 0}
    for form in forms:
        d = _device(polys, form)
        cols = _split(d) if split else d
        h1, res = ctx.open_quotient(cols, set_of, sets, Y, V, k, form=form, out=_prefilled(n))
        assert res == res1, (form, res)
        assert np.array_equal(_canonical(h1, form)[0], _cells(want1)), (k, form, "h1")
        h2, res = ctx.open_linearise(cols, set_of, sets, Y, V, U, h1, k, form=form, out=_prefilled(n))
        assert res == dict(res1, passes=1, remainder=rem), (form, res)
        assert np.array_equal(_canonical(h2, form)[0], _cells(want2)), (k, form, "h2")
        assert np.array_equal(_canonical(d, form), np.stack([_cells(p) for p in polys]))   # the inputs as they were
    return want1, want2, rem


# ------------------------------------------------------------------ 1. sizes
@pytest.mark.parametrize("k", sorted({1, 2, LOG_TILE - 1, LOG_TILE, LOG_TILE + 1, LOG_TILE + 2}))
def test_sizes_around_the_tile(ctx, k):
    """One set of one point, then (from 16 coefficients on) two sets, one of 8
    points: a single partial tile, exactly one tile, two and four tiles."""
    n = 1 << k
    polys = [rand_poly(n, 10 * k + j) for j in range(3)]
    _, _, rem = _chain(ctx, polys[:2], [0, 0], [[X_POINT]], k)
    assert rem == constant(polys[:2], [0, 0], [[X_POINT]], Y, V, U)
    if n >= 16:
        sets = [[X_POINT * pow(omega(k), r, P_MOD) % P_MOD for r in range(8)], [X_POINT, 5]]
        _chain(ctx, polys, [1, 0, 1], sets, k, split=True)


def test_second_round_of_the_carry_stage(ctx):
    """Two columns and one one-point set at the smallest k at which the tile
    totals do not fit one round of the carry stage."""
    k = SECOND_ROUND_K
    polys = [rand_poly(1 << k, 170 + j) for j in range(2)]
    _chain(ctx, polys, [0, 0], [[X_POINT]], k)


# ----------------------------------------------------------------- 2. shapes
def _circuit(k: int, seed: int, unusable: int = 6):
    set_of, sets = circuit_sets(k, unusable, X_POINT)
    return [rand_poly(1 << k, seed + j) for j in range(len(set_of))], set_of, sets


def test_one_set_of_eight_points(ctx):
    k = 10
    pts = [X_POINT * pow(omega(k), r, P_MOD) % P_MOD for r in (0, 1, 2, 3, 1018, 1023)] + [3, P_MOD - 1]
    _chain(ctx, [rand_poly(1 << k, 21), rand_poly(1 << k, 22)], [0, 0], [pts], k)


def test_circuit_shape_set_of_not_sorted_and_split_tensors(ctx):
    """The five rotation sets of the circuit shape with eleven polynomials,
    set_of not sorted, as one tensor and as several."""
    k = 10
    polys, set_of, sets = _circuit(k, 30)
    assert len(polys) == 11 and len(sets) == 5 and set_of != sorted(set_of) and len(union(sets)) == 6
    _chain(ctx, polys, set_of, sets, k)
    _chain(ctx, polys, set_of, sets, k, split=True, forms=FORMS[1:])
    k = 5                                                   # the issue's own size
    polys, set_of, sets = _circuit(k, 40)
    _chain(ctx, polys, set_of, sets, k)


# ----------------------------------------------- 3. degenerate coefficients, points
@pytest.mark.parametrize("name", ["zero", "top", "constant", "minus_one"])
def test_degenerate_coefficients(ctx, name):
    k = LOG_TILE + 1
    n = 1 << k
    col = {"zero": [0] * n, "top": [0] * (n - 1) + [X_POINT], "constant": [U] + [0] * (n - 1),
           "minus_one": [P_MOD - 1] * n}[name]
    sets = [[X_POINT, X_POINT * omega(k) % P_MOD, 7], [X_POINT]]
    want1, want2, rem = _chain(ctx, [col, col, col], [0, 1, 0], sets, k)
    if name in ("zero", "constant"):                        # nothing to divide: constants fold into the remainders
        assert not any(want1) and (name == "constant" or (not any(want2) and rem == 0))


@pytest.mark.parametrize("s", [0, 1, P_MOD - 1])
def test_points_where_the_power_tables_degenerate(ctx, s):
    k = LOG_TILE + 2
    polys = [rand_poly(1 << k, 50 + j) for j in range(3)]
    want1, _, _ = _chain(ctx, polys, [0, 1, 1], [[s], [X_POINT, s]], k)
    assert any(want1)


# ------------------------------------------------------------------ 4. chain
def test_chain_through_the_checker(ctx):
    """check_open passes on the device's h1 and h2 and returns the oracle's
    evals and both sides of both identities; a changed cell of h1, of h2 or of an
    input column, or another u, fails the identity concerned; open_linearise on a
    tampered h1 reports a remainder that is not the constant."""
    k = 10
    n = 1 << k
    polys, set_of, sets = _circuit(k, 60)
    want1 = open_h1(polys, set_of, sets, Y, V)
    want2, rem = open_h2(polys, set_of, sets, Y, V, U, want1)
    cst = constant(polys, set_of, sets, Y, V, U)
    assert rem == cst
    l1, r1 = identity1(polys, set_of, sets, Y, V, want1, T_POINT)
    l2, r2 = identity2(polys, set_of, sets, Y, V, U, want1, want2, T_POINT)
    assert l1 == r1 and l2 == r2
    clean = {"lhs1": l1, "rhs1": r1, "lhs2": l2, "rhs2": r2, "constant": cst, "identity1_failures": 0,
             "identity2_failures": 0, "h1_top_checked": 1, "h1_top_nonzero": 0, "h2_top_checked": 1,
             "h2_top_nonzero": 0, "evals": evals(polys, set_of, sets)}
    one = _device([[1]], "canonical")[0, 0]
    for form in FORMS:
        d = _device(polys, form)
        h1, _ = ctx.open_quotient(d, set_of, sets, Y, V, k, form=form)
        h2, res = ctx.open_linearise(d, set_of, sets, Y, V, U, h1, k, form=form)
        assert res["remainder"] == cst
        args = (set_of, sets, Y, V)
        assert ctx.check_open(d, *args, U, h1, h2, T_POINT, k, form=form) == clean, form
        assert ctx.check_open(_split(d), *args, U, h1, h2, gamma_for(9), k, form=form)["identity1_failures"] == 0
        # a cell of h1: identity 1 (and G, so identity 2); its top cell is counted too
        bad = h1.clone()
        bad[0, 5] = one
        got = ctx.check_open(d, *args, U, bad, h2, T_POINT, k, form=form)
        assert got["identity1_failures"] == 1 and got["identity2_failures"] == 1 and got["evals"] == clean["evals"]
        _, res = ctx.open_linearise(d, *args, U, bad, k, form=form)
        assert res["remainder"] != cst
        bad = h1.clone()
        bad[0, n - 1] = one
        assert ctx.check_open(d, *args, U, bad, h2, T_POINT, k, form=form)["h1_top_nonzero"] == 1
        # a cell of h2: identity 2 alone
        bad = h2.clone()
        bad[0, 700] = one
        got = ctx.check_open(d, *args, U, h1, bad, T_POINT, k, form=form)
        assert (got["identity1_failures"], got["identity2_failures"]) == (0, 1), (form, got)
        bad = h2.clone()
        bad[0, n - 1] = one
        assert ctx.check_open(d, *args, U, h1, bad, T_POINT, k, form=form)["h2_top_nonzero"] == 1
        # a cell of an input column: identity 1
        bad = d.clone()
        bad[4, 600] = one
        got = ctx.check_open(bad, *args, U, h1, h2, T_POINT, k, form=form)
        assert got["identity1_failures"] == 1 and got["evals"] != clean["evals"]
        # another u: identity 1 does not know it, identity 2 fails
        got = ctx.check_open(d, *args, U + 1, h1, h2, T_POINT, k, form=form)
        assert (got["identity1_failures"], got["identity2_failures"]) == (0, 1), (form, got)


# ------------------------------------------------------ 5. linear combination
def test_linear_combination_and_the_pieces_of_h(ctx):
    import torch
    k, E = LOG_TILE + 1, 4
    n = 1 << k
    polys = [rand_poly(n, 70 + j) for j in range(5)]
    scalars = [Y, 0, 1, P_MOD - 1, V]
    want = linear_combination(polys, scalars)
    h = rand_poly(E * n, 80)
    xs = [pow(X_POINT, n * i, P_MOD) for i in range(E)]
    pieces = [h[i * n:(i + 1) * n] for i in range(E)]
    combined = linear_combination(pieces, xs)
    assert horner(combined, X_POINT) == horner(h, X_POINT)  # the one polynomial create_proof opens for h
    for form in FORMS:
        d = _device(polys, form)
        out = ctx.linear_combination(d, scalars, k, form=form, out=_prefilled(n))
        assert np.array_equal(_canonical(out, form)[0], _cells(want)), form
        out = ctx.linear_combination(_split(d), scalars, k, form=form)
        assert np.array_equal(_canonical(out, form)[0], _cells(want)), form
        hc = _device([h], form)                             # [1, E n, 32], as extended_to_coeff leaves h
        out = ctx.linear_combination(hc.view(E, n, 32), xs, k, form=form, out=_prefilled(n))
        assert np.array_equal(_canonical(out, form)[0], _cells(combined)), form
        small = ctx.linear_combination(_device([[3, 4]], form), [5], 1, form=form)
        assert np.array_equal(_canonical(small, form)[0], _cells([15, 20])), form
        assert torch.equal(d, _device(polys, form))


# ------------------------------------------------------- 6. a witness end to end
def test_witness_end_to_end(ctx):
    """The assigned advice columns and selectors of a 6 x 6 SVD witness at k = 8
    (the size of the SRS, below what a lookup table of 2^8 rows needs, so the
    gates and the permutation argument alone), through the existing calls to
    coefficient form, the quotient and the pieces of h; the rotation sets from
    shplonk_queries; h1 and h2 committed on the SRS equal the naive MSM of the
    oracle's coefficients, and the checker passes."""
    import torch
    import halo2_svd041_amd as hs
    K, EK, MIN_ROWS, UNUSABLE, CHUNK = 8, 10, 19, 6, 2      # at minimum_rows 20 the gates' breaks need a column more
    rows, E = 1 << K, 4
    beta, gamma, yq, x = gamma_for(1), gamma_for(2), gamma_for(3), gamma_for(4)
    k_srs, g, _ = parse_srs()
    assert k_srs == K
    bases = torch.from_numpy(np.frombuffer(point_bytes(g, "montgomery"), dtype=np.uint8).reshape(-1, 64).copy()).cuda()
    m, u, d, v = gen_svd_input(6, 6, seed=66)
    hs.svd_witness(ctx, m, u, v, d, gamma_for(K))
    ctx.physical_layout(K, MIN_ROWS)
    want = None
    for form in FORMS:
        assigned = [ctx.assign_columns(ph, form=form) for ph in (0, 1)]
        adv = torch.cat([a[0] for a in assigned])
        sel8 = torch.cat([a[1] for a in assigned])
        assert adv.shape[0] >= 2
        sel = np.zeros((sel8.shape[0], rows, 32), dtype=np.uint8)      # the selector bytes widened to cells
        sel[:, :, 0] = sel8.cpu().numpy()
        sel = torch.from_numpy(_in_form(sel, form)).cuda()
        sigma, bad = ctx.permutation_values(K, ncols=adv.shape[0], form=form)
        pz, res = ctx.permutation_product(adv, sigma, beta, gamma, CHUNK, K, UNUSABLE, form)
        assert bad == 0 and res["final_not_one"] == 0
        lag = dict(advice=adv, selectors=sel, perm_columns=adv, sigma=sigma, perm_z=pz)
        co = {f: ctx.lagrange_to_coeff(t, K, form)[0] for f, t in lag.items()}
        ext = {f: ctx.coeff_to_extended(t, K, EK, ZETA, form=form)[0] for f, t in co.items()}
        par = dict(k=K, extended_k=EK, shift=ZETA, beta=beta, gamma=gamma, y=yq, chunk_len=CHUNK,
                   unusable_rows=UNUSABLE, form=form)
        h_ext, _ = ctx.quotient(**par, **ext)
        hc, _ = ctx.extended_to_coeff(h_ext, EK, ZETA * ZETA % P_MOD, form=form)
        assert ctx.check_quotient(hc, x, **par, **co)["identity_failures"] == 0
        h = ctx.linear_combination(hc.view(E, rows, 32), [pow(x, rows * i, P_MOD) for i in range(E)], K, form=form)
        # the columns in the order shplonk_queries documents
        cols = [co["advice"], co["selectors"], co["sigma"], co["perm_z"], h]
        set_of, sets = hs.zk.shplonk_queries(K, UNUSABLE, adv.shape[0], adv.shape[0], CHUNK, 0, x)
        assert len(set_of) == sum(t.shape[0] for t in cols) and len(sets) == 4 and pz.shape[0] >= 2
        if want is None:
            assert form == "canonical"
            polys = [cell_values(c) for t in cols for c in t.cpu().numpy()]
            h1 = open_h1(polys, set_of, sets, Y, V)
            h2, rem = open_h2(polys, set_of, sets, Y, V, U, h1)
            want = (h1, h2, rem, [msm(g, h1), msm(g, h2)], evals(polys, set_of, sets))
            assert rem == constant(polys, set_of, sets, Y, V, U) and any(h1) and any(h2)
            # the oracle reads the device's coefficients: they are those of the assigned column
            assert ntt_forward(polys[0], K, K) == cell_values(adv[0].cpu().numpy())
        d1, res = ctx.open_quotient(cols, set_of, sets, Y, V, K, form=form, out=_prefilled(rows))
        assert res["columns"] == len(set_of) and res["points"] == 5 and res["passes"] == 10
        d2, res = ctx.open_linearise(cols, set_of, sets, Y, V, U, d1, K, form=form, out=_prefilled(rows))
        assert res["remainder"] == want[2]
        assert np.array_equal(_canonical(d1, form)[0], _cells(want[0])), form
        assert np.array_equal(_canonical(d2, form)[0], _cells(want[1])), form
        pts, _ = ctx.commit_coeffs([d1, d2], bases, K, form=form)
        assert pts.cpu().numpy().tobytes() == point_bytes(want[3], "montgomery"), form
        got = ctx.check_open(cols, set_of, sets, Y, V, U, d1, d2, T_POINT, K, form=form)
        assert got["identity1_failures"] == got["identity2_failures"] == 0 and got["constant"] == want[2]
        assert got["evals"] == want[4] and got["h1_top_nonzero"] == got["h2_top_nonzero"] == 0


# ------------------------------------------------------------ 7. edge arguments
def test_every_documented_refusal_in_order(ctx):
    import torch
    import halo2_svd041_amd as hs
    from halo2_svd041_amd._lib import OpenCheck, OpenResult
    L = hs.zk.lib()
    k = 6
    n = 1 << k
    polys = [rand_poly(n, 90 + j) for j in range(3)]
    d = _device(polys, "canonical")
    set_of, sets = [0, 1, 0], [[3, 5], [7]]
    h1, h2 = _prefilled(n), _prefilled(n)
    good = dict(columns=d, set_of=set_of, sets=sets, y=Y, v=V, k=k)
    none = torch.empty((3, 0, 32), dtype=torch.uint8, device="cuda")   # what k = 40 makes of 2^k rows: k is checked first
    refusals = [
        (dict(form="bogus", sets=[[3, 3], [7]]), -1, "form"),
        (dict(y=P_MOD, sets=[[3, 3], [7]]), -1, "challenge"),
        (dict(sets=[[3, P_MOD], [7, 7]]), -1, "challenge"),    # the wrapper's own refusal of a point
        (dict(sets=[[3, 3], [7]], set_of=[0, 2, 0]), -1, "equal points"),
        (dict(set_of=[0, 2, 0], k=40, columns=none, out=None), -1, "set_of"),
        (dict(set_of=[0, 0, 0], k=40, columns=none, out=None), -1, "without a polynomial"),
        (dict(k=40, columns=none, out=None), -2, "k must be"),
        (dict(columns=[d[:1]] * 65536, set_of=[i % 256 for i in range(65536)], sets=[[i + 1] for i in range(256)]),
         -2, "65535"),
        (dict(sets=[[3, 5], [7], []] + [[9 + i] for i in range(253)], set_of=[0, 1, 2]), -1, "without a polynomial"),
        (dict(sets=[[3, 5], list(range(10, 19))]), -2, "npoints"),
        (dict(columns=[d[:1], d[1:2]] + [d[2:]] * 254, set_of=list(range(256)), sets=[[i + 1] for i in range(256)]),
         -2, "nsets"),
    ]
    for over, code, word in refusals:
        kw = dict(good, **over)
        o1, o2 = kw.pop("out", h1), (h2 if "out" not in over else None)
        with pytest.raises(hs.SvdwError) as e:
            ctx.open_quotient(out=o1, **kw)
        assert e.value.code == code and word in str(e.value), (over, str(e.value))
        with pytest.raises(hs.SvdwError) as e:
            ctx.open_linearise(kw["columns"], kw["set_of"], kw["sets"], kw["y"], kw["v"], U, o1, kw["k"],
                               form=kw.get("form", "canonical"), out=o2)
        assert e.value.code == code and word in str(e.value), (over, str(e.value))
    # u in T, after the empty set and before k
    for u in (3, 7):
        with pytest.raises(hs.SvdwError) as e:
            ctx.open_linearise(none, set_of, sets, Y, V, u, None, 40)
        assert e.value.code == -1 and "one of the points" in str(e.value)
        with pytest.raises(hs.SvdwError) as e:
            ctx.check_open(none, set_of, sets, Y, V, u, None, None, T_POINT, 40)
        assert e.value.code == -1 and "one of the points" in str(e.value)
    # null pointers, through the ABI
    so = (ct.c_uint32 * 3)(*set_of)
    npts = (ct.c_uint32 * 2)(2, 1)
    pts = (ct.c_uint64 * 64)()
    pts[0], pts[4], pts[32] = 3, 5, 7
    w = lambda x: (ct.c_uint64 * 4)(*[(x >> (64 * i)) & (2 ** 64 - 1) for i in range(4)])
    cp = (ct.c_void_p * 3)(*[d.data_ptr() + i * n * 32 for i in range(3)])
    holed = (ct.c_void_p * 3)(d.data_ptr(), None, d.data_ptr())
    r, c = OpenResult(), OpenCheck()
    ev = (ct.c_uint64 * 96)()
    common = lambda cols: (ctx._h, k, 0, cols, 3, so, pts, npts, 2, w(Y), w(V))
    assert L.svdw_open_quotient(*common(cp), None, ct.byref(r)) == -1
    assert L.svdw_open_quotient(*common(None), h1.data_ptr(), ct.byref(r)) == -1
    assert L.svdw_open_quotient(*common(holed), h1.data_ptr(), ct.byref(r)) == -1
    assert L.svdw_open_quotient(*common(cp), h1.data_ptr(), None) == -1
    assert L.svdw_open_linearise(*common(cp), w(U), None, h2.data_ptr(), ct.byref(r)) == -1
    assert L.svdw_open_linearise(*common(cp), w(U), h1.data_ptr(), None, ct.byref(r)) == -1
    assert L.svdw_check_open(*common(cp), w(U), h1.data_ptr(), None, w(T_POINT), ev, ct.byref(c)) == -1
    assert L.svdw_check_open(*common(cp), w(U), h1.data_ptr(), h2.data_ptr(), w(T_POINT), None, ct.byref(c)) == -1
    assert L.svdw_linear_combination(ctx._h, k, 0, holed, 3, pts, h1.data_ptr()) == -1
    assert L.svdw_linear_combination(ctx._h, k, 0, cp, 3, pts, None) == -1
    # ncols == 0: SVDW_OK, nothing is touched
    assert L.svdw_open_quotient(ctx._h, k, 0, None, 0, None, None, None, 0, w(Y), w(V), h1.data_ptr(), ct.byref(r)) == 0
    assert (r.columns, r.sets, r.points, r.passes, r.rows) == (0, 0, 0, 0, n)
    assert L.svdw_open_linearise(ctx._h, k, 0, None, 0, None, None, None, 0, w(Y), w(V), w(U), h1.data_ptr(),
                                 h2.data_ptr(), ct.byref(r)) == 0
    assert L.svdw_check_open(ctx._h, k, 0, None, 0, None, None, None, 0, w(Y), w(V), w(U), h1.data_ptr(),
                             h2.data_ptr(), w(T_POINT), ev, ct.byref(c)) == 0
    assert L.svdw_linear_combination(ctx._h, k, 0, None, 0, None, h1.data_ptr()) == 0
    empty = torch.empty((0, n, 32), dtype=torch.uint8, device="cuda")
    _, res = ctx.open_quotient(empty, [], [], Y, V, k, out=h1)
    assert res["columns"] == 0
    ctx.sync()
    assert bool((h1 == SENTINEL).all()) and bool((h2 == SENTINEL).all())
    # an output over an input column, whole or in part, and h2 over h1
    before = d.clone()
    flat = torch.cat([d, _prefilled(n)])
    shifted = flat.view(-1)[(2 * n + 16) * 32:(3 * n + 16) * 32].view(1, n, 32)     # 16 rows into column 2
    for dst in (flat[1:2], shifted):
        with pytest.raises(hs.SvdwError) as e:
            ctx.open_quotient(flat[:3], set_of, sets, Y, V, k, out=dst)
        assert e.value.code == -1 and "overlaps" in str(e.value)
        with pytest.raises(hs.SvdwError) as e:
            ctx.open_linearise(flat[:3], set_of, sets, Y, V, U, flat[3:4], k, out=dst)
        assert e.value.code == -1 and "overlaps" in str(e.value)
        with pytest.raises(hs.SvdwError) as e:
            ctx.linear_combination(flat[:3], [1, 2, 3], k, out=dst)
        assert e.value.code == -1 and "overlaps" in str(e.value)
    with pytest.raises(hs.SvdwError) as e:
        ctx.open_linearise(d, set_of, sets, Y, V, U, h1, k, out=h1)
    assert e.value.code == -1 and "overlaps h1" in str(e.value)
    with pytest.raises(hs.SvdwError) as e:
        ctx.linear_combination(d, [1, 2, P_MOD], k)
    assert e.value.code == -1
    ctx.sync()
    assert torch.equal(flat[:3], before) and torch.equal(d, before) and bool((flat[3] == SENTINEL).all())
    # an out tensor of the caller's is filled in place
    got, _ = ctx.open_quotient(d, set_of, sets, Y, V, k, out=h1)
    assert got is h1 and np.array_equal(h1.cpu().numpy()[0], _cells(open_h1(polys, set_of, sets, Y, V)))


def test_openings_alternate_with_the_other_families(ctx):
    """The opening calls stage in the scratch the other prover calls use: an
    opening, a transform, a commitment, a linear combination and the opening
    again on one context, each against its restatement, the last byte for byte
    as the first."""
    import torch
    k = 8
    n = 1 << k
    polys, set_of, sets = _circuit(k, 100)
    d = _device(polys, "canonical")
    want1 = open_h1(polys, set_of, sets, Y, V)
    want2, rem = open_h2(polys, set_of, sets, Y, V, U, want1)
    first, _ = ctx.open_quotient(d, set_of, sets, Y, V, k, out=_prefilled(n))
    assert np.array_equal(first.cpu().numpy()[0], _cells(want1))
    lag, _ = ctx.coeff_to_lagrange(d[:2].contiguous(), k)
    assert np.array_equal(lag.cpu().numpy(), np.stack([_cells(ntt_forward(p, k, k)) for p in polys[:2]]))
    h2, res = ctx.open_linearise(d, set_of, sets, Y, V, U, first, k, out=_prefilled(n))
    assert res["remainder"] == rem and np.array_equal(h2.cpu().numpy()[0], _cells(want2))
    g = parse_srs()[1]
    bases = torch.from_numpy(np.frombuffer(point_bytes(g, "montgomery"), dtype=np.uint8).reshape(-1, 64).copy()).cuda()
    pts, _ = ctx.commit_coeffs(first, bases, k)
    assert pts.cpu().numpy().tobytes() == point_bytes([msm(g, want1)], "montgomery")
    lc = ctx.linear_combination(d[:3].contiguous(), [1, Y, V], k)
    assert np.array_equal(lc.cpu().numpy()[0], _cells(linear_combination(polys[:3], [1, Y, V])))
    ev = ctx.eval_polynomial(first, k, [T_POINT])
    assert cell_values(ev.cpu().numpy()[0]) == [horner(want1, T_POINT)]
    assert ctx.check_open(d, set_of, sets, Y, V, U, first, h2, T_POINT, k)["identity2_failures"] == 0
    again, _ = ctx.open_quotient(d, set_of, sets, Y, V, k, out=_prefilled(n))
    assert torch.equal(again, first)
