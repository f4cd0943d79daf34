"""The two-level power tables (csrc/pow_table.hpp) and the context's per-k cache
of the domain's omega tables, through the calls that read them, byte for byte
against the restatements of ntt_cases.py, permutation_cases.py,
quotient_cases.py and open_cases.py: the splits at the smallest and at odd and
even k with the top exponent of both levels read, calls at two k alternating on
one context, the quotient with a cold and with a warm basis, openings whose
table is wider than their polynomial, and a context released with several
slots filled. Outputs are prefilled with a sentinel byte; both cell forms."""
import numpy as np
import pytest

from ntt_cases import P_MOD, WIDE_SHIFT, ntt_forward, ntt_inverse, spikes_forward, spikes_inverse
from open_cases import (T_POINT, U, V, X_POINT, Y, constant, evals, identity1, identity2, kernel_constant, open_h1,
                        open_h2, poly_mul, rand_poly, vanishing)
from permutation_cases import cells_of, identity_mapping, sigma_values
from quotient_cases import FAMILIES, SMALL_CASES, honest_instance, quotient_ext, to_coeffs, to_extended

pytestmark = pytest.mark.gpu

SENTINEL = 0xAB
FORMS = ("canonical", "montgomery")
SPLIT_KS = (1, 2, 5, 11)                                    # h = 1 with one upper cell; even; odd; two passes
LOG_TILE = kernel_constant("kOpenLogTile")


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


# ------------------------------------------------------ the transform cases
def _spikes(k: int) -> list:
    """Two spikes, one at the last row: its shift power and its omega powers are
    the top exponent of both levels of their tables."""
    n = 1 << k
    return [(n - 1, P_MOD - 5), (n // 3, WIDE_SHIFT)]


def _column(k: int) -> list:
    col = [0] * (1 << k)
    for row, value in _spikes(k):
        col[row] = value
    return col


def _want_transform(k: int, inverse: bool, shift: int) -> list:
    """The transform of _column(k) by the spike oracles; the shift as the
    header's formulas place it."""
    if inverse:
        return [c * pow(shift, i, P_MOD) % P_MOD for i, c in enumerate(spikes_inverse(_spikes(k), k))]
    return spikes_forward([(row, value * pow(shift, row, P_MOD) % P_MOD) for row, value in _spikes(k)], k)


_WANT = {}


def _want_cells(k: int, inverse: bool, shifted: bool) -> np.ndarray:
    """The oracle's cells, computed once per case and left unchanged."""
    key = (k, inverse, shifted)
    if key not in _WANT:
        want = _want_transform(k, inverse, WIDE_SHIFT if shifted else 1)
        if k <= 5:                                          # the two restatements agree where both are cheap
            direct = ntt_inverse(_column(k), k, WIDE_SHIFT if shifted else 1) if inverse else \
                ntt_forward(_column(k), k, k, WIDE_SHIFT if shifted else 1)
            assert direct == want
        _WANT[key] = _cells(want)[None]
        _WANT[key].setflags(write=False)
    return _WANT[key]


def _transform(ctx, k: int, inverse: bool, shifted: bool, form: str):
    out, res = ctx.ntt(_device([_column(k)], form), k, inverse=inverse, shift=WIDE_SHIFT if shifted else None,
                       form=form, out=_prefilled(1, 1 << k))
    assert res["columns"] == 1 and res["rows_out"] == 1 << k
    return out


# ---------------------------------------------------------- 1. split edge cases
@pytest.mark.parametrize("k", SPLIT_KS)
def test_split_edge_cases(gpu_ctx_factory, k):
    import halo2_svd041_amd as hs
    assert hs.zk.lib().svdw_ntt_passes(11) == 2 and hs.zk.lib().svdw_ntt_passes(5) == 1
    ctx = gpu_ctx_factory(32, 8)
    for form in FORMS:
        for inverse in (False, True):
            for shifted in (False, True):
                out = _transform(ctx, k, inverse, shifted, form)
                assert np.array_equal(_canonical(out, form), _want_cells(k, inverse, shifted)), \
                    (k, form, inverse, shifted)


# ------------------------------------------- 2. slots do not contaminate each other
def _alternate(ctx, form: str = "canonical"):
    """Calls at k = 5 and k = 11 in turn on one context; every output against its oracle."""
    import torch
    first = _transform(ctx, 5, False, True, form)
    assert np.array_equal(_canonical(first, form), _want_cells(5, False, True)), form
    wide = _transform(ctx, 11, False, True, form)
    assert np.array_equal(_canonical(wide, form), _want_cells(11, False, True)), form
    sigma, bad = ctx.permutation_values(5, ncols=3, form=form)
    want = np.stack([cells_of(c) for c in sigma_values(identity_mapping(3, 32), 5)])       # delta^c omega^r
    assert bad == 0 and np.array_equal(_canonical(sigma, form), want), form
    d = _device([_column(5)], form)
    assert ctx.check_ntt(d, first, 5, shift=WIDE_SHIFT, form=form, log_samples=5) == \
        {"rows_checked": 32, "row_failures": 0}
    again = _transform(ctx, 5, False, True, form)
    assert torch.equal(again, first), form
    assert np.array_equal(_canonical(again, form), _want_cells(5, False, True)), form
    inv11 = _transform(ctx, 11, True, False, form)          # the k = 11 slot after the k = 5 calls
    assert np.array_equal(_canonical(inv11, form), _want_cells(11, True, False)), form


@pytest.mark.parametrize("form", FORMS)
def test_slots_do_not_contaminate_each_other(gpu_ctx_factory, form):
    _alternate(gpu_ctx_factory(32, 8), form)


# --------------------------------------------------- 3. quotient order independence
def test_quotient_with_cold_and_warm_basis(gpu_ctx_factory):
    """The extended columns come from the host, so the first quotient is the
    context's first prover call: no transform has run, the basis is cold and no
    slot is filled. The second finds the basis and both slots as the first left
    them, after a transform at k that is not the quotient's extended k."""
    import torch
    inst = honest_instance(*SMALL_CASES[0])
    assert inst["perm_columns"] and inst["lookup_input"]     # the l columns are needed: the basis is built
    ext = to_extended(to_coeffs(inst))
    want = _cells(quotient_ext(ext))
    k, ek = inst["k"], inst["extended_k"]
    par = dict(k=k, extended_k=ek, shift=inst["shift"], beta=inst["beta"], gamma=inst["gamma"], y=inst["y"],
               chunk_len=inst["chunk_len"], unusable_rows=inst["unusable"])
    for form in FORMS:
        ctx = gpu_ctx_factory(32, 8)
        fams = {f: _device(ext[f], form) for f in FAMILIES if ext[f]}
        cold, _ = ctx.quotient(form=form, out=_prefilled(1, 1 << ek), **par, **fams)
        assert np.array_equal(_canonical(cold, form)[0], want), (form, "cold")
        ctx.ntt(_device([[1] * (1 << k)], form), k, form=form)
        warm, _ = ctx.quotient(form=form, out=_prefilled(1, 1 << ek), **par, **fams)
        assert torch.equal(warm, cold), form
        assert np.array_equal(_canonical(warm, form)[0], want), (form, "warm")


# ------------------------------------------------------- 4. opening below the tile
@pytest.mark.parametrize("k", [3, LOG_TILE + 1])
def test_opening_with_a_table_wider_than_the_polynomial(gpu_ctx_factory, k):
    """k = 3: the points' tables cover 2^kOpenLogTile exponents, not 2^k. Two
    point sets; every polynomial vanishes on its set, so the interpolants, the
    verifier's constant and with it the remainder of the linearisation are zero."""
    assert LOG_TILE > 3
    ctx = gpu_ctx_factory(32, 8)
    n = 1 << k
    sets = [[X_POINT, 5], [X_POINT * 7 % P_MOD]]
    set_of = [1, 0, 1]
    polys = [poly_mul(vanishing(sets[s]), rand_poly(n - len(sets[s]), 300 + 10 * k + j)) for j, s in enumerate(set_of)]
    assert all(len(p) == n for p in polys)
    want1 = open_h1(polys, set_of, sets, Y, V)
    want2, rem = open_h2(polys, set_of, sets, Y, V, U, want1)
    assert rem == 0 == constant(polys, set_of, sets, Y, V, U) and any(want1) and any(want2)
    l1, r1 = identity1(polys, set_of, sets, Y, V, want1, T_POINT)
    l2, r2 = identity2(polys, set_of, sets, Y, V, U, want1, want2, T_POINT)
    assert l1 == r1 and l2 == r2
    clean = {"lhs1": l1, "rhs1": r1, "lhs2": l2, "rhs2": r2, "constant": 0, "identity1_failures": 0,
             "identity2_failures": 0, "h1_top_checked": 1, "h1_top_nonzero": 0, "h2_top_checked": 1,
             "h2_top_nonzero": 0, "evals": evals(polys, set_of, sets)}
    res1 = {"columns": 3, "sets": 2, "points": 3, "passes": 3, "rows": n, "remainder": 0}
    for form in FORMS:
        d = _device(polys, form)
        h1, res = ctx.open_quotient(d, set_of, sets, Y, V, k, form=form, out=_prefilled(1, n))
        assert res == res1, (form, res)
        assert np.array_equal(_canonical(h1, form)[0], _cells(want1)), (k, form, "h1")
        h2, res = ctx.open_linearise(d, set_of, sets, Y, V, U, h1, k, form=form, out=_prefilled(1, n))
        assert res == dict(res1, passes=1), (form, res)
        assert np.array_equal(_canonical(h2, form)[0], _cells(want2)), (k, form, "h2")
        assert ctx.check_open(d, set_of, sets, Y, V, U, h1, h2, T_POINT, k, form=form) == clean, form


# ------------------------------------------------------------------- 5. release
def test_release_with_filled_slots(gpu_ctx_factory):
    """A context with the slots of k = 5 and k = 11 filled is reset, used again
    and closed; a context made afterwards starts from empty slots and gives the
    same bytes."""
    ctx = gpu_ctx_factory(32, 8)
    _alternate(ctx)
    ctx.reset()
    out = _transform(ctx, 5, True, True, "canonical")       # the slots outlive a reset
    assert np.array_equal(out.cpu().numpy(), _want_cells(5, True, True))
    ctx.close()
    second = gpu_ctx_factory(32, 8)
    for inverse in (False, True):
        for shifted in (False, True):
            out = _transform(second, 5, inverse, shifted, "canonical")
            assert np.array_equal(out.cpu().numpy(), _want_cells(5, inverse, shifted)), (inverse, shifted)
