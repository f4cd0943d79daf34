"""svdw_quotient / svdw_check_quotient on the device against the literal
restatement (quotient_cases.py; parity of the rule itself unpinned):
h_ext in full at one block and at several, with each family alone, each family
left out, two lookup arguments and column lists split over tensors; the round
trip through extended_to_coeff and the checker; the checker itself against the
restatement's h and against tampering; an SVD witness end to end; one mid size
through the checker alone; no-ops and refusals. Outputs are prefilled with a
sentinel byte; both forms throughout; comparisons byte for byte after
fr_convert."""
import ctypes as ct
import functools

import numpy as np
import pytest

from conftest import gamma_for, gen_svd_input
from lookup_perm_cases import table_column
from quotient_cases import (BETA, FAMILIES, GAMMA, P_MOD, SMALL_CASES, Y, ZETA, combined_at, degree, honest_instance,
                            horner, inv, ntt_inverse, quotient_ext, tail_start, to_coeffs, to_extended, without)

pytestmark = pytest.mark.gpu

SENTINEL = 0xAB
FORMS = ("canonical", "montgomery")
X = 0x1d2c3b4a59687766554433221100ffeeddccbbaa99887766554433221100abcd % P_MOD
BLOCK_CASES = [(8, 10, 6, 2), (8, 11, 6, 3)]               # several blocks; rotations wrap across block and array ends


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


def _families(inst: dict, form: str) -> dict:
    """The instance's non-empty families as device tensors in `form`."""
    return {f: _device(inst[f], form) for f in FAMILIES if inst[f]}


def _params(inst: dict, **over) -> dict:
    kw = dict(k=inst["k"], extended_k=inst["extended_k"], shift=inst["shift"], beta=inst["beta"], gamma=inst["gamma"],
              y=inst["y"], chunk_len=inst["chunk_len"], unusable_rows=inst["unusable"])
    kw.update(over)
    return kw


def _extend(ctx, inst: dict, fams: dict, form: str) -> dict:
    """Coefficient tensors onto the coset, by the device's own coeff_to_extended."""
    return {f: ctx.coeff_to_extended(t, inst["k"], inst["extended_k"], inst["shift"], form=form)[0]
            for f, t in fams.items()}


def _split(t):
    """A column tensor as a list of tensors, one column first."""
    return [t[:1].contiguous(), t[1:].contiguous()] if t.shape[0] > 1 else [t]


@functools.lru_cache(maxsize=None)
def _case(case, n_lookup=1):
    """(instance, coefficient columns, h_ext and the coefficients of h by the restatement)."""
    inst = honest_instance(*case, n_lookup=n_lookup)
    co = to_coeffs(inst)
    h_ext = quotient_ext(to_extended(co))
    return inst, co, h_ext, ntt_inverse(h_ext, inst["extended_k"], inv(inst["shift"]))


def _want_result(inst: dict) -> dict:
    ncols, nsets = len(inst["perm_columns"]), -(-len(inst["perm_columns"]) // inst["chunk_len"])
    return {"gate_expressions": len(inst["advice"]), "permutation_expressions": 1 + 2 * nsets if ncols else 0,
            "lookup_expressions": 5 * len(inst["lookup_input"]), "rows": 1 << inst["extended_k"],
            "extension": 1 << (inst["extended_k"] - inst["k"]), "degree": degree(inst)}


def _compare(ctx, co: dict, want_ext, split: bool = False):
    N = 1 << co["extended_k"]
    for form in FORMS:
        ext = _extend(ctx, co, _families(co, form), form)
        if split:
            ext = {f: _split(t) for f, t in ext.items()}
        h, res = ctx.quotient(form=form, out=_prefilled(1, N), **_params(co), **ext)
        assert res == _want_result(co), (form, res)
        assert np.array_equal(_canonical(h, form)[0], _cells(want_ext)), form


# ------------------------------------------- 1. full compare with the restatement
@pytest.mark.parametrize("case", SMALL_CASES + BLOCK_CASES)
def test_full_compare(ctx, case):
    _, co, h_ext, _ = _case(case)
    _compare(ctx, co, h_ext)


@pytest.mark.parametrize("case", [SMALL_CASES[1], BLOCK_CASES[0]])
def test_families_alone_and_left_out(ctx, case):
    _, co, _, _ = _case(case)
    for drop in (("permutation", "lookups"), ("gates", "lookups"), ("gates", "permutation"), ("gates",),
                 ("permutation",), ("lookups",)):
        part = without(co, *drop)
        _compare(ctx, part, quotient_ext(to_extended(part)))


@pytest.mark.parametrize("case", [SMALL_CASES[2], BLOCK_CASES[1]])
def test_two_lookups_and_split_lists(ctx, case):
    _, co, h_ext, _ = _case(case, n_lookup=2)
    assert len(co["lookup_z"]) == 2 and len(co["perm_columns"]) == 5
    _compare(ctx, co, h_ext, split=True)


# ------------------------------------------------------------------ 2. round trip
@pytest.mark.parametrize("case", [SMALL_CASES[0], SMALL_CASES[3], BLOCK_CASES[1]])
def test_round_trip_through_the_checker(ctx, case):
    inst, co, _, h = _case(case)
    n, N = 1 << inst["k"], 1 << inst["extended_k"]
    for form in FORMS:
        fams = _families(co, form)
        h_ext, _ = ctx.quotient(form=form, **_params(inst), **_extend(ctx, inst, fams, form))
        hc, _ = ctx.extended_to_coeff(h_ext, inst["extended_k"], inv(inst["shift"]), form=form)
        got = ctx.check_quotient(hc, X, form=form, **_params(inst), **fams)
        lhs = horner(h, X) * (pow(X, n, P_MOD) - 1) % P_MOD
        assert got == {"lhs": lhs, "rhs": lhs, "identity_failures": 0, "tail_checked": N - tail_start(inst),
                       "tail_nonzero": 0}, form
        assert N - tail_start(inst) == N - 1 - (degree(inst) * (n - 1) - n)


# --------------------------------------------------- 3. the checker earns its trust
def _tampered(inst, family, col, row):
    out = dict(inst)
    out[family] = [list(c) for c in inst[family]]
    out[family][col][row] = (out[family][col][row] + 1) % P_MOD
    return out


@pytest.mark.parametrize("case", [SMALL_CASES[1], SMALL_CASES[2]])
def test_checker_against_the_restatement_and_tampering(ctx, case):
    """The restatement's h, uploaded from the host, is accepted with the
    restatement's values on both sides. A tampered column (with the h the
    restatement then computes), a changed coefficient of h and a wrong shift
    leave a remainder: the identity fails and the tail is not zero. A wrong y
    still divides exactly for an honest witness (every expression vanishes on
    its own), so there only the identity fails."""
    import torch
    inst, co, _, h = _case(case)
    n, N = 1 << inst["k"], 1 << inst["extended_k"]
    usable = n - inst["unusable"]
    tail = N - tail_start(inst)
    for form in FORMS:
        fams = _families(co, form)
        hd = _device([h], form)
        before = {f: t.clone() for f, t in fams.items()}, hd.clone()
        got = ctx.check_quotient(hd, X, form=form, **_params(inst), **fams)
        rhs = combined_at(co, X)
        assert got == {"lhs": horner(h, X) * (pow(X, n, P_MOD) - 1) % P_MOD, "rhs": rhs, "identity_failures": 0,
                       "tail_checked": tail, "tail_nonzero": 0}, form
        # a second point, on the domain itself: x = omega^usable
        x_dom = pow(pow(7, (P_MOD - 1) >> inst["k"], P_MOD), usable, P_MOD)
        got = ctx.check_quotient(hd, x_dom, form=form, **_params(inst), **fams)
        assert got["identity_failures"] == 0 and got["lhs"] == 0 and got["rhs"] == combined_at(co, x_dom) == 0
        for family, col, row in (("advice", 1, 3), ("perm_z", 0, usable // 2), ("permuted_table", 0, 2)):
            bad = to_coeffs(_tampered(inst, family, col, row))
            h_bad = ntt_inverse(quotient_ext(to_extended(bad)), inst["extended_k"], inv(inst["shift"]))
            got = ctx.check_quotient(_device([h_bad], form), X, form=form, **_params(inst), **_families(bad, form))
            assert got["identity_failures"] == 1 and got["tail_nonzero"] > 0 and got["tail_checked"] == tail, \
                (form, family, got)
            assert got["rhs"] == combined_at(bad, X) and got["lhs"] != got["rhs"]
            # the honest h against the tampered columns: its tail is clean, the identity is not
            got = ctx.check_quotient(hd, X, form=form, **_params(inst), **_families(bad, form))
            assert got["identity_failures"] == 1 and got["tail_nonzero"] == 0, (form, family, got)
        h_off = list(h)
        h_off[N - 1] = 1
        got = ctx.check_quotient(_device([h_off], form), X, form=form, **_params(inst), **fams)
        assert got["identity_failures"] == 1 and got["tail_nonzero"] == 1, (form, got)
        h_off = list(h)
        h_off[1] = (h_off[1] + 1) % P_MOD
        got = ctx.check_quotient(_device([h_off], form), X, form=form, **_params(inst), **fams)
        assert got["identity_failures"] == 1 and got["tail_nonzero"] == 0, (form, got)
        # a wrong y: the device's own h for y + 1, checked with y
        ext = _extend(ctx, inst, fams, form)
        h_y, _ = ctx.quotient(form=form, **_params(inst, y=inst["y"] + 1), **ext)
        hc, _ = ctx.extended_to_coeff(h_y, inst["extended_k"], inv(inst["shift"]), form=form)
        got = ctx.check_quotient(hc, X, form=form, **_params(inst), **fams)
        assert got["identity_failures"] == 1 and got["tail_nonzero"] == 0, (form, got)
        assert ctx.check_quotient(hc, X, form=form, **_params(inst, y=inst["y"] + 1), **fams)["identity_failures"] == 0
        # a wrong shift: columns on the coset of the shift, the quotient told ZETA
        h_s, _ = ctx.quotient(form=form, **_params(inst, shift=ZETA), **ext)
        hc, _ = ctx.extended_to_coeff(h_s, inst["extended_k"], inv(inst["shift"]), form=form)
        got = ctx.check_quotient(hc, X, form=form, **_params(inst), **fams)
        assert got["identity_failures"] == 1 and got["tail_nonzero"] > 0, (form, got)
        wrong = to_extended(co)
        wrong["shift"] = ZETA
        assert np.array_equal(_canonical(h_s, form)[0], _cells(quotient_ext(wrong))), form
        ctx.sync()
        assert all(torch.equal(fams[f], before[0][f]) for f in fams) and torch.equal(hd, before[1]), form


# -------------------------------------------------- 4. end to end on a witness
def test_witness_end_to_end(ctx):
    """The 4 x 4 SVD witness of test_witness_columns_to_coefficients: its advice
    columns and selectors as gates, its lookup columns with A', S' and Z, the
    permutation over all of them with the identity sigma and its Z; through the
    transforms, the quotient and back, the identity holds at two points and h
    ends at its degree. One gated cell changed before the transforms breaks it."""
    import torch
    import halo2_svd041_amd as hs
    K, EK, MIN_ROWS, UNUSABLE, CHUNK = 10, 12, 20, 6, 2
    rows = 1 << K
    beta, gamma, y = gamma_for(1), gamma_for(2), gamma_for(3)
    zeta_inv = ZETA * ZETA % P_MOD
    m, u, d, v = gen_svd_input(4, 4, seed=44)
    hs.svd_witness(ctx, m, u, v, d, gamma_for(K))
    ctx.physical_layout(K, MIN_ROWS)
    for form in FORMS:
        assigned = [ctx.assign_columns(ph, form=form) for ph in (0, 1)]
        adv = torch.cat([a[0] for a in assigned])
        sel8 = torch.cat([a[1] for a in assigned])
        lk = assigned[0][2]
        assert adv.shape[0] >= 1 and lk.shape[0] >= 1 and assigned[1][2].shape[0] == 0
        sel = np.zeros((sel8.shape[0], rows, 32), dtype=np.uint8)      # the selector bytes widened to cells
        sel[:, :, 0] = sel8.cpu().numpy()
        sel = torch.from_numpy(_in_form(sel, form)).cuda()
        table = _device([table_column(8, rows)] * lk.shape[0], form)
        ap, sp, res = ctx.lookup_permute(0, UNUSABLE, form)
        assert res["out_of_table"] == 0
        lz, res = ctx.lookup_product(0, ap, sp, beta, gamma, UNUSABLE, form)
        assert res["final_not_one"] == 0
        gate_row = int(torch.nonzero(sel8[0])[0])

        def run(adv):
            pcols = torch.cat([adv, lk])
            sigma, bad = ctx.permutation_values(K, ncols=pcols.shape[0], form=form)
            pz, res = ctx.permutation_product(pcols, sigma, beta, gamma, CHUNK, K, UNUSABLE, form)
            assert bad == 0 and res["final_not_one"] == 0
            lag = dict(advice=adv, selectors=sel, perm_columns=pcols, sigma=sigma, perm_z=pz, lookup_input=lk,
                       lookup_table=table, permuted_input=ap, permuted_table=sp, lookup_z=lz)
            co = {f: ctx.lagrange_to_coeff(t, K, form)[0] for f, t in lag.items()}
            ext = {f: ctx.coeff_to_extended(t, K, EK, ZETA, form=form)[0] for f, t in co.items()}
            par = dict(k=K, extended_k=EK, shift=ZETA, beta=beta, gamma=gamma, y=y, chunk_len=CHUNK,
                       unusable_rows=UNUSABLE, form=form)
            h_ext, res = ctx.quotient(out=_prefilled(1, 1 << EK), **par, **ext)
            assert res["degree"] == 4 and res["extension"] == 4 and res["gate_expressions"] == adv.shape[0]
            hc, _ = ctx.extended_to_coeff(h_ext, EK, zeta_inv, form=form)
            return [ctx.check_quotient(hc, x, **par, **co) for x in (X, gamma_for(4))]

        for got in run(adv):
            assert got["identity_failures"] == 0 and got["tail_nonzero"] == 0 and got["lhs"] != 0, (form, got)
            assert got["tail_checked"] == (1 << EK) - 1 - (4 * (rows - 1) - rows)
        bad = adv.clone()
        bad[0, gate_row + 3, 0] ^= 1                       # the output cell of an enabled gate
        for got in run(bad):
            assert got["identity_failures"] == 1 and got["tail_nonzero"] > 0, (form, got)


# ------------------------------------------------ 5. a mid size, the checker alone
def test_mid_size_through_the_checker(ctx):
    k, ek = 14, 16
    inst = honest_instance(k, ek, 6, 2, seed=5, n_gate=2)
    for form in FORMS:
        lag = _families(inst, form)
        co = {f: ctx.lagrange_to_coeff(t, k, form)[0] for f, t in lag.items()}
        ext = _extend(ctx, inst, co, form)
        h_ext, res = ctx.quotient(form=form, out=_prefilled(1, 1 << ek), **_params(inst), **ext)
        assert res == _want_result(inst)
        hc, _ = ctx.extended_to_coeff(h_ext, ek, inv(inst["shift"]), form=form)
        got = ctx.check_quotient(hc, X, form=form, **_params(inst), **co)
        assert got["identity_failures"] == 0 and got["tail_nonzero"] == 0 and got["lhs"] == got["rhs"] != 0, (form, got)
        assert got["tail_checked"] == (1 << ek) - tail_start(inst)


# ------------------------------------------------------- 6. no-ops and refusals
def test_no_families_and_refusals(ctx):
    import torch
    import halo2_svd041_amd as hs
    from halo2_svd041_amd._lib import QuotientArgs, QuotientCheck, QuotientResult
    L = hs.zk.lib()
    inst, co, _, _ = _case(SMALL_CASES[1])
    N = 1 << inst["extended_k"]
    out = _prefilled(1, N)
    # no families: SVDW_OK, nothing is touched
    h, res = ctx.quotient(out=out, **_params(inst))
    assert res == {"gate_expressions": 0, "permutation_expressions": 0, "lookup_expressions": 0, "rows": N,
                   "extension": 4, "degree": 0}
    got = ctx.check_quotient(out, X, **_params(inst))
    assert got == {"lhs": 0, "rhs": 0, "identity_failures": 0, "tail_checked": 0, "tail_nonzero": 0}
    a, r, c = QuotientArgs(), QuotientResult(), QuotientCheck()
    a.k, a.extended_k, a.unusable_rows, a.chunk_len = 5, 7, 6, 2
    w = lambda x: (ct.c_uint64 * 4)(*[(x >> (64 * i)) & (2 ** 64 - 1) for i in range(4)])
    a.shift, a.beta, a.gamma, a.y = w(ZETA), w(BETA), w(GAMMA), w(Y)
    assert L.svdw_quotient(ctx._h, ct.byref(a), None, ct.byref(r)) == 0
    assert L.svdw_check_quotient(ctx._h, ct.byref(a), None, w(X), ct.byref(c)) == 0
    ctx.sync()
    assert bool((out == SENTINEL).all())
    # h_ext over an input column, whole or in part
    ext = _extend(ctx, inst, _families(co, "canonical"), "canonical")
    before = {f: t.clone() for f, t in ext.items()}
    z = ext["lookup_z"]
    flat = torch.cat([ext["advice"], _prefilled(1, N)])
    shifted = flat.view(-1)[16 * 32:(16 + N) * 32].view(1, N, 32)          # 16 rows into advice column 0
    for fams, dst in ((ext, z), (dict(ext, advice=flat[:3]), shifted), (dict(ext, advice=flat[:3]), flat[2:3])):
        with pytest.raises(hs.SvdwError) as e:
            ctx.quotient(out=dst, **_params(inst), **fams)
        assert e.value.code == -1 and "overlaps" in str(e.value)
    ctx.sync()
    assert all(torch.equal(ext[f], before[f]) for f in ext)
    # every refusal comes through the wrapper with its code
    gates = dict(advice=ext["advice"], selectors=ext["selectors"])
    perm = dict(perm_columns=ext["perm_columns"], sigma=ext["sigma"], perm_z=ext["perm_z"])
    refusals = [
        (dict(form="bogus"), gates, -1, "form"),
        (dict(shift=0), gates, -1, "shift"),
        (dict(y=P_MOD), gates, -1, "challenge"),
        (dict(unusable_rows=0), gates, -2, "unusable_rows"),
        (dict(unusable_rows=32), gates, -2, "unusable_rows"),
        (dict(chunk_len=0), perm, -1, "chunk_len"),
        (dict(k=9), gates, -2, "extended_k"),
        (dict(chunk_len=4), dict(perm, perm_z=ext["perm_z"][:1]), -2, "degree"),
        (dict(shift=1), gates, -1, "root of unity"),
        (dict(), dict(advice=[ext["advice"][:1]] * 65536, selectors=[ext["selectors"][:1]] * 65536), -2, "65535"),
    ]
    for over, fams, code, word in refusals:
        with pytest.raises(hs.SvdwError) as e:
            ctx.quotient(out=_prefilled(1, N), **_params(inst, **over), **fams)
        assert e.value.code == code and word in str(e.value), (over, str(e.value))
    with pytest.raises(hs.SvdwError) as e:
        ctx.check_quotient(out, X, **_params(inst, shift=1), **{f: t for f, t in _families(co, "canonical").items()
                                                                  if f in ("advice", "selectors")})
    assert e.value.code == -1 and "root of unity" in str(e.value)
    ctx.sync()
    assert bool((out == SENTINEL).all())
