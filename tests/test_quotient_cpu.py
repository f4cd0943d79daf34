"""The quotient polynomial without a GPU: on the literal restatement the
verifier's identity holds at a random point and the top coefficient sits exactly
at the degree bound, and one tampered cell breaks both; the new C entries and
structs exist and keep the ABI version; the arguments are checked in the
documented order on a planning context; the wrappers refuse a challenge outside
the field."""
import ctypes as ct

import pytest

import halo2_svd041_amd as hs
from halo2_svd041_amd import _lib
from quotient_cases import (BETA, GAMMA, P_MOD, SMALL_CASES, WIDE_SHIFT, Y, ZETA, honest_instance, identity_holds,
                            inv, ntt_inverse, quotient_ext, tail_start, to_coeffs, to_extended, top_nonzero, without)

ENTRIES = ("svdw_quotient", "svdw_check_quotient")
STRUCTS = ("QuotientArgs", "QuotientResult", "QuotientCheck")
X = 0x1d2c3b4a59687766554433221100ffeeddccbbaa99887766554433221100abcd % P_MOD


def _h_coeffs(inst):
    """(coefficient columns, the coefficients of h) of an instance in Lagrange form."""
    co = to_coeffs(inst)
    h_ext = quotient_ext(to_extended(co))
    return co, ntt_inverse(h_ext, inst["extended_k"], inv(inst["shift"]))


def _tampered(inst, family, col, row):
    out = dict(inst)
    out[family] = [list(c) for c in inst[family]]
    out[family][col][row] = (out[family][col][row] + 1) % P_MOD
    return out


@pytest.mark.parametrize("case", SMALL_CASES)
def test_identity_and_degree_on_the_restatement(case):
    inst = honest_instance(*case)
    assert inst["shift"] == WIDE_SHIFT and WIDE_SHIFT.bit_length() >= 250
    n, N = 1 << inst["k"], 1 << inst["extended_k"]
    co, h = _h_coeffs(inst)
    assert identity_holds(co, h, X)
    want = {2: 3 * n - 4, 3: 4 * n - 5}[inst["chunk_len"]]
    assert tail_start(inst) - 1 == want
    assert top_nonzero(h) == want
    # each family alone and each family left out still divide exactly
    for drop in (("permutation", "lookups"), ("gates", "lookups"), ("gates", "permutation"), ("gates",),
                 ("permutation",), ("lookups",)):
        part = without(inst, *drop)
        co_p, h_p = _h_coeffs(part)
        assert identity_holds(co_p, h_p, X), drop
        assert top_nonzero(h_p) == tail_start(part) - 1, drop
    # one cell off: the division leaves a remainder, which shows at the top and at x
    usable = n - inst["unusable"]
    for family, col, row in (("advice", 1, 3), ("perm_z", 0, usable // 2), ("lookup_z", 0, usable // 2),
                             ("permuted_table", 0, 2), ("sigma", 1, 5)):
        co_t, h_t = _h_coeffs(_tampered(inst, family, col, row))
        assert h_t[N - 1] != 0, (family, col, row)
        assert not identity_holds(co_t, h_t, X), (family, col, row)


def test_symbols_and_abi_version():
    L = _lib.lib()
    for name in ENTRIES:
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES, name
    for name in STRUCTS:
        assert hasattr(_lib, name), name
    assert ct.sizeof(_lib.QuotientArgs) == 16 + 4 * 32 + 2 * 8 + 16 + 8 * 8
    assert ct.sizeof(_lib.QuotientResult) == 40 and ct.sizeof(_lib.QuotientCheck) == 88
    assert L.svdw_abi_version() == 2


def _words(x):
    return (ct.c_uint64 * 4)(*[(x >> (64 * i)) & (2 ** 64 - 1) for i in range(4)])


def _call_both(ctx, k=5, extended_k=7, unusable=6, form=0, shift=ZETA, beta=BETA, gamma=GAMMA, y=Y, x=X, n_gate=2,
               n_perm=3, chunk_len=2, n_lookup=1):
    """Return codes of the quotient and its check on ctx with null column and
    output pointers: every check of the arguments comes before them."""
    L = _lib.lib()
    a = _lib.QuotientArgs()
    a.k, a.extended_k, a.unusable_rows, a.form = k, extended_k, unusable, form
    a.shift, a.beta, a.gamma, a.y = _words(shift), _words(beta), _words(gamma), _words(y)
    a.n_gate, a.n_perm, a.chunk_len, a.n_lookup = n_gate, n_perm, chunk_len, n_lookup
    r, c = _lib.QuotientResult(), _lib.QuotientCheck()
    return [L.svdw_quotient(ctx._h, ct.byref(a), None, ct.byref(r)),
            L.svdw_check_quotient(ctx._h, ct.byref(a), None, _words(x), ct.byref(c))]


def test_argument_checks_come_in_the_documented_order():
    """Each call breaks one rule and every rule after it; the code and the
    message are those of the first rule broken."""
    err = lambda: _lib.lib().svdw_last_error().decode()
    EINVAL, ERANGE = -1, -2
    many = 70000
    with hs.Context(device=-1, precision_bits=32, lookup_bits=8) as ctx:
        # 1. form
        assert _call_both(ctx, form=7, y=P_MOD, unusable=0, chunk_len=0, k=29, n_gate=many) == [EINVAL] * 2
        assert "form" in err()
        # 2. a challenge or the shift >= p, shift == 0
        for kw in ({"shift": P_MOD}, {"shift": 0}, {"beta": P_MOD}, {"gamma": 2 ** 256 - 1}, {"y": P_MOD}):
            assert _call_both(ctx, unusable=0, chunk_len=0, k=29, n_gate=many, **kw) == [EINVAL] * 2
            assert ("shift" if "shift" in kw else ">= p") in err()
        assert _call_both(ctx, x=P_MOD, unusable=0, k=29)[1] == EINVAL
        assert ">= p" in err()
        # 3. unusable_rows == 0 or >= 2^k
        for unusable in (0, 32, 33):
            assert _call_both(ctx, unusable=unusable, chunk_len=0, extended_k=30, n_gate=many) == [ERANGE] * 2
            assert "unusable_rows" in err()
        # 4. chunk_len == 0 with permutation columns
        assert _call_both(ctx, chunk_len=0, extended_k=30, n_gate=many) == [EINVAL] * 2
        assert "chunk_len" in err()
        # 5. k outside 1..28, extended_k outside k..28
        for k, ek in ((29, 29), (5, 4), (5, 29)):
            assert _call_both(ctx, k=k, extended_k=ek, unusable=1, chunk_len=4, n_perm=4, n_gate=many) == [ERANGE] * 2
            assert "k must be in" in err()
        # 6. the degree does not fit: sets of 4 columns need D = 6 > E + 1 = 5
        assert _call_both(ctx, chunk_len=4, n_perm=4, shift=1, n_gate=many) == [ERANGE] * 2
        assert "degree" in err()
        assert _call_both(ctx, k=5, extended_k=6, n_perm=0, n_lookup=1, shift=1) == [ERANGE] * 2   # D = 4 > E + 1 = 3
        assert "degree" in err()
        # 7. a zero divisor: shift = 1, or any 2^extended_k-th root of unity
        for shift in (1, P_MOD - 1, pow(7, (P_MOD - 1) >> 7, P_MOD)):
            assert _call_both(ctx, shift=shift, n_gate=many) == [EINVAL] * 2
            assert "root of unity" in err()
        # 8. a planning context, with and without columns
        assert _call_both(ctx, n_gate=many) == [EINVAL] * 2
        assert "device context" in err()
        assert _call_both(ctx, n_gate=0, n_perm=0, n_lookup=0) == [EINVAL] * 2
        assert "device context" in err()
        assert _call_both(ctx, shift=WIDE_SHIFT) == [EINVAL] * 2
        assert "device context" in err()


def test_python_wrappers_raise_on_a_challenge_outside_the_field():
    with hs.Context(device=-1, precision_bits=32, lookup_bits=8) as ctx:
        good = dict(shift=ZETA, beta=BETA, gamma=GAMMA, y=Y)
        for name in good:
            for bad in (P_MOD, -1, 2 ** 256) + ((0,) if name == "shift" else ()):
                kw = dict(good, **{name: bad})
                with pytest.raises(hs.SvdwError) as e:
                    ctx.quotient(5, 7, **kw)
                assert e.value.code == -1
                with pytest.raises(hs.SvdwError) as e:
                    ctx.check_quotient(None, X, 5, 7, **kw)
                assert e.value.code == -1
        with pytest.raises(hs.SvdwError) as e:
            ctx.check_quotient(None, P_MOD, 5, 7, **good)
        assert e.value.code == -1
