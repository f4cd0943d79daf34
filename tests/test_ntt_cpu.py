"""The domain transforms without a GPU: the recursive restatement equals the
O(n^2) one, inverse after forward is the identity, the extended evaluations
contain the Lagrange values, ZETA's powers cycle; the new C entries exist, keep
the ABI version and check their arguments in the documented order on a planning
context; the wrappers refuse a shift outside the field."""
import ctypes as ct

import numpy as np
import pytest

import halo2_svd041_amd as hs
from halo2_svd041_amd import _lib
from ntt_cases import (P_MOD, WIDE_SHIFT, ZETA, dft_forward, dft_inverse, horner, inv, ntt_forward, ntt_inverse,
                       omega, sample_rows, spikes_forward, spikes_inverse)

ENTRIES = ("svdw_ntt", "svdw_ntt_passes", "svdw_eval_polynomial", "svdw_check_ntt")
STRUCTS = ("NttResult", "NttCheck")


def _column(k: int, seed: int) -> list:
    rs = np.random.RandomState(seed)
    return [int.from_bytes(rs.bytes(32), "little") % P_MOD for _ in range(1 << k)]


@pytest.mark.parametrize("k", range(1, 9))
def test_recursive_restatement_equals_the_sums(k):
    a = _column(k, k)
    k_in = max(1, k - 2)
    for shift in (1, ZETA, WIDE_SHIFT):
        assert ntt_forward(a, k, k, shift) == dft_forward(a, k, k, shift)
        assert ntt_forward(a, k_in, k, shift) == dft_forward(a, k_in, k, shift)
        assert ntt_inverse(a, k, shift) == dft_inverse(a, k, shift)


@pytest.mark.parametrize("k", (1, 4, 9, 12))
def test_inverse_after_forward_is_the_identity(k):
    a = _column(k, 100 + k)
    for shift in (1, ZETA, WIDE_SHIFT):
        assert ntt_inverse(ntt_forward(a, k, k, shift), k, inv(shift)) == a
        assert ntt_forward(ntt_inverse(a, k, shift), k, k, inv(shift)) == a


@pytest.mark.parametrize("k_in,k", [(3, 4), (3, 6), (7, 9)])
def test_extended_evaluations_contain_the_lagrange_values(k_in, k):
    lagrange = _column(k_in, 7 * k)
    coeffs = ntt_inverse(lagrange, k_in)
    ext = ntt_forward(coeffs, k_in, k)
    assert ext[::1 << (k - k_in)] == lagrange
    # a row of the extended domain is the polynomial at that power of omega
    for j in (0, 1, (1 << k) - 1):
        assert ext[j] == horner(coeffs, pow(omega(k), j, P_MOD))
    # and the inverse over the extended domain gives the coefficients back, then zeros
    assert ntt_inverse(ext, k) == coeffs + [0] * ((1 << k) - (1 << k_in))


def test_zeta_powers_cycle():
    assert ZETA != 1 and pow(ZETA, 3, P_MOD) == 1 and ZETA * ZETA % P_MOD == inv(ZETA)
    pattern = [1, ZETA, ZETA * ZETA % P_MOD]
    assert [pow(ZETA, i, P_MOD) for i in range(12)] == [pattern[i % 3] for i in range(12)]
    assert 0 < WIDE_SHIFT < P_MOD and WIDE_SHIFT.bit_length() >= 250


def test_spikes_are_geometric_sequences():
    k = 6
    spikes = [((1 << k) - 1, 5), ((1 << (k // 2)) + 1, P_MOD - 3)]
    a = [0] * (1 << k)
    for r, v in spikes:
        a[r] = v
    assert spikes_forward(spikes, k) == dft_forward(a, k, k)
    assert spikes_inverse(spikes, k) == dft_inverse(a, k)


def test_sampling_rule():
    assert sample_rows(9, 9, 12345) == list(range(512))
    for k, ls, seed in ((9, 3, 0), (21, 10, 7), (12, 0, 2 ** 64 - 1)):
        rows = sample_rows(k, ls, seed)
        q = (1 << k) >> ls
        assert len(rows) == 1 << ls and all(s * q <= j < (s + 1) * q for s, j in enumerate(rows))
    assert len({j % 2048 for j in sample_rows(21, 10, 7)}) > 500     # the offsets vary over the strata


def test_symbols_and_abi_version():
    L = _lib.lib()
    for name in ENTRIES:
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES, name
    for name in STRUCTS:
        assert hasattr(_lib, name), name
    assert len(ENTRIES) + len(STRUCTS) == 6
    assert L.svdw_abi_version() == 2


def test_passes_are_monotone():
    L = _lib.lib()
    p = [L.svdw_ntt_passes(k) for k in range(1, 29)]
    assert p[0] == 1 and all(a <= b for a, b in zip(p, p[1:]))
    assert max(p) == 3 and min(k for k in range(1, 29) if p[k - 1] == 3) <= 23


def _words(x):
    return (ct.c_uint64 * 4)(*[(x >> (64 * i)) & (2 ** 64 - 1) for i in range(4)])


def _call_both(ctx, k_in=9, k=9, form=0, inverse=0, shift=None, ncols=3, log_samples=3):
    """Return codes of the transform and its check on ctx with null column and
    out pointers: every check of the arguments comes before them."""
    L = _lib.lib()
    r, c = _lib.NttResult(), _lib.NttCheck()
    sh = None if shift is None else _words(shift)
    return [L.svdw_ntt(ctx._h, k_in, k, form, inverse, sh, None, ncols, None, ct.byref(r)),
            L.svdw_check_ntt(ctx._h, k_in, k, form, inverse, sh, None, ncols, None, log_samples, 0, ct.byref(c))]


def _eval(ctx, k=9, form=0, ncols=2, points=(5,), npoints=None):
    buf = (ct.c_uint64 * (4 * max(len(points), 1)))(*[w for x in points for w in _words(x)])
    return _lib.lib().svdw_eval_polynomial(ctx._h, k, form, None, ncols, buf,
                                           len(points) if npoints is None else npoints, None)


def test_argument_checks_come_in_the_documented_order():
    """Each call breaks one rule and every rule after it; the code and the
    message are those of the first rule broken."""
    err = lambda: _lib.lib().svdw_last_error().decode()
    EINVAL, ERANGE = -1, -2
    many = 70000
    with hs.Context(device=-1, precision_bits=32, lookup_bits=8) as ctx:
        # 1. form
        assert _call_both(ctx, k_in=30, k=29, form=7, inverse=2, shift=P_MOD, ncols=many) == [EINVAL] * 2
        assert "form" in err()
        # 2. shift >= p or shift == 0
        for shift in (P_MOD, 0, 2 ** 256 - 1):
            assert _call_both(ctx, k_in=30, k=29, inverse=2, shift=shift, ncols=many) == [EINVAL] * 2
            assert "shift" in err()
        # 3. inverse not 0 or 1
        for inverse in (2, -1):
            assert _call_both(ctx, k_in=30, k=29, inverse=inverse, ncols=many) == [EINVAL] * 2
            assert "inverse" in err()
        # 4. k outside 1..28
        for k in (0, 29):
            assert _call_both(ctx, k_in=30, k=k, ncols=many) == [ERANGE] * 2
            assert "k must be" in err()
        # 5. k_in outside 1..k, or an inverse with k_in != k
        for k_in in (0, 10):
            assert _call_both(ctx, k_in=k_in, k=9, ncols=many) == [ERANGE] * 2
            assert "k_in" in err()
        assert _call_both(ctx, k_in=8, k=9, inverse=1, ncols=many) == [ERANGE] * 2
        assert "k_in == k" in err()
        assert _call_both(ctx, k_in=8, k=9, ncols=many, log_samples=10)[1] == ERANGE
        assert "log_samples" in err()
        # 6. a planning context, with and without columns
        assert _call_both(ctx, ncols=many) == [EINVAL] * 2
        assert "device context" in err()
        assert _call_both(ctx, ncols=0) == [EINVAL] * 2
        assert "device context" in err()
        assert _call_both(ctx, shift=ZETA, inverse=1) == [EINVAL] * 2
        assert "device context" in err()
        # svdw_eval_polynomial: form, a point >= p, k, a planning context
        assert _eval(ctx, k=29, form=7, points=(P_MOD,)) == EINVAL
        assert "form" in err()
        assert _eval(ctx, k=29, points=(5, P_MOD)) == EINVAL
        assert ">= p" in err()
        assert _eval(ctx, k=29) == ERANGE
        assert "k must be" in err()
        assert _eval(ctx, ncols=many) == EINVAL
        assert "device context" in err()
        assert _eval(ctx, ncols=0, npoints=0) == EINVAL
        assert "device context" in err()


def test_python_wrappers_raise_on_a_shift_outside_the_field():
    with hs.Context(device=-1, precision_bits=32, lookup_bits=8) as ctx:
        calls = (lambda s: ctx.ntt([], 9, shift=s),
                 lambda s: ctx.ntt([], 9, inverse=True, shift=s),
                 lambda s: ctx.coeff_to_extended([], 9, 11, s),
                 lambda s: ctx.extended_to_coeff([], 11, s),
                 lambda s: ctx.check_ntt([], None, 9, shift=s))
        for call in calls:
            for shift in (P_MOD, 0, -1, 2 ** 256):
                with pytest.raises(hs.SvdwError) as e:
                    call(shift)
                assert e.value.code == -1
        with pytest.raises(hs.SvdwError) as e:
            ctx.eval_polynomial([], 9, [5, P_MOD])
        assert e.value.code == -1
