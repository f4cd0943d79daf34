"""Permutation grand products without a GPU: the literal restatement
(permutation_cases.py) closes on the last set only, for an honest sigma made by
value_cycles and by the restated keygen merge, does not close after one sigma
entry or one cell changes, and shows inv0 zeroing the rest of a set and every
later set; svdw_permutation_constants equals the pow values; the four C entries
exist, keep the ABI version, and check their arguments in the documented order
on a planning context."""
import ctypes as ct

import numpy as np
import pytest

import halo2_svd041_amd as hs
from halo2_svd041_amd import _lib
from halo2_svd041_amd._lib import PermutationProductCheck, PermutationProductResult
from permutation_cases import (CHALLENGES, DELTA, P_MOD, Assembly, first_placement, grand_products, identity,
                               identity_mapping, omega, recurrence_holds, sigma_values, value_cycles)

ENTRIES = ("svdw_permutation_constants", "svdw_permutation_values", "svdw_permutation_product",
           "svdw_check_permutation_product")
K, UNUSABLE, NCOLS = 8, 6, 5
CHUNKS = (1, 2, 3, 5, 7)


def _columns(k=K, unusable=UNUSABLE, ncols=NCOLS, seed=3):
    """Columns of few distinct small values (so that cycles cross columns) and
    one of full-width values; rows >= usable zero."""
    rows = 1 << k
    rs = np.random.RandomState(seed)
    cols = [[int(x) for x in rs.randint(0, 8, size=rows - unusable)] + [0] * unusable for _ in range(ncols - 1)]
    wide = [int.from_bytes(rs.bytes(32), "little") % P_MOD for _ in range(rows - unusable)] + [0] * unusable
    return cols[:1] + [wide] + cols[1:]                      # not last: a set of its own would start and end alike


@pytest.fixture(scope="module")
def honest():
    cols = _columns()
    mapping = value_cycles(cols, (1 << K) - UNUSABLE, seed=5)
    assert mapping != identity_mapping(NCOLS, 1 << K)
    return cols, mapping, sigma_values(mapping, K)


def test_constants_are_roots_of_unity():
    for k in (1, 9, 24, 28):
        w = omega(k)
        assert pow(w, 1 << k, P_MOD) == 1 and pow(w, 1 << (k - 1), P_MOD) == P_MOD - 1
    assert identity(0, 0, K) == 1 and identity(2, 3, K) == DELTA * DELTA * omega(K) ** 3 % P_MOD
    # delta generates a subgroup that meets the 2^28 roots of unity in 1 only
    assert pow(DELTA, (P_MOD - 1) >> 28, P_MOD) == 1


@pytest.mark.parametrize("chunk_len", CHUNKS)
@pytest.mark.parametrize("beta,gamma", CHALLENGES, ids=["plain", "top_bits"])
def test_restatement_closes_on_the_last_set_only(honest, chunk_len, beta, gamma):
    cols, mapping, sigma = honest
    rows, usable = 1 << K, (1 << K) - UNUSABLE
    Z, zeros = grand_products(cols, sigma, beta, gamma, chunk_len, K, UNUSABLE)
    assert len(Z) == -(-NCOLS // chunk_len) and zeros == 0
    assert Z[0][0] == 1 and Z[-1][usable] == 1
    for s in range(1, len(Z)):
        assert Z[s][0] == Z[s - 1][usable] != 1, s
    assert all(not any(z[usable + 1:]) for z in Z)
    assert recurrence_holds(cols, sigma, Z, beta, gamma, chunk_len, K, UNUSABLE) == [[]] * len(Z)


def test_restatement_does_not_close_on_a_changed_sigma_or_cell(honest):
    cols, mapping, sigma = honest
    usable = (1 << K) - UNUSABLE
    beta, gamma = CHALLENGES[0]
    for chunk_len in (2, 5):
        s2 = [list(c) for c in sigma]
        s2[1][usable // 2] = identity(3, 7, K) if s2[1][usable // 2] != identity(3, 7, K) else identity(3, 8, K)
        Z, zeros = grand_products(cols, s2, beta, gamma, chunk_len, K, UNUSABLE)
        assert Z[-1][usable] not in (0, 1) and zeros == 0
        # the recurrence still holds row by row: only the last row tells
        assert not any(recurrence_holds(cols, s2, Z, beta, gamma, chunk_len, K, UNUSABLE))
        c2 = [list(c) for c in cols]
        c2[2][11] += 1
        Z, zeros = grand_products(c2, sigma, beta, gamma, chunk_len, K, UNUSABLE)
        assert Z[-1][usable] not in (0, 1) and zeros == 0


def test_restatement_inv0_zeroes_the_rest_of_the_set_and_all_later_sets(honest):
    cols, mapping, sigma = honest
    usable = (1 << K) - UNUSABLE
    beta = CHALLENGES[0][0]
    r0 = 100
    gamma = (-(cols[0][r0] + beta * sigma[0][r0])) % P_MOD      # column 0's factor of D_0[r0] is zero
    Z, zeros = grand_products(cols, sigma, beta, gamma, 2, K, UNUSABLE)
    assert zeros == 1 and len(Z) == 3
    assert all(Z[0][:r0 + 1]) and not any(Z[0][r0 + 1:])
    assert not any(Z[1]) and not any(Z[2])
    bad = recurrence_holds(cols, sigma, Z, beta, gamma, 2, K, UNUSABLE)
    assert bad == [[r0], [], []]                             # Z[r0 + 1] D = 0 but Z[r0] N != 0


def test_keygen_merge_gives_an_honest_sigma():
    """Assembly.copy on copies between equal cells gives cycles of equal values:
    the product closes. Copying twice and closing a triangle change nothing."""
    cols = _columns(seed=9)
    usable = (1 << K) - UNUSABLE
    asm = Assembly(NCOLS, 1 << K)
    where = {}
    rs = np.random.RandomState(1)
    pairs = 0
    for c in range(NCOLS):
        for r in rs.permutation(usable)[:120]:
            first = where.setdefault(cols[c][r], (c, int(r)))
            if first != (c, int(r)):
                asm.copy(first, (c, int(r)))
                asm.copy((c, int(r)), first)
                pairs += 1
    assert pairs > 300
    for c in range(NCOLS):
        for r in range(1 << K):
            cc, rr = asm.mapping[c][r]
            assert cols[cc][rr] == cols[c][r]
            assert asm.sizes[asm.aux[c][r][0]][asm.aux[c][r][1]] >= 1
    assert max(max(s) for s in asm.sizes) > 10
    sigma = sigma_values(asm.mapping, K)
    Z, zeros = grand_products(cols, sigma, *CHALLENGES[1], 2, K, UNUSABLE)
    assert zeros == 0 and Z[-1][usable] == 1 and Z[0][usable] != 1


def test_first_placement():
    bp = [10, 12, 9]
    assert first_placement(bp, 0) == (0, 0) and first_placement(bp, 10) == (0, 10)
    assert first_placement(bp, 11) == (1, 1) and first_placement(bp, 22) == (1, 12)
    assert first_placement(bp, 23) == (2, 1) and first_placement(bp, 31) == (2, 9)
    assert first_placement(bp, 32) == (3, 1) and first_placement([], 5) == (0, 5)


def test_constants_entry_matches_pow():
    for k in (1, 9, 24, 28):
        assert hs.permutation_constants(k) == (DELTA, omega(k)), k
    d, w = (ct.c_uint64 * 4)(), (ct.c_uint64 * 4)()
    for k in (0, 29):
        assert _lib.lib().svdw_permutation_constants(k, d, w) == -2


def test_symbols_and_abi_version():
    L = _lib.lib()
    for name in ENTRIES:
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES
    assert L.svdw_abi_version() == 2


def _words(x):
    return (ct.c_uint64 * 4)(*[(x >> (64 * i)) & (2 ** 64 - 1) for i in range(4)])


def _call_both(ctx, k=9, ncols=3, unusable=6, form=0, chunk_len=2, beta=CHALLENGES[0][0], gamma=CHALLENGES[0][1]):
    """Return codes of the product and its check on ctx with null column, sigma
    and z pointers: every check of the arguments comes before them."""
    L = _lib.lib()
    r, c = PermutationProductResult(), PermutationProductCheck()
    b, g = _words(beta), _words(gamma)
    return [L.svdw_permutation_product(ctx._h, k, unusable, form, None, None, ncols, chunk_len, b, g, None,
                                       ct.byref(r)),
            L.svdw_check_permutation_product(ctx._h, k, unusable, form, None, None, ncols, chunk_len, b, g, None,
                                             ct.byref(c))]


def test_argument_checks_come_in_the_documented_order():
    """Each call breaks one rule and every rule after it; the code and the
    message are those of the first rule broken."""
    err = lambda: _lib.lib().svdw_last_error().decode()
    EINVAL, ERANGE = -1, -2
    with hs.Context(device=-1, precision_bits=32, lookup_bits=8) as ctx:
        # 1. form, with everything after it wrong too
        assert _call_both(ctx, k=29, unusable=0, form=7, chunk_len=0, beta=P_MOD) == [EINVAL] * 2
        assert "form" in err()
        # 2. beta or gamma >= p
        for beta, gamma in ((P_MOD, 5), (5, P_MOD), (2 ** 256 - 1, 5)):
            assert _call_both(ctx, k=29, unusable=0, chunk_len=0, beta=beta, gamma=gamma) == [EINVAL] * 2
            assert ">= p" in err()
        # 3. unusable_rows == 0 or >= 2^k
        assert _call_both(ctx, k=29, unusable=0, chunk_len=0) == [ERANGE] * 2
        assert "unusable_rows" in err()
        assert _call_both(ctx, k=3, unusable=8, chunk_len=0) == [ERANGE] * 2
        assert "unusable_rows" in err()
        # 4. chunk_len == 0
        assert _call_both(ctx, k=29, chunk_len=0) == [EINVAL] * 2
        assert "chunk_len" in err()
        # 5. k outside 1..28 (k = 0 has no usable row: rule 3 answers first)
        assert _call_both(ctx, k=29) == [ERANGE] * 2
        assert "k must be" in err()
        assert _call_both(ctx, k=0, unusable=1) == [ERANGE] * 2
        # 6. a planning context
        assert _call_both(ctx) == [EINVAL] * 2
        assert "device context" in err()
        assert _call_both(ctx, ncols=0) == [EINVAL] * 2
        assert "device context" in err()
        bad = ct.c_uint64()
        L = _lib.lib()
        assert L.svdw_permutation_values(ctx._h, 9, 7, None, 0, 1, 1, None, ct.byref(bad)) == EINVAL
        assert L.svdw_permutation_values(ctx._h, 29, 0, None, 0, 1, 1, None, ct.byref(bad)) == ERANGE
        assert L.svdw_permutation_values(ctx._h, 9, 0, None, 0, 1, 1, None, ct.byref(bad)) == EINVAL
        assert "device context" in err()


def test_python_wrappers_raise_on_bad_challenges():
    with hs.Context(device=-1, precision_bits=32, lookup_bits=8) as ctx:
        for call in (lambda b, g: ctx.permutation_product([], [], b, g, 2, k=9),
                     lambda b, g: ctx.check_permutation_product([], [], None, b, g, 2, k=9)):
            for beta, gamma in ((P_MOD, 5), (5, -1)):
                with pytest.raises(hs.SvdwError) as e:
                    call(beta, gamma)
                assert e.value.code == -1
