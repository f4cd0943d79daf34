"""The commitments without a GPU: what the reference's SRS file holds (layout,
curve membership, the Lagrange sum, Lagrange / coefficient agreement through
ntt_cases.ntt_inverse), the oracle's group law on its edge cases, the
progression closed form; the new C entries exist, keep the ABI version and check
their arguments in the documented order on a planning context; svdw_commit_plan;
read_srs; the wrappers refuse wrong shapes and dtypes."""
import ctypes as ct
import os

import numpy as np
import pytest

import halo2_svd041_amd as hs
from halo2_svd041_amd import _lib
from halo2_svd041_amd.srs import read_srs
from commit_cases import (G, IDENTITY, JID, Q, R, SRS8, jadd, jdouble, jmul, kernel_constant, msm, mul, neg,
                          on_curve, parse_srs, point_bytes, points_from_bytes, progression, progression_msm,
                          signed_digits, to_affine, to_jac)
from ntt_cases import ntt_inverse

ENTRIES = ("svdw_commit", "svdw_check_commit", "svdw_commit_plan", "svdw_commit_add_probe")
STRUCTS = ("CommitResult", "CommitCheck")


@pytest.fixture(scope="module")
def srs():
    return parse_srs()


def _scalars(n: int, seed: int) -> list:
    rs = np.random.RandomState(seed)
    return [int.from_bytes(rs.bytes(32), "little") % R for _ in range(n)]


# ------------------------------------------------------------ the SRS file
def test_srs_layout_and_first_point(srs):
    k, g, gl = srs
    assert os.path.getsize(SRS8) == 33028 and k == 8 and len(g) == len(gl) == 256
    assert g[0] == G                                       # the file's first 32 bytes are 2^256 mod q
    assert open(SRS8, "rb").read()[4:36] == ((1 << 256) % Q).to_bytes(32, "little")


def test_srs_points_are_on_the_curve(srs):
    _, g, gl = srs
    assert all(on_curve(p) for p in g + gl) and IDENTITY not in g + gl


def test_srs_lagrange_sum_is_g0(srs):
    _, g, gl = srs
    acc = JID
    for p in gl:
        acc = jadd(acc, to_jac(p))
    assert to_affine(acc) == g[0]


def test_srs_lagrange_and_coefficient_commitments_agree(srs):
    k, g, gl = srs
    c = _scalars(1 << k, 8)
    assert msm(gl, c) == msm(g, ntt_inverse(c, k))


# ------------------------------------------------------------ the oracle
def test_group_law_edges():
    p, q = mul(G, 5), mul(G, 7)
    assert on_curve(p) and on_curve(q)
    assert to_affine(jadd(to_jac(p), to_jac(q))) == mul(G, 12)
    assert to_affine(jadd(to_jac(p), to_jac(p))) == to_affine(jdouble(to_jac(p))) == mul(G, 10)   # equal points
    assert jadd(to_jac(p), to_jac(neg(p)))[2] == 0                                              # opposite points
    assert to_affine(jadd(JID, to_jac(p))) == p == to_affine(jadd(to_jac(p), JID))
    assert jdouble(JID)[2] == 0 and to_affine(JID) == IDENTITY and to_jac(IDENTITY) == JID
    assert mul(G, 0) == IDENTITY and mul(G, R) == IDENTITY and mul(G, R - 1) == neg(G) and mul(G, R + 1) == G
    assert to_affine(jadd(jmul(G, 3), jmul(G, R - 3))) == IDENTITY
    assert msm([G, IDENTITY, G], [0, 5, 9]) == mul(G, 9)
    for form in ("canonical", "montgomery"):
        assert points_from_bytes(point_bytes([p, IDENTITY, q], form), form) == [p, IDENTITY, q]


def test_progression_closed_form_equals_the_naive_msm():
    n, a0, d = 32, 123456789, 2 ** 200 + 77
    bases = progression(n, a0, d)
    assert bases[0] == mul(G, a0) and bases[5] == mul(G, a0 + 5 * d) and all(on_curve(p) for p in bases)
    s = _scalars(n, 32)
    s[3], s[4] = 0, R - 1
    assert progression_msm(n, a0, d, s) == msm(bases, s)


def test_signed_digits_restate_the_scalar():
    for c in (2, 7, 13, 16):
        w = -(-255 // c)
        for s in [0, 1, R - 1, 1 << (c - 1), (1 << (c - 1)) + 1] + _scalars(4, c):
            d = signed_digits(s, c, w)
            assert sum(x << (c * i) for i, x in enumerate(d)) == s
            assert all(-(1 << (c - 1)) < x <= 1 << (c - 1) for x in d)


# ------------------------------------------------------------ the C entries
def test_symbols_and_abi_version():
    L = _lib.lib()
    for name in ENTRIES:
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES, name
    for name in STRUCTS:
        assert hasattr(_lib, name), name
    assert [n for n, _ in _lib.CommitResult._fields_] == ["columns", "window_bits", "windows", "rows", "zero_scalars",
                                                         "identity_bases", "identity_outputs"]
    assert [n for n, _ in _lib.CommitCheck._fields_] == ["columns_checked", "commit_failures", "bases_checked",
                                                        "bases_off_curve"]
    assert L.svdw_abi_version() == 2


def test_plan_covers_the_scalar_and_is_monotone():
    plans = [hs.commit_plan(k) for k in range(1, 29)]
    for c, w in plans:
        assert 2 <= c <= kernel_constant("kCommitMaxBits") and w * c >= 255 and (w - 1) * c < 255
    assert all(a[0] <= b[0] for a, b in zip(plans, plans[1:]))
    assert len({c for c, _ in plans}) > 4
    assert hs.commit_plan(0) == plans[0] and hs.commit_plan(40) == plans[-1]
    _lib.lib().svdw_commit_plan(9, None, None)             # either pointer may be null


def _call_both(ctx, k=9, form=0, bases_form=1, ncols=3):
    """Return codes of the commitment and its check with null bases, column and
    out pointers: every check of the arguments comes before them."""
    L = _lib.lib()
    r, c = _lib.CommitResult(), _lib.CommitCheck()
    return [L.svdw_commit(ctx._h, k, form, bases_form, None, None, ncols, None, ct.byref(r)),
            L.svdw_check_commit(ctx._h, k, form, bases_form, None, None, ncols, None, ct.byref(c))]


def test_argument_checks_come_in_the_documented_order():
    """Each call breaks one rule and every rule after it; the code and the
    message are those of the first rule broken."""
    err = lambda: _lib.lib().svdw_last_error().decode()
    EINVAL, ERANGE = -1, -2
    many = 70000
    with hs.Context(device=-1, precision_bits=32, lookup_bits=8) as ctx:
        # 1. form, then bases_form
        assert _call_both(ctx, k=29, form=7, bases_form=7, ncols=many) == [EINVAL] * 2
        assert "form" in err()
        assert _call_both(ctx, k=29, bases_form=2, ncols=many) == [EINVAL] * 2
        assert "form" in err()
        # 2. k outside 1..28
        for k in (0, 29):
            assert _call_both(ctx, k=k, ncols=many) == [ERANGE] * 2
            assert "k must be" in err()
        # 3. a planning context, with and without columns
        assert _call_both(ctx, ncols=many) == [EINVAL] * 2
        assert "device context" in err()
        assert _call_both(ctx, ncols=0) == [EINVAL] * 2
        assert "device context" in err()
        # a null result comes before everything
        L = _lib.lib()
        assert L.svdw_commit(ctx._h, 29, 7, 7, None, None, many, None, None) == EINVAL
        assert L.svdw_check_commit(ctx._h, 29, 7, 7, None, None, many, None, None) == EINVAL
        assert L.svdw_commit_add_probe(ctx._h, None, 0, 0, 0, None) == EINVAL


# ------------------------------------------------------------ read_srs, the wrappers
def test_read_srs_round_trip(tmp_path, srs):
    k, g, gl = srs
    s = read_srs(SRS8)
    assert s["k"] == k and s["g"].shape == s["g_lagrange"].shape == (256, 64) and s["g"].dtype == np.uint8
    assert points_from_bytes(s["g"].tobytes(), "montgomery") == g
    assert points_from_bytes(s["g_lagrange"].tobytes(), "montgomery") == gl
    # a file written from the oracle's points reads back the same
    small = (3).to_bytes(4, "little") + point_bytes(g[:8] + gl[:8], "montgomery") + bytes(256)
    path = tmp_path / "k3.srs"
    path.write_bytes(small)
    t = read_srs(path)
    assert t["k"] == 3 and points_from_bytes(t["g"].tobytes(), "montgomery") == g[:8]
    assert points_from_bytes(t["g_lagrange"].tobytes(), "montgomery") == gl[:8]


def test_read_srs_refuses_a_truncated_file(tmp_path):
    raw = open(SRS8, "rb").read()
    cases = {"cut": raw[:-1], "half": raw[:4 + 64 * 256], "header": raw[:3], "empty": b"",
             "k": (9).to_bytes(4, "little") + raw[4:], "k0": bytes(4) + raw[4:], "long": raw + b"\0"}
    for name, data in cases.items():
        path = tmp_path / (name + ".srs")
        path.write_bytes(data)
        with pytest.raises(hs.SvdwError) as e:
            read_srs(path)
        assert e.value.code == -1, name


def test_python_wrappers_refuse_wrong_shapes_and_dtypes():
    import torch
    k = 4
    cols = torch.zeros((2, 16, 32), dtype=torch.uint8)     # host tensors: not device tensors
    bases = torch.zeros((16, 64), dtype=torch.uint8)
    with hs.Context(device=-1, precision_bits=32, lookup_bits=8) as ctx:
        calls = (lambda: ctx.commit(cols, bases, k),
                 lambda: ctx.commit([], bases, k),
                 lambda: ctx.commit([], np.zeros((16, 64), np.uint8), k),
                 lambda: ctx.commit([], None, k),
                 lambda: ctx.commit_lagrange([cols], bases, k),
                 lambda: ctx.commit_coeffs(np.zeros((2, 16, 32), np.uint8), bases, k),
                 lambda: ctx.check_commit([], bases, None, k),
                 lambda: ctx.check_commit(cols, bases, torch.zeros((2, 64), dtype=torch.uint8), k),
                 lambda: ctx.commit([], bases, k, form="wide"),
                 lambda: ctx.commit([], bases, -1))
        for i, call in enumerate(calls):
            with pytest.raises(hs.SvdwError) as e:
                call()
            assert e.value.code == -1, i
