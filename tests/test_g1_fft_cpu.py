"""The G1 transforms without a GPU: the three C entries exist, keep the ABI
version and check their arguments in the documented order on a planning
context; the wrappers and the SRS helpers refuse host tensors, wrong shapes and
a k above the dict's; read_srs returns the file's G2 bytes and write_srs writes
them back without a secret; the multiplication counts against a direct count
over the stages; and the scalar oracle itself: the inverse DFT of the powers of
the secret is the Lagrange column of the setup, which is what g_to_lagrange
claims about the points."""
import ctypes as ct

import numpy as np
import pytest

import halo2_svd041_amd as hs
from commit_cases import R, SRS8, signed_digits
from g1_fft_cases import (big_scalars, dft_scalars, doubling_scalar, edge_vectors, g1_constant, mul_products,
                          multiplication_count, multiplications_by_stage, pieces, planned_window, point_bytes_per,
                          quadratic_points)
from halo2_svd041_amd import _lib, srs
from permutation_cases import omega
from srs_cases import SECRET, golden, lagrange_scalars, power_scalars

EINVAL, ERANGE = -1, -2


def _err() -> str:
    return _lib.lib().svdw_last_error().decode()


def _words(x: int):
    return (ct.c_uint64 * 4)(*[(x >> (64 * i)) & (2 ** 64 - 1) for i in range(4)])


def test_entries_exist_and_the_abi_version_stays():
    L = _lib.lib()
    assert L.svdw_abi_version() == 2
    for name in ("svdw_g1_mul", "svdw_g1_fft", "svdw_check_lagrange"):
        assert name in _lib.SIGNATURES and getattr(L, name)


def _mul(ctx, form=0, bases_form=1, window_bits=0, n=5, points=4096, scalars=8192, out=16384, result=True):
    r = _lib.G1MulResult()
    return _lib.lib().svdw_g1_mul(ctx.handle, form, bases_form, points, scalars, n, window_bits, out,
                                  ct.byref(r) if result else None)


def test_g1_mul_checks_its_arguments_in_the_documented_order():
    """Each call breaks one rule and every rule after it."""
    with hs.Context(device=-1, precision_bits=32, lookup_bits=8) as ctx:
        assert _mul(ctx, form=7, bases_form=7, window_bits=7, result=False) == EINVAL and "null" in _err()
        assert _mul(ctx, form=7, bases_form=7, window_bits=7) == EINVAL and "form" in _err()
        assert _mul(ctx, bases_form=2, window_bits=7) == EINVAL and "form" in _err()
        for wb in (1, 7, 16, 1 << 31):
            assert _mul(ctx, window_bits=wb) == ERANGE and "window_bits" in _err()
            assert _mul(ctx, window_bits=wb, points=None, out=None) == ERANGE
        for wb in (0, 2, 6):
            assert _mul(ctx, window_bits=wb, points=None) == EINVAL and "device context" in _err()
            assert _mul(ctx, window_bits=wb, n=0) == EINVAL and "device context" in _err()
            assert _mul(ctx, window_bits=wb, out=4096) == EINVAL and "device context" in _err()   # an overlap


def _fft(ctx, k=3, bases_form=1, inverse=0, points=4096, out=65536, result=True):
    r = _lib.G1FftResult()
    return _lib.lib().svdw_g1_fft(ctx.handle, k, bases_form, inverse, points, out, ct.byref(r) if result else None)


def _check(ctx, k=3, bases_form=1, g=4096, gl=65536, rho=7, result=True):
    r = _lib.LagrangeCheck()
    return _lib.lib().svdw_check_lagrange(ctx.handle, k, bases_form, g, gl, _words(rho),
                                          ct.byref(r) if result else None)


def test_g1_fft_and_check_lagrange_check_their_arguments_in_the_documented_order():
    with hs.Context(device=-1, precision_bits=32, lookup_bits=8) as ctx:
        for call in (_fft, _check):
            assert call(ctx, k=29, bases_form=7, result=False) == EINVAL and "null" in _err()
            assert call(ctx, k=29, bases_form=7) == EINVAL and "form" in _err()
            for k in (0, 29, 1 << 31):
                assert call(ctx, k=k) == ERANGE and "k must be" in _err()
            for k in (1, 28):
                assert call(ctx, k=k) == EINVAL and "device context" in _err()
        assert _fft(ctx, k=29, points=None, out=None) == ERANGE
        assert _fft(ctx, points=None, out=None) == EINVAL and "device context" in _err()
        assert _fft(ctx, out=4096) == EINVAL and "device context" in _err()             # an overlap
        assert _check(ctx, k=29, bases_form=7, rho=R) == EINVAL and "form" in _err()
        assert _check(ctx, k=29, rho=R) == EINVAL and "rho must be below p" in _err()
        assert _check(ctx, k=29, rho=2 ** 256 - 1) == EINVAL and "rho must be below p" in _err()
        assert _check(ctx, g=None, gl=None) == EINVAL and "device context" in _err()
        r = _lib.LagrangeCheck()
        assert _lib.lib().svdw_check_lagrange(ctx.handle, 3, 1, 4096, 65536, None, ct.byref(r)) == EINVAL
        assert "null" in _err()


def test_python_wrappers_refuse_host_tensors_wrong_shapes_and_values():
    import torch
    host = torch.zeros((8, 64), dtype=torch.uint8)          # host tensors: not device tensors
    cells = torch.zeros((8, 32), dtype=torch.uint8)
    g8 = srs.read_srs(SRS8)
    with hs.Context(device=-1, precision_bits=32, lookup_bits=8) as ctx:
        calls = (lambda: ctx.g1_mul(host, cells),
                 lambda: ctx.g1_mul(np.zeros((8, 64), np.uint8), np.zeros((8, 32), np.uint8)),
                 lambda: ctx.g1_mul(None, None),
                 lambda: ctx.g1_fft(host, 3),
                 lambda: ctx.g1_fft(host, 3, inverse=True, bases_form="jacobian"),
                 lambda: ctx.g1_fft(None, 3),
                 lambda: ctx.check_lagrange(host, host, 3, 7),
                 lambda: ctx.check_lagrange(None, None, 3, 7),
                 lambda: ctx.check_lagrange(host, host, 3, R),
                 lambda: ctx.check_lagrange(host, host, 3, -1),
                 lambda: srs.downsize(ctx, g8, 9),              # above the dict's k
                 lambda: srs.downsize(ctx, g8, 0),
                 lambda: srs.g_to_lagrange(ctx, host, 4),       # 16 points of 8
                 lambda: srs.g_to_lagrange(ctx, host[:7]),      # not a power of two
                 lambda: srs.g_to_lagrange(ctx, host[:0]),
                 lambda: srs.g_to_lagrange(ctx, host, 3))       # a host tensor
        for i, call in enumerate(calls):
            with pytest.raises(hs.SvdwError):
                call()
                pytest.fail(f"call {i} was accepted")


def test_read_srs_returns_g2_and_write_srs_writes_it_back(tmp_path):
    raw = open(SRS8, "rb").read()
    d = srs.read_srs(SRS8)
    assert set(d) == {"k", "g", "g_lagrange", "g2"} and d["g2"] == raw[-256:] and len(d["g2"]) == 256
    srs.write_srs(tmp_path / "out.srs", d)                  # no "s": the G2 bytes go back unchanged
    assert (tmp_path / "out.srs").read_bytes() == raw
    # with "s" the G2 half is computed, exactly as before, whatever "g2" holds
    srs.write_srs(tmp_path / "s.srs", {**d, "s": SECRET, "g2": bytes(256)})
    assert (tmp_path / "s.srs").read_bytes() == raw
    # the generator is the first G2 point of any file
    assert d["g2"][:128] == srs._g2_bytes(srs._G2)
    for bad in ({"g2": None}, {"g2": raw[-255:]}, {"g2": None, "s": None}):
        with pytest.raises(hs.SvdwError):
            srs.write_srs(tmp_path / "bad.srs", {**d, **bad})
    with pytest.raises(hs.SvdwError):
        srs.write_srs(tmp_path / "bad.srs", {key: d[key] for key in ("k", "g", "g_lagrange")})


@pytest.mark.parametrize("inverse", (False, True))
def test_multiplication_counts_against_a_direct_count_over_the_stages(inverse):
    for k in range(1, 15):
        assert multiplication_count(k, inverse) == multiplications_by_stage(k, inverse), k
    n = 1 << 20
    assert multiplication_count(20, True) - multiplication_count(20, False) == n // 2 + 1
    assert (multiplication_count(1, False), multiplication_count(1, True)) == (0, 2)
    assert (multiplication_count(2, False), multiplication_count(2, True)) == (1, 4)


def test_the_plan_and_the_pieces():
    assert [mul_products(c) for c in range(2, 7)] == [4110, 3527, 3298, 3219, 3358]
    assert g1_constant("kG1MaxBits") == 6 and point_bytes_per(4) == 9 * 128
    assert g1_constant("kG1PlanBits") == 4
    assert planned_window() == 4 and planned_window(1) == 2 and planned_window(65536) == 4
    # the smallest cap that still admits c = 4 for a piece of kG1PlanPoints points, and one below
    edge = point_bytes_per(4) * g1_constant("kG1PlanPoints") >> 20
    assert planned_window(edge) == 4 and planned_window(edge - 1) == 3
    # a stage of a 2^20 transform: one piece under the default cap at the planned window, two at c = 5
    assert pieces(1 << 19, 4, 1024) == 1 and pieces(1 << 19, 5, 1024) == 2
    assert pieces(4099, 3, 1) == 3 and pieces(1 << 10, 6, 1) == 5
    # the digits of a window fit a byte with the sign, and a block's digits fit the 8 KiB the kernel declares
    assert (1 << (g1_constant("kG1MaxBits") - 1)) < 0x80
    assert -(-255 // 2) == g1_constant("kG1MaxWindows") and 64 * g1_constant("kG1MaxWindows") == 8192


@pytest.mark.parametrize("c", range(2, 7))
def test_the_doubling_scalar_by_its_digits(c):
    v = doubling_scalar(c)
    W = -(-255 // c)
    d = signed_digits(v, c, W)
    assert abs(d[0]) <= 1 << (c - 1) and d[0] % 2 == 1 and v < 1 << 255
    assert (v - d[0]) % R == d[0] % R                      # the accumulator before the last add is [d0] P
    assert big_scalars(c)[:2] == [R, R + 5] and signed_digits(R, c, W)[0] == -d[0]
    assert sum(x << (c * i) for i, x in enumerate(signed_digits(R, c, W))) == R


@pytest.mark.parametrize("k", range(1, 9))
def test_the_inverse_dft_of_the_powers_is_the_lagrange_column(k):
    """g_to_lagrange in scalars: g[j] = [s^j] G, so the inverse transform is
    [l_i(s)] G; and the forward transform undoes it."""
    ps, ls = power_scalars(k, SECRET), lagrange_scalars(k, SECRET)
    assert dft_scalars(ps, k, inverse=True) == ls
    if k <= 6:
        assert dft_scalars(ls, k) == ps


def test_the_oracle_on_the_edge_vectors():
    k, a, t = 3, 0x1234567, 3
    n, v = 1 << k, edge_vectors(3, 0x1234567, 3, 1)
    assert dft_scalars(v["identity"], k) == [0] * n
    assert dft_scalars(v["single_first"], k) == [a] * n
    assert dft_scalars(v["single_last"], k) == [a * pow(omega(k), (n - 1) * i, R) % R for i in range(n)]
    assert dft_scalars(v["constant"], k) == [n * a % R] + [0] * (n - 1)
    assert dft_scalars(v["alternating"], k) == [n * a % R if i == n // 2 else 0 for i in range(n)]
    assert dft_scalars(v["geometric"], k) == [n * a % R if i == n - t else 0 for i in range(n)]
    assert dft_scalars(v["geometric"], k, inverse=True) == [a if i == t else 0 for i in range(n)]
    for name, vals in v.items():
        assert dft_scalars(dft_scalars(vals, k), k, inverse=True) == vals, name


def test_quadratic_points_are_the_products():
    from commit_cases import mul, progression
    a0, d, s0, e = 0x1234567, (1 << 251) + 0x89abcdef, 0xfeedface, (1 << 250) + 12345
    pts = progression(9, a0, d)
    assert quadratic_points(9, a0, d, s0, e) == [mul(p, (s0 + i * e) % R) for i, p in enumerate(pts)]


def test_the_golden_file_is_its_own_lagrange_form_at_sampled_rows():
    """The pin in scalars: row i of the file's g_lagrange is [idft(s^j)_i] G."""
    from commit_cases import G, mul
    k, _, gl = golden()
    ls = dft_scalars(power_scalars(k, SECRET), k, inverse=True)
    for i in (0, 1, 100, 255):
        assert mul(G, ls[i]) == gl[i], i
