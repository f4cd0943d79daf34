"""The SRS without a GPU: the secret halo2-base's gen_srs draws and what the
reference's file says about it; write_srs against that file byte for byte (the
G2 arithmetic, its encoding, the layout) and through read_srs; the oracle's two
scalar columns against the file; the three C entries exist, keep the ABI
version and check their arguments in the documented order on a planning
context; the wrappers refuse wrong shapes."""
import ctypes as ct

import numpy as np
import pytest

import halo2_svd041_amd as hs
from commit_cases import G, Q, R, SRS8, mul, point_bytes
from halo2_svd041_amd import _lib, srs
from permutation_cases import omega
from srs_cases import (CHACHA_HEAD, SECRET, boundary_indices, edge_secrets, golden, lagrange_scalars, planned_window,
                       power_scalars)

EINVAL, ERANGE = -1, -2


def _err() -> str:
    return _lib.lib().svdw_last_error().decode()


def _words(x: int):
    return (ct.c_uint64 * 4)(*[(x >> (64 * i)) & (2 ** 64 - 1) for i in range(4)])


def test_default_secret_is_the_chacha_derivation():
    assert srs._chacha20_block0()[:8] == CHACHA_HEAD
    assert srs.default_secret() == SECRET
    assert mul(G, srs.default_secret()) == golden()[1][1]


def test_the_golden_file_follows_from_the_secret_at_sampled_rows():
    """The oracle's two columns against the file (every row is the issue's
    check; here the rows the device tests do not compare point-wise)."""
    k, g, gl = golden()
    ps, ls = power_scalars(k, SECRET), lagrange_scalars(k, SECRET)
    assert sum(ls) % R == 1
    for i in boundary_indices(1 << k, 100, 12):
        assert mul(G, ps[i]) == g[i] and mul(G, ls[i]) == gl[i], i


def test_write_srs_reproduces_the_golden_file(tmp_path):
    raw = open(SRS8, "rb").read()
    d = srs.read_srs(SRS8)
    d["s"] = SECRET
    srs.write_srs(tmp_path / "out.srs", d)
    assert (tmp_path / "out.srs").read_bytes() == raw


def test_write_then_read_round_trips(tmp_path):
    k, s = 3, 5
    g = np.frombuffer(point_bytes([mul(G, v) for v in power_scalars(k, s)], "montgomery"), np.uint8).reshape(-1, 64)
    gl = np.frombuffer(point_bytes([mul(G, v) for v in lagrange_scalars(k, s)], "montgomery"), np.uint8).reshape(-1, 64)
    path = tmp_path / "k3.srs"
    srs.write_srs(path, {"k": k, "g": g, "g_lagrange": gl, "s": s})
    back = srs.read_srs(path)
    assert back["k"] == k and np.array_equal(back["g"], g) and np.array_equal(back["g_lagrange"], gl)
    assert len(path.read_bytes()) == 4 + 2 * 64 * 8 + 256
    for bad in ({"k": 0}, {"k": 29}, {"s": R}, {"g": g[:4]}, {"g_lagrange": gl.astype(np.uint16)}):
        with pytest.raises(hs.SvdwError):
            srs.write_srs(path, {"k": k, "g": g, "g_lagrange": gl, "s": s, **bad})


def test_the_oracle_handles_the_edge_secrets():
    k = 3
    n, sec = 1 << k, edge_secrets(k)
    assert lagrange_scalars(k, 0) == [pow(n, -1, R)] * n
    assert power_scalars(k, 0) == [1] + [0] * (n - 1)
    for name, j in (("one", 0), ("omega3", 3), ("minus_one", n // 2)):
        assert lagrange_scalars(k, sec[name]) == [int(i == j) for i in range(n)], name
    for name in ("two", "minus_two"):
        ls = lagrange_scalars(k, sec[name])
        assert sum(ls) % R == 1 and 0 not in ls
        # the interpolation of X at s
        assert sum(l * w for l, w in zip(ls, power_scalars(k, omega(k)))) % R == sec[name]


def test_planned_window_keeps_the_table_in_l2():
    for n in (1, 8, 1 << 10, 1 << 20, 1 << 28):
        c = planned_window(n)
        assert 2 <= c <= 12 and (-(-255 // c) << (c - 1)) * 64 <= 4 << 20
    assert planned_window(1 << 20) == 12 and planned_window(1) < planned_window(1 << 10)


def test_entries_exist_and_the_abi_version_stays():
    L = _lib.lib()
    assert L.svdw_abi_version() == 2
    for name in ("svdw_fixed_base_mul", "svdw_srs_setup", "svdw_check_srs"):
        assert name in _lib.SIGNATURES and getattr(L, name)


def _fixed(ctx, form=0, base_form=1, base=None, window_bits=0, n=5, result=True):
    base = point_bytes([G], "montgomery") if base is None else base
    r = _lib.FixedBaseResult()
    return _lib.lib().svdw_fixed_base_mul(ctx.handle, form, base_form, base, 4096, n, window_bits, 8192,
                                          ct.byref(r) if result else None)


def test_fixed_base_mul_checks_its_arguments_in_the_documented_order():
    """Each call breaks one rule and every rule after it."""
    off = point_bytes([(1, 3)], "montgomery")
    big = (Q).to_bytes(32, "little") + (2).to_bytes(32, "little")
    with hs.Context(device=-1, precision_bits=32, lookup_bits=8) as ctx:
        assert _fixed(ctx, form=7, base=off, window_bits=17, result=False) == EINVAL and "null" in _err()
        assert _fixed(ctx, form=7, base_form=7, base=off, window_bits=17) == EINVAL and "form" in _err()
        assert _fixed(ctx, base_form=2, base=off, window_bits=17) == EINVAL and "form" in _err()
        assert _fixed(ctx, base=off, window_bits=17) == EINVAL and "curve" in _err()
        assert _fixed(ctx, base_form=0, base=big, window_bits=1) == EINVAL and "below q" in _err()
        # a Montgomery G read as canonical is not on the curve; the canonical G is
        assert _fixed(ctx, base_form=0, window_bits=1) == EINVAL and "curve" in _err()
        for wb in (1, 17, 1 << 31):
            assert _fixed(ctx, window_bits=wb) == ERANGE and "window_bits" in _err()
            assert _fixed(ctx, base_form=0, base=point_bytes([G], "canonical"), window_bits=wb) == ERANGE
            assert _fixed(ctx, base=bytes(64), window_bits=wb) == ERANGE      # the identity is a base
        for wb in (0, 2, 16):
            assert _fixed(ctx, window_bits=wb) == EINVAL and "device context" in _err()
            assert _fixed(ctx, window_bits=wb, n=0) == EINVAL and "device context" in _err()


def _setup(ctx, k=3, s=5, bases_form=1, g=4096, gl=8192, result=True):
    r = _lib.SrsResult()
    return _lib.lib().svdw_srs_setup(ctx.handle, k, _words(s), bases_form, g, gl, ct.byref(r) if result else None)


def _check(ctx, k=3, s=5, rho=7, bases_form=1, g=4096, gl=8192, result=True):
    r = _lib.SrsCheck()
    return _lib.lib().svdw_check_srs(ctx.handle, k, bases_form, g, gl, _words(s), _words(rho),
                                     ct.byref(r) if result else None)


def test_srs_setup_and_check_srs_check_their_arguments_in_the_documented_order():
    with hs.Context(device=-1, precision_bits=32, lookup_bits=8) as ctx:
        for call in (_setup, _check):
            assert call(ctx, k=29, s=R, bases_form=7, result=False) == EINVAL and "null" in _err()
            assert call(ctx, k=29, s=R, bases_form=7) == EINVAL and "form" in _err()
            assert call(ctx, k=29, s=R) == EINVAL and "s must be below p" in _err()
            assert call(ctx, k=29, s=2 ** 256 - 1) == EINVAL and "s must be below p" in _err()
            for k in (0, 29):
                assert call(ctx, k=k) == ERANGE and "k must be" in _err()
            for k in (1, 28):
                assert call(ctx, k=k, g=None, gl=None) == EINVAL and "device context" in _err()
        assert _check(ctx, k=29, rho=R) == EINVAL and "rho must be below p" in _err()
        assert _check(ctx, k=29, s=R, rho=R) == EINVAL and "s must be below p" in _err()


def test_python_wrappers_refuse_wrong_shapes_and_values():
    import torch
    host = torch.zeros((8, 64), dtype=torch.uint8)          # host tensors: not device tensors
    cells = torch.zeros((8, 32), dtype=torch.uint8)
    with hs.Context(device=-1, precision_bits=32, lookup_bits=8) as ctx:
        calls = (lambda: ctx.fixed_base_mul(point_bytes([G], "montgomery"), cells),
                 lambda: ctx.fixed_base_mul(bytes(63), cells),
                 lambda: ctx.fixed_base_mul(bytes(64), np.zeros((8, 32), np.uint8)),
                 lambda: ctx.srs_setup(3, R),
                 lambda: ctx.srs_setup(3, -1),
                 lambda: ctx.srs_setup(3, 5, g=host),
                 lambda: ctx.srs_setup(3, 5, bases_form="jacobian", g=None, g_lagrange=None),
                 lambda: ctx.check_srs(host, host, 3, 5, 7),
                 lambda: ctx.check_srs(None, None, 3, 5, 7))
        for i, call in enumerate(calls):
            with pytest.raises(hs.SvdwError):
                call()
                pytest.fail(f"call {i} was accepted")
