"""Read-out helpers that need no GPU: svdw_fr_convert between the canonical and
Montgomery forms against Python big integers, svdw_quantization against the
oracle's quantize, svdw_dequantization against the restatement of the chip's
construction (bit for bit), Rust's {:?} float formatting, and the documented
errors of the context read-out calls on a planning context."""
import ctypes as ct
import math
import struct

import numpy as np
import pytest

import halo2_svd041_amd as hs
import pyoracle as po
from halo2_svd041_amd import _lib
from halo2_svd041_amd._lib import Mat, Vec
from conftest import P_MOD

R_MOD = (1 << 256) % P_MOD


def exact_values():
    """The values of the form-conversion tests (also loaded as cells on the GPU)."""
    v = [0, 1, 2, P_MOD - 1, P_MOD - 2, (P_MOD - 1) // 2, (P_MOD + 1) // 2]
    for k in (31, 32, 33, 63, 64, 127, 128, 253):
        v += [1 << k, (1 << k) - 1]
    v += [R_MOD, R_MOD * R_MOD % P_MOD]
    rs = np.random.RandomState(20261)
    v += [int.from_bytes(rs.bytes(40), "little") % P_MOD for _ in range(200)]
    return v


def to_mont(x: int) -> int:
    return (x << 256) % P_MOD


def ints(a) -> list:
    return [hs.words_to_int(r) for r in np.asarray(a).reshape(-1, 4)]


def dequant_ref(x: int, P: int) -> float:
    """The construction svdw.h states for FixedPointChip041::dequantization."""
    neg = x > (P_MOD - 1) // 2
    m = (P_MOD - x if neg else x) % (1 << 128)
    S = 1 << P
    r = float(m // S) + float(m % S) / float(S)
    return -r if neg else r


def bits(x: float) -> bytes:
    return struct.pack("<d", x)


def test_fr_convert_matches_big_integers():
    vals = exact_values()
    mont = hs.fr_convert(vals, "canonical", "montgomery")
    assert mont.shape == (len(vals), 4) and mont.dtype == np.uint64
    assert ints(mont) == [to_mont(x) for x in vals]
    back = hs.fr_convert(mont, "montgomery", "canonical")
    assert ints(back) == vals
    assert ints(hs.fr_convert(vals, "canonical", "canonical")) == vals
    assert ints(hs.fr_convert(mont, "montgomery", "montgomery")) == ints(mont)


def test_fr_convert_in_place():
    vals = exact_values()
    a = np.array([hs.int_to_words(v) for v in vals], dtype=np.uint64)
    rc = _lib.lib().svdw_fr_convert(a.ctypes.data, len(vals), 0, 1, a.ctypes.data)
    assert rc == 0
    assert ints(a) == [to_mont(x) for x in vals]
    rc = _lib.lib().svdw_fr_convert(a.ctypes.data, len(vals), 1, 0, a.ctypes.data)
    assert rc == 0 and ints(a) == vals


@pytest.mark.parametrize("bad", [P_MOD, P_MOD + 1, (1 << 256) - 1])
@pytest.mark.parametrize("from_,to", [("canonical", "montgomery"), ("montgomery", "canonical")])
def test_fr_convert_rejects_unreduced_input(bad, from_, to):
    with pytest.raises(hs.SvdwError) as e:
        hs.fr_convert([1, bad, 2], from_, to)
    assert e.value.code == -1 and ">= p" in str(e.value)


def test_fr_convert_rejects_unknown_form():
    a = np.zeros((1, 4), dtype=np.uint64)
    L = _lib.lib()
    for f, t in ((2, 0), (0, 2), (-1, 1), (1, 7)):
        assert L.svdw_fr_convert(a.ctypes.data, 1, f, t, a.ctypes.data) == -1
        assert b"form" in L.svdw_last_error()
    with pytest.raises(hs.SvdwError):
        hs.fr_convert([1], "canonical", "mont")
    assert L.svdw_fr_convert(None, 1, 0, 1, a.ctypes.data) == -1


def quant_inputs(P):
    rs = np.random.RandomState(77 + P)
    tie = 0.5 * 2.0 ** -P
    xs = [0.0, -0.0, tie, -tie, 3 * tie, -3 * tie, float("nan"), float("inf"), float("-inf"), 1e300, -1e300]
    xs += list(rs.uniform(-100.0, 100.0, 64)) + list(rs.uniform(-1e-9, 1e-9, 16))
    return xs


@pytest.mark.parametrize("P", [1, 32, 42, 63])
def test_quantization_matches_oracle(P):
    for x in quant_inputs(P):
        assert hs.quantization(x, P) == po.quantize(float(x), P), (x, P)
    assert hs.quantization(0.5 * 2.0 ** -P, P) == 1               # the tie rounds away from zero
    assert hs.quantization(-0.5 * 2.0 ** -P, P) == P_MOD - 1
    assert hs.quantization(1e300, P) == (1 << 128) - 1            # saturates
    assert hs.quantization(float("nan"), P) == 0


def test_quantization_rejects_bad_precision():
    w = (ct.c_uint64 * 4)()
    d = ct.c_double()
    for P in (0, 64):
        assert _lib.lib().svdw_quantization(1.0, P, w) == -2
        assert _lib.lib().svdw_dequantization(w, P, ct.byref(d)) == -2
    assert _lib.lib().svdw_quantization(1.0, 32, None) == -1
    assert _lib.lib().svdw_dequantization(None, 32, ct.byref(d)) == -1
    with pytest.raises(hs.SvdwError):
        _lib.check(_lib.lib().svdw_dequantization(hs.int_to_words(P_MOD).ctypes.data, 32, ct.byref(d)))


def dequant_cases():
    cases = []
    for P in (1, 32, 63):
        for x in quant_inputs(P):
            cases.append((po.quantize(float(x), P), P))
    cases += [((1 << 54) + 3, 1)]
    top = (1 << 128) - 1
    for P in (1, 32, 63):
        cases += [(top, P), (P_MOD - top, P), ((1 << 200) + (1 << 130) + 12345, P),
                  (P_MOD - ((1 << 140) + 99), P), ((P_MOD - 1) // 2, P), ((P_MOD + 1) // 2, P),
                  (0, P), (1, P), (P_MOD - 1, P)]
    cases += [((1 << 63) - 1, 63), ((1 << 62) + 1, 63), ((5 << 63) + (1 << 63) - 1, 63),
              ((1 << 127) + (1 << 62) + 1, 63), (P_MOD - ((1 << 63) - 1), 63)]
    # integer parts that need rounding to 53 bits: ties, just above and below a tie
    for k in (54, 60, 64, 65, 100, 126):
        for low in (0, 1, (1 << (k - 53)) - 1, 1 << (k - 53), (1 << (k - 53)) + 1, 3 << (k - 53)):
            cases.append(((((1 << k) + low) << 1) + 1, 1))
    return cases


def test_dequantization_bit_exact():
    for x, P in dequant_cases():
        got, want = hs.dequantization(x, P), dequant_ref(x, P)
        assert bits(got) == bits(want), (x, P, got, want)
    assert hs.dequantization((1 << 54) + 3, 1) == 2.0 ** 53       # tie to even, then an absorbed 0.5
    assert bits(hs.dequantization(0, 32)) == bits(0.0)            # +0.0
    # only the low 128 bits of the magnitude count
    assert hs.dequantization((1 << 200) + (7 << 32), 32) == 7.0
    # the sign boundary
    assert hs.dequantization((P_MOD - 1) // 2, 32) > 0 > hs.dequantization((P_MOD + 1) // 2, 32)


@pytest.mark.parametrize("P", [1, 32, 42, 63])
def test_dequantization_inverts_quantization(P):
    rs = np.random.RandomState(5 + P)
    for x in list(rs.uniform(-100.0, 100.0, 200)) + [0.0, -0.0, 99.999, -99.999]:
        assert abs(hs.dequantization(hs.quantization(x, P), P) - x) <= 2.0 ** -(P + 1), (x, P)


@pytest.mark.parametrize("x,want", [
    (1.0, "1.0"), (-0.0, "-0.0"), (0.0, "0.0"), (0.1, "0.1"), (1e-7, "1e-7"), (1e16, "1e16"),
    (123456789.125, "123456789.125"), (5e-324, "5e-324"), (1e-5, "0.00001"), (9.999e-6, "9.999e-6"),
    (1e15, "1000000000000000.0"), (1.5e16, "1.5e16"), (-2.5, "-2.5"), (1.2345e-7, "1.2345e-7"),
    (1.7976931348623157e308, "1.7976931348623157e308"), (100.0, "100.0"), (0.001, "0.001"),
    (float("inf"), "inf"), (float("-inf"), "-inf"), (float("nan"), "NaN"), (-1e-7, "-1e-7"),
    (9007199254740993.0, "9007199254740992.0"), (0.30000000000000004, "0.30000000000000004")])
def test_format_f64_debug(x, want):
    assert hs.format_f64_debug(x) == want
    if not math.isnan(x):
        assert float(hs.format_f64_debug(x)) == x


def test_dry_context_has_no_cells():
    """A planning context answers every read-out call with SVDW_EINVAL and the
    reason; argument errors come first."""
    L = _lib.lib()
    ctx = hs.Context(device=-1, precision_bits=32, lookup_bits=19)
    m = hs.ZkMatrix.new(ctx, np.ones((2, 3)))
    v = hs.ZkVector.new(ctx, np.ones(3))
    buf = np.zeros((8, 4), dtype=np.uint64)
    dbl = np.zeros(8)
    p, d = buf.ctypes.data, dbl.ctypes.data
    calls = [
        lambda: L.svdw_export_cells(ctx.handle, 0, 0, 0, 1, 1, p),
        lambda: L.svdw_copy_cells(ctx.handle, 0, 0, 0, 1, 1, p),
        lambda: L.svdw_copy_cells(ctx.handle, 0, 1, 0, 0, 0, p),
        lambda: L.svdw_export_mat(ctx.handle, ct.byref(m.mat), 0, p, 0),
        lambda: L.svdw_export_mat(ctx.handle, ct.byref(m.mat), 1, p, 1),
        lambda: L.svdw_export_vec(ctx.handle, ct.byref(v.vec), 1, p, 0),
        lambda: L.svdw_dequantize_mat(ctx.handle, ct.byref(m.mat), d, 0),
        lambda: L.svdw_dequantize_vec(ctx.handle, ct.byref(v.vec), d, 0),
    ]
    for call in calls:
        assert call() == -1
        assert L.svdw_last_error() == b"planning context has no cells"
    assert L.svdw_assign_columns_form(ctx.handle, 0, 1, p, None, None) == -1
    assert b"needs a device context" in L.svdw_last_error()
    for fn in (lambda: ctx.cells(0), lambda: ctx.cells(1, lookup=True, form="montgomery"), m.values, v.values, m.dequantize, v.dequantize, m.print, v.print):
        with pytest.raises(hs.SvdwError, match="planning context has no cells"):
            fn()
    # argument errors: null pointers, unknown forms
    assert L.svdw_copy_cells(ctx.handle, 0, 0, 0, 1, 2, p) == -1 and b"form" in L.svdw_last_error()
    assert L.svdw_export_mat(ctx.handle, ct.byref(m.mat), -1, p, 0) == -1 and b"form" in L.svdw_last_error()
    assert L.svdw_assign_columns_form(ctx.handle, 0, 5, p, None, None) == -1 and b"form" in L.svdw_last_error()
    assert L.svdw_copy_cells(None, 0, 0, 0, 1, 0, p) == -1
    assert L.svdw_copy_cells(ctx.handle, 0, 0, 0, 1, 0, None) == -1
    assert L.svdw_export_cells(ctx.handle, 0, 0, 0, 1, 0, None) == -1
    assert L.svdw_export_mat(ctx.handle, None, 0, p, 0) == -1
    assert L.svdw_export_vec(ctx.handle, ct.byref(v.vec), 0, None, 0) == -1
    assert L.svdw_dequantize_mat(ctx.handle, ct.byref(m.mat), None, 0) == -1
    assert L.svdw_dequantize_vec(None, ct.byref(v.vec), d, 0) == -1
    assert L.svdw_copy_cells(ctx.handle, 2, 0, 0, 1, 0, p) == -1
    with pytest.raises(hs.SvdwError):
        ctx.cells(0, form="mont")
    ctx.close()
