"""The commitments without a GPU: what the reference's SRS file holds (layout,
curve membership, the Lagrange sum, Lagrange / coefficient agreement through
ntt_cases.ntt_inverse), the oracle's group law on its edge cases, the
progression closed form and its tiled variant; the regimes restated from
commit.hpp against svdw_commit_plan and the documented workspace figures, the
digit-edge scalars, and what the device cases cover; the new C entries exist, keep the ABI version and check
their arguments in the documented order on a planning context; svdw_commit_plan;
read_srs; the wrappers refuse wrong shapes and dtypes."""
import ctypes as ct
import os
import re

import numpy as np
import pytest

import halo2_svd041_amd as hs
from halo2_svd041_amd import _lib
from halo2_svd041_amd.srs import read_srs
from commit_cases import (G, GPU_CASES, IDENTITY, JID, Q, R, ROOT, SRS8, commit_regimes, digit_edge_scalars, jadd,
                          jdouble, jmul, kernel_constant, msm, mul, neg, on_curve, parse_srs, point_bytes,
                          points_from_bytes, progression, progression_msm, signed_digits, task_cap, tiled_msm,
                          to_affine, to_jac)
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


def test_tiled_closed_form_equals_the_naive_msm():
    a0, d = 987654321, 2 ** 199 + 5
    for n, tile in ((64, 16), (32, 32), (8, 1)):
        bases = progression(tile, a0, d)
        s = _scalars(n, n + tile)
        s[1], s[n - 1] = 0, R - 1
        assert tiled_msm(tile, a0, d, s) == msm([bases[i % tile] for i in range(n)], s), (n, tile)
    assert tiled_msm(32, a0, d, s[:8]) == progression_msm(8, a0, d, s[:8])   # fewer rows than the tile


# ------------------------------------------------------------ the regimes
def test_regimes_restate_the_plan():
    for k in range(1, 29):
        r = commit_regimes(k)
        assert (r["c"], r["W"]) == hs.commit_plan(k), k
        assert r["B"] == 1 << (r["c"] - 1) and r["W"] * r["c"] >= 255 > (r["W"] - 1) * r["c"]
    # what DESIGN.md says of the table and of the tree
    assert [commit_regimes(k)["c"] for k in (10, 14, 16, 18, 20, 28)] == [8, 11, 13, 15, 16, 16]
    levels = [commit_regimes(k)["levels"] for k in (7, 8, 11, 12, 15, 16, 19, 20, 23, 24)]
    assert levels == [0, 1, 1, 2, 2, 3, 3, 4, 4, 5]
    assert commit_regimes(20)["chunks"] == 1024 and commit_regimes(13)["check_blocks"] == 64
    assert commit_regimes(13)["check_trips"] == 1 and commit_regimes(14)["check_trips"] == 2


def test_regimes_reproduce_the_documented_task_bytes():
    """include/svdw.h gives a task's workspace in whole bytes per row and per
    bucket; commit_task_bytes, restated, rounds to those from the sizes on at
    which the tree's and the chunks' own rounding is below half a byte."""
    text = open(os.path.join(ROOT, "include", "svdw.h")).read()
    row, bucket = map(int, re.search(r"about\s+\*?\s*(\d+) B per row and (\d+) B per bucket", text).groups())
    for k in range(8, 29):
        for c in {commit_regimes(k)["c"], 7, kernel_constant("kCommitMaxBits")}:
            r = commit_regimes(k, c)
            assert abs(r["row_bytes"] / (1 << k) - row) <= 0.5, (k, c)
            assert abs((r["task_bytes"] - r["row_bytes"]) / r["B"] - bucket) <= 0.5, (k, c)
    # under the default cap one task is the whole batch from k = 26 on
    assert [commit_regimes(k)["cap_over_per"] == 0 for k in (25, 26, 28)] == [False, True, True]


@pytest.mark.parametrize("c", range(2, 17))
def test_digit_edge_scalars_hit_every_edge(c):
    w, half, full = -(-255 // c), 1 << (c - 1), 1 << c
    edges = digit_edge_scalars(c)
    assert len(set(edges)) == len(edges) and all(0 < s < R for s in edges)
    digits = {s: signed_digits(s, c, w) for s in edges}    # asserts that no carry leaves the top window
    raw = {s: [(s >> (c * i)) & (full - 1) for i in range(w)] for s in edges}
    flat = [(i, d, raw[s][i]) for s in edges for i, d in enumerate(digits[s])]
    for s in edges:
        assert sum(d << (c * i) for i, d in enumerate(digits[s])) == s
    # the last positive and the first negative digit: in window 0, in a middle window, and in the windows that hold
    # bit 32 and bit 64 of the cell
    for at in (0, w // 2, 32 // c, 64 // c):
        assert {half, -(half - 1)} <= {d for i, d, _ in flat if i == at}, (c, at)
    # an all-ones digit that receives a carry: magnitude 0, and the carry goes on
    assert any(d == 0 and r == full - 1 for _, d, r in flat)
    # the carry ripples through every window whose bits are all ones
    ripple = digits[(1 << 253) - 1]
    ones = 253 // c
    assert ripple[0] == -1 and ripple[1:ones] == [0] * (ones - 1) and any(ripple[ones:])
    # the top window: non-zero, at its largest, and reached through a carry into it by the smallest such value
    top = digits[R - 1][-1]
    assert top > 0 and all(d[-1] <= top for d in digits.values())
    reached = [s for s in edges if digits[s][-1] == top]
    assert any(raw[s][-1] == top - 1 for s in reached) and signed_digits(min(reached) - 1, c, w)[-1] == top - 1


def _device_recoder(s: int, c: int, windows: int):
    """g1_signed_digits (csrc/g1_mul.hpp) restated word for word: eight 32-bit
    words shifted down c bits per window, the digit from the low word and the
    carry, and what it emits for every window: (magnitude, negative)."""
    w = [(s >> (32 * i)) & 0xFFFFFFFF for i in range(8)]
    full, half, carry, out = 1 << c, 1 << (c - 1), 0, []
    for _ in range(windows):
        d = (w[0] & (full - 1)) + carry
        for i in range(7):
            w[i] = (w[i] >> c) | ((w[i + 1] << (32 - c)) & 0xFFFFFFFF)
        w[7] >>= c
        carry = 1 if d > half else 0
        out.append((full - d if carry else d, carry))
    return out, carry, w


@pytest.mark.parametrize("c", range(2, 17))
def test_device_recoder_restates_the_signed_digits(c):
    """The one recoder the commit, SRS and G1 transform kernels share gives the
    digits of commit_cases.signed_digits at 0, 1, r - 1 and every window's half
    and half + 1 edge: they sum back to the scalar, zero digits are emitted with
    magnitude 0, and nothing is left above the top window."""
    windows, half = -(-255 // c), 1 << (c - 1)
    edges = [0, 1, R - 1] + [v << (c * i) for i in range(windows) for v in (half, half + 1)]
    for s in (v for v in edges if v < R):
        emitted, carry, left = _device_recoder(s, c, windows)
        digits = [-mag if neg else mag for mag, neg in emitted]
        assert digits == signed_digits(s, c, windows), (c, s)
        assert sum(d << (c * i) for i, d in enumerate(digits)) == s
        assert carry == 0 and not any(left), (c, s)
        assert all(0 <= mag <= half and (not neg or mag < half) for mag, neg in emitted)


def test_gpu_cases_cover_every_regime():
    """The cases test_commit_gpu.py takes from GPU_CASES reach every window
    size, every depth of the slot tree up to k = 20's, the loops that take a
    second trip only at size, both ends of the batch size and the checker's
    column chunks."""
    reg = [dict(commit_regimes(k, c, ncols, mib), k=k, name=name, ncols=ncols) for name, k, c, ncols, mib in GPU_CASES]
    max_bits = kernel_constant("kCommitMaxBits")
    assert {r["c"] for r in reg} >= set(range(2, max_bits + 1))
    assert {r["c"] * r["W"] for r in reg if r["c"] >= max_bits - 1} == {255, 256}      # the workload's two top windows
    assert {r["levels"] for r in reg} >= set(range(commit_regimes(20)["levels"] + 1))
    assert commit_regimes(20)["levels"] == 4 and max(r["k"] for r in reg) == 20
    assert any(r["chunks"] > kernel_constant("kCommitTreeThreads") and r["window_trips"] > 1 for r in reg)
    assert any(r["j0_top_bit"] == max_bits - 2 for r in reg)
    assert max(r["scan_per_thread"] for r in reg) == (1 << (max_bits - 1)) // kernel_constant("kCommitThreads") > 4
    assert any(r["check_blocks"] == kernel_constant("kCommitCheckBlocks") and r["check_trips"] >= 2
               for r in reg if r["name"] == "checker")
    assert any(1 < r["check_columns"] < r["ncols"] < 2 * r["check_columns"] for r in reg if r["name"] == "checker")
    # a batch at the grid's limit, with a column split between it and the next; one task larger than the cap
    assert any(r["T"] == task_cap() < r["tasks"] and r["T"] % r["W"] for r in reg)
    assert any(r["cap_over_per"] == 0 and r["T"] == 1 < r["tasks"] for r in reg)
    # the plan's own window on the deep trees
    deep = {r["k"]: r for r in reg if r["name"] == "deep"}
    assert (deep[16]["levels"], deep[18]["c"], deep[18]["chunks"]) == (3, 15, 512)
    assert (deep[20]["c"], deep[20]["levels"], deep[20]["chunks"]) == (16, 4, 1024)


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
