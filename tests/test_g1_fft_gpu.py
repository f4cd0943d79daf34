"""svdw_g1_mul, svdw_g1_fft and svdw_check_lagrange on the device against the
scalar oracle (g1_fft_cases.py: a transform of [a_j] G is [A_i] G with A the DFT
of a mod r) and against the reference's own file: the inverse transform of the
golden g is the golden g_lagrange byte for byte (the parity pin, no secret
involved), and downsize() of the file rewrites it. Then downsize to every
smaller k, the edge vectors in both directions, the multiplication alone at
every window with the digit edges and the scalars from r on, lengths ragged
against a thread's group and a block, pieces under a small scratch cap, larger
sizes device against device, and the independent check against tampering.
Outputs are prefilled with a sentinel byte; comparisons are byte for byte."""
import functools

import numpy as np
import pytest

from commit_cases import G, IDENTITY, R, SRS8, digit_edge_scalars, mul, point_bytes, points_from_bytes, progression
from g1_fft_cases import (big_scalars, dft_scalars, edge_vectors, multiplication_count, pieces, planned_window,
                          points_of, quadratic_points)
from permutation_cases import omega
from srs_cases import SECRET, block_outputs, golden, lagrange_scalars, srs_constant

pytestmark = pytest.mark.gpu

SENTINEL = 0xAB
FORMS = ("canonical", "montgomery")
COMBOS = [(f, b) for f in FORMS for b in FORMS]            # (cells' form, points' form)
A0, D = 0x1234567, (1 << 251) + 0x89abcdef                 # points [A0 + i D] G: commit_cases.progression
S0, E = 0xfeedface12345, (1 << 250) + 0x13579bdf           # scalars S0 + i E
RHO = 0x1f2e3d4c5b6a79880123456789abcdef0fedcba9876543210011223344556677 % R


@pytest.fixture(scope="module")
def ctx(gpu_ctx_factory):
    return gpu_ctx_factory(32, 8)


def _rand(n: int, seed: int) -> list:
    rs = np.random.RandomState(seed)
    return [int.from_bytes(rs.bytes(32), "little") % R for _ in range(n)]


def _scalars(vals, form: str):
    """[n, 32] u8 device cells in `form`."""
    import torch
    import halo2_svd041_amd as hs
    a = np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint8).reshape(-1, 32).copy()
    if form == "montgomery":
        a = hs.fr_convert(a.view("<u8").reshape(-1, 4), "canonical", "montgomery").view(np.uint8).reshape(a.shape)
    return torch.from_numpy(a).cuda()


def _device_points(points, form: str = "montgomery"):
    import torch
    return torch.from_numpy(np.frombuffer(point_bytes(points, form), dtype=np.uint8).reshape(-1, 64).copy()).cuda()


def _prefilled(n: int):
    import torch
    return torch.full((n, 64), SENTINEL, dtype=torch.uint8, device="cuda")


def _raw(t) -> bytes:
    return t.cpu().numpy().tobytes()


def _points(t, form: str = "montgomery") -> list:
    return points_from_bytes(_raw(t), form)


# ------------------------------------------------------------ 1. the parity pin
def test_the_inverse_transform_of_the_golden_g_is_the_golden_g_lagrange(ctx, tmp_path):
    from halo2_svd041_amd import srs
    k, g, gl = golden()
    n = 1 << k
    for bf in FORMS:
        out, res = ctx.g1_fft(_device_points(g, bf), k, inverse=True, bases_form=bf, out=_prefilled(n))
        assert _raw(out) == point_bytes(gl, bf), bf
        assert res == {"k": 8, "stages": 8, "window_bits": planned_window(), "windows": -(-255 // planned_window()),
                       "rows": n, "multiplications": multiplication_count(k, True), "identity_inputs": 0,
                       "identity_outputs": 0}
        back, res = ctx.g1_fft(_device_points(gl, bf), k, bases_form=bf, out=_prefilled(n))
        assert _raw(back) == point_bytes(g, bf), bf
        assert res["multiplications"] == multiplication_count(k, False)
    # the file rewrites itself without its secret
    d = srs.read_srs(SRS8)
    assert "s" not in d
    small = srs.downsize(ctx, d, 8)
    assert small["k"] == 8 and "s" not in small and small["g2"] == d["g2"]
    srs.write_srs(tmp_path / "kzg_bn254_8.srs", small)
    assert (tmp_path / "kzg_bn254_8.srs").read_bytes() == open(SRS8, "rb").read()
    assert _raw(srs.g_to_lagrange(ctx, d["g"])) == point_bytes(gl, "montgomery")      # k from the length


# -------------------------------------------------- 2. downsize below the file's
@pytest.mark.parametrize("k", range(1, 8))
def test_downsize_to_the_sizes_below_the_file(ctx, k):
    """k = 1: the first stage is the last; k = 2: no middle stage; k = 3: one."""
    from halo2_svd041_amd import srs
    n = 1 << k
    d = srs.read_srs(SRS8)
    small = srs.downsize(ctx, {**d, "s": SECRET}, k)
    assert small["k"] == k and small["s"] == SECRET and small["g2"] == d["g2"]
    assert small["g"].tobytes() == point_bytes(golden()[1][:n], "montgomery")
    assert _raw(small["g_lagrange"]) == point_bytes(points_of(lagrange_scalars(k, SECRET)), "montgomery")
    # a device tensor for g, longer than 2^k, serves as well
    dg = _device_points(golden()[1][:2 * n])
    assert _raw(srs.g_to_lagrange(ctx, dg, k)) == _raw(small["g_lagrange"])


# ------------------------------------- 3. edge vectors, forward and inverse
@pytest.mark.parametrize("k", range(1, 7))
def test_edge_vectors_against_the_scalar_oracle(ctx, k):
    n, a, t = 1 << k, 0x1234567 + k, 3 % (1 << k)
    vectors = edge_vectors(k, a, t, 40 + k)
    assert vectors["geometric"][1] == a * pow(omega(k), t, R) % R
    for v, (name, vals) in enumerate(vectors.items()):
        for inverse in (False, True):
            bf = FORMS[(k + v + inverse) % 2]
            want_s = dft_scalars(vals, k, inverse)
            want = points_of(want_s)
            out, res = ctx.g1_fft(_device_points(points_of(vals), bf), k, inverse=inverse, bases_form=bf,
                                  out=_prefilled(n))
            assert _raw(out) == point_bytes(want, bf), (name, inverse, bf, _points(out, bf), want)
            assert res["identity_inputs"] == vals.count(0), (name, inverse)
            assert res["identity_outputs"] == want.count(IDENTITY) == want_s.count(0), (name, inverse)
            assert res["multiplications"] == multiplication_count(k, inverse), (name, inverse)
            assert (res["k"], res["stages"], res["rows"]) == (k, k, n)
        if name == "identity":
            assert want.count(IDENTITY) == n
        if name in ("constant", "alternating", "geometric"):
            assert want.count(IDENTITY) == n - 1           # (of the inverse transform, the last one made)


# --------------------------------- 4. g1_mul: every window, bases, digit edges
@functools.lru_cache(maxsize=None)
def _window_bases():
    return (G, golden()[1][5], IDENTITY)


@pytest.mark.parametrize("c", range(2, 7))
def test_g1_mul_every_window_size(ctx, c):
    vals = list(dict.fromkeys([0, 1, R - 1] + digit_edge_scalars(c))) + _rand(3, 200 + c)
    big = big_scalars(c)
    assert big[:2] == [R, R + 5] and 0 < big[2] < 1 << 255
    for b, base in enumerate(_window_bases()):
        form, bf = COMBOS[(c + b) % 4]
        pts = _device_points([base] * len(vals), bf)
        out, res = ctx.g1_mul(pts, _scalars(vals, form), form=form, bases_form=bf, window_bits=c,
                              out=_prefilled(len(vals)))
        want = [mul(base, v) for v in vals]
        assert _raw(out) == point_bytes(want, bf), (c, b, form, bf, _points(out, bf), want)
        assert res == {"window_bits": c, "windows": -(-255 // c), "points": len(vals), "zero_scalars": 1,
                       "identity_inputs": len(vals) if base == IDENTITY else 0,
                       "identity_outputs": want.count(IDENTITY)}
        assert want.count(IDENTITY) == (len(vals) if base == IDENTITY else 1)
        # the integers from r on, which only a canonical cell holds: r cancels in its last add, r + 5 is 5, and
        # the doubling scalar meets its own table entry
        out, res = ctx.g1_mul(pts[:3], _scalars(big, "canonical"), bases_form=bf, window_bits=c, out=_prefilled(3))
        want = [IDENTITY, mul(base, 5), mul(base, big[2] - R)]
        assert _raw(out) == point_bytes(want, bf), (c, b, bf, _points(out, bf), want)
        assert (res["zero_scalars"], res["identity_outputs"]) == (0, 3 if base == IDENTITY else 1)


# ------------------------------------------- 5. g1_mul: lengths, buffers, pieces
@functools.lru_cache(maxsize=None)
def _length_oracle(n: int):
    return progression(n, A0, D), [(S0 + i * E) % R for i in range(n)], quadratic_points(n, A0, D, S0, E)


@pytest.mark.parametrize("n", (1, 7, 257, 4099))
def test_g1_mul_lengths_and_buffers(ctx, n):
    group, block = srs_constant("kFbGroup"), block_outputs()
    assert 1 < group and 7 % group and 257 % block and 4099 % block and 4099 > block   # ragged, more than one block
    assert 257 % 64 and 4099 % 64                                                     # and against k_g1_mul's block
    pts, vals, want = _length_oracle(n)
    tail = 3
    for form, bf in ((FORMS[0], FORMS[1]), (FORMS[1], FORMS[0])):
        out, res = ctx.g1_mul(_device_points(pts, bf), _scalars(vals, form), form=form, bases_form=bf,
                              out=_prefilled(n + tail))
        raw = _raw(out)
        assert raw[:64 * n] == point_bytes(want, bf), (n, form, bf)
        assert raw[64 * n:] == bytes([SENTINEL]) * (64 * tail), (n, form)
        assert res == {"window_bits": planned_window(), "windows": -(-255 // planned_window()), "points": n,
                       "zero_scalars": 0, "identity_inputs": 0, "identity_outputs": 0}
    empty, res = ctx.g1_mul(_device_points(pts)[:0], _scalars(vals, "canonical")[:0], out=_prefilled(tail))
    assert _raw(empty) == bytes([SENTINEL]) * (64 * tail) and res["points"] == 0


def test_g1_mul_in_three_pieces(ctx):
    n, c, mib = 4099, 3, 1
    assert pieces(n, c, mib) == 3
    pts, vals, want = _length_oracle(n)
    ctx.set_option("commit_scratch_mib", mib)
    try:
        out, res = ctx.g1_mul(_device_points(pts), _scalars(vals, "canonical"), window_bits=c, out=_prefilled(n + 1))
        assert planned_window(mib) == 2
        _, planned = ctx.g1_mul(_device_points(pts[:4]), _scalars(vals[:4], "canonical"))
    finally:
        ctx.set_option("commit_scratch_mib", 1024)
    assert _raw(out) == point_bytes(want, "montgomery") + bytes([SENTINEL]) * 64
    assert (res["window_bits"], res["points"], res["identity_outputs"]) == (c, n, 0)
    assert planned["window_bits"] == 2                     # the plan follows the cap


# ------------------------------------------ 6. larger sizes, device against device
@pytest.mark.parametrize("k,window_bits,mib", [(11, 0, 1024), (11, 6, 1), (14, 0, 1024)])
def test_larger_sizes_device_against_device(ctx, k, window_bits, mib):
    """srs_setup's g_lagrange comes from the fixed-base kernels and the setup's
    own Lagrange column; the inverse transform of its g must be the same bytes."""
    n = 1 << k
    dg, dl, _ = ctx.srs_setup(k, SECRET)
    if mib != 1024:
        assert pieces(n // 2, window_bits, mib) >= 3       # several pieces per stage
    ctx.set_option("commit_scratch_mib", mib)
    ctx.set_option("g1_window_bits", window_bits)
    try:
        out, res = ctx.g1_fft(dg, k, inverse=True, out=_prefilled(n))
        back, res_f = ctx.g1_fft(out, k, out=_prefilled(n))
    finally:
        ctx.set_option("commit_scratch_mib", 1024)
        ctx.set_option("g1_window_bits", 0)
    assert _raw(out) == _raw(dl)
    assert _raw(back) == _raw(dg)
    assert res["window_bits"] == (window_bits or planned_window())
    assert (res["multiplications"], res_f["multiplications"]) == (multiplication_count(k, True),
                                                                  multiplication_count(k, False))
    assert (res["identity_inputs"], res["identity_outputs"], res_f["identity_outputs"]) == (0, 0, 0)
    assert ctx.check_lagrange(dg, out, k, RHO) == {"points_checked": 2 * n, "points_off_curve": 0, "failed": 0}


# ------------------------------------------------------------------ 7. the check
@pytest.mark.parametrize("bf", FORMS)
def test_check_lagrange_passes_and_finds_tampering(ctx, bf):
    import torch
    k, g, gl = golden()
    n = 1 << k
    dg, dl = _device_points(g, bf), _device_points(gl, bf)
    ok = {"points_checked": 2 * n, "points_off_curve": 0, "failed": 0}
    before = (_raw(dg), _raw(dl))
    assert ctx.check_lagrange(dg, dl, k, RHO, bases_form=bf) == ok
    assert ctx.check_lagrange(dg, dl, k, 1, bases_form=bf) == ok
    assert (_raw(dg), _raw(dl)) == before                  # it writes to no input
    swapped = dl.clone()
    swapped[17], swapped[200] = dl[200], dl[17]
    assert ctx.check_lagrange(dg, swapped, k, RHO, bases_form=bf) == {**ok, "failed": 1}
    bad = dg.clone()
    bad[5] = dg[6]
    assert ctx.check_lagrange(bad, dl, k, RHO, bases_form=bf) == {**ok, "failed": 1}
    # rho = 0 sees row 0 of g_lagrange alone: the swap of rows 17 and 200 passes, a wrong row 0 does not
    assert ctx.check_lagrange(dg, dl, k, 0, bases_form=bf) == ok
    assert ctx.check_lagrange(dg, swapped, k, 0, bases_form=bf) == ok
    row0 = dl.clone()
    row0[0] = dl[1]
    assert ctx.check_lagrange(dg, row0, k, 0, bases_form=bf) == {**ok, "failed": 1}
    off = dl.clone()
    off[3] = torch.from_numpy(np.frombuffer(point_bytes([(1, 3)], bf), dtype=np.uint8).copy()).cuda()
    res = ctx.check_lagrange(dg, off, k, RHO, bases_form=bf)
    assert (res["points_checked"], res["points_off_curve"], res["failed"]) == (2 * n, 1, 1)
    assert (_raw(dg), _raw(dl)) == before
