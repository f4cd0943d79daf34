"""svdw_fixed_base_mul, svdw_srs_setup and svdw_check_srs on the device against
the integer oracle (srs_cases.py, commit_cases.py) and against the reference's
own file: gen_srs(8) is tests/golden/kzg_bn254_8.srs byte for byte (the parity
pin), the smaller sizes are its prefixes, the edge secrets (0, members of the
domain, their neighbours), every window size with the digit edges placed,
lengths ragged against a thread's group and a block, chunked setups, either
output left out, and the independent check against tampering. Outputs are
prefilled with a sentinel byte; comparisons are byte for byte."""
import functools

import numpy as np
import pytest

from commit_cases import (G, IDENTITY, R, SRS8, digit_edge_scalars, kernel_constant, mul, point_bytes, points_from_bytes,
                          progression)
from srs_cases import (SECRET, block_outputs, boundary_indices, doubling_scalar, edge_secrets, golden,
                       lagrange_scalars, planned_window, points_of, power_scalars, srs_constant, window_scalars)

pytestmark = pytest.mark.gpu

SENTINEL = 0xAB
FORMS = ("canonical", "montgomery")
COMBOS = [(f, b) for f in FORMS for b in FORMS]            # (cells' form, base's form)
A0, D = 0x1234567, (1 << 251) + 0x89abcdef                 # scalars A0 + i D: the points are commit_cases.progression
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


def _prefilled(n: int):
    import torch
    return torch.full((n, 64), SENTINEL, dtype=torch.uint8, device="cuda")


def _raw(t) -> bytes:
    return t.cpu().numpy().tobytes()


def _points(t, form: str = "montgomery") -> list:
    return points_from_bytes(_raw(t), form)


# ------------------------------------------------------------ 1. the parity pin
def test_gen_srs_8_is_the_golden_file(ctx, tmp_path):
    from halo2_svd041_amd import srs
    k, g, gl = golden()
    for bf in FORMS:
        dg, dl, res = ctx.srs_setup(k, srs.default_secret(), bases_form=bf, g=_prefilled(1 << k),
                                    g_lagrange=_prefilled(1 << k))
        assert _raw(dg) == point_bytes(g, bf), bf
        assert _raw(dl) == point_bytes(gl, bf), bf
        assert (res["k"], res["rows"], res["chunks"], res["chunk_rows"], res["secret_in_domain"]) == (8, 256, 1, 256, 0)
        assert res["window_bits"] == planned_window(512) and res["windows"] == -(-255 // res["window_bits"])
        assert [res[key] for key in ("g_zero_scalars", "g_identity_outputs", "lagrange_zero_scalars",
                                     "lagrange_identity_outputs")] == [0] * 4
    made = srs.gen_srs(ctx, 8)
    assert made["k"] == 8 and made["s"] == SECRET
    srs.write_srs(tmp_path / "kzg_bn254_8.srs", made)
    assert (tmp_path / "kzg_bn254_8.srs").read_bytes() == open(SRS8, "rb").read()


# ------------------------------------------------- 2. the sizes below the file's
@pytest.mark.parametrize("k", range(1, 8))
def test_small_sizes_with_the_default_secret(ctx, k):
    n = 1 << k
    dg, dl, res = ctx.srs_setup(k, SECRET, g=_prefilled(n), g_lagrange=_prefilled(n))
    assert _raw(dg) == point_bytes(golden()[1][:n], "montgomery")
    assert _raw(dl) == point_bytes(points_of(lagrange_scalars(k, SECRET)), "montgomery")
    assert res["window_bits"] == planned_window(2 * n) and res["chunks"] == 1


# ------------------------------------------------------------ 3. edge secrets
@pytest.mark.parametrize("k", (3, 5))
@pytest.mark.parametrize("name", sorted(edge_secrets(3)))
def test_edge_secrets(ctx, k, name):
    n, s = 1 << k, edge_secrets(k)[name]
    ps, ls = power_scalars(k, s), lagrange_scalars(k, s)
    want_g, want_l = points_of(ps), points_of(ls)
    bf = FORMS[(k + len(name)) % 2]
    dg, dl, res = ctx.srs_setup(k, s, bases_form=bf, g=_prefilled(n), g_lagrange=_prefilled(n))
    assert _raw(dg) == point_bytes(want_g, bf), _points(dg, bf)
    assert _raw(dl) == point_bytes(want_l, bf), _points(dl, bf)
    assert res["secret_in_domain"] == int(pow(s, n, R) == 1)
    assert (res["g_zero_scalars"], res["lagrange_zero_scalars"]) == (ps.count(0), ls.count(0))
    assert res["g_identity_outputs"] == want_g.count(IDENTITY)
    assert res["lagrange_identity_outputs"] == want_l.count(IDENTITY)
    if name == "zero":
        assert want_g.count(IDENTITY) == n - 1 and want_l == [mul(G, pow(n, -1, R))] * n
    if res["secret_in_domain"]:
        assert want_l.count(IDENTITY) == n - 1 and want_l.count(G) == 1
    chk = ctx.check_srs(dg, dl, k, s, RHO, bases_form=bf)
    assert chk == {"points_checked": 2 * n, "points_off_curve": 0, "g_failed": 0, "lagrange_failed": 0}


# ---------------------------------- 4. fixed_base_mul: bases, scalars, windows
@functools.lru_cache(maxsize=None)
def _window_bases():
    return (G, golden()[1][5], IDENTITY)


@pytest.mark.parametrize("c", range(2, kernel_constant("kCommitMaxBits") + 1))
def test_fixed_base_mul_every_window_size(ctx, c):
    vals = window_scalars(c) + _rand(3, 100 + c)
    assert set(digit_edge_scalars(c)) <= set(vals) and {0, 1, R - 1} <= set(vals)
    for b, base in enumerate(_window_bases()):
        form, bf = COMBOS[(c + b) % 4]
        out, res = ctx.fixed_base_mul(point_bytes([base], bf), _scalars(vals, form), form=form, base_form=bf,
                                      window_bits=c, out=_prefilled(len(vals)))
        want = [mul(base, v) for v in vals]
        assert _raw(out) == point_bytes(want, bf), (c, b, form, bf, _points(out, bf), want)
        assert res == {"window_bits": c, "windows": -(-255 // c), "points": len(vals), "zero_scalars": 1,
                       "identity_outputs": want.count(IDENTITY)}
        assert want.count(IDENTITY) == (len(vals) if base == IDENTITY else 1)


def test_fixed_base_mul_meets_its_table_entries(ctx):
    """The accumulator equal to the entry the top window adds (the add is a
    doubling: srs_cases.doubling_scalar), and its negative (a cancellation): the
    integer r itself, which a canonical cell can hold; the digits are those of
    the integer, so the answer is the identity, and [5] base for r + 5."""
    found = {c: doubling_scalar(c) for c in (3, 4, 12, kernel_constant("kCommitMaxBits"))}
    assert found[4] is not None and found[12] is not None, found
    for b, base in enumerate(_window_bases()[:2]):
        for c, v in found.items():
            if v is None:
                continue
            vals = [v, R - v, R, R + 5]
            bf = FORMS[(c + b) % 2]
            out, res = ctx.fixed_base_mul(point_bytes([base], bf), _scalars(vals, "canonical"), base_form=bf,
                                          window_bits=c, out=_prefilled(len(vals)))
            want = [mul(base, v), mul(base, R - v), IDENTITY, mul(base, 5)]
            assert _raw(out) == point_bytes(want, bf), (c, b, _points(out, bf), want)
            assert (res["zero_scalars"], res["identity_outputs"]) == (0, 1)


# --------------------------------------- 5. fixed_base_mul: lengths and buffers
@pytest.mark.parametrize("n", (1, 7, 257, 4099))
def test_fixed_base_mul_lengths_and_buffers(ctx, n):
    group, block = srs_constant("kFbGroup"), block_outputs()
    assert 1 < group and 7 % group and 257 % block and 4099 % block and 4099 > block   # ragged, more than one block
    vals = [(A0 + i * D) % R for i in range(n)]
    want = progression(n, A0, D)
    tail = 3
    for form in FORMS:
        out, res = ctx.fixed_base_mul(point_bytes([G], "montgomery"), _scalars(vals, form), form=form,
                                      out=_prefilled(n + tail))
        raw = _raw(out)
        assert raw[:64 * n] == point_bytes(want, "montgomery"), (n, form)
        assert raw[64 * n:] == bytes([SENTINEL]) * (64 * tail), (n, form)
        assert (res["points"], res["window_bits"], res["zero_scalars"], res["identity_outputs"]) == \
            (n, planned_window(n), 0, 0)
    empty, res = ctx.fixed_base_mul(point_bytes([G], "montgomery"), _scalars(vals, "canonical")[:0], out=_prefilled(tail))
    assert _raw(empty) == bytes([SENTINEL]) * (64 * tail) and res["points"] == 0


# -------------------------------------------- 6. larger sizes, through commits
@functools.lru_cache(maxsize=None)
def _large_oracle(k: int):
    """(s^i, l_i(s), two random columns) for the default secret."""
    return power_scalars(k, SECRET), lagrange_scalars(k, SECRET), [_rand(1 << k, 7 * k), _rand(1 << k, 7 * k + 1)]


@pytest.mark.parametrize("k,chunk_rows", [(11, 700), (11, 0), (14, 0), (12, 1365)])
def test_larger_sizes_commit_to_the_polynomials_value(ctx, k, chunk_rows):
    import torch
    n = 1 << k
    ps, ls, cols = _large_oracle(k)
    ctx.set_option("srs_chunk_rows", chunk_rows)
    try:
        dg, dl, res = ctx.srs_setup(k, SECRET, g=_prefilled(n), g_lagrange=_prefilled(n))
    finally:
        ctx.set_option("srs_chunk_rows", 0)
    rows = chunk_rows or n
    assert (res["chunk_rows"], res["chunks"], res["window_bits"]) == (rows, -(-n // rows), planned_window(2 * n))
    if chunk_rows:
        assert res["chunks"] >= 3 and n % rows                       # a ragged last chunk
    dc = torch.stack([_scalars(col, "canonical") for col in cols])
    cg, _ = ctx.commit_coeffs(dc, dg, k)
    cl, _ = ctx.commit_lagrange(dc, dl, k)
    assert _points(cg) == [mul(G, sum(a * b for a, b in zip(col, ps)) % R) for col in cols]
    assert _points(cl) == [mul(G, sum(a * b for a, b in zip(col, ls)) % R) for col in cols]
    idx = boundary_indices(n, rows, 64)
    assert len(idx) == 64 and {0, n - 1} <= set(idx)
    it = torch.tensor(idx, device="cuda")
    assert _points(dg[it]) == [mul(G, ps[i]) for i in idx]
    half = idx[::2]                                                # every other one of them in the Lagrange array
    assert _points(dl[torch.tensor(half, device="cuda")]) == [mul(G, ls[i]) for i in half]
    chk = ctx.check_srs(dg, dl, k, SECRET, RHO)
    assert chk == {"points_checked": 2 * n, "points_off_curve": 0, "g_failed": 0, "lagrange_failed": 0}


# ------------------------------------------------------- 7. either output alone
def test_either_output_may_be_left_out(ctx):
    k, n = 4, 16
    both_g, both_l, _ = ctx.srs_setup(k, SECRET)
    g_only, none_l, res_g = ctx.srs_setup(k, SECRET, g=_prefilled(n), g_lagrange=None)
    none_g, l_only, res_l = ctx.srs_setup(k, SECRET, g=None, g_lagrange=_prefilled(n))
    assert none_l is None and none_g is None
    assert _raw(g_only) == _raw(both_g) == point_bytes(golden()[1][:n], "montgomery")
    assert _raw(l_only) == _raw(both_l) == point_bytes(points_of(lagrange_scalars(k, SECRET)), "montgomery")
    assert res_g["window_bits"] == res_l["window_bits"] == planned_window(n)
    nothing = ctx.srs_setup(k, SECRET, g=None, g_lagrange=None)
    assert nothing[:2] == (None, None) and nothing[2]["rows"] == n


# ------------------------------------------------------------------ 8. the check
@pytest.mark.parametrize("bf", FORMS)
def test_check_srs_passes_and_finds_tampering(ctx, bf):
    k, n = 8, 256
    dg, dl, _ = ctx.srs_setup(k, SECRET, bases_form=bf)
    ok = {"points_checked": 2 * n, "points_off_curve": 0, "g_failed": 0, "lagrange_failed": 0}
    before = (_raw(dg), _raw(dl))
    assert ctx.check_srs(dg, dl, k, SECRET, RHO, bases_form=bf) == ok
    assert (_raw(dg), _raw(dl)) == before                  # it writes to no input
    assert ctx.check_srs(dg, dl, k, SECRET, 0, bases_form=bf) == ok      # rho = 0 sees row 0 alone
    # the inverse of s: rho s = 1, the geometric sum is n
    assert ctx.check_srs(dg, dl, k, SECRET, pow(SECRET, -1, R), bases_form=bf) == ok
    bad = dg.clone()
    bad[5] = dg[6]
    assert ctx.check_srs(bad, dl, k, SECRET, RHO, bases_form=bf) == {**ok, "g_failed": 1}
    swapped = dl.clone()
    swapped[17], swapped[200] = dl[200], dl[17]
    assert ctx.check_srs(dg, swapped, k, SECRET, RHO, bases_form=bf) == {**ok, "lagrange_failed": 1}
    assert ctx.check_srs(dg, dl, k, SECRET + 1, RHO, bases_form=bf) == {**ok, "g_failed": 1, "lagrange_failed": 1}
    import torch
    off = dl.clone()
    off[3] = torch.from_numpy(np.frombuffer(point_bytes([(1, 3)], bf), dtype=np.uint8).copy()).cuda()
    res = ctx.check_srs(dg, off, k, SECRET, RHO, bases_form=bf)
    assert (res["points_checked"], res["points_off_curve"], res["g_failed"], res["lagrange_failed"]) == (2 * n, 1, 0, 1)
