"""svdw_commit / svdw_check_commit on the device against the integer oracle
(commit_cases.py): the reference's SRS at every size up to 2^8, Lagrange against
coefficient commitments through the device's own transform, skewed and
degenerate scalars, degenerate bases (every addition a doubling or a
cancellation), the sizes at which the plan changes its window, the checker
against tampering, the pieces of h, the columns and Z of an SVD witness end to
end, the edge arguments, and the regimes that depend on the size (commit_cases.
GPU_CASES: every window size through the option "commit_window_bits" with the
digit edges placed, slot trees up to k = 20's, a batch at the grid's limit, a
task larger than the workspace cap, the checker where its blocks are capped and
its columns chunked). Sizes beyond the SRS use progression bases, whose MSM is
one scalar multiplication, tiled beyond 2^14. Outputs are prefilled with a
sentinel byte; both cell forms and both base forms unless noted; comparisons
byte for byte after conversion."""
import ctypes as ct
import functools

import numpy as np
import pytest

from commit_cases import (G, IDENTITY, Q, R, commit_regimes, digit_edge_scalars, gpu_cases, kernel_constant, msm, mul,
                          neg, parse_srs, point_bytes, points_from_bytes, progression, progression_msm, signed_digits,
                          task_cap, tiled_msm)
from conftest import gamma_for, gen_svd_input
from lookup_perm_cases import cell_values
from ntt_cases import inv, ntt_inverse
from quotient_cases import FAMILIES, honest_instance, quotient_ext, to_coeffs, to_extended

pytestmark = pytest.mark.gpu

SENTINEL = 0xAB
FORMS = ("canonical", "montgomery")
COMBOS = [(f, b) for f in FORMS for b in FORMS]            # (cells' form, bases' form)
A0, D = 0x1234567, (1 << 251) + 0x89abcdef                 # the progression P_i = [A0 + i D] G


@pytest.fixture(scope="module")
def ctx(gpu_ctx_factory):
    return gpu_ctx_factory(32, 8)


@functools.lru_cache(maxsize=None)
def _srs():
    return parse_srs()


@functools.lru_cache(maxsize=None)
def _progression():
    """2^14 progression bases; a size-2^k case takes the first 2^k."""
    return progression(1 << 14, A0, D)


def _closed(scalars):
    return progression_msm(len(scalars), A0, D, scalars)


def _rand(n: int, seed: int) -> list:
    rs = np.random.RandomState(seed)
    return [int.from_bytes(rs.bytes(32), "little") % R for _ in range(n)]


def _cells(vals) -> np.ndarray:
    """[len(vals), 32] u8 canonical cells."""
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint8).reshape(-1, 32).copy()


def _device(cols, form: str, cells=None):
    """Value lists (or their canonical cells [n, rows, 32] u8, where the caller
    has them) -> [n, rows, 32] u8 device tensor in `form`."""
    import torch
    import halo2_svd041_amd as hs
    a = np.ascontiguousarray(np.stack([_cells(c) for c in cols])) if cells is None else cells
    if form == "montgomery":
        a = hs.fr_convert(a.view("<u8").reshape(-1, 4), "canonical", "montgomery").view(np.uint8).reshape(a.shape)
    return torch.from_numpy(a).cuda()


def _bases(points, bases_form: str):
    import torch
    return torch.from_numpy(np.frombuffer(point_bytes(points, bases_form), dtype=np.uint8).reshape(-1, 64).copy()).cuda()


def _points(t, bases_form: str) -> list:
    return points_from_bytes(t.cpu().numpy().tobytes(), bases_form)


def _prefilled(n: int):
    import torch
    return torch.full((n, 64), SENTINEL, dtype=torch.uint8, device="cuda")


def _commit_all(ctx, cols, bases, k: int, want: list, counts=None, split: bool = False, plan=None, combos=COMBOS,
                cells=None, repeat: int = 1, outs=None):
    """Every combination of forms: the device's points are `want`, byte for byte.
    plan: the (c, W) the call must report where an option overrides
    svdw_commit_plan's. repeat: the bases are `bases` that many times over.
    outs: collects (form, bases' form, cells, bases, points) on the device."""
    import halo2_svd041_amd as hs
    c, w = plan or hs.commit_plan(k)
    for form, bf in combos:
        dc, db = _device(cols, form, cells), _bases(bases, bf).repeat(repeat, 1)
        arg = [dc[:1].contiguous(), dc[1:].contiguous()] if split and len(cols) > 1 else dc
        out, res = ctx.commit(arg, db, k, form=form, bases_form=bf, out=_prefilled(len(cols)))
        assert out.cpu().numpy().tobytes() == point_bytes(want, bf), (k, form, bf, _points(out, bf), want)
        assert (res["columns"], res["rows"], res["window_bits"], res["windows"]) == (len(cols), 1 << k, c, w)
        assert res["zero_scalars"] == sum(v == 0 for col in cols for v in col)
        assert res["identity_outputs"] == sum(p == IDENTITY for p in want)
        assert res["identity_bases"] == repeat * sum(p == IDENTITY for p in bases)
        if counts is not None:
            counts.append(res)
        if outs is not None:
            outs.append((form, bf, dc, db, out))


# ------------------------------------------------------ 1. small sizes on the SRS
@functools.lru_cache(maxsize=None)
def _small_case(k: int):
    n = 1 << k
    g = _srs()[1][:n]
    small = [(0, 1, R - 1, 2, 255, 256, 65535)[i % 7] for i in range(n)]
    cols = [_rand(n, k), small, [0] * (n - 1) + [_rand(1, 50 + k)[0]]]
    return g, cols, [msm(g, c) for c in cols]


@pytest.mark.parametrize("k", range(1, 9))
def test_small_sizes_on_the_srs(ctx, k):
    g, cols, want = _small_case(k)
    assert want[2] == mul(g[-1], cols[2][-1])
    _commit_all(ctx, cols, g, k, want, split=(k % 2 == 0))


# ------------------------------------------ 2. Lagrange against coefficients, k = 8
def test_lagrange_against_coefficients(ctx):
    k, g, gl = _srs()
    cols = [_rand(1 << k, 81), [0] * 255 + [R - 2]]
    want = [msm(gl, c) for c in cols]
    assert want[1] == msm(g, ntt_inverse(cols[1], k))      # the oracle's own agreement (in full: the CPU suite)
    for form, bf in COMBOS:
        dc = _device(cols, form)
        coeffs, _ = ctx.lagrange_to_coeff(dc, k, form)
        lag, _ = ctx.commit(dc, _bases(gl, bf), k, form=form, bases_form=bf, out=_prefilled(2))
        co, _ = ctx.commit(coeffs, _bases(g, bf), k, form=form, bases_form=bf, out=_prefilled(2))
        assert lag.cpu().numpy().tobytes() == co.cpu().numpy().tobytes() == point_bytes(want, bf), (form, bf)
        if bf == "montgomery":                             # the thin names take an SRS as read_srs gives it
            assert ctx.commit_lagrange(dc, _bases(gl, bf), k, form=form)[0].cpu().numpy().tobytes() == \
                ctx.commit_coeffs(coeffs, _bases(g, bf), k, form=form)[0].cpu().numpy().tobytes() == \
                point_bytes(want, bf)


# ------------------------------------------------ 3. skew and degenerate scalars
def _skewed(n: int, seed: int):
    wide = _rand(1, seed)[0] % (1 << 252) | (1 << 252)     # 253 bits, below r
    rs = np.random.RandomState(seed)
    return {"zeros": [0] * n, "ones": [1] * n, "bits": [int(b) for b in rs.randint(0, 2, n)],
            "wide": [wide] * n, "minus_one": [R - 1] * n, "bytes": [int(b) for b in rs.randint(0, 256, n)]}


def test_skewed_scalars_on_the_srs(ctx):
    k, g, gl = _srs()
    cols = _skewed(1 << k, 3)
    want = {"zeros": IDENTITY, "ones": g[0], "bits": msm(gl, cols["bits"]), "wide": mul(g[0], cols["wide"][0]),
            "minus_one": neg(g[0]), "bytes": msm(gl, cols["bytes"])}   # sum g_lagrange = g[0] (CPU suite)
    counts = []
    _commit_all(ctx, list(cols.values()), gl, k, [want[name] for name in cols], counts)
    assert all(r["identity_outputs"] == 1 and r["zero_scalars"] >= 1 << k for r in counts)


def test_skewed_scalars_on_progression_bases(ctx):
    k = 13
    n = 1 << k
    bases = _progression()[:n]
    cols = _skewed(n, 13)
    want = [_closed(c) for c in cols.values()]
    assert want[0] == IDENTITY and IDENTITY not in want[1:]
    # one bucket holds every entry of a window: its run spans many threads' runs and more than one block
    assert n > kernel_constant("kCommitRun") * kernel_constant("kCommitThreads")
    counts = []
    _commit_all(ctx, list(cols.values()), bases, k, want, counts)
    assert all(r["identity_outputs"] == 1 for r in counts)


def test_batches_under_a_small_workspace_cap(ctx):
    """With the cap at 1 MiB a batch holds a few (column, window) tasks, so the
    call runs tens of batches and columns are split between them; the points and
    the counters are those of one batch."""
    import halo2_svd041_amd as hs
    k = 12
    n = 1 << k
    c, w = hs.commit_plan(k)
    task_bytes = 21 * n + 140 * (1 << (c - 1))             # include/svdw.h, "commitments"
    cols = dict(_skewed(n, 12), random=_rand(n, 120), spike=[0] * (n - 1) + [R - 1])
    assert (1 << 20) // task_bytes < w and (len(cols) * w * task_bytes) >> 20 >= 20
    want = [_closed(col) for col in cols.values()]
    ctx.set_option("commit_scratch_mib", 1)
    try:
        _commit_all(ctx, list(cols.values()), _progression()[:n], k, want)
    finally:
        ctx.set_option("commit_scratch_mib", 1024)


# ------------------------------------------------------------ 4. degenerate bases
def test_equal_bases_every_addition_a_doubling(ctx):
    k = 6
    s = _rand(64, 6)
    cols = [s, [5] * 64, [1] * 64]
    _commit_all(ctx, cols, [G] * 64, k, [mul(G, sum(c) % R) for c in cols])


def test_opposite_bases_cancel(ctx):
    k = 6
    p = mul(G, 0xdecaf)
    s = _rand(32, 7)
    paired = [v for v in s for _ in (0, 1)]                # equal scalars on P and -P
    _commit_all(ctx, [paired, [9] * 64, [R - 1] * 64], [p, neg(p)] * 32, k, [IDENTITY] * 3)


def test_identity_bases_are_skipped_and_counted(ctx):
    k = 6
    g = list(_srs()[1][:64])
    for i in (0, 7, 8, 63):
        g[i] = IDENTITY
    cols = [_rand(64, 8), [1] * 64]
    counts = []
    _commit_all(ctx, cols, g, k, [msm(g, c) for c in cols], counts)
    assert all(r["identity_bases"] == 4 for r in counts)
    _commit_all(ctx, cols, [IDENTITY] * 64, k, [IDENTITY] * 2)


def test_two_rows(ctx):
    p = mul(G, 77)
    for bases, cols in (([G, p], [[3, 4], [0, R - 1], [0, 0]]), ([p, p], [[R - 5, 5], [1, 1]]),
                        ([p, neg(p)], [[6, 6], [6, 7]])):
        _commit_all(ctx, cols, bases, 1, [msm(bases, c) for c in cols])


# ------------------------------------------------------------------ 5. plan edges
def _plan_ks():
    import halo2_svd041_amd as hs
    bits = {k: hs.commit_plan(k)[0] for k in range(10, 15)}
    return bits, sorted({min(k for k in bits if bits[k] == c) for c in set(bits.values())} | {14})


def test_plan_edges(ctx):
    """Full-width scalars at the smallest k of every window size the plan uses
    in 10..14 and at 14, against the closed form."""
    import halo2_svd041_amd as hs
    bits, ks = _plan_ks()
    assert len({bits[k] for k in ks}) >= 2, bits
    run, threads = kernel_constant("kCommitRun"), kernel_constant("kCommitThreads")
    spans = False
    for k in ks:
        n = 1 << k
        col = _rand(n, 100 + k)
        c, w = hs.commit_plan(k)
        # window 0's sorted list: where its buckets begin, and whether one crosses a run's end beyond the first block
        hist = np.bincount([abs(signed_digits(s, c, w)[0]) for s in col], minlength=(1 << (c - 1)) + 1)[1:]
        start = np.concatenate([[0], np.cumsum(hist)])
        crossing = [(a, b) for a, b in zip(start[:-1], start[1:]) if b > a and a // run != (b - 1) // run]
        spans = spans or (start[-1] > run * threads and any(a >= run * threads for a, _ in crossing))
        _commit_all(ctx, [col], _progression()[:n], k, [_closed(col)])
    assert spans, "no size left at which a bucket spans two runs beyond the first block"


# -------------------------------------------------------------------- 6. the checker
def test_checker(ctx):
    import torch
    k, g, gl = _srs()
    n = 1 << k
    _, cols, want = _small_case(k)
    clean = {"columns_checked": 3, "commit_failures": 0, "bases_checked": n, "bases_off_curve": 0}
    for form, bf in COMBOS:
        dc, db = _device(cols, form), _bases(g, bf)
        keep = (dc.clone(), db.clone())
        out, _ = ctx.commit(dc, db, k, form=form, bases_form=bf)
        assert ctx.check_commit(dc, db, out, k, form=form, bases_form=bf) == clean, (form, bf)
        up = torch.from_numpy(np.frombuffer(point_bytes(want, bf), dtype=np.uint8).reshape(3, 64).copy()).cuda()
        assert ctx.check_commit(dc, db, up, k, form=form, bases_form=bf) == clean, (form, bf)
        # one flipped byte in one commitment: exactly that column fails
        for col, byte in ((1, 0), (2, 40), (0, 63)):
            bad = out.clone()
            bad[col, byte] ^= 0x10
            assert ctx.check_commit(dc, db, bad, k, form=form, bases_form=bf) == dict(clean, commit_failures=1)
            for j in range(3):
                got = ctx.check_commit(dc[j:j + 1], db, bad[j:j + 1].contiguous(), k, form=form, bases_form=bf)
                assert got == dict(clean, columns_checked=1, commit_failures=int(j == col)), (form, bf, col, j)
        # a commitment replaced by its negation
        bad = up.clone()
        bad[1] = _bases([neg(want[1])], bf)[0]
        assert ctx.check_commit(dc, db, bad, k, form=form, bases_form=bf) == dict(clean, commit_failures=1)
        # one changed scalar cell
        cells = dc.clone()
        cells[2, 5] = _device([[12345]], form)[0, 0]
        assert ctx.check_commit(cells, db, out, k, form=form, bases_form=bf) == dict(clean, commit_failures=1)
        # one base moved off the curve: counted, and every column whose cell there is not zero fails
        off = list(g)
        off[9] = (g[9][0], (g[9][1] + 1) % Q)
        got = ctx.check_commit(dc, _bases(off, bf), out, k, form=form, bases_form=bf)
        assert got == dict(clean, bases_off_curve=1, commit_failures=sum(c[9] != 0 for c in cols)), (form, bf)
        # the identity among the bases is not off the curve
        off[9] = IDENTITY
        assert ctx.check_commit(dc, _bases(off, bf), out, k, form=form, bases_form=bf)["bases_off_curve"] == 0
        assert torch.equal(dc, keep[0]) and torch.equal(db, keep[1])


# ------------------------------------------------------------------ 7. pieces of h
def test_pieces_of_h(ctx):
    inst = honest_instance(4, 6, 3, 2)
    co = to_coeffs(inst)
    k, ek = inst["k"], inst["extended_k"]
    h = ntt_inverse(quotient_ext(to_extended(co)), ek, inv(inst["shift"]))
    g = _srs()[1][:1 << k]
    pieces = [h[i << k:(i + 1) << k] for i in range(1 << (ek - k))]
    want = [msm(g, p) for p in pieces]
    assert len(pieces) == 4 and any(pieces[2]) and want[0] != IDENTITY
    par = dict(k=k, extended_k=ek, shift=inst["shift"], beta=inst["beta"], gamma=inst["gamma"], y=inst["y"],
               chunk_len=inst["chunk_len"], unusable_rows=inst["unusable"])
    for form, bf in COMBOS:
        fams = {f: _device(co[f], form) for f in FAMILIES if co[f]}
        ext = {f: ctx.coeff_to_extended(t, k, ek, inst["shift"], form=form)[0] for f, t in fams.items()}
        h_ext, _ = ctx.quotient(form=form, **par, **ext)
        hc, _ = ctx.extended_to_coeff(h_ext, ek, inv(inst["shift"]), form=form)
        out, res = ctx.commit(hc.view(4, 1 << k, 32), _bases(g, bf), k, form=form, bases_form=bf, out=_prefilled(4))
        assert res["columns"] == 4
        assert out.cpu().numpy().tobytes() == point_bytes(want, bf), (form, bf)


# ------------------------------------------------------- 8. a witness end to end
def test_witness_columns_and_z(ctx):
    """The advice columns of a 4 x 4 SVD witness at K = 10 and the Z of their
    permutation argument, committed on progression bases."""
    import halo2_svd041_amd as hs
    K, MIN_ROWS, UNUSABLE = 10, 20, 6
    rows = 1 << K
    m, u, d, v = gen_svd_input(4, 4, seed=44)
    hs.svd_witness(ctx, m, u, v, d, gamma_for(K))
    assert sum(ctx.physical_layout(K, MIN_ROWS)["columns_used"]) >= 1
    bases = _progression()[:rows]
    want = None
    for form, bf in COMBOS:
        adv = [ctx.assign_columns(ph, form=form)[0] for ph in (0, 1)]
        adv = [t for t in adv if t.shape[0]]
        ncols = sum(t.shape[0] for t in adv)
        sigma, bad = ctx.permutation_values(K, ncols=ncols, form=form)
        z, res = ctx.permutation_product(adv, sigma, gamma_for(1), gamma_for(2), 2, K, UNUSABLE, form)
        assert bad == 0 and res["final_not_one"] == 0
        cols = adv + [z]
        total = ncols + z.shape[0]
        if want is None:
            lag = np.concatenate([t.cpu().numpy() for t in cols])
            assert form == "canonical" and lag[:ncols].any() and lag[ncols:].any()
            want = [_closed(cell_values(c)) for c in lag]
        db = _bases(bases, bf)
        out, res = ctx.commit(cols, db, K, form=form, bases_form=bf, out=_prefilled(total))
        assert res["columns"] == total and res["rows"] == rows
        assert out.cpu().numpy().tobytes() == point_bytes(want, bf), (form, bf)
        assert ctx.check_commit(cols, db, out, K, form=form, bases_form=bf) == \
            {"columns_checked": total, "commit_failures": 0, "bases_checked": rows, "bases_off_curve": 0}


# ------------------------------------------------------------ 9. edge arguments
def test_no_columns_overlap_and_out_in_place(ctx):
    import torch
    import halo2_svd041_amd as hs
    from halo2_svd041_amd._lib import CommitCheck, CommitResult
    L = hs.zk.lib()
    k = 6
    n = 1 << k
    g = _srs()[1][:n]
    db = _bases(g, "montgomery")
    out = _prefilled(2)
    r, c = CommitResult(), CommitCheck()
    ptrs = (ct.c_void_p * 1)(out.data_ptr())
    assert L.svdw_commit(ctx._h, k, 0, 1, db.data_ptr(), ptrs, 0, out.data_ptr(), ct.byref(r)) == 0
    assert (r.columns, r.rows, r.window_bits, r.windows) == (0, n, *hs.commit_plan(k))
    assert L.svdw_check_commit(ctx._h, k, 0, 1, db.data_ptr(), ptrs, 0, out.data_ptr(), ct.byref(c)) == 0
    assert (c.columns_checked, c.bases_checked) == (0, 0)
    empty = torch.empty((0, n, 32), dtype=torch.uint8, device="cuda")
    pts, res = ctx.commit(empty, db, k)
    assert tuple(pts.shape) == (0, 64) and res["columns"] == 0
    assert bool((out == SENTINEL).all())
    # out inside a column, and inside the bases
    buf = torch.zeros((n * 32 + 128,), dtype=torch.uint8, device="cuda")
    col = buf[:n * 32].view(1, n, 32)
    for dst in (buf[64:128].view(1, 64), buf[n * 32 - 32:n * 32 + 32].view(1, 64)):
        with pytest.raises(hs.SvdwError) as e:
            ctx.commit(col, db, k, out=dst)
        assert e.value.code == -1 and "overlaps" in str(e.value)
    ok, _ = ctx.commit(col, db, k, out=buf[n * 32:n * 32 + 64].view(1, 64))   # adjacent is fine
    assert ok.cpu().numpy().tobytes() == point_bytes([IDENTITY], "montgomery")
    cols = _device([_rand(n, 9)], "canonical")
    with pytest.raises(hs.SvdwError) as e:
        ctx.commit(cols, db, k, out=db[5:6])
    assert e.value.code == -1 and "overlaps" in str(e.value)
    assert bool((buf == 0).all()) and db.cpu().numpy().tobytes() == point_bytes(g, "montgomery")
    # an out tensor of the caller's is filled in place
    dst = _prefilled(1)
    got, _ = ctx.commit(cols, db, k, out=dst)
    assert got is dst and dst.cpu().numpy().tobytes() == point_bytes([msm(g, _rand(n, 9))], "montgomery")
    with pytest.raises(hs.SvdwError):
        ctx.commit(cols, db, k, out=_prefilled(2))


# ------------------------------------- 10. the regimes that depend on the size
# The cases and their parameters are commit_cases.GPU_CASES; test_commit_cpu.py
# asserts what they cover. Each is placed by commit_regimes, which restates the
# constants of commit.hpp, and expects what the integer oracle gives.
TILE = 1 << 14                                             # beyond 2^14 rows the bases are _progression() over and over


def _tiled(scalars):
    return tiled_msm(TILE, A0, D, scalars)


def _rand_many(n: int, seed: int) -> list:
    """_rand for many values: one draw of bytes."""
    raw = np.random.RandomState(seed).bytes(32 * n)
    return [int.from_bytes(raw[i:i + 32], "little") % R for i in range(0, 32 * n, 32)]


def _small_cells(vals) -> np.ndarray:
    """_cells for values below 2^63."""
    a = np.zeros((len(vals), 4), dtype="<u8")
    a[:, 0] = vals
    return a.view(np.uint8).reshape(-1, 32)


def _reported_plan(ctx, k: int):
    """The (c, W) a call without columns reports."""
    import torch
    n = 1 << k
    _, res = ctx.commit(torch.empty((0, n, 32), dtype=torch.uint8, device="cuda"),
                        torch.zeros((n, 64), dtype=torch.uint8, device="cuda"), k)
    return res["window_bits"], res["windows"]


def _edge_column(c: int, n: int) -> list:
    """digit_edge_scalars(c) among zeros: each value alone, and on two adjacent
    rows (two entries of one bucket side by side in every window)."""
    col = [0] * n
    for i, v in enumerate(digit_edge_scalars(c)):
        col[7 * i + 3] = col[7 * i + 5] = col[7 * i + 6] = v
    return col


@functools.lru_cache(maxsize=None)
def _window_shared(k: int, srs: bool):
    """The bases, and the two columns every window size shares with their sums."""
    n = 1 << k
    bases = _srs()[1][:n] if srs else _progression()[:n]
    cols = [_rand(n, 300 + k), [1] * n]
    return bases, cols, [msm(bases, c) if srs else _closed(c) for c in cols]


def _window_case(ctx, k: int, c: int, ncols: int, srs: bool):
    import halo2_svd041_amd as hs
    bases, (wide, ones), (want_wide, want_ones) = _window_shared(k, srs)
    edge = _edge_column(c, 1 << k)
    assert sum(v != 0 for v in edge) == 3 * len(digit_edge_scalars(c)) and ncols == 3
    want = [want_wide, msm(bases, edge) if srs else _closed(edge), want_ones]
    assert IDENTITY not in want
    ctx.set_option("commit_window_bits", c)
    try:
        assert _reported_plan(ctx, k) == (c, -(-255 // c))
        _commit_all(ctx, [wide, edge, ones], bases, k, want, plan=(c, -(-255 // c)))
    finally:
        ctx.set_option("commit_window_bits", 0)
    assert _reported_plan(ctx, k) == hs.commit_plan(k)      # option 0: the plan's figures again


@pytest.mark.parametrize("k,c,ncols,mib", gpu_cases("window"))
def test_every_window_size(ctx, k, c, ncols, mib):
    """A full-width column, the digit edges of this c and an all-ones column
    under the option "commit_window_bits", against the closed form."""
    _window_case(ctx, k, c, ncols, srs=False)


@pytest.mark.parametrize("k,c,ncols,mib", gpu_cases("window_srs"))
def test_window_sizes_on_the_srs(ctx, k, c, ncols, mib):
    """The same on bases that are no progression, against the naive sum."""
    _window_case(ctx, k, c, ncols, srs=True)


@pytest.mark.parametrize("k,c,ncols,mib", gpu_cases("few_rows"))
def test_few_rows_against_the_most_buckets(ctx, k, c, ncols, mib):
    """2 or 4 rows and 2^15 buckets: nearly every bucket, chunk and slot is the identity."""
    import halo2_svd041_amd as hs
    n, half = 1 << k, 1 << (c - 1)
    reg = commit_regimes(k, c)
    assert reg["B"] == half >= 1024 * n and reg["levels"] == 0 and reg["chunks"] > kernel_constant("kCommitTreeThreads")
    cols = [_rand(n, 400 + k), [half, half + 1, 2 * half - 1, R - 1][:n], [0] * (n - 1) + [1]]
    assert len(cols) == ncols
    ctx.set_option("commit_window_bits", c)
    try:
        _commit_all(ctx, cols, _progression()[:n], k, [_closed(col) for col in cols], plan=(c, reg["W"]))
    finally:
        ctx.set_option("commit_window_bits", 0)
    assert _reported_plan(ctx, k) == hs.commit_plan(k)


def _staircase(n: int) -> list:
    """Cells 1, 2, 3, ... in runs of these lengths, round after round over a
    quarter of the rows, the rest one long run and a short one: window 0's
    sorted list is one spanning bucket after another, which begin and end on
    both sides of the multiples of 16, 256 and 4096 (a round is 1 mod 16), and
    the long one spans most of the list and ends short of it."""
    lengths = (1, 15, 16, 17, 255, 256, 257, 4095, 4097)
    out, v = [], 1
    for _ in range(max(1, n // (4 * sum(lengths)))):
        for m in lengths:
            out += [v] * m
            v += 1
    return out + [v] * (n - len(out) - 37) + [v + 1] * 37


@pytest.mark.parametrize("k,c,ncols,mib", gpu_cases("deep"))
def test_deep_slot_trees(ctx, k, c, ncols, mib):
    """The plan's own window at sizes whose slot trees have three and four
    levels, on tiled bases: a full-width column, an all-ones column (one bucket
    over every run: slots_sum climbs to the top level) and the staircase; then
    the checker on the same points."""
    n = 1 << k
    reg = commit_regimes(k)
    assert c is None and mib is None and n % TILE == 0
    assert {16: reg["levels"] == 3, 18: (reg["c"], reg["chunks"]) == (15, 512),
            20: (reg["c"], reg["levels"]) == (16, 4)}[k], reg
    stairs = _staircase(n)
    assert max(stairs) < reg["B"]                           # window 0 only
    # its buckets hold whole nodes of every level below the top one (which has two nodes: the all-ones column's),
    # with partial nodes on both sides
    ends = np.cumsum(np.bincount(stairs)[1:]).tolist()
    spans = list(zip([0] + ends[:-1], ends))
    node = kernel_constant("kCommitRun") * kernel_constant("kCommitFan") // 2      # entries under a node of level 1
    for level in range(1, reg["levels"]):
        assert any(s % node and e % node and e // node > -(-s // node) for s, e in spans), (k, level)
        node *= kernel_constant("kCommitFan")
    cols = [_rand_many(n, 200 + k), [1] * n, stairs]
    cells = np.stack([_cells(cols[0]), _small_cells(cols[1]), _small_cells(cols[2])])
    want = [_tiled(col) for col in cols]
    assert len(cols) == ncols and IDENTITY not in want
    outs = []
    _commit_all(ctx, cols, _progression(), k, want, combos=COMBOS if k == 16 else COMBOS[1:2], cells=cells,
                repeat=n // TILE, outs=outs)
    form, bf, dc, db, out = outs[-1]
    assert ctx.check_commit(dc, db, out, k, form=form, bases_form=bf) == \
        {"columns_checked": ncols, "commit_failures": 0, "bases_checked": n, "bases_off_curve": 0}


def test_a_batch_at_the_task_cap(ctx):
    """More tasks than a grid has rows: the first batch holds 65535 of them and
    ends inside a column, whose other windows the second batch sums."""
    (k, c, ncols, mib), = gpu_cases("task_cap")
    reg = commit_regimes(k, c, ncols, mib)
    split, inside = divmod(reg["T"], reg["W"])
    assert reg["T"] == task_cap() == 65535 < reg["tasks"] <= 2 * reg["T"] and (split, inside) == (511, 127)
    bases = [G, mul(G, 77)]
    fixed = {1: [0, R - 1], 2: [1, 1]}                      # the split column is a random one
    cols = [fixed.get((j - split) % 3) or _rand(2, 500 + j) for j in range(ncols)]
    sums = {j: msm(bases, col) for j, col in fixed.items()}
    want = [sums.get((j - split) % 3) or msm(bases, col) for j, col in enumerate(cols)]
    assert cols[split] not in fixed.values() and IDENTITY not in want
    counts = []
    _commit_all(ctx, cols, bases, k, want, counts)
    assert all(r["zero_scalars"] == ncols // 3 and r["columns"] == ncols for r in counts)


def test_one_task_larger_than_the_cap(ctx):
    """A cap below one task's workspace: the task runs all the same, one per batch."""
    from commit_cases import default_scratch_mib
    (k, c, ncols, mib), = gpu_cases("one_task")
    reg = commit_regimes(k, c, ncols, mib)
    assert reg["task_bytes"] > mib << 20 and reg["cap_over_per"] == 0 and reg["T"] == 1 < reg["tasks"]
    n = 1 << k
    cols = [_rand_many(n, 600 + j) for j in range(ncols)]
    ctx.set_option("commit_scratch_mib", mib)
    try:
        _commit_all(ctx, cols, _progression(), k, [_tiled(col) for col in cols], combos=(COMBOS[1], COMBOS[2]),
                    repeat=n // TILE)
    finally:
        ctx.set_option("commit_scratch_mib", default_scratch_mib())


@pytest.mark.parametrize("k,c,ncols,mib", gpu_cases("checker"))
def test_checker_at_size(ctx, k, c, ncols, mib):
    """The checker where its row blocks are capped (every thread strides over
    the rows, twice from k = 14) and where the columns are checked in chunks:
    clean on the commitments, and a flipped byte fails exactly its column, in
    the first chunk, at its end and in the second."""
    n = 1 << k
    reg = commit_regimes(k, c, ncols, mib)
    blocks, tree = kernel_constant("kCommitCheckBlocks"), kernel_constant("kCommitTreeThreads")
    chunk = reg["check_columns"]
    assert reg["check_blocks"] == blocks and (ncols > chunk or reg["check_trips"] >= 2)
    form, bf = COMBOS[1] if ncols > chunk else COMBOS[2]
    cols = [_rand_many(n, 700 + 40 * k + j) for j in range(ncols)]
    outs = []
    _commit_all(ctx, cols, _progression()[:n], k, [_closed(col) for col in cols], combos=[(form, bf)], outs=outs)
    _, _, dc, db, out = outs[0]
    clean = {"columns_checked": ncols, "commit_failures": 0, "bases_checked": n, "bases_off_curve": 0}
    assert ctx.check_commit(dc, db, out, k, form=form, bases_form=bf) == clean
    tampered = sorted({0, chunk - 1, chunk} & set(range(ncols)))
    assert tampered == ([0, chunk - 1, chunk] if ncols > chunk else [0, ncols - 1])
    for col in tampered:
        bad = out.clone()
        bad[col, (17 * col + 3) % 64] ^= 0x04
        assert ctx.check_commit(dc, db, bad, k, form=form, bases_form=bf) == dict(clean, commit_failures=1), col
        for j in range(ncols):
            got = ctx.check_commit(dc[j:j + 1], db, bad[j:j + 1].contiguous(), k, form=form, bases_form=bf)
            assert got == dict(clean, columns_checked=1, commit_failures=int(j == col)), (col, j)
    if reg["check_trips"] >= 2:                             # a cell only the second trip of the stride loop reads
        for row in (blocks * tree, n - 1):
            cells = dc.clone()
            cells[ncols - 1, row] = _device([[12345]], form)[0, 0]
            assert ctx.check_commit(cells, db, out, k, form=form, bases_form=bf) == dict(clean, commit_failures=1), row
