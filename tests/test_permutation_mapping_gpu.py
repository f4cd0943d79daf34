"""svdw_permutation_cycles / svdw_check_permutation_mapping on the device
against the host restatement of the rule (cycle_cases.py; parity of the rule
itself unpinned): the mapping byte for byte, with the output filled with a
sentinel before every call, for no edges, one chain through every usable cell,
a hub, thousands of small classes whose ids need three digits, any order and
repetition of the edges, edges out of range; the checker on honest and
tampered mappings; and one run of 2^22 cells against a torch sort."""
import numpy as np
import pytest

from cycle_cases import (K, UNUSABLE, canonical_mapping, cell, chain_case, cycles_of, hub_case, out_of_range_edges,
                         small_classes_case, summary)

pytestmark = pytest.mark.gpu

SENTINEL = -0x5455545554555456


@pytest.fixture(scope="module")
def ctx(gpu_ctx_factory):
    return gpu_ctx_factory(32, 8)


@pytest.fixture(scope="module")
def small():
    """Case 4 with its expected mapping, computed once and never written."""
    e, ncols = small_classes_case()
    want = canonical_mapping(e, ncols, K, UNUSABLE)
    want.setflags(write=False)
    return e, ncols, want


def _cycles(ctx, e, ncols, k=K, unusable=UNUSABLE):
    """(mapping on the host, mapping on the device, result) with a sentinel-filled output."""
    import torch
    out = torch.full((ncols, 1 << k), SENTINEL, dtype=torch.int64, device="cuda")
    edges = torch.from_numpy(np.ascontiguousarray(e, dtype=np.int64).reshape(-1, 2)).cuda()
    m, res = ctx.permutation_cycles(edges, k, ncols, unusable, out=out)
    assert m is out
    return m.cpu().numpy(), m, res


def _clean(e, ncols, res, k=K, unusable=UNUSABLE) -> dict:
    s = summary(e, ncols, k, unusable)
    return {"cells_checked": ncols << k, "not_permutation": 0, "order_failures": 0, "padding_failures": 0,
            "edges_checked": s["edges"] - s["out_of_range"], "edge_failures": 0, "cycles": res["classes"]}


def _check(ctx, e, mapping, ncols, k=K, unusable=UNUSABLE):
    import torch
    edges = torch.from_numpy(np.ascontiguousarray(e, dtype=np.int64).reshape(-1, 2)).cuda()
    return ctx.check_permutation_mapping(edges, mapping, k, ncols, unusable)


# ----------------------------------------------------------------- 1. no edges
@pytest.mark.parametrize("ncols,k,unusable", [(4, K, UNUSABLE), (2, 3, 2), (1, 1, 1)])
def test_no_edges_is_the_identity(ctx, ncols, k, unusable):
    e = np.zeros((0, 2), dtype=np.int64)
    got, dev, res = _cycles(ctx, e, ncols, k, unusable)
    assert np.array_equal(got, (np.arange(ncols)[:, None] << 32) | np.arange(1 << k)[None, :])
    assert np.array_equal(got, canonical_mapping(e, ncols, k, unusable))
    assert res == summary(e, ncols, k, unusable) and res["classes"] == 0 and res["linked_cells"] == 0
    assert _check(ctx, e, dev, ncols, k, unusable) == _clean(e, ncols, res, k, unusable)


# ---------------------------------------------------------------- 2. one chain
def test_one_chain_through_every_usable_cell(ctx):
    e, ncols = chain_case()
    got, dev, res = _cycles(ctx, e, ncols)
    assert np.array_equal(got, canonical_mapping(e, ncols, K, UNUSABLE))
    assert res == summary(e, ncols, K, UNUSABLE)
    assert res["classes"] == 1 and res["largest_class"] == 3 * ((1 << K) - UNUSABLE) and res["sort_passes"] == 2
    assert _check(ctx, e, dev, ncols) == _clean(e, ncols, res)


# -------------------------------------------------------------------- 3. a hub
def test_hub_with_doubled_and_self_edges(ctx):
    e, ncols = hub_case()
    got, dev, res = _cycles(ctx, e, ncols)
    assert np.array_equal(got, canonical_mapping(e, ncols, K, UNUSABLE))
    assert res == summary(e, ncols, K, UNUSABLE)
    assert res["self_edges"] == 100 and res["classes"] == 1 and res["largest_class"] == 5001
    assert _check(ctx, e, dev, ncols) == _clean(e, ncols, res)


# ----------------------------------------------------- 4. many small classes
def test_many_small_classes_over_three_digits(ctx, small):
    e, ncols, want = small
    got, _, res = _cycles(ctx, e, ncols)
    assert np.array_equal(got, want)
    assert res == summary(e, ncols, K, UNUSABLE)
    assert res["classes"] == 6000 and res["sort_passes"] == 3 and res["cells"] == 71680


# ------------------------------------------------------ 5. order independence
def test_any_order_of_the_edges_gives_the_same_bytes(ctx, small):
    e, ncols, want = small
    rs = np.random.RandomState(17)
    swapped = e[rs.permutation(e.shape[0])][:, ::-1]
    runs = [_cycles(ctx, x, ncols)[0] for x in (e, e[::-1], swapped, swapped)]
    for got in runs:
        assert got.tobytes() == want.tobytes()
    doubled = np.concatenate([e, swapped, e[::2]])
    got, _, res = _cycles(ctx, doubled, ncols)
    assert got.tobytes() == want.tobytes() and res["classes"] == 6000 and res["edges"] == doubled.shape[0]


# ------------------------------------------------------------ 6. out of range
def test_edges_out_of_range_are_counted_and_skipped(ctx, small):
    e, ncols, want = small
    bad = out_of_range_edges(ncols)
    mixed = np.concatenate([bad[:3], e, bad[3:]])
    got, dev, res = _cycles(ctx, mixed, ncols)
    assert res["out_of_range"] == bad.shape[0] and res["self_edges"] == 0
    assert np.array_equal(got, want)
    assert res == summary(mixed, ncols, K, UNUSABLE)
    assert _check(ctx, mixed, dev, ncols) == _clean(mixed, ncols, res)


# ---------------------------------------------------------------- 7. checker
def test_checker_names_each_kind_of_damage(ctx, small):
    import torch
    e, ncols, want = small
    _, dev, res = _cycles(ctx, e, ncols)
    clean = _clean(e, ncols, res)
    assert _check(ctx, e, dev, ncols) == clean and clean["cycles"] == 6000 == res["classes"]
    ent = lambda i: (i >> K << 32) | (i & ((1 << K) - 1))
    put = lambda t, i, to: t.view(-1).__setitem__(i, ent(to))
    three = next(c for c in cycles_of(want) if len(c) == 3)
    two = next(c for c in cycles_of(want) if len(c) == 2)
    a, b, c = three
    # two cells of one cycle change places: a -> c -> b -> a, two descents
    t = dev.clone()
    put(t, a, c), put(t, c, b), put(t, b, a)
    assert _check(ctx, e, t, ncols) == dict(clean, order_failures=1)
    # one entry copied over another: b is hit twice, c never
    t = dev.clone()
    put(t, b, b)
    got = _check(ctx, e, t, ncols)
    assert got["not_permutation"] == 2 and got["padding_failures"] == 0
    # an entry out of range
    t = dev.clone()
    t.view(-1)[two[0]] = cell(ncols, 0)
    assert _check(ctx, e, t, ncols)["not_permutation"] == 2
    # a class cut in two, each part a well-formed cycle: a alone, b <-> c
    t = dev.clone()
    put(t, a, a), put(t, b, c), put(t, c, b)
    got = _check(ctx, e, t, ncols)
    assert got["edge_failures"] >= 1 and got["not_permutation"] == 0 and got["order_failures"] == 0
    assert got["cycles"] == 6000
    # a 2-cycle in the blinding rows
    t = dev.clone()
    usable = (1 << K) - UNUSABLE
    t[5, usable], t[5, usable + 1] = cell(5, usable + 1), cell(5, usable)
    assert _check(ctx, e, t, ncols) == dict(clean, padding_failures=2, cycles=6001)
    torch.cuda.synchronize()


def test_device_argument_checks(ctx):
    """What a planning context does not reach: the 32-bit cell ids, the column
    limit, null pointers, a mapping that overlaps the edges."""
    import ctypes as ct
    import torch
    from halo2_svd041_amd import _lib
    L = _lib.lib()
    buf = torch.zeros(4096, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    for fn, res in (("svdw_permutation_cycles", _lib.PermutationCyclesResult),
                    ("svdw_check_permutation_mapping", _lib.PermutationMappingCheck)):
        f, r = getattr(L, fn), res()
        assert f(ctx.handle, 28, 6, 17, None, 0, buf.data_ptr(), ct.byref(r)) == -2
        assert b"2^32" in L.svdw_last_error()
        assert f(ctx.handle, 4, 6, 65536, None, 0, buf.data_ptr(), ct.byref(r)) == -2
        assert f(ctx.handle, 4, 6, 2, None, 0, None, ct.byref(r)) == -1
        assert f(ctx.handle, 4, 6, 2, None, 3, buf.data_ptr(), ct.byref(r)) == -1
        assert f(ctx.handle, 4, 6, 0, None, 0, None, ct.byref(r)) == 0
    r = _lib.PermutationCyclesResult()
    f = L.svdw_permutation_cycles
    assert f(ctx.handle, 4, 6, 2, buf.data_ptr() + 8 * 16, 4, buf.data_ptr(), ct.byref(r)) == -1
    assert b"overlaps" in L.svdw_last_error()
    assert f(ctx.handle, 4, 6, 2, buf.data_ptr() + 8 * 32, 4, buf.data_ptr(), ct.byref(r)) == 0
    assert int(buf[:32].ne(torch.arange(32, device="cuda") // 16 << 32 | torch.arange(32, device="cuda") % 16).sum()) == 0


# ------------------------------------------------------------ 9. a larger run
def test_two_pow_22_cells_against_a_torch_sort(ctx):
    """k = 18, 16 columns: every usable cell gets one of 2^16 labels; the classes
    are the cells of equal label. Expected: a stable torch sort by label, each
    run linked in order. All of it stays on the device."""
    import torch
    k, ncols, unusable = 18, 16, UNUSABLE
    rows = 1 << k
    g = torch.Generator(device="cuda").manual_seed(5)
    ids = torch.arange(ncols * rows, device="cuda", dtype=torch.int64)
    ids = ids[(ids & (rows - 1)) < rows - unusable]
    lab = torch.randint(0, 1 << 16, (ids.numel(),), device="cuda", generator=g)
    lab, order = torch.sort(lab, stable=True)
    s = ids[order]                                          # by label, ascending id within a label
    same = lab[1:] == lab[:-1]
    at = torch.arange(s.numel(), device="cuda")
    head = torch.cummax(torch.where(torch.cat([same.new_zeros(1), same]), at.new_zeros(()), at), 0).values
    nxt = torch.where(torch.cat([same, same.new_zeros(1)]), torch.roll(s, -1), s[head])
    ent = lambda i: (i >> k << 32) | (i & (rows - 1))
    want = ent(torch.arange(ncols * rows, device="cuda", dtype=torch.int64))
    want[s] = ent(nxt)
    edges = ent(torch.stack([s[:-1][same], s[1:][same]], dim=1))
    edges = edges[torch.randperm(edges.shape[0], device="cuda", generator=g)].contiguous()
    sizes = torch.bincount(lab, minlength=1 << 16)
    out = torch.full((ncols, rows), SENTINEL, dtype=torch.int64, device="cuda")
    got, res = ctx.permutation_cycles(edges, k, ncols, unusable, out=out)
    assert torch.equal(got.view(-1), want)
    assert res == {"cells": ncols * rows, "edges": edges.shape[0], "out_of_range": 0, "self_edges": 0,
                   "classes": int((sizes > 1).sum()), "linked_cells": int(sizes[sizes > 1].sum()),
                   "largest_class": int(sizes.max()), "sort_passes": 3}
    assert res["classes"] > 60000 and res["largest_class"] > 64
    chk = ctx.check_permutation_mapping(edges, got, k, ncols, unusable)
    assert chk == {"cells_checked": ncols * rows, "not_permutation": 0, "order_failures": 0, "padding_failures": 0,
                   "edges_checked": edges.shape[0], "edge_failures": 0, "cycles": res["classes"]}


# ------------------------------------------------------------- 8. witnesses
W_K, W_MIN_ROWS, W_LB = 10, 20, 8
FORMS = ("canonical", "montgomery")


def _cells(values, form: str):
    """Ints -> [len, 32] u8 device cells in `form`."""
    import torch
    import halo2_svd041_amd as hs
    from permutation_cases import cells_of
    a = cells_of(values)
    if form == "montgomery":
        a = hs.fr_convert(a.view("<u8").reshape(-1, 4), "canonical", "montgomery").view(np.uint8).reshape(a.shape)
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("N,M,P,prefix", [(5, 3, 63, 0), (6, 6, 42, 0), (5, 3, 63, 1)])
def test_witness_sigma_closes_the_argument(gpu_ctx_factory, N, M, P, prefix):
    """The edge list, the fixed columns and the mapping of an SVD witness against
    their host rebuild; then the columns [advice 0, advice 1, fixed, external]
    with sigma from witness_sigma close the permutation argument for both chunk
    lengths, both pairs of challenges and both forms, and stop closing when a
    constant's fixed cell or the gamma cell is changed."""
    import torch
    import halo2_svd041_amd as hs
    from conftest import gamma_for, gen_svd_input
    from cycle_cases import witness_edges
    from halo2_svd041_amd.zk import words_to_int
    from permutation_cases import CHALLENGES
    m, u, d, v = gen_svd_input(N, M, seed=N + M + P)
    gamma = gamma_for(W_K)
    rows = 1 << W_K
    # a context of its own: the rlc_prefix option changes the layout of every later witness
    with hs.Context(device=0, precision_bits=P, lookup_bits=W_LB) as ctx:
        if prefix:
            ctx.set_option("rlc_prefix", 1)
        hs.svd_witness(ctx, m, u, v, d, gamma)
        phys = ctx.physical_layout(W_K, W_MIN_ROWS)
        want_edges, want_lay, constants = witness_edges(ctx, phys)
        edges, lay = ctx.permutation_edges()
        assert lay == want_lay and lay["external"] == 1 and lay["break_edges"] >= 1 and lay["fixed"] == 1
        assert lay["external_edges"] >= 1 + 2 * prefix and len(constants) >= 3
        assert np.array_equal(edges.cpu().numpy(), want_edges)
        ncols = lay["total_cols"]
        want_map = canonical_mapping(want_edges, ncols, W_K, UNUSABLE)
        trace = ctx.rlc_trace()
        assert (trace is not None) == bool(prefix)
        ext_vals = [words_to_int(c) for c in trace["cells"]] if prefix else [gamma]
        assert ext_vals[-1] == gamma
        fixed_vals = [constants[r] if r < len(constants) else 0 for r in range(rows)]
        for form in FORMS:
            fixed = ctx.assign_fixed(form)
            assert torch.equal(fixed, _cells(fixed_vals, form)[None])
            sigma, mapping, lay2 = ctx.witness_sigma(UNUSABLE, form)
            assert lay2 == lay and np.array_equal(mapping.cpu().numpy(), want_map)
            chk = ctx.check_permutation_mapping(edges, mapping, W_K, ncols, UNUSABLE)
            assert chk["not_permutation"] == chk["order_failures"] == chk["edge_failures"] == 0
            assert chk["padding_failures"] == 0 and chk["edges_checked"] == lay["edges"]
            ext = _cells(ext_vals + [0] * (rows - len(ext_vals)), form)[None]
            cols = [ctx.assign_columns(0, form=form)[0], ctx.assign_columns(1, form=form)[0], fixed, ext]
            assert sum(c.shape[0] for c in cols) == ncols
            for chunk_len in (2, 3):
                nsets = -(-ncols // chunk_len)
                for beta, g2 in CHALLENGES:
                    z, res = ctx.permutation_product(cols, sigma, beta, g2, chunk_len, W_K, UNUSABLE, form)
                    assert res == {"columns": ncols, "sets": nsets, "usable_rows": rows - UNUSABLE,
                                   "zero_denominators": 0, "final_not_one": 0}, (form, chunk_len, res)
                    c = ctx.check_permutation_product(cols, sigma, z, beta, g2, chunk_len, W_K, UNUSABLE, form)
                    assert c["recurrence_failures"] == c["boundary_failures"] == c["padding_failures"] == 0
                    assert c["recurrence_checked"] == nsets * (rows - UNUSABLE)
            beta, g2 = CHALLENGES[0]
            # one constant's fixed cell changed: its class no longer holds one value
            bad = fixed.clone()
            bad[0, 1] = _cells([constants[1] + 1], form)[0]
            _, res = ctx.permutation_product(cols[:2] + [bad, ext], sigma, beta, g2, 2, W_K, UNUSABLE, form)
            assert res["final_not_one"] == 1, (form, res)
            # the gamma cell changed
            bad = ext.clone()
            bad[0, len(ext_vals) - 1] = _cells([gamma + 1], form)[0]
            _, res = ctx.permutation_product(cols[:3] + [bad], sigma, beta, g2, 2, W_K, UNUSABLE, form)
            assert res["final_not_one"] == 1, (form, res)
