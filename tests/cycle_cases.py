"""Sigma from the copy constraints, restated on the host, and the cases the
permutation-mapping tests run (include/svdw.h, "permutation argument"; parity
of the rule unpinned).

A cell is col << 32 | row, an edge list an int64 array [n, 2] of cells. The
classes are the connected components over the cells of rows < usable, found
with a plain union-find; canonical_mapping links each class in ascending
(col, row) into one cycle and leaves every other cell to itself. It shares
nothing with the device: no minimum roots, no sort by digits.

Each generator asserts the property it is named for before it returns."""
import numpy as np

K = 10
UNUSABLE = 6


def cell(col: int, row: int) -> int:
    return col << 32 | row


def edge_array(pairs) -> np.ndarray:
    return np.array(list(pairs), dtype=np.int64).reshape(-1, 2)


class UnionFind:
    """Union by size with path compression, over whatever keys it is given."""

    def __init__(self):
        self.parent, self.size = {}, {}

    def find(self, x):
        if x not in self.parent:
            self.parent[x], self.size[x] = x, 1
            return x
        root = x
        while self.parent[root] != root:
            root = self.parent[root]
        while self.parent[x] != root:
            self.parent[x], x = root, self.parent[x]
        return root

    def union(self, a, b):
        a, b = self.find(a), self.find(b)
        if a == b:
            return
        if self.size[a] < self.size[b]:
            a, b = b, a
        self.parent[b] = a
        self.size[a] += self.size[b]


def in_range(edges, total_cols: int, k: int, unusable: int) -> np.ndarray:
    """Per edge: both ends are cells of the columns' usable rows."""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    col, row = e >> 32, e & 0xFFFFFFFF
    ok = (e >= 0) & (col < total_cols) & (row < (1 << k) - unusable)
    return ok[:, 0] & ok[:, 1]


def classes(edges, total_cols: int, k: int, unusable: int) -> list:
    """The classes of two or more cells, each a sorted list of flat ids col << k | row."""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    e = e[in_range(e, total_cols, k, unusable)]
    flat = (e >> 32 << k) | (e & 0xFFFFFFFF)
    uf = UnionFind()
    for a, b in flat.tolist():
        uf.union(a, b)
    groups = {}
    for x in list(uf.parent):
        groups.setdefault(uf.find(x), []).append(x)
    return sorted(sorted(g) for g in groups.values() if len(g) > 1)


def canonical_mapping(edges, total_cols: int, k: int, unusable: int) -> np.ndarray:
    """[total_cols, 2^k] int64 entries col << 32 | row: the rule of include/svdw.h."""
    rows = 1 << k
    nxt = np.arange(total_cols * rows, dtype=np.int64)
    for g in classes(edges, total_cols, k, unusable):
        nxt[g] = g[1:] + g[:1]
    return ((nxt >> k << 32) | (nxt & (rows - 1))).reshape(total_cols, rows)


def summary(edges, total_cols: int, k: int, unusable: int) -> dict:
    """What svdw_permutation_cycles reports besides the mapping."""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    ok = in_range(e, total_cols, k, unusable)
    cl = classes(e, total_cols, k, unusable)
    bits = max(1, (total_cols * (1 << k) - 1).bit_length())
    return {"cells": total_cols << k, "edges": e.shape[0], "out_of_range": int((~ok).sum()),
            "self_edges": int((e[ok][:, 0] == e[ok][:, 1]).sum()), "classes": len(cl),
            "linked_cells": sum(len(g) for g in cl), "largest_class": max([len(g) for g in cl], default=0),
            "sort_passes": -(-bits // 8)}


def cycles_of(mapping: np.ndarray) -> list:
    """The cycles of two or more cells of a mapping, each from its smallest cell
    on in the mapping's order, as flat ids; the mapping must be a permutation."""
    total_cols, rows = mapping.shape
    k = rows.bit_length() - 1
    nxt = ((mapping >> 32 << k) | (mapping & 0xFFFFFFFF)).reshape(-1).tolist()
    seen, out = [False] * len(nxt), []
    for i in range(len(nxt)):
        if seen[i] or nxt[i] == i:
            continue
        cyc, j = [], i
        while not seen[j]:
            seen[j] = True
            cyc.append(j)
            j = nxt[j]
        assert j == i, "not a permutation"
        out.append(cyc)
    return out


# ------------------------------------------------------------------- cases
def chain_case(seed: int = 1, ncols: int = 3):
    """(edges, ncols): all usable cells of the columns in a random order, joined
    neighbour to neighbour, the edges shuffled: one class, found through deep
    trees that span every block."""
    rs = np.random.RandomState(seed)
    usable = (1 << K) - UNUSABLE
    cells = np.array([cell(c, r) for c in range(ncols) for r in range(usable)], dtype=np.int64)
    cells = cells[rs.permutation(cells.size)]
    e = np.stack([cells[:-1], cells[1:]], axis=1)[rs.permutation(cells.size - 1)]
    s = summary(e, ncols, K, UNUSABLE)
    assert s["classes"] == 1 and s["largest_class"] == ncols * usable == s["linked_cells"]
    return e, ncols


def hub_case(seed: int = 2, ncols: int = 8, spokes: int = 5000, selfs: int = 100):
    """(edges, ncols): one cell of the last column joined to `spokes` cells
    spread over the columns, every edge in both directions, and `selfs` edges
    from a cell to itself."""
    rs = np.random.RandomState(seed)
    usable = (1 << K) - UNUSABLE
    hub = cell(ncols - 1, 777)
    pool = np.array([cell(c, r) for c in range(ncols) for r in range(usable)], dtype=np.int64)
    pool = pool[pool != hub][rs.permutation(pool.size - 1)]
    ends, loops = pool[:spokes], pool[spokes - selfs // 2:spokes + selfs - selfs // 2]
    e = np.concatenate([np.stack([np.full(spokes, hub), ends], axis=1), np.stack([ends, np.full(spokes, hub)], axis=1),
                        np.stack([loops, loops], axis=1)])
    e = e[rs.permutation(e.shape[0])]
    s = summary(e, ncols, K, UNUSABLE)
    assert s["self_edges"] == selfs and s["classes"] == 1 and s["largest_class"] == spokes + 1
    assert len(set((ends >> 32).tolist())) == ncols
    return e, ncols


def small_classes_case(seed: int = 3, ncols: int = 70, groups: int = 6000):
    """(edges, ncols): pairs and triples that cross columns; 71,680 cells, so the
    ids need a third 8-bit digit. Some roots (the smallest id of a class) differ
    from another root in that digit alone, some lie below 256, some above 65,536."""
    rs = np.random.RandomState(seed)
    rows, usable = 1 << K, (1 << K) - UNUSABLE
    assert ncols * rows > 1 << 16 and (ncols * rows - 1).bit_length() > 16
    flat = lambda c: (c >> 32 << K) | (c & 0xFFFFFFFF)
    # forced roots: (0, r) and (64, r) have ids r and r + 65,536; their other cells lie above them
    forced, taken = [], set()
    for r in (5, 77, 200, 1000):
        for c0 in (0, 64):
            g = [cell(c0, r), cell(c0 + 2, r + 1), cell(c0 + 5, r + 2)]
            forced.append(g)
            taken.update(g)
    pool = [c for c in (cell(c, r) for c in range(ncols) for r in range(usable)) if c not in taken]
    pool = [pool[i] for i in rs.permutation(len(pool))]
    cl, at = list(forced), 0
    while len(cl) < groups:
        n = 2 + (len(cl) & 1)
        g = pool[at:at + n]
        at += n
        if len({c >> 32 for c in g}) > 1:                  # crosses columns
            cl.append(g)
    pairs = []
    for g in cl:
        for a, b in zip(g[:-1], g[1:]):
            pairs.append((a, b) if rs.randint(2) else (b, a))
    e = edge_array(pairs)[rs.permutation(len(pairs))]
    roots = sorted(min(flat(c) for c in g) for g in cl)
    low = {}
    for r in roots:
        low.setdefault(r & 0xFFFF, set()).add(r >> 16)
    assert sum(len(tops) > 1 for tops in low.values()) >= 3
    assert roots[0] < 256 and roots[-1] > 65536
    s = summary(e, ncols, K, UNUSABLE)
    assert s["classes"] == groups and s["largest_class"] == 3 and s["sort_passes"] == 3
    return e, ncols


def out_of_range_edges(ncols: int) -> np.ndarray:
    """Edges with an end in a blinding row, beyond the rows, beyond the columns
    (one with both ends the same cell): none of them is a copy."""
    rows, usable = 1 << K, (1 << K) - UNUSABLE
    return edge_array([(cell(0, 1), cell(1, usable)), (cell(2, rows - 1), cell(3, 4)), (cell(0, 2), cell(1, rows)),
                       (cell(1, 1 << 31), cell(0, 3)), (cell(ncols, 0), cell(0, 4)), (cell(0, 5), cell(65535, 5)),
                       (cell(ncols, 7), cell(ncols, 7)), (-1, cell(0, 6))])


# ------------------------------------------------------- a witness's edges
def witness_edges(ctx, phys: dict):
    """(edges, layout, constants): the edge list of svdw_permutation_edges for the
    context's last witness, rebuilt from its equality records, break points and
    rlc trace (also on a planning context), the layout svdw_permutation_edges
    reports, and the distinct constants in the order of their placement:
    constant i in fixed column i % num_fixed, row i // num_fixed. phys:
    physical_layout's result. Columns: advice of phase 0, of phase 1, the fixed
    columns, the external column if any record comes from init_rand or the
    witness has the rlc prefix."""
    from permutation_cases import first_placement
    used, nfixed = phys["columns_used"], phys["num_fixed"]
    base, fixed_col = [0, used[0]], used[0] + used[1]
    ext_col = fixed_col + nfixed
    bps = [ctx.break_points(ph) for ph in (0, 1)]
    eqs = [ctx.equalities(ph) for ph in (0, 1)]
    trace = ctx.rlc_trace()

    def place(ph, i):
        c, r = first_placement(bps[ph], int(i))
        return cell(base[ph] + c, r)

    breaks = [(cell(base[ph] + j, int(b)), cell(base[ph] + j + 1, 0)) for ph in (0, 1) for j, b in enumerate(bps[ph])]
    copies, ext, consts, order = [], [], [], {}
    for ph in (0, 1):
        for sp, s, d in eqs[ph][0].tolist():
            if sp == 2:
                ext.append((cell(ext_col, s), place(ph, d)))
            else:
                copies.append((place(sp, s), place(ph, d)))
    for ph in (0, 1):
        for c, v in eqs[ph][1]:
            i = order.setdefault(v, len(order))
            consts.append((place(ph, c), cell(fixed_col + i % nfixed, i // nfixed)))
    if trace is not None:
        ext += [(place(ph, off), cell(ext_col, i)) for i, (ph, off) in enumerate(trace["copies"])]
    external = 1 if ext else 0
    layout = {"k": phys["k"], "advice": list(used), "fixed": nfixed, "external": external,
              "total_cols": fixed_col + nfixed + external, "edges": len(breaks) + len(copies) + len(consts) + len(ext),
              "break_edges": len(breaks), "copy_edges": len(copies), "const_edges": len(consts),
              "external_edges": len(ext), "constants": len(order)}
    assert len(order) == phys["constants"]
    return edge_array(breaks + copies + consts + ext), layout, list(order)
