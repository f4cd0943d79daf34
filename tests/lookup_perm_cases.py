"""The lookup argument's permuted columns, restated literally, and the columns
the lookup-argument tests run on.

permute_expression_pair is halo2's lookup::prover::permute_expression_pair as
include/svdw.h restates it (parity unpinned): sort the usable rows of the input
column, walk them, hand the leftover table entries to the repeated rows with
rep.pop(). It is the reference of the device's closed form (histogram, scans,
fill) and shares no arithmetic with it."""
import collections

import numpy as np

# N, M, P, LB, k, lookup cells of phase 0, lookup columns (minimum_rows = 20)
WITNESS_CASES = [
    (4, 4, 32, 8, 9, 895, 2),
    (6, 5, 63, 8, 10, 3459, 4),
    (8, 8, 63, 10, 11, 5925, 3),
    (5, 3, 42, 9, 10, 998, 1),
]
MINIMUM_ROWS = 20


def table_column(LB: int, rows: int) -> list:
    """RangeChip's table column: 0 .. 2^LB - 1, padded with its first value."""
    return list(range(1 << LB)) + [0] * (rows - (1 << LB))


def permute_expression_pair(inp, table, usable: int):
    """(A', S') over the rows [0, usable); ValueError where the lookup fails."""
    a = sorted(inp[:usable])
    left = collections.Counter(table[:usable])
    s = [None] * usable
    rep = []
    for r, x in enumerate(a):
        if r == 0 or x != a[r - 1]:
            s[r] = x
            if left.get(x, 0) <= 0:
                raise ValueError(f"{x} is not in the table")
            left[x] -= 1
        else:
            rep.append(r)
    for value in sorted(left):
        for _ in range(left[value]):
            s[rep.pop()] = value
    assert not rep
    return a, s


def argument_holds(inp, table, a, s, usable: int) -> None:
    """The lookup argument's constraints on (A', S'): adjacency and multisets."""
    assert len(a) == usable and len(s) == usable
    assert a[0] == s[0]
    bad = [r for r in range(1, usable) if a[r] != s[r] and a[r] != a[r - 1]]
    assert not bad, bad[:8]
    assert collections.Counter(a) == collections.Counter(inp[:usable])
    assert collections.Counter(s) == collections.Counter(table[:usable])


def lookup_columns(values, k: int, minimum_rows: int = MINIMUM_ROWS) -> list:
    """A lookup stream cut into physical columns of 2^k rows (max_rows cells each)."""
    rows = 1 << k
    R = rows - minimum_rows
    cols = [list(values[i:i + R]) for i in range(0, len(values), R)]
    return [c + [0] * (rows - len(c)) for c in cols]


def cells(vals, rows: int) -> np.ndarray:
    """[rows, 32] u8: the canonical 32-byte little-endian cells of vals, zero below."""
    out = np.zeros((rows, 32), dtype=np.uint8)
    for r, x in enumerate(vals):
        if x:
            out[r] = np.frombuffer(int(x).to_bytes(32, "little"), dtype=np.uint8)
    return out


def cell_values(a: np.ndarray) -> list:
    """The integers of [n, 32] u8 canonical cells."""
    w = np.ascontiguousarray(a).view("<u8").reshape(-1, 4)
    return [int(r[0]) | int(r[1]) << 64 | int(r[2]) << 128 | int(r[3]) << 192 for r in w]


def synthetic_columns(LB: int, k: int, unusable: int, seed: int = 7) -> dict:
    """name -> column of 2^k values whose usable rows are the degenerate inputs of
    the closed form; rows >= usable are zero."""
    rows, B = 1 << k, 1 << LB
    usable = rows - unusable
    assert B <= usable
    rs = np.random.RandomState(seed)
    once = list(range(B)) + [0] * (usable - B)
    rs.shuffle(once)
    cols = {
        "same_nonzero": [5] * usable,                                   # one run, D = 1, no zero
        "all_zero": [0] * usable,
        "no_zero": rs.randint(1, B, size=usable).tolist(),              # present[0] = 0
        "each_once": [int(x) for x in once],                            # absent is empty
        "hot_bins": rs.choice([0, B - 1], size=usable).tolist(),        # only the register-counted bins
        "uniform": rs.randint(0, B, size=usable).tolist(),
    }
    return {n: [int(x) for x in c] + [0] * unusable for n, c in cols.items()}
