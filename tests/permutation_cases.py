"""The permutation argument's grand products Z, restated literally, and what
the permutation-product tests build their columns and sigma from.

grand_products is halo2's permutation::prover::Argument::commit as
include/svdw.h restates it (parity unpinned): per set of chunk_len columns the
per-row fraction with batch_invert's inv0, then the running product, each set
starting where the one before ended. It is the reference of the device's
prefix / suffix products and shares no arithmetic with them; recurrence_holds
is the division-free form the device checker evaluates. delta and omega come
from 7 with pow, as halo2curves derives them.

A sigma is kept as a mapping: mapping[c][r] = (c', r'), the cell that (c, r)
maps to; sigma_values turns it into the field elements delta^c' omega^r'."""
import numpy as np

from lookup_product_cases import CHALLENGES, P_MOD, inv0  # noqa: F401  (CHALLENGES: re-exported)

DELTA = pow(7, 1 << 28, P_MOD)


def omega(k: int) -> int:
    return pow(7, (P_MOD - 1) >> k, P_MOD)


def identity(c: int, r: int, k: int) -> int:
    """The identity permutation's value of cell (c, r): delta^c omega_k^r."""
    return pow(DELTA, c, P_MOD) * pow(omega(k), r, P_MOD) % P_MOD


def identity_mapping(ncols: int, rows: int) -> list:
    return [[(c, r) for r in range(rows)] for c in range(ncols)]


def sigma_values(mapping, k: int) -> list:
    """Per column the list of delta^c' omega^r' of its mapping entries."""
    rows = 1 << k
    w, wp = omega(k), [1] * rows
    for r in range(1, rows):
        wp[r] = wp[r - 1] * w % P_MOD
    dp = [1] * (1 + max(c for col in mapping for c, _ in col))
    for c in range(1, len(dp)):
        dp[c] = dp[c - 1] * DELTA % P_MOD
    return [[dp[c] * wp[r] % P_MOD for c, r in col] for col in mapping]


def mapping_entries(mapping) -> np.ndarray:
    """[ncols, rows] int64: col << 32 | row, the device form of a mapping."""
    return np.array([[c << 32 | r for c, r in col] for col in mapping], dtype=np.int64)


def grand_products(cols, sigma, beta, gamma, chunk_len, k, unusable):
    """(Z: per set a list of 2^k ints, the number of zero denominators).
    cols, sigma: per column a list of 2^k ints."""
    rows = 1 << k
    usable = rows - unusable
    w, wp = omega(k), [1] * rows
    for r in range(1, rows):
        wp[r] = wp[r - 1] * w % P_MOD
    Z, zeros, start = [], 0, 1
    for j0 in range(0, len(cols), chunk_len):
        js = range(j0, min(j0 + chunk_len, len(cols)))
        bd = {j: beta * pow(DELTA, j, P_MOD) % P_MOD for j in js}
        z = [0] * rows
        z[0] = start
        for r in range(usable):
            den = num = 1
            for j in js:
                den = den * (cols[j][r] + beta * sigma[j][r] + gamma) % P_MOD
                num = num * (cols[j][r] + bd[j] * wp[r] + gamma) % P_MOD
            zeros += den == 0
            z[r + 1] = z[r] * (num * inv0(den) % P_MOD) % P_MOD
        start = z[usable]
        Z.append(z)
    return Z, zeros


def recurrence_holds(cols, sigma, Z, beta, gamma, chunk_len, k, unusable) -> list:
    """Per set the rows r < usable where Z_s[r+1] D_s[r] != Z_s[r] N_s[r]."""
    rows = 1 << k
    usable = rows - unusable
    w = omega(k)
    out = []
    for s, j0 in enumerate(range(0, len(cols), chunk_len)):
        js = range(j0, min(j0 + chunk_len, len(cols)))
        bad, wr = [], 1
        for r in range(usable):
            den = num = 1
            for j in js:
                den = den * (cols[j][r] + beta * sigma[j][r] + gamma) % P_MOD
                num = num * (cols[j][r] + beta * pow(DELTA, j, P_MOD) * wr + gamma) % P_MOD
            if Z[s][r + 1] * den % P_MOD != Z[s][r] * num % P_MOD:
                bad.append(r)
            wr = wr * w % P_MOD
        out.append(bad)
    return out


def value_cycles(cols, usable: int, seed: int) -> list:
    """An honest mapping for arbitrary columns: the cells of rows < usable
    grouped by value, each group shuffled and linked into one cycle; everything
    else the identity."""
    rs = np.random.RandomState(seed)
    mapping = identity_mapping(len(cols), len(cols[0]))
    groups = {}
    for c, col in enumerate(cols):
        for r in range(usable):
            groups.setdefault(col[r], []).append((c, r))
    for value in sorted(groups):
        g = groups[value]
        g = [g[i] for i in rs.permutation(len(g))]
        for i, (c, r) in enumerate(g):
            mapping[c][r] = g[(i + 1) % len(g)]
    return mapping


class Assembly:
    """halo2 keygen's permutation Assembly (mapping, aux, sizes) and its copy,
    restated from memory (parity unpinned): the smaller cycle is relabelled into
    the larger, then mapping[a] and mapping[b] are swapped; nothing happens if
    both already share aux."""

    def __init__(self, ncols: int, rows: int):
        self.mapping = identity_mapping(ncols, rows)
        self.aux = identity_mapping(ncols, rows)
        self.sizes = [[1] * rows for _ in range(ncols)]

    def copy(self, a, b) -> None:
        (ac, ar), (bc, br) = a, b
        if self.aux[ac][ar] == self.aux[bc][br]:
            return
        lc, lr = self.aux[ac][ar]
        rc, rr = self.aux[bc][br]
        if self.sizes[lc][lr] < self.sizes[rc][rr]:
            (ac, ar), (bc, br) = (bc, br), (ac, ar)
            (lc, lr), (rc, rr) = (rc, rr), (lc, lr)
        self.sizes[lc][lr] += self.sizes[rc][rr]
        c, r = bc, br
        while True:
            self.aux[c][r] = (lc, lr)
            c, r = self.mapping[c][r]
            if (c, r) == (bc, br):
                break
        self.mapping[ac][ar], self.mapping[bc][br] = self.mapping[bc][br], self.mapping[ac][ar]


def first_placement(bp, i: int):
    """(column, row) of stream cell i at its first physical placement, from the
    phase's break points bp (ctx.break_points): column j's row 0 is cell
    S_j = sum(bp[:j]), and cell i lies in the column with S_j < i <= S_{j+1};
    column 0 also takes i = 0. The last column is open-ended."""
    s = 0
    for j, b in enumerate(bp):
        if i <= s + b:
            return j, i - s
        s += b
    return len(bp), i - s


def cells_of(vals) -> np.ndarray:
    """[len(vals), 32] u8: canonical 32-byte little-endian cells."""
    out = np.zeros((len(vals), 32), dtype=np.uint8)
    for r, x in enumerate(vals):
        if x:
            out[r] = np.frombuffer(int(x).to_bytes(32, "little"), dtype=np.uint8)
    return out
