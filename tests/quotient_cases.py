"""The quotient polynomial of include/svdw.h ("quotient"; parity with halo2's
evaluate_h unpinned), restated literally in Python ints, and the honest instance
the quotient tests run on.

fold is the header's list of expressions, h <- h y + e in its order, over values
handed in by a callback; quotient_ext applies it on the rows of the extended
domain (a rotation is a row E r away) and divides by X^n - 1, combined_at applies
it to the polynomials evaluated at one point. Both are the reference of the
device's kernel and checker and share no arithmetic with them. The instance is
built from the restatements of the earlier steps: permute_expression_pair, the
lookup and permutation grand products, value_cycles and the transforms."""
import numpy as np

from lookup_perm_cases import permute_expression_pair, table_column
from lookup_product_cases import grand_product
from ntt_cases import WIDE_SHIFT, ZETA, horner, inv, ntt_forward, ntt_inverse  # noqa: F401  (re-exported)
from permutation_cases import DELTA, P_MOD, grand_products, omega, sigma_values, value_cycles

FAMILIES = ("advice", "selectors", "perm_columns", "sigma", "perm_z", "lookup_input", "lookup_table",
            "permuted_input", "permuted_table", "lookup_z")
# (k, extended_k, unusable_rows, chunk_len)
SMALL_CASES = [(4, 6, 3, 2), (5, 7, 6, 2), (5, 7, 6, 3), (5, 8, 6, 2)]
Y = 0x2f1e0d3c4b5a69788796a5b4c3d2e1f00f1e2d3c4b5a69788796a5b4c3d2e1f1 % P_MOD
BETA = P_MOD - 0x0fedcba987654321
GAMMA = (0x30644e72 << 224) | int("9abcdef1" * 7, 16)
assert all(0 < v < P_MOD and v.bit_length() >= 250 for v in (Y, BETA, GAMMA))


def _wide(rs) -> int:
    return int.from_bytes(rs.bytes(32), "little") % P_MOD


def gated_column(rows: int, usable: int, rs, wide: bool):
    """(advice, selector): halo2-base's vertical gate a[r] + a[r+1] a[r+2] =
    a[r+3] wherever the selector is 1. Gates chain (the output cell is the next
    gate's first input) or leave a gap of one or two free cells, at random; rows
    from `usable` on are zero and carry no gate."""
    a, q = [0] * rows, [0] * rows
    draw = (lambda: _wide(rs)) if wide else (lambda: int(rs.randint(0, 4)))
    r = 0
    a[0] = draw()
    while r + 3 < usable:
        a[r + 1], a[r + 2] = draw(), draw()
        a[r + 3] = (a[r] + a[r + 1] * a[r + 2]) % P_MOD
        q[r] = 1
        r += 3
        gap = int(rs.randint(0, 3))                         # 0: the gates chain
        for _ in range(gap):
            if r + 1 < usable:
                r += 1
                a[r] = draw()
    return a, q


def honest_instance(k: int, extended_k: int, unusable: int, chunk_len: int, seed: int = 1, n_gate: int = 3,
                    n_lookup: int = 1, shift: int = WIDE_SHIFT, lookup_bits: int = 8) -> dict:
    """Lagrange columns (lists of 2^k ints) of an honest witness with the zero
    blinding rows the engine writes: n_gate gated advice columns (the first of
    full-width values, the others small so that values repeat), n_lookup lookup
    columns against the 2^LB range table with A', S' and Z, and the permutation
    over all of them with a non-identity sigma and its Z."""
    rs = np.random.RandomState(seed)
    rows = 1 << k
    usable = rows - unusable
    LB = min(lookup_bits, usable.bit_length() - 1)
    inst = {f: [] for f in FAMILIES}
    inst.update(k=k, extended_k=extended_k, unusable=unusable, chunk_len=chunk_len, beta=BETA, gamma=GAMMA, y=Y,
                shift=shift, lookup_bits=LB)
    for i in range(n_gate):
        a, q = gated_column(rows, usable, rs, wide=i == 0)
        inst["advice"].append(a)
        inst["selectors"].append(q)
    table = table_column(LB, rows)
    for i in range(n_lookup):
        A = [int(x) for x in rs.randint(0, 1 << LB, size=usable)] + [0] * unusable
        ap, sp = permute_expression_pair(A, table, usable)
        ap, sp = ap + [0] * unusable, sp + [0] * unusable
        z, zeros = grand_product(A, table, ap, sp, BETA, GAMMA, usable, rows)
        assert zeros == 0 and z[usable] == 1
        inst["lookup_input"].append(A)
        inst["lookup_table"].append(list(table))
        inst["permuted_input"].append(ap)
        inst["permuted_table"].append(sp)
        inst["lookup_z"].append(z)
    cols = [list(c) for c in inst["advice"] + inst["lookup_input"]]
    if cols:
        mapping = value_cycles(cols, usable, seed + 1)
        assert any(mapping[c][r] != (c, r) for c in range(len(cols)) for r in range(usable))
        inst["perm_columns"] = cols
        inst["sigma"] = sigma_values(mapping, k)
        Z, zeros = grand_products(cols, inst["sigma"], BETA, GAMMA, chunk_len, k, unusable)
        assert zeros == 0 and Z[-1][usable] == 1
        inst["perm_z"] = Z
    return inst


def without(inst: dict, *families) -> dict:
    """The instance with the named families ("gates", "permutation", "lookups") empty."""
    names = {"gates": ("advice", "selectors"), "permutation": ("perm_columns", "sigma", "perm_z"),
             "lookups": ("lookup_input", "lookup_table", "permuted_input", "permuted_table", "lookup_z")}
    out = dict(inst)
    for fam in families:
        for f in names[fam]:
            out[f] = []
    return out


def degree(inst: dict) -> int:
    """D of the header: 3 with gates, 4 with lookups, 2 + the columns of the largest set."""
    d = 0
    if inst["advice"]:
        d = 3
    if inst["lookup_input"]:
        d = 4
    if inst["perm_columns"]:
        d = max(d, 2 + min(inst["chunk_len"], len(inst["perm_columns"])))
    return d


def tail_start(inst: dict) -> int:
    """The first coefficient index of h that must be zero: D (n - 1) - n + 1."""
    n = 1 << inst["k"]
    return degree(inst) * (n - 1) - n + 1


def lagrange_basis(k: int, unusable: int):
    """The Lagrange columns of l_0, l_last, l_active."""
    rows = 1 << k
    usable = rows - unusable
    return ([int(r == 0) for r in range(rows)], [int(r == usable) for r in range(rows)],
            [int(r < usable) for r in range(rows)])


def fold(inst: dict, val, l0: int, llast: int, lact: int, X: int) -> int:
    """The header's expressions in its order, h <- h y + e. val(family, i, r) is
    column i of the family at the rotation r (rows of the original domain;
    "usable" for the rotation by usable rows); X the point itself."""
    b, g, y = inst["beta"], inst["gamma"], inst["y"]
    h = 0

    def push(e):
        nonlocal h
        h = (h * y + e) % P_MOD

    for i in range(len(inst["advice"])):
        push(val("selectors", i, 0) * (val("advice", i, 0) + val("advice", i, 1) * val("advice", i, 2)
                                        - val("advice", i, 3)))
    ncols, chunk = len(inst["perm_columns"]), inst["chunk_len"]
    if ncols:
        nsets = -(-ncols // chunk)
        push(l0 * (1 - val("perm_z", 0, 0)))
        zl = val("perm_z", nsets - 1, 0)
        push(llast * (zl * zl - zl))
        for s in range(1, nsets):
            push(l0 * (val("perm_z", s, 0) - val("perm_z", s - 1, "usable")))
        for s in range(nsets):
            left, right = val("perm_z", s, 1), val("perm_z", s, 0)
            for j in range(s * chunk, min((s + 1) * chunk, ncols)):
                v = val("perm_columns", j, 0)
                left = left * (v + b * val("sigma", j, 0) + g) % P_MOD
                right = right * (v + b * pow(DELTA, j, P_MOD) * X + g) % P_MOD
            push(lact * (left - right))
    for i in range(len(inst["lookup_input"])):
        z, ap, sp = val("lookup_z", i, 0), val("permuted_input", i, 0), val("permuted_table", i, 0)
        push(l0 * (1 - z))
        push(llast * (z * z - z))
        push(lact * (val("lookup_z", i, 1) * (ap + b) * (sp + g)
                     - z * (val("lookup_input", i, 0) + b) * (val("lookup_table", i, 0) + g)))
        push(l0 * (ap - sp))
        push(lact * (ap - sp) * (ap - val("permuted_input", i, -1)))
    return h


def to_coeffs(inst: dict) -> dict:
    """Every column of the instance in coefficient form."""
    out = dict(inst)
    for f in FAMILIES:
        out[f] = [ntt_inverse(c, inst["k"]) for c in inst[f]]
    return out


def to_extended(coeffs: dict) -> dict:
    """Coefficient columns onto the coset shift <omega_extended_k>."""
    out = dict(coeffs)
    for f in FAMILIES:
        out[f] = [ntt_forward(c, coeffs["k"], coeffs["extended_k"], coeffs["shift"]) for c in coeffs[f]]
    return out


def quotient_ext(ext: dict) -> list:
    """h_ext over the 2^extended_k rows from extended columns."""
    k, ek, shift = ext["k"], ext["extended_k"], ext["shift"]
    n, N = 1 << k, 1 << ek
    E = N // n
    usable = n - ext["unusable"]
    L = [ntt_forward(ntt_inverse(c, k), k, ek, shift) for c in lagrange_basis(k, ext["unusable"])]
    we = omega(ek)
    divisor = [inv((pow(shift, n, P_MOD) * pow(we, n * i, P_MOD) - 1) % P_MOD) for i in range(E)]
    out, X = [0] * N, shift
    for j in range(N):
        def val(f, i, r):
            r = usable if r == "usable" else r
            return ext[f][i][(j + r * E) % N]
        out[j] = fold(ext, val, L[0][j], L[1][j], L[2][j], X) * divisor[j % E] % P_MOD
        X = X * we % P_MOD
    return out


def combined_at(coeffs: dict, x: int) -> int:
    """The fold of the polynomials (coefficient columns) at the point x: what
    h(x) (x^n - 1) must equal."""
    k = coeffs["k"]
    usable = (1 << k) - coeffs["unusable"]
    w = omega(k)

    def val(f, i, r):
        r = usable if r == "usable" else r
        return horner(coeffs[f][i], x * pow(w, r % (1 << k), P_MOD) % P_MOD)

    l0, llast, lact = (horner(ntt_inverse(c, k), x) for c in lagrange_basis(k, coeffs["unusable"]))
    return fold(coeffs, val, l0, llast, lact, x)


def identity_holds(coeffs: dict, h_coeffs, x: int) -> bool:
    n = 1 << coeffs["k"]
    return horner(h_coeffs, x) * (pow(x, n, P_MOD) - 1) % P_MOD == combined_at(coeffs, x)


def top_nonzero(h_coeffs) -> int:
    return max((i for i, c in enumerate(h_coeffs) if c), default=-1)
