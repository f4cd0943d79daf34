"""The oracle of the opening tests, Python integers only: include/svdw.h's
"openings" restated literally (fold per set, synthetic division, Lagrange
interpolation, h1, G, h2, the verifier's constant and both identities of the
checker). It shares no arithmetic with the device; kernel_constant reads
csrc/open.hpp to place cases, never to produce an expected value."""
import os
import re

import numpy as np

P_MOD = 21888242871839275222246405745257275088548364400416034343698204186575808495617
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Y = 0x1f2e3d4c5b6a79888796a5b4c3d2e1f00f1e2d3c4b5a69788796a5b4c3d2e1f3 % P_MOD
V = P_MOD - 0x0123456789abcdef0f1e2d3c
U = (0x2a64de72 << 224) | int("13579bdf" * 7, 16)
T_POINT = (0x1b0c4e72 << 224) | int("2468ace0" * 7, 16)
X_POINT = (0x0d644e72 << 224) | int("9e3779b1" * 7, 16)
assert all(0 < c < P_MOD and c.bit_length() >= 250 for c in (Y, V, U, T_POINT, X_POINT))


def inv(a: int) -> int:
    return pow(a, -1, P_MOD)


def horner(coeffs, x: int) -> int:
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % P_MOD
    return acc


def rand_poly(n: int, seed: int) -> list:
    rs = np.random.RandomState(seed)
    raw = rs.bytes(32 * n)
    return [int.from_bytes(raw[32 * i:32 * i + 32], "little") % P_MOD for i in range(n)]


def fold(polys, c: int) -> list:
    """Horner in c over the polynomials in order: acc <- acc c + p."""
    acc = [0] * len(polys[0])
    for p in polys:
        acc = [(a * c + b) % P_MOD for a, b in zip(acc, p)]
    return acc


def divide(a, s: int):
    """(quotient, remainder) of a by (X - s): synthetic division, the quotient
    padded to len(a) cells (its top cell is zero)."""
    q, carry = [0] * len(a), 0
    for i in range(len(a) - 1, -1, -1):
        q[i] = carry
        carry = (a[i] + s * carry) % P_MOD
    return q, carry


def divide_closed(a, s: int) -> list:
    """q[i] = sum_{j > i} a[j] s^(j - i - 1), term by term."""
    return [sum(a[j] * pow(s, j - i - 1, P_MOD) for j in range(i + 1, len(a))) % P_MOD for i in range(len(a))]


def divide_by_set(a, points) -> list:
    """The Euclidean quotient by Z_S: successive divisions, remainders dropped."""
    for s in points:
        a, _ = divide(a, s)
    return a


def poly_mul(a, b) -> list:
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                out[i + j] = (out[i + j] + x * y) % P_MOD
    return out


def poly_sub(a, b) -> list:
    n = max(len(a), len(b))
    return [((a[i] if i < len(a) else 0) - (b[i] if i < len(b) else 0)) % P_MOD for i in range(n)]


def vanishing(points) -> list:
    """The coefficients of Z_A(X) = prod (X - s)."""
    z = [1]
    for s in points:
        z = poly_mul(z, [-s % P_MOD, 1])
    return z


def vanish_at(points, x: int) -> int:
    z = 1
    for s in points:
        z = z * (x - s) % P_MOD
    return z


def interpolate(points, values) -> list:
    """The coefficients of the polynomial of degree < len(points) through (points, values)."""
    out = [0] * len(points)
    for a, (s, val) in enumerate(zip(points, values)):
        others = [t for b, t in enumerate(points) if b != a]
        w = val * inv(vanish_at(others, s)) % P_MOD
        for i, c in enumerate(vanishing(others)):
            out[i] = (out[i] + w * c) % P_MOD
    return out


def union(sets) -> list:
    T = []
    for S in sets:
        for s in S:
            if s not in T:
                T.append(s)
    return T


def folded(polys, set_of, nsets: int, y: int) -> list:
    """F_i per set: the polynomials of set i in index order, folded with y."""
    return [fold([p for p, s in zip(polys, set_of) if s == i], y) for i in range(nsets)]


def open_h1(polys, set_of, sets, y: int, v: int) -> list:
    F = folded(polys, set_of, len(sets), y)
    return fold([divide_by_set(f, S) for f, S in zip(F, sets)], v)


def set_weights(sets, u: int) -> list:
    """c_i = Z_{T \\ S_i}(u) / Z_{T \\ S_0}(u)."""
    T = union(sets)
    z = [vanish_at([t for t in T if t not in S], u) for S in sets]
    return [zi * inv(z[0]) % P_MOD for zi in z]


def open_g(polys, set_of, sets, y: int, v: int, u: int, h1) -> list:
    F = folded(polys, set_of, len(sets), y)
    c = set_weights(sets, u)
    g = fold([[ci * a % P_MOD for a in f] for ci, f in zip(c, F)], v)
    z0 = vanish_at(sets[0], u)
    return [(a - z0 * b) % P_MOD for a, b in zip(g, h1)]


def open_h2(polys, set_of, sets, y: int, v: int, u: int, h1):
    """(h2, the dropped remainder G(u))."""
    return divide(open_g(polys, set_of, sets, y, v, u, h1), u)


def remainders(polys, set_of, sets, y: int) -> list:
    """r_i: the interpolant of F_i on S_i, as coefficients."""
    F = folded(polys, set_of, len(sets), y)
    return [interpolate(S, [horner(f, s) for s in S]) for f, S in zip(F, sets)]


def constant(polys, set_of, sets, y: int, v: int, u: int) -> int:
    """The verifier's constant: Horner in v of c_i r_i(u)."""
    c = set_weights(sets, u)
    acc = 0
    for ci, r in zip(c, remainders(polys, set_of, sets, y)):
        acc = (acc * v + ci * horner(r, u)) % P_MOD
    return acc


def evals(polys, set_of, sets) -> list:
    return [[horner(p, s) for s in sets[i]] for p, i in zip(polys, set_of)]


def identity1(polys, set_of, sets, y: int, v: int, h1, t: int):
    """(lhs, rhs): h1(t) Z_T(t) and the Horner in v of Z_{T \\ S_i}(t) (F_i(t) - r_i(t))."""
    T = union(sets)
    F = folded(polys, set_of, len(sets), y)
    acc = 0
    for f, S, r in zip(F, sets, remainders(polys, set_of, sets, y)):
        acc = (acc * v + vanish_at([x for x in T if x not in S], t) * (horner(f, t) - horner(r, t))) % P_MOD
    return horner(h1, t) * vanish_at(T, t) % P_MOD, acc


def identity2(polys, set_of, sets, y: int, v: int, u: int, h1, h2, t: int):
    """(lhs, rhs): G(t) - constant and h2(t) (t - u)."""
    g = horner(open_g(polys, set_of, sets, y, v, u, h1), t)
    return (g - constant(polys, set_of, sets, y, v, u)) % P_MOD, horner(h2, t) * (t - u) % P_MOD


def linear_combination(polys, scalars) -> list:
    return [sum(c * p[i] for c, p in zip(scalars, polys)) % P_MOD for i in range(len(polys[0]))]


def omega(k: int) -> int:
    """omega_k = 7^((p - 1) / 2^k), as the permutation section derives it."""
    return pow(7, (P_MOD - 1) >> k, P_MOD)


def circuit_sets(k: int, unusable: int, x: int):
    """The five rotation sets of the circuit shape, {0,1,2,3}, {0}, {0,1,usable},
    {0,1}, {0,-1} at x, and a set_of for eleven polynomials that is not sorted."""
    n, w = 1 << k, omega(k)
    rot = [(0, 1, 2, 3), (0,), (0, 1, n - unusable), (0, 1), (0, n - 1)]
    return [0, 1, 0, 1, 2, 3, 3, 4, 1, 2, 1], [[x * pow(w, r, P_MOD) % P_MOD for r in rs] for rs in rot]


def kernel_constant(name: str) -> int:
    """A constexpr of csrc/open.hpp, so that a test placed by it follows it."""
    src = open(os.path.join(ROOT, "halo2_svd041_amd", "csrc", "open.hpp")).read()
    return int(re.search(r"\b%s\s*=\s*(\d+)" % re.escape(name), src).group(1))
