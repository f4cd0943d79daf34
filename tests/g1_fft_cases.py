"""The oracle of the G1 transform tests, Python integers only, on top of
commit_cases (G1), srs_cases (the SRS's two scalar columns) and
permutation_cases (omega). Every G1 point is [a] G, so a transform of the points
[a_j] G is [A_i] G with A the same DFT over the integers mod r: the oracle costs
a direct O(n^2) sum and one scalar multiplication per point. Restated from
g1_fft.hpp to place cases and to assert what a result reports, never to produce
an expected point: the multiplication counts, the planned window, the bytes of
scratch per point, and the scalar whose last add is a doubling."""
import functools

from commit_cases import G, IDENTITY, R, _source, jadd, jmul, kernel_constant, mul, signed_digits, to_affine
from permutation_cases import omega

POINT_BYTES = 128                                          # a G1Xyzz: table entries and accumulators


def dft_scalars(vals, k: int, inverse: bool = False) -> list:
    """out[i] = sum_j omega^(i j) vals[j] mod r; inverse: 2^-k sum_j omega^(-i j) vals[j]."""
    n = 1 << k
    assert len(vals) == n
    w = omega(k)
    if inverse:
        w = pow(w, -1, R)
    pw = [pow(w, e, R) for e in range(n)]
    scale = pow(n, -1, R) if inverse else 1
    return [scale * sum(v * pw[i * j % n] for j, v in enumerate(vals) if v) % R for i in range(n)]


@functools.lru_cache(maxsize=None)
def gmul(v: int):
    """[v] G, remembered."""
    return mul(G, v)


def points_of(scalars) -> list:
    return [gmul(v % R) for v in scalars]


def multiplication_count(k: int, inverse: bool) -> int:
    """g1_fft.hpp's formulas, restated: what the result reports."""
    n = 1 << k
    return k * n // 2 - n // 2 + 2 if inverse else k * n // 2 - n + 1


def multiplications_by_stage(k: int, inverse: bool) -> int:
    """The same by a direct count over the stages: stage 0 multiplies nothing
    (its twiddle is 1); butterfly t of stage s has the twiddle index
    (t mod 2^s) 2^(k-1-s) and is multiplied unless that is 0; the inverse's
    last stage multiplies both inputs of every butterfly, and at k = 1, where
    the first stage is the last, both of its outputs."""
    n, total = 1 << k, 0
    for s in range(1, k):
        if inverse and s == k - 1:
            total += 2 * (n // 2)
            continue
        total += sum(1 for t in range(n // 2) if (t & ((1 << s) - 1)) << (k - 1 - s))
    if inverse and k == 1:
        total += 2
    return total


def g1_constant(name: str) -> int:
    return kernel_constant(name, "g1_fft.hpp")


def mul_products(c: int) -> int:
    """Field products of one multiplication with window c: 9 per doubling, 14 per
    add of a window, 14 per entry of the table after the first."""
    W = -(-255 // c)
    return 9 * c * W + 14 * W + 14 * ((1 << (c - 1)) - 1)


def point_bytes_per(c: int) -> int:
    """Scratch per point: 2^(c-1) table entries and the accumulator."""
    return ((1 << (c - 1)) + 1) * POINT_BYTES


def planned_window(scratch_mib: int = 1024) -> int:
    """g1_fft.hpp's g1_plan, restated: the cheapest c up to kG1PlanBits whose
    scratch for kG1PlanPoints points fits the cap, the smallest among equal
    costs, 2 when none fits."""
    fits = [c for c in range(2, g1_constant("kG1PlanBits") + 1)
            if c == 2 or point_bytes_per(c) * g1_constant("kG1PlanPoints") <= scratch_mib << 20]
    return min(fits, key=lambda c: (mul_products(c), c))


def pieces(items: int, c: int, scratch_mib: int) -> int:
    """The pieces `items` multiplications with window c run in under the cap."""
    rows = min(max((scratch_mib << 20) // point_bytes_per(c), 1), items)
    return -(-items // rows)


def doubling_scalar(c: int) -> int:
    """r + 2 d0 with d0 the signed residue of -r mod 2^c: its lowest digit is d0
    and its higher digits sum to r + d0, so the accumulator before the last add
    is [r + d0] P = [d0] P, the very entry that add looks up: a doubling (of the
    negated entry for a negative d0). Confirmed with signed_digits."""
    W, full = -(-255 // c), 1 << c
    d0 = -R % full
    if d0 > full >> 1:
        d0 -= full
    v = R + 2 * d0
    digits = signed_digits(v, c, W)
    assert d0 and digits[0] == d0
    assert sum(d << (c * i) for i, d in enumerate(digits) if i) == R + d0
    return v


def big_scalars(c: int) -> list:
    """The integers from r on that a canonical cell can hold: r (the last add
    cancels: the identity), r + 5, and the doubling scalar."""
    return [R, R + 5, doubling_scalar(c)]


def edge_vectors(k: int, a: int, t: int, seed: int) -> dict:
    """name -> the scalars a_j of an input [a_j] G of 2^k points."""
    import numpy as np
    n, w = 1 << k, omega(k)
    rs = np.random.RandomState(seed)
    one = lambda j: [a if i == j else 0 for i in range(n)]   # noqa: E731
    return {
        "identity": [0] * n,
        "single_first": one(0),
        "single_last": one(n - 1),
        "constant": [a] * n,
        "alternating": [a if j % 2 == 0 else R - a for j in range(n)],
        "geometric": [a * pow(w, j * t, R) % R for j in range(n)],
        "random": [int.from_bytes(rs.bytes(32), "little") % R for _ in range(n)],
    }


def quadratic_points(n: int, a0: int, d: int, s0: int, e: int) -> list:
    """[(a0 + i d) (s0 + i e)] G for i < n by second differences, two additions a
    point: the products of the progression points [a0 + i d] G with the scalars
    s0 + i e."""
    f = lambda i: (a0 + i * d) * (s0 + i * e) % R          # noqa: E731
    cur, step, step2 = jmul(G, f(0)), jmul(G, (f(1) - f(0)) % R), jmul(G, 2 * d * e % R)
    out = []
    for _ in range(n):
        out.append(to_affine(cur))
        cur = jadd(cur, step)
        step = jadd(step, step2)
    return out


__all__ = ["G", "IDENTITY", "R", "dft_scalars", "gmul", "points_of", "multiplication_count", "multiplications_by_stage",
           "g1_constant", "mul_products", "point_bytes_per", "planned_window", "pieces", "doubling_scalar",
           "big_scalars", "edge_vectors", "quadratic_points", "_source"]
