"""The oracle of the SRS tests, Python integers only, on top of commit_cases (G1)
and permutation_cases (omega): the secret halo2-base's gen_srs draws, the two
scalar columns of ParamsKZG::setup, the edge secrets, the scalars of the
fixed-base cases and, restated from srs.hpp to place cases, never to produce an
expected value, the sizes at which the kernels change what they do."""
import functools
import re

from commit_cases import G, IDENTITY, R, _source, digit_edge_scalars, mul, parse_srs, signed_digits
from permutation_cases import omega

# The secret the issue derives from ChaCha20's first block (zero key, zero nonce): Fr::from_u512 of its 64 bytes.
SECRET = 12823152127514425064804466095718558469400680768825704966376735311210996432058
CHACHA_HEAD = bytes.fromhex("76b8e0ada0f13d90")


@functools.lru_cache(maxsize=None)
def golden():
    """(k, g, g_lagrange) of the reference's file, canonical integer pairs."""
    return parse_srs()


def power_scalars(k: int, s: int) -> list:
    out, v = [], 1
    for _ in range(1 << k):
        out.append(v)
        v = v * s % R
    return out


def lagrange_scalars(k: int, s: int) -> list:
    """l_i(s) for i < 2^k: the indicator of s = omega^i when s lies in the
    domain, else (s^n - 1) omega^i / (n (s - omega^i))."""
    n, w = 1 << k, omega(k)
    ws = power_scalars(k, w)
    if pow(s, n, R) == 1:
        return [1 if s == x else 0 for x in ws]
    c = (pow(s, n, R) - 1) * pow(n, -1, R) % R
    return [c * x * pow(s - x, -1, R) % R for x in ws]


def points_of(scalars) -> list:
    """[v] G for every scalar, equal scalars multiplied once."""
    memo = {}
    return [memo.setdefault(v, mul(G, v)) for v in scalars]


def edge_secrets(k: int) -> dict:
    """name -> secret: 0, 1 = omega^0, omega^3, r - 1 = omega^(n/2), and two
    secrets next to those that are not in the domain."""
    return {"zero": 0, "one": 1, "omega3": pow(omega(k), 3, R), "minus_one": R - 1, "two": 2, "minus_two": R - 2}


def srs_constant(name: str) -> int:
    """A constexpr of csrc/srs.hpp, so that a test placed by it follows it."""
    return int(re.search(r"\b%s\s*=\s*(\d+)" % re.escape(name), _source("srs.hpp")).group(1))


def block_outputs() -> int:
    """The outputs one block of the multiplication kernel owns."""
    return srs_constant("kFbThreads") * srs_constant("kFbGroup")


def planned_window(n: int) -> int:
    """srs.hpp's fb_plan, restated: to assert what the result reports."""
    cost = {c: 10.0 * -(-255 // c) * n + 800.0 * (-(-255 // c) << (c - 1))
            for c in range(2, srs_constant("kFbMaxTableBits") + 1)}
    return min(cost, key=lambda c: (cost[c], c))


def window_scalars(c: int) -> list:
    """The scalars of a fixed-base case with window c: the digit edges, 0, 1 and r - 1."""
    return list(dict.fromkeys([0, 1, R - 1] + digit_edge_scalars(c)))


def doubling_scalar(c: int):
    """A scalar below r whose last mixed add meets its own table entry, or None
    where window c has none. With T = 2^(c (W - 1)) the top window's weight and
    r = t T + rem, the scalar t T - rem has the top digit t while its lower
    digits sum to -rem, and [-rem] G = [r - rem] G = [t T] G: the accumulator
    is the very point the top window adds, so that add is a doubling. (Below
    the top window a partial sum is smaller in magnitude than the next entry's
    scalar, so nothing else can meet; a cancellation needs the sum to be a
    multiple of r, which below r only 0 is.)"""
    W = -(-255 // c)
    T = 1 << (c * (W - 1))
    t, rem = divmod(R, T)
    v = t * T - rem
    if not 0 < v < R or t > 1 << (c - 1):
        return None
    digits = signed_digits(v, c, W)
    lower = sum(d << (c * i) for i, d in enumerate(digits[:-1]))
    return v if digits[-1] == t and lower == -rem else None


def boundary_indices(n: int, chunk_rows: int, count: int = 64) -> list:
    """`count` indices below n: the first, the last, both sides of every chunk
    boundary, then evenly spread ones."""
    idx = [0, n - 1]
    for b in range(chunk_rows, n, chunk_rows):
        idx += [b - 1, b]
    idx = list(dict.fromkeys(idx))[:count]
    step = max(n // count, 1)
    for i in range(step // 2, n, step):
        if len(idx) >= count:
            break
        if i not in idx:
            idx.append(i)
    return sorted(idx)


__all__ = ["G", "IDENTITY", "R", "SECRET", "CHACHA_HEAD", "golden", "power_scalars", "lagrange_scalars", "points_of",
           "edge_secrets", "srs_constant", "block_outputs", "planned_window", "window_scalars", "doubling_scalar", "boundary_indices"]
