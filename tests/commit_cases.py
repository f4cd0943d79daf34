"""The oracle of the commitment tests, Python integers only: BN254 G1 in
Jacobian coordinates, a naive multi-scalar multiplication, the SRS file parser,
"progression" bases P_i = [a0 + i d] G whose MSM has a closed form, and the
signed-digit split the device documents (include/svdw.h, commit.hpp), restated
here to place test cases, never to produce an expected value."""
import os
import re

Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617   # the group order, Fr's p
G = (1, 2)
MONT = 1 << 256
MONT_INV = pow(MONT, -1, Q)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRS8 = os.path.join(ROOT, "tests", "golden", "kzg_bn254_8.srs")
IDENTITY = (0, 0)                                          # affine, as halo2curves
JID = (1, 1, 0)                                            # Jacobian


def on_curve(p) -> bool:
    return (p[1] * p[1] - p[0] ** 3 - 3) % Q == 0


def parse_srs(path=SRS8):
    """(k, g, g_lagrange): affine points as canonical integer pairs."""
    raw = open(path, "rb").read()
    k = int.from_bytes(raw[:4], "little")
    n = 1 << k
    assert len(raw) == 4 + 2 * 64 * n + 256

    def pt(o):
        return tuple(int.from_bytes(raw[o + 32 * j:o + 32 * j + 32], "little") * MONT_INV % Q for j in (0, 1))
    return k, [pt(4 + 64 * i) for i in range(n)], [pt(4 + 64 * (n + i)) for i in range(n)]


def jdouble(p):
    x, y, z = p
    if z == 0:
        return JID
    a, b = x * x % Q, y * y % Q
    c = b * b % Q
    d = 2 * ((x + b) ** 2 - a - c) % Q
    e = 3 * a % Q
    x3 = (e * e - 2 * d) % Q
    return x3, (e * (d - x3) - 8 * c) % Q, 2 * y * z % Q


def jadd(p, q):
    if p[2] == 0:
        return q
    if q[2] == 0:
        return p
    z1z1, z2z2 = p[2] * p[2] % Q, q[2] * q[2] % Q
    u1, u2 = p[0] * z2z2 % Q, q[0] * z1z1 % Q
    s1, s2 = p[1] * q[2] * z2z2 % Q, q[1] * p[2] * z1z1 % Q
    if u1 == u2:
        return jdouble(p) if s1 == s2 else JID
    h, r = (u2 - u1) % Q, (s2 - s1) % Q
    hh = h * h % Q
    hhh, v = h * hh % Q, u1 * hh % Q
    x3 = (r * r - hhh - 2 * v) % Q
    return x3, (r * (v - x3) - s1 * hhh) % Q, p[2] * q[2] * h % Q


def to_jac(a):
    return JID if a == IDENTITY else (a[0], a[1], 1)


def to_affine(p):
    if p[2] == 0:
        return IDENTITY
    zi = pow(p[2], -1, Q)
    return p[0] * zi * zi % Q, p[1] * zi * zi * zi % Q


def neg(a):
    return (a[0], -a[1] % Q)


def jmul(a, s: int):
    """[s] a for an affine a, Jacobian out."""
    acc, base = JID, to_jac(a)
    for bit in bin(s)[2:] if s else "":
        acc = jdouble(acc)
        if bit == "1":
            acc = jadd(acc, base)
    return acc


def mul(a, s: int):
    return to_affine(jmul(a, s % R))


def msm(points, scalars):
    """The naive sum of [s_i] P_i, affine."""
    acc = JID
    for p, s in zip(points, scalars):
        if s % R and p != IDENTITY:
            acc = jadd(acc, jmul(p, s % R))
    return to_affine(acc)


def progression(n: int, a0: int, d: int):
    """P_i = [a0 + i d] G for i < n, by repeated addition."""
    step, cur, out = jmul(G, d % R), jmul(G, a0 % R), []
    for _ in range(n):
        out.append(to_affine(cur))
        cur = jadd(cur, step)
    return out


def progression_msm(n: int, a0: int, d: int, scalars):
    """The MSM over progression(n, a0, d) as one scalar multiplication."""
    return mul(G, sum((a0 + i * d) * s for i, s in zip(range(n), scalars)) % R)


def point_bytes(points, form: str) -> bytes:
    """64 bytes per affine point, coordinates canonical or Montgomery."""
    f = MONT if form == "montgomery" else 1
    return b"".join((c * f % Q).to_bytes(32, "little") for p in points for c in p)


def points_from_bytes(raw: bytes, form: str):
    f = MONT_INV if form == "montgomery" else 1
    v = [int.from_bytes(raw[i:i + 32], "little") * f % Q for i in range(0, len(raw), 32)]
    return list(zip(v[0::2], v[1::2]))


def signed_digits(s: int, c: int, windows: int):
    """The digits in (-2^(c-1), 2^(c-1)] with carry that commit.hpp documents."""
    out, carry = [], 0
    for _ in range(windows):
        d = (s & ((1 << c) - 1)) + carry
        s >>= c
        carry = 1 if d > (1 << (c - 1)) else 0
        out.append(d - (carry << c))
    assert s == 0 and carry == 0
    return out


def kernel_constant(name: str) -> int:
    """A constexpr of csrc/commit.hpp, so that a test placed by it follows it."""
    src = open(os.path.join(ROOT, "halo2_svd041_amd", "csrc", "commit.hpp")).read()
    return int(re.search(r"\b%s\s*=\s*(\d+)" % re.escape(name), src).group(1))
