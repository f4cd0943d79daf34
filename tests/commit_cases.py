"""The oracle of the commitment tests, Python integers only: BN254 G1 in
Jacobian coordinates, a naive multi-scalar multiplication, the SRS file parser,
"progression" bases P_i = [a0 + i d] G whose MSM has a closed form (also tiled),
and, restated here to place test cases, never to produce an expected value: the
signed-digit split the device documents (include/svdw.h, commit.hpp) with the
scalars at its edges, the regimes the code goes through as the size grows, and
the list of device cases that reach them."""
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


def _source(file: str) -> str:
    return open(os.path.join(ROOT, "halo2_svd041_amd", "csrc", file)).read()


def kernel_constant(name: str, file: str = "commit.hpp") -> int:
    """A constexpr of csrc/commit.hpp (or a named integer of another source
    file), so that a test placed by it follows it."""
    return int(re.search(r"\b%s\s*=\s*(\d+)" % re.escape(name), _source(file)).group(1))


def tiled_msm(tile: int, a0: int, d: int, scalars):
    """The MSM over the bases P_i = progression(tile, a0, d)[i mod tile] as one
    scalar multiplication: [sum_i (a0 + (i mod tile) d) s_i] G."""
    return mul(G, sum((a0 + j * d) * sum(scalars[j::tile]) for j in range(min(tile, len(scalars)))) % R)


# ---- the size-dependent regimes of svdw_commit / svdw_check_commit, restated from
# commit.hpp's constants and prover.cpp's literals: to place and to assert cases,
# never to produce an expected point
POINT_BYTES = 128                                          # a G1Xyzz accumulator: X, Y, ZZ, ZZZ of 32 bytes


def task_cap() -> int:
    """The tasks of one batch at the most (the grid's y limit), prover.cpp."""
    return int(re.search(r"min<uint64_t>\(tasks,\s*(\d+)\)", _source("prover.cpp")).group(1))


def check_partial_bytes() -> int:
    """The partial sums svdw_check_commit holds at a time, prover.cpp."""
    return int(re.search(r"\(\(size_t\)(\d+) << 20\) / per", _source("prover.cpp")).group(1)) << 20


def default_scratch_mib() -> int:
    return kernel_constant("commit_scratch_mib", "engine_internal.hpp")


def _plan(k: int):
    max_bits, best = kernel_constant("kCommitMaxBits"), 2
    for kk in range(1, k + 1):
        cost = {c: -(-255 // c) * (2 ** kk + 1.4 * 2.0 * 2 ** (c - 1)) for c in range(best, max_bits + 1)}
        best = min(cost, key=lambda c: (cost[c], c))       # the smallest c among equal costs, as a strict < keeps it
    return best


def commit_regimes(k: int, c=None, ncols: int = 1, scratch_mib=None) -> dict:
    """What the code does at size 2^k with window c (None: the plan's), ncols
    columns and the workspace cap scratch_mib (None: the default):
    c, W, B = 2^(c-1) buckets, chunks per task and the trips of
    k_commit_window's strided loop over them, the most significant bit of a
    chunk's first bucket j0, levels of the slot tree above the slots, buckets per
    thread of k_commit_scan, commit_check_blocks and the trips of
    k_commit_check_bits's stride loop, commit_task_bytes, tasks, cap / per, the
    tasks T of a full batch, and the columns svdw_check_commit checks at a time."""
    run, fan, chunk = kernel_constant("kCommitRun"), kernel_constant("kCommitFan"), kernel_constant("kCommitChunk")
    threads, tree = kernel_constant("kCommitThreads"), kernel_constant("kCommitTreeThreads")
    n = 1 << k
    c = _plan(k) if c is None else c
    W, B = -(-255 // c), 1 << (c - 1)
    chunks = -(-B // chunk)
    ns = 2 * -(-n // run)
    slots, levels = ns, 0
    while ns > fan:
        ns = -(-ns // fan)
        slots, levels = slots + ns, levels + 1
    blocks = min(-(-n // tree), kernel_constant("kCommitCheckBlocks"))
    per = 4 * B + 4 * (B + 1 + 3) + 4 * n + POINT_BYTES * (slots + B + chunks)
    cap = (default_scratch_mib() if scratch_mib is None else scratch_mib) << 20
    tasks = ncols * W
    part = kernel_constant("kCommitScalarBits") * blocks * POINT_BYTES
    return {"c": c, "W": W, "B": B, "chunks": chunks, "window_trips": -(-chunks // tree),
            "j0_top_bit": ((chunks - 1) * chunk).bit_length() - 1, "levels": levels,
            "scan_per_thread": -(-B // threads), "check_blocks": blocks, "check_trips": -(-n // (blocks * tree)),
            "task_bytes": per, "row_bytes": 4 * n + POINT_BYTES * slots, "tasks": tasks, "cap_over_per": cap // per,
            "T": min(max(cap // per, 1), tasks, task_cap()),
            "check_columns": min(max(check_partial_bytes() // part, 1), ncols)}


def top_digit(s: int, c: int) -> int:
    return signed_digits(s, c, -(-255 // c))[-1]


def digit_edge_scalars(c: int) -> list:
    """Values below r at the edges of the signed-digit split with window c: the
    last positive digit 2^(c-1), the first negative one 2^(c-1) + 1, the
    all-ones digit 2^c - 1, 2^c; 2^253 - 1, whose every digit is all ones, so
    that the carry ripples from window 0 to the top; r - 1, the largest value
    and (the top digit is monotone in the value) the one with the largest top
    digit; the smallest value with that top digit, which reaches it through a
    carry; and the first three shifted into a middle window and into the
    windows that hold bit 32 and bit 64 of the cell."""
    W, half = -(-255 // c), 1 << (c - 1)
    first = [half, half + 1, (1 << c) - 1]
    # the largest value whose digits below the top are all 2^(c-1): one more carries into the top window
    below = sum(half << (c * i) for i in range(W - 1))
    top = top_digit(R - 1, c)
    assert top >= 1
    out = first + [1 << c, (1 << 253) - 1, R - 1, ((top - 1) << (c * (W - 1))) + below + 1]
    for w in (W // 2, 32 // c, 64 // c):
        out += [v << (c * w) for v in first]
    assert all(0 < v < R for v in out)
    return list(dict.fromkeys(out))


def _gpu_cases():
    """(name, k, c or None for the plan's, columns, scratch MiB or None for the
    default) of every case test_commit_gpu.py adds for the regimes above; that
    file takes its parameters from here, test_commit_cpu.py asserts what the
    list covers."""
    max_bits = kernel_constant("kCommitMaxBits")
    cases = [("window", 10, c, 3, None) for c in range(2, max_bits + 1)]
    cases += [("window_srs", 8, c, 3, None) for c in (2, 3, max_bits - 1, max_bits)]
    cases += [("few_rows", k, max_bits, 3, None) for k in (1, 2)]
    cases += [("deep", k, None, 3, None) for k in (16, 18, 20)]
    cases += [("task_cap", 1, None, 600, None), ("one_task", 16, None, 2, 1)]
    cases += [("checker", 13, None, 33, None), ("checker", 14, None, 2, None)]
    return cases


GPU_CASES = _gpu_cases()


def gpu_cases(name: str) -> list:
    return [case[1:] for case in GPU_CASES if case[0] == name]
