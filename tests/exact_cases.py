"""Exact-arithmetic edge cases for the verify_mul recipe (no pytest hooks).

cases() returns a deterministic list of (id, P, N, K, M, a, b): float64 inputs
a (N x K) and b (K x M) whose quantized entries q = x * 2^P are chosen integers
placed at the bit widths where the exact-integer kernels switch code path:

  * the CRT GEMM's modulus count n, the smallest n with cum[n] >= need,
    need = bits_a + bits_b + lk + 2, lk = ceil(log2 K);
  * the residue words NW = 2 / 3 / 4 for max(bits_a, bits_b) <= 64 / <= 96 / more;
  * the digit planes 5 / 8 / 9 of the digit GEMM, 0 = Montgomery fallback;
  * the small-operand words na of the Freivalds row scans: ceil(bits / 32) up
    to 192 bits, 8 (full Montgomery) above;
  * the K <= 8192 gate of the exact GEMMs and its i32 accumulator bound;
  * the bit-length fold over the quantize blocks (1024 values each below 2^21).

Everything here is recomputed from first principles (the modulus ladder, the
digit capacities); nothing is read from the kernels' tables, so a wrong table
entry shows as a wrong cell rather than as a moved test.
"""
from __future__ import annotations

from math import gcd

import numpy as np

N_BASE, M_BASE = 6, 5          # small and non-square: an a / b^T mix-up shows
MAX_BITS = 128                 # ZkMatrix::new saturates at 2^128 - 1
K_GATE = 8192                  # the exact GEMMs' K limit
N_MOD = 40                     # moduli in the ladder
LADDER_K = (1, 2, 64, 256, 512)
QUANT_BLOCK = 1024             # values per quantize block for inputs below 2^21 values
DIGIT_PLANES = (1, 5, 8, 9)    # plane counts whose capacity edges are visited


# ------------------------------------------------------------------ ladder
def ladder():
    """(moduli, cum): the 40 largest pairwise-coprime integers <= 256, greedy
    from 256 down, and cum[n] = floor(log2(m_0 ... m_{n-1})), cum[0] = 0."""
    mods = []
    m = 256
    while len(mods) < N_MOD:
        if all(gcd(m, x) == 1 for x in mods):
            mods.append(m)
        m -= 1
    cum, prod = [0], 1
    for x in mods:
        prod *= x
        cum.append(prod.bit_length() - 1)
    return mods, cum


def clog2(k: int) -> int:
    return (k - 1).bit_length()


def need_bits(ba: int, bb: int, K: int) -> int:
    return ba + bb + clog2(K) + 2


def nmod(ba: int, bb: int, K: int, cum=None) -> int:
    """Moduli the CRT GEMM needs: smallest n with cum[n] >= need (0: none)."""
    if cum is None:
        cum = ladder()[1]
    if ba > MAX_BITS or bb > MAX_BITS:
        return 0
    need = need_bits(ba, bb, K)
    for n in range(1, len(cum)):
        if cum[n] >= need:
            return n
    return 0


def nw_of(bmax: int) -> int:
    return 2 if bmax <= 64 else 3 if bmax <= 96 else 4


def na_of(bits: int) -> int:
    if bits > 192:
        return 8
    return max(1, (bits + 31) // 32)


def digit_capacity_bits(D: int) -> int:
    """Largest b with 2^b - 1 <= 127 (256^D - 1) / 255, the largest magnitude
    D balanced base-256 digits (each in [-128, 127]) hold."""
    cap = 127 * (256 ** D - 1) // 255
    b = 0
    while (1 << (b + 1)) - 1 <= cap:
        b += 1
    return b


def digit_boundaries():
    """[(b, b + 1)] for each plane count of DIGIT_PLANES: b fits, b + 1 does not."""
    return [(digit_capacity_bits(D), digit_capacity_bits(D) + 1) for D in DIGIT_PLANES]


def planes_of(bits: int) -> int:
    """Digit planes for |x| < 2^bits: the first of 5, 8, 9 that holds it, else 0."""
    for D in (5, 8, 9):
        if bits <= digit_capacity_bits(D):
            return D
    return 0


# ----------------------------------------------------------------- entries
def max_q(bits: int) -> int:
    """Largest integer of bit length `bits` that is exact in f64."""
    t = min(bits, 53)
    return ((1 << t) - 1) << (bits - t)


def min_q(bits: int) -> int:
    return 1 << (bits - 1)


def byte_q(byte: int, bits: int) -> int:
    """`byte` repeated, truncated to `bits` bits, with the top bit set (so the
    width stays `bits`) and only the top 53 bits kept (exact in f64)."""
    full = int.from_bytes(bytes([byte]) * 16, "little")
    q = (full & ((1 << bits) - 1)) | (1 << (bits - 1))
    if bits > 53:
        q &= ~((1 << (bits - 53)) - 1)
    return q


def to_f64(q, P: int) -> np.ndarray:
    """Nested lists of Python integers q -> float64 array of q / 2^P (exact)."""
    flat = np.array([float(v) for row in q for v in row], dtype=np.float64)
    for v, f in zip((v for row in q for v in row), flat):
        assert int(f) == v, "entry is not exact in f64"
    return np.ldexp(flat, -P).reshape(len(q), len(q[0]))


def base_pattern(ba: int, bb: int, K: int, va=None, vb=None):
    """Integer matrices qa (6 x K), qb (K x 5) of max widths ba, bb.
    Rows of a: +max, -max, alternating, a lone +max at k = K - 1, all 2^(ba-1),
    a unit row (q = 1 at k0). Columns of b: +max, -max, alternating in phase
    with a's row, out of phase, -1 at k0. C holds +-K maxa maxb, 0, +-1 and
    mid-range values. va / vb replace the max magnitudes (same widths)."""
    xa = max_q(ba) if va is None else va
    xb = max_q(bb) if vb is None else vb
    assert xa.bit_length() == ba and xb.bit_length() == bb
    k0 = K // 2
    alt = [1 if k % 2 == 0 else -1 for k in range(K)]
    qa = [[xa] * K,
          [-xa] * K,
          [s * xa for s in alt],
          [0] * (K - 1) + [xa],
          [min_q(ba)] * K,
          [1 if k == k0 else 0 for k in range(K)]]
    cols = [[xb] * K,
            [-xb] * K,
            [s * xb for s in alt],
            [-s * xb for s in alt],
            [-1 if k == k0 else 0 for k in range(K)]]
    qb = [[cols[j][k] for j in range(M_BASE)] for k in range(K)]
    return qa, qb


# ------------------------------------------------------------------- cases
FLAGS = {}      # id -> set of tags: family name, "tight", "first", "margin", "worst"


def _emit(out, cid, P, qa, qb, *tags):
    a, b = to_f64(qa, P), to_f64(qb, P)
    assert cid not in FLAGS, cid
    FLAGS[cid] = set(tags)
    out.append((cid, P, a.shape[0], a.shape[1], b.shape[1], a, b))


def _split(W: int, pref, flip: bool):
    """ba + bb = W, 1 <= ba, bb <= 128; max(ba, bb) = pref where that is possible."""
    if pref is not None and 1 <= W - pref <= pref:
        hi, lo = pref, W - pref
    else:
        hi = (W + 1) // 2
        lo = W - hi
    assert 1 <= lo <= MAX_BITS and 1 <= hi <= MAX_BITS, (W, pref)
    return (lo, hi) if flip else (hi, lo)


_PREFS = (None, 64, 65, 96, 97, 128)


def _ladder_params(S: int, i: int):
    """(ba, bb, K) with ba + bb + lk == S, K from LADDER_K (cycled by i), the
    wider operand's width from _PREFS (cycled by i) where S allows it."""
    for t in range(len(LADDER_K)):
        K = LADDER_K[(i + t) % len(LADDER_K)]
        W = S - clog2(K)
        if 2 <= W <= 2 * MAX_BITS:
            ba, bb = _split(W, _PREFS[i % len(_PREFS)], i % 2 == 1)
            return ba, bb, K
    raise AssertionError(S)


def _family_ladder(out, cum):
    """For every modulus count n: a tight case (need == cum[n], or the largest
    need this family reaches), a first case (need == cum[n-1] + 1, where the
    count switches) and a margin case (need == cum[n-1] + 2, where the value
    itself outgrows n - 1 moduli)."""
    lo_need = need_bits(1, 1, 1)
    hi_need = need_bits(MAX_BITS, MAX_BITS, max(LADDER_K))
    n_max = nmod(MAX_BITS, MAX_BITS, K_GATE, cum)
    # wide and narrow interleaved: 37, 1, 36, 2, ...
    order = []
    lo, hi = 1, n_max
    while lo <= hi:
        order.append(hi)
        if lo != hi:
            order.append(lo)
        lo, hi = lo + 1, hi - 1
    i = 0
    for n in order:
        first = min(max(cum[n - 1] + 1, lo_need), hi_need)
        tight = min(cum[n], hi_need)
        # margin: need == cum[n-1] + 2, i.e. |C| just below 2^cum[n-1] <= m_0 ... m_{n-2}:
        # the first width at which n - 1 moduli could not hold the (signed) value
        margin = first + 1 if n > 1 else None
        done = set()
        for kind, need in (("tight", tight), ("first", first), ("margin", margin)):
            if need is None or need in done or need > tight:
                continue
            done.add(need)
            ba, bb, K = _ladder_params(need - 2, i)
            assert nmod(ba, bb, K, cum) == n
            P = 32 if i % 5 == 4 else 63
            qa, qb = base_pattern(ba, bb, K)
            tags = ["ladder", "worst"] + ([kind] if kind != "tight" else []) + \
                (["tight"] if need == cum[n] else [])
            _emit(out, f"ladder-n{n:02d}-{kind}-a{ba}-b{bb}-k{K}", P, qa, qb, *tags)
            i += 1


def _family_scan(out):
    i = 0
    for j in range(1, 7):
        for S in (32 * j, 32 * j + 1):
            K = (1, 2, 64)[i % 3]
            ba, bb = _split(S - clog2(K), None, i % 2 == 1)
            qa, qb = base_pattern(ba, bb, K)
            _emit(out, f"scan-cs{S}-a{ba}-b{bb}-k{K}", 32 if i % 4 == 3 else 63, qa, qb, "scan", "worst")
            i += 1
    for w in (32, 33, 64, 65, 96, 97, 128):
        for side in ("a", "b"):
            ba, bb = (w, 8) if side == "a" else (8, w)
            qa, qb = base_pattern(ba, bb, 2)
            _emit(out, f"scan-{side}{w}-k2", 63, qa, qb, "scan", "worst")


def _family_digits(out):
    edges = [b for pair in digit_boundaries() for b in pair]
    for i, w in enumerate(edges):
        other = edges[(i + 3) % len(edges)]
        K = 64 if i % 2 == 0 else 7
        for side in ("a", "b"):
            ba, bb = (w, other) if side == "a" else (other, w)
            qa, qb = base_pattern(ba, bb, K)
            _emit(out, f"digits-{side}{w}-o{other}-k{K}", 32 if w == 39 else 63, qa, qb, "digits")
    for byte in (0x7f, 0x80, 0xff):
        for ba, bb in ((38, 39), (63, 62), (70, 71), (8, 7)):
            qa, qb = base_pattern(ba, bb, 64, byte_q(byte, ba), byte_q(byte, bb))
            _emit(out, f"digits-byte{byte:02x}-a{ba}-b{bb}-k64", 63, qa, qb, "digits")


def _family_kgate(out):
    K = K_GATE
    # every low byte 0x80: residue -128 for the modulus 256, accumulator K * 2^14 = 2^27
    qa = [[(1 if (i + k) % 3 else -1) * (0x80 + 256 * ((i + 2 * k) % 3)) for k in range(K)]
          for i in range(N_BASE)]
    qb = [[(1 if (j + k) % 4 else -1) * (0x80 + 256 * ((2 * j + k) % 3)) for j in range(M_BASE)]
          for k in range(K)]
    _emit(out, "kgate-k8192-lowbyte80", 63, qa, qb, "kgate")
    _emit(out, "kgate-k8192-a128-b128", 63, *base_pattern(128, 128, K), "kgate", "worst")
    _emit(out, "kgate-k8192-a7-b8", 32, *base_pattern(7, 8, K), "kgate", "worst")
    _emit(out, "kgate-k8193-a70-b33", 63, *base_pattern(70, 33, K + 1), "kgate")
    _emit(out, "kgate-k8193-a128-b128", 63, *base_pattern(128, 128, K + 1), "kgate")
    for K2, ba, bb in ((257, 64, 65), (257, 128, 128), (300, 97, 30), (300, 33, 96)):
        _emit(out, f"kgate-k{K2}-a{ba}-b{bb}", 32 if (K2, ba) == (300, 33) else 63,
              *base_pattern(ba, bb, K2), "kgate")


def _family_lone(out):
    N, K, M = 8, 512, 6

    def narrow(rows, cols, allmax):
        if allmax:
            return [[(1 if (r + c) % 2 == 0 else -1) * 255 for c in range(cols)] for r in range(rows)]
        return [[(1 if (r + 2 * c) % 3 else -1) * (128 + (7 * r + 3 * c) % 128) for c in range(cols)]
                for r in range(rows)]

    widths = (40, 65, 97, 128)
    i = 0
    for where in ("a", "b", "ab"):
        for pos in ("0", str(QUANT_BLOCK - 1), str(QUANT_BLOCK), "last"):
            qa = narrow(N, K, where != "a")
            qb = narrow(K, M, where != "b")
            w = widths[(i + i // 4) % len(widths)]        # every position meets three widths
            for side, q, cols, total in (("a", qa, K, N * K), ("b", qb, M, K * M)):
                if side in where:
                    f = total - 1 if pos == "last" else int(pos)
                    q[f // cols][f % cols] = (-1 if i % 2 else 1) * max_q(w)
            _emit(out, f"lone-{where}-at{pos}-w{w}", 32 if i % 6 == 5 else 63, qa, qb, "lone")
            i += 1


def cases():
    """The deterministic case list, in the order the GPU tests run it: each
    family alternates wide and narrow widths, so state a wide case leaves on a
    context (residue planes, bit words) would show in the narrow case after it."""
    FLAGS.clear()
    out = []
    cum = ladder()[1]
    _family_ladder(out, cum)
    _family_scan(out)
    _family_digits(out)
    _family_kgate(out)
    _family_lone(out)
    return out


def family(cid: str) -> str:
    return cid.split("-", 1)[0]


def routes(cs) -> dict:
    """Case ids per GPU route (tests/test_exact_edges_gpu.py), in case order."""
    ids = [c[0] for c in cs]
    digits = [i for i in ids if family(i) == "digits"]
    scan = [i for i in ids if family(i) == "scan"]
    return {"A device inputs": ids,
            "A host inputs": ids,
            "A gemm_kern 1": [c[0] for c in cs if family(c[0]) in ("ladder", "kgate") and c[3] >= 257],
            "A gemm_crt 0": digits,
            "B default": ids,
            "B gemm_crt 0 mfma": digits + scan,
            "B gemm_crt 0 valu": digits}


# --------------------------------------------------------------- expectations
def quantized(a: np.ndarray, P: int):
    """Signed integers q = x * 2^P of the entries (exact: the generator's inputs
    are q / 2^P with q exact in f64)."""
    out = []
    for row in np.ldexp(a, P).tolist():
        out.append([int(v) for v in row])
    return out


def info(case, cum=None) -> dict:
    """Widths and code-path selectors of a case, from its actual entries."""
    cid, P, N, K, M, a, b = case
    qa, qb = quantized(a, P), quantized(b, P)
    ba = max(abs(v).bit_length() for r in qa for v in r)
    bb = max(abs(v).bit_length() for r in qb for v in r)
    lk = clog2(K)
    top_neg = any(v < 0 and abs(v).bit_length() == max(ba, bb) for q in (qa, qb) for r in q for v in r)
    return {"ba": ba, "bb": bb, "lk": lk, "need": ba + bb + lk + 2, "n": nmod(ba, bb, K, cum),
            "nw": nw_of(max(ba, bb)), "top_neg": top_neg, "na_cs": na_of(ba + bb + lk),
            "na_a": na_of(ba), "na_b": na_of(bb), "planes_a": planes_of(ba), "planes_b": planes_of(bb),
            "qa": qa, "qb": qb}


def describe() -> str:
    """Case counts per family and the selector values each family visits."""
    cs = cases()
    cum = ladder()[1]
    lines = []
    fams = {}
    for c in cs:
        fams.setdefault(family(c[0]), []).append(info(c, cum))
    for f, infos in fams.items():
        def vals(key):
            return sorted({i[key] for i in infos})
        lines.append(f"{f}: {len(infos)} cases; n {vals('n')}; NW {vals('nw')}; na(c_s) {vals('na_cs')}; "
                     f"na(a) {vals('na_a')}; na(b) {vals('na_b')}; planes(a) {vals('planes_a')}; "
                     f"planes(b) {vals('planes_b')}")
    lines.append(f"total: {len(cs)} cases")
    by_id = {c[0]: info(c, cum) for c in cs}
    for r, ids in routes(cs).items():
        def vals(*keys):
            return sorted({by_id[i][k] for i in ids for k in keys})
        lines.append(f"route {r}: {len(ids)} cases; n {vals('n')}; NW {vals('nw')}; "
                     f"na {vals('na_cs', 'na_a', 'na_b')}; planes {vals('planes_a', 'planes_b')}")
    return "\n".join(lines)


if __name__ == "__main__":
    print(describe())
