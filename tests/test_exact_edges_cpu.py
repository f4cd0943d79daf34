"""The exact-arithmetic edge cases (tests/exact_cases.py) on the CPU.

Two things are pinned here, without a GPU:

  * the reference: for every case the C oracle's c_s cells
    (corc.verify_mul_witness) equal sum_k qa[i][k] * qb[k][j] mod p in Python
    integers, with qa, qb from corc.quantize (and those equal the integers the
    generator meant to place);
  * the coverage: the conditions below are requirements on the generator, not
    measurements; a case list that no longer reaches a code-path boundary fails.
"""
import numpy as np
import pytest

import corc
import exact_cases as ec
from conftest import P_MOD, gamma_for

CASES = ec.cases()
IDS = [c[0] for c in CASES]
MODS, HELPER_CUM = ec.ladder()


def _cum_of(mods):
    out, prod = [0], 1
    for m in mods:
        prod *= m
        out.append(prod.bit_length() - 1)
    return out


# the coverage conditions count moduli with this file's own exact products, not
# with the helper's table: a wrong helper entry then also shows as a missing
# tight case, not only in test_ladder_from_first_principles
CUM = _cum_of(MODS)
INFO = {c[0]: ec.info(c, CUM) for c in CASES}
N_MAX = 37      # moduli that bits <= 128 and K <= 8192 can ask for


def _signed(v: int) -> int:
    return v - P_MOD if v > P_MOD // 2 else v


def _ints(cells):
    return [int(r[0]) | int(r[1]) << 64 | int(r[2]) << 128 | int(r[3]) << 192 for r in cells]


def _exact_products(i):
    qa, qb = i["qa"], i["qb"]
    cols = list(zip(*qb))
    return [[sum(x * y for x, y in zip(row, col)) for col in cols] for row in qa]


def test_ladder_from_first_principles():
    """The helper's ladder is what it claims: pairwise coprime, <= 256, greedy
    (no skipped integer is coprime to all larger picks), 2^cum[n] <= m_0 ... m_{n-1} < 2^(cum[n] + 1)."""
    from math import gcd
    assert len(MODS) == ec.N_MOD and len(CUM) == ec.N_MOD + 1 and CUM[0] == 0
    assert HELPER_CUM == CUM
    assert MODS[0] == 256 and all(x > y for x, y in zip(MODS, MODS[1:]))
    for i, m in enumerate(MODS):
        assert all(gcd(m, x) == 1 for x in MODS[:i])
    for skipped in set(range(MODS[-1], 257)) - set(MODS):
        assert any(gcd(skipped, x) != 1 for x in MODS if x > skipped)
    prod = 1
    for n, m in enumerate(MODS, 1):
        prod *= m
        assert (1 << CUM[n]) <= prod < (1 << (CUM[n] + 1)), n


def test_case_list_is_deterministic_and_bounded():
    again = ec.cases()
    assert [c[0] for c in again] == IDS and len(set(IDS)) == len(IDS)
    for c, d in zip(CASES, again):
        assert np.array_equal(c[5], d[5]) and np.array_equal(c[6], d[6])
    for cid, P, N, K, M, a, b in CASES:
        assert a.shape == (N, K) and b.shape == (K, M) and a.dtype == b.dtype == np.float64
        assert P in (32, 63) and N <= 8 and M <= 8 and K <= ec.K_GATE + 1, cid
    fams = [ec.family(i) for i in IDS]
    assert set(fams) == {"ladder", "scan", "digits", "kgate", "lone"}
    assert all(fams.count(f) <= 120 for f in set(fams))
    assert sum(1 for c in CASES if c[1] == 32) >= 10


@pytest.mark.parametrize("cid", IDS)
def test_oracle_cs_equals_integer_sums(cid):
    _, P, N, K, M, a, b = CASES[IDS.index(cid)]
    i = INFO[cid]
    # corc.quantize gives the integers the generator placed
    for x, q in ((a, i["qa"]), (b, i["qb"])):
        qcache = {v: _signed(corc.quantize(v, P)) for v in np.unique(x).tolist()}
        assert [[qcache[v] for v in row] for row in x.tolist()] == q
    c0, _ = corc.verify_mul_witness(a, b, P, gamma_for(IDS.index(cid)))
    assert c0.shape[0] == N * K + K * M + N * M
    want = [v % P_MOD for row in _exact_products(i) for v in row]
    assert _ints(c0[N * K + K * M:]) == want


def test_every_modulus_count_is_visited():
    seen = {INFO[c]["n"] for c in IDS}
    assert set(range(1, N_MAX + 1)) <= seen and 0 not in seen
    lo = ec.need_bits(1, 1, 1)
    hi = ec.need_bits(ec.MAX_BITS, ec.MAX_BITS, ec.K_GATE)
    assert ec.nmod(ec.MAX_BITS, ec.MAX_BITS, ec.K_GATE, CUM) == N_MAX
    for n in range(1, N_MAX + 1):
        if lo <= CUM[n] <= hi:              # need == cum[n] is reachable: a tight case exists
            assert any(INFO[c]["n"] == n and INFO[c]["need"] == CUM[n] and "tight" in ec.FLAGS[c]
                       for c in IDS), n
        # and a case at the first need of that count (or the smallest reachable need)
        first = max(CUM[n - 1] + 1, lo)
        assert any(INFO[c]["need"] == first for c in IDS), n
    # margin cases: need == cum[n-1] + 2, where the value itself stops fitting n - 1
    # moduli (|C| >= m_0 ... m_{n-2} / 2), so too small a margin in the modulus
    # count gives a wrong cell, not just an unused spare modulus. The narrowest
    # operands cannot fill their bound that far: at least 30 of n = 2..36 must.
    beyond = set()
    for n in range(2, N_MAX):
        some = [c for c in IDS if "margin" in ec.FLAGS[c] and INFO[c]["n"] == n]
        assert some and all(INFO[c]["need"] == CUM[n - 1] + 2 for c in some), n
        prod = 1
        for m in MODS[:n - 1]:
            prod *= m
        if any(2 * max(abs(v) for row in _exact_products(INFO[c]) for v in row) >= prod for c in some):
            beyond.add(n)
    assert len(beyond) >= 30, sorted(beyond)
    # every "tight" tag is honest
    for c in IDS:
        if "tight" in ec.FLAGS[c]:
            assert INFO[c]["need"] == CUM[INFO[c]["n"]], c


def test_worst_cases_fill_the_bound():
    """|C| comes within two bits of K 2^ba 2^bb: a margin wrong by lk bits would show."""
    worst = [c for c in IDS if "worst" in ec.FLAGS[c]]
    assert len(worst) >= 90 and all("worst" in ec.FLAGS[c] for c in IDS if ec.family(c) == "ladder")
    for c in worst:
        i = INFO[c]
        top = max(abs(v) for row in _exact_products(i) for v in row)
        assert top >= 1 << (i["ba"] + i["bb"] + i["lk"] - 2), c
        assert top.bit_length() <= i["ba"] + i["bb"] + i["lk"], c


def test_scan_and_residue_widths_are_visited():
    assert {INFO[c]["na_cs"] for c in IDS} == {1, 2, 3, 4, 5, 6, 8}
    sums = {INFO[c]["ba"] + INFO[c]["bb"] + INFO[c]["lk"] for c in IDS if "worst" in ec.FLAGS[c]}
    assert {32 * j + d for j in range(1, 7) for d in (0, 1)} <= sums
    for side in ("ba", "bb"):
        assert {32, 33, 64, 65, 96, 97, 128} <= {INFO[c][side] for c in IDS if ec.family(c) == "scan"}
    for nw in (2, 3, 4):
        assert any(INFO[c]["nw"] == nw and INFO[c]["top_neg"] for c in IDS), nw
    # both sides of each residue-word switch, on either operand
    for side in ("ba", "bb"):
        other = "bb" if side == "ba" else "ba"
        for edge in (64, 65, 96, 97):
            assert any(INFO[c][side] == edge and INFO[c][other] <= edge for c in IDS), (side, edge)


def test_digit_boundaries_are_visited():
    assert ec.digit_boundaries() == [(7, 8), (38, 39), (62, 63), (70, 71)]
    edges = [b for pair in ec.digit_boundaries() for b in pair]
    dig = [c for c in IDS if ec.family(c) == "digits"]
    for side in ("ba", "bb"):
        assert set(edges) <= {INFO[c][side] for c in dig}, side
    assert {INFO[c]["planes_a"] for c in dig} == {INFO[c]["planes_b"] for c in dig} == {0, 5, 8, 9}
    for byte in (0x7f, 0x80, 0xff):
        some = [c for c in dig if f"byte{byte:02x}" in c]
        assert len(some) >= 3
        for c in some:
            for q, bits in ((max(INFO[c]["qa"][0]), INFO[c]["ba"]), (max(INFO[c]["qb"][0]), INFO[c]["bb"])):
                assert q == ec.byte_q(byte, bits) and q.bit_length() == bits, c
                # every whole byte below the top bit that f64 can hold carries the pattern
                whole = [s for s in range(0, bits - 8, 8) if s >= bits - 53]
                assert all((q >> s) & 0xff == byte for s in whole) and (whole or bits <= 8), c


def test_k_gate_cases():
    ks = {c[3] for c in CASES if ec.family(c[0]) == "kgate"}
    assert {257, 300, ec.K_GATE, ec.K_GATE + 1} <= ks
    i = INFO["kgate-k8192-lowbyte80"]
    assert all(abs(v) & 0xff == 0x80 for q in (i["qa"], i["qb"]) for row in q for v in row)
    # balanced residue -128 for the modulus 256 everywhere: every sum is K * 2^14 = 2^27
    assert MODS[0] == 256 and ec.K_GATE * 128 * 128 == 1 << 27
    assert any(v < 0 for row in i["qa"] for v in row) and any(v < 0 for row in i["qb"] for v in row)
    full = INFO["kgate-k8192-a128-b128"]
    assert (full["ba"], full["bb"], full["n"]) == (128, 128, N_MAX)


def test_lone_wide_entries_sit_on_block_edges():
    lone = [c for c in CASES if ec.family(c[0]) == "lone"]
    seen = set()
    for cid, P, N, K, M, a, b in lone:
        assert (N, K, M) == (8, 512, 6)
        i = INFO[cid]
        for side, q, bits in (("a", i["qa"], i["ba"]), ("b", i["qb"], i["bb"])):
            flat = [abs(v).bit_length() for row in q for v in row]
            if side in cid.split("-")[1]:
                assert flat.count(bits) == 1 and bits >= 40 and sorted(set(flat))[-2] == 8, cid
                seen.add((side, flat.index(bits) if flat.index(bits) != len(flat) - 1 else -1, cid.split("-")[1]))
            else:
                assert set(flat) == {8}, cid
    for side in ("a", "b"):
        for where in (side, "ab"):
            assert {(side, p, where) for p in (0, ec.QUANT_BLOCK - 1, ec.QUANT_BLOCK, -1)} <= seen
    # an under-reported width (8 bits for everything) would drop moduli
    for cid, P, N, K, M, a, b in lone:
        assert ec.nmod(8, 8, K, CUM) < INFO[cid]["n"], cid


def test_witness_counts_match_the_oracle():
    """Cell counts of the one-call recipe and of the modular calls (dry contexts)
    for one case of each shape class: what the GPU tests compare stream lengths with."""
    import halo2_svd041_amd as hs
    for cid in ("ladder-n01-first-a1-b1-k1", "kgate-k300-a97-b30", "lone-a-at0-w40"):
        _, P, N, K, M, a, b = CASES[IDS.index(cid)]
        c0, c1 = corc.verify_mul_witness(a, b, P, 7)
        with hs.Context(device=-1, precision_bits=P, lookup_bits=19) as ctx:
            got = hs.verify_mul_witness(ctx, a, b, 7)
        assert got == {"advice0": c0.shape[0], "advice1": c1.shape[0], "lookup0": 0, "lookup1": 0}
