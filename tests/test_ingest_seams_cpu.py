"""The host parser (svdw_parse_svd_input, serde mode) against the plain restatement
in ingest_cases.py on every text of its families: the same f64 bits and shapes
wherever restate accepts, a refusal wherever a family states one. This anchors
the chain restate -> host parser -> device parser (test_ingest_seams_gpu.py)."""
import collections

import numpy as np
import pytest

import halo2_svd041_amd as hs
import ingest_cases as ic


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def _same_as_restate(text, name):
    want = ic.restate(text)                               # the family says valid: restate accepts
    got = hs.parse_svd_input(text, "serde")
    for k in "muvd":
        assert got[k].shape == want[k][0], (name, k, got[k].shape, want[k][0])
        assert np.array_equal(_bits(got[k]), want[k][1]), (name, k)


def _host_refuses(text, name):
    with pytest.raises(hs.SvdwError):
        hs.parse_svd_input(text, "serde")
        pytest.fail(f"{name}: the host parser accepted")


def _judge(case):
    if case.verdict in (ic.ACCEPT, ic.LIMIT):
        _same_as_restate(case.text, case.name)
    elif case.verdict == ic.REFUSE:
        _host_refuses(case.text, case.name)
    else:
        assert case.verdict == ic.HOST, case.name         # pinned in test_host_only_texts


def test_serde_number_restates_the_table_path():
    f = ic.serde_number
    assert f("2.5E3") == 2500.0 and f("-17") == -17.0 and f("1e-05") == 1 / 1e5
    assert f("18446744073709551615") == float(2**64 - 1) and f("1844674407370955161.5") == float(2**64 - 1) / 10
    assert _bits([f("-0e999")])[0] == 1 << 63 and _bits([f("0.0e400000")])[0] == 0
    assert f("4.9e-324") == 5e-324 and f("1e-99999999999999999999") == 0.0
    assert f("1e-309") == 1 / 1e308 / 10 and f("1e308") == 1e308
    for tok in ("18446744073709551616", "1.8446744073709551616", "1.8446744073709551616e-5", "1e309", "1e400000"):
        with pytest.raises(ic.Refused):
            f(tok)
    # one multiply / divide, not correct rounding: differs from float() somewhere
    toks = [f"{k}.{k * 7919123457 % 10**15:015d}e-7" for k in range(1, 200)]
    assert 0 < sum(f(t) != float(t) for t in toks) < len(toks) // 2


def test_core_document():
    assert 450 <= len(ic.CORE) <= 550
    _same_as_restate(ic.CORE, "core")
    got = hs.parse_svd_input(ic.CORE, "serde")
    assert got["d"].shape == (0,) and got["v"].shape == (2, 2)
    assert _bits(got["v"])[1, 0] == 1 << 63                                   # -0.0
    assert got["v"][1, 1] == float(1234567890123456789) and got["u"][0, 0] == 1e5


@pytest.mark.parametrize("kind", ic.PAD_KINDS)
def test_slides(kind):
    n = 0
    for off, text in ic.slide(pad_kind=kind):
        assert text[off:off + len(ic.CORE_BODY)] == ic.CORE_BODY, (kind, off)
        _same_as_restate(text, f"{kind} pad, core at {off}")
        n += 1
    assert n == ic.SLIDE_HI - ic.SLIDE_LO + 1 and ic.SLIDE_LO + len(ic.CORE_BODY) == ic.CHUNK - ic.HALO


@pytest.mark.parametrize("family", ["runs", "tokens", "limits", "members", "sizes"])
def test_family(family):
    cases = list(ic.FAMILIES[family]())
    assert len({c.name for c in cases}) == len(cases)
    for c in cases:
        _judge(c)


def test_dense_pad_fills_the_number_list():
    """2048 one-digit tokens in a whole chunk of the dense pad; 4096 structural
    bytes in a whole chunk of the bracket pad."""
    big = ic.big().text
    assert len(big) == 1024 * ic.CHUNK + 1 and big[ic.CHUNK:2 * ic.CHUNK].count(b"1") == ic.CHUNK // 2
    br = [c for c in ic.limits() if c.name == "brackets"][0].text
    assert set(br[ic.CHUNK:2 * ic.CHUNK]) == set(b"[],")


def test_fuzz_shares():
    cases = list(ic.fuzz())
    assert len(cases) == 2000
    ok = sum(c.verdict == ic.ACCEPT for c in cases)
    assert 2 * ok >= len(cases), ok                       # refused texts test no value
    assert 10 * (len(cases) - ok) >= len(cases), ok
    for c in cases:
        assert ic.accepts(c.text) == (c.verdict == ic.ACCEPT), c.name
        _judge(c)


def test_mutations_against_host():
    """Every variant is invalid for restate and every base accepted; a defect inside
    m, u, v (REFUSE) is refused by the host parser, which decides the others itself
    (HOST: it is lenient inside unknown members). All nine kinds occur among the
    REFUSE variants, and each defect of the "seam" variants lies on byte 4095 or 4096."""
    kinds, bases = collections.Counter(), set()
    for c in ic.mutation_cases():
        assert not ic.accepts(c.text), c.name
        if c.base not in bases:
            bases.add(c.base)
            _same_as_restate(c.base, c.name + " (base)")
        _judge(c)
        how, rest = c.name.split("-", 2)[1:]
        if how == "seam":
            assert int(rest.split("@")[1]) in (ic.CHUNK - 1, ic.CHUNK), c.name
        if c.verdict == ic.REFUSE:
            kinds[(how, rest.split("@")[0])] += 1
    assert len({k for h, k in kinds if h == "near"}) == 9 and len({k for h, k in kinds if h == "seam"}) == 8, kinds


def test_big_text():
    _judge(ic.big())


def test_unaligned_text():
    _same_as_restate(ic.unaligned_text(), "unaligned")


def test_host_only_texts():
    """Three texts Python's json reads differently, pinned on today's host values:
    '\\m' as a key reads as m, 007 as 7, and 1.8e308 as inf (serde_json, we believe,
    refuses the last; left alone)."""
    want = {"backslash-m-key": [[5.0]], "leading-zeros": [[7.0]], "1.8e308-pair": [[np.inf, -np.inf]]}
    assert {c.name for c in ic.HOST_ONLY} == set(want)
    for c in ic.HOST_ONLY:
        got = hs.parse_svd_input(c.text, "serde")
        assert np.array_equal(_bits(got["m"]), _bits(want[c.name])), c.name
        assert got["u"].shape == (1, 1) and got["d"].shape == (1,)
    for tok in ("1.8e308", "-1.8e308"):
        for c in ic.tokens():
            if c.name.startswith(tok + "-"):
                assert c.verdict == ic.HOST
                got = hs.parse_svd_input(c.text, "serde")
                assert np.isinf(got["m"][0, 0]) or np.isinf(got["d"][-1])
