"""Texts for the ingest parsers (svdw_parse_svd_input, svdw_parse_svd_input_device)
and a plain restatement of what they must read.

serde_number(token) is serde_json's default float path in plain Python: all
digits as one integer (refused at or above 2^64), float(sig), then one * or /
by float("1e%d") for |e| <= 308, and division by 1e308 in steps past the table.
Python's int -> float and float arithmetic are IEEE, so this is exact, not an
approximation. restate(text) is json.loads with that function on every number
token; it judges the VALUES of every text below that is valid JSON. It is not a
judge of rejections: the host parser is lenient inside unknown members and
stricter elsewhere, and Python's json differs from both, so "refused" is what a
family states (REFUSE) or what the host parser does (HOST, mutations).

The generators never emit leading zeros, escapes other than backslash-quote and
backslash-backslash in keys, NaN or Infinity, or mismatched bracket kinds such
as `[1}` inside unknown members. The last is a known divergence left open: the
host's skip_value counts one bracket kind, the device counts both. A second one
is 1.8e308: both parsers return inf where serde_json, we believe, refuses.

The boundaries of the device parser (csrc/ingest_dev.hip, csrc/ingest.cpp) that
the families cross: 16 bytes per thread, 4096 per chunk, the staged window's
edges 256 bytes either side of a chunk, the host's 256-byte read-backs, 1024
chunks (k_scan1 / k_scan2 then give a thread two), the 2048 number and 4096
structural slots per chunk in LDS, and the 255-entry irregularity list.
"""
import functools
import json
import math
import random
from collections import namedtuple

import numpy as np

CHUNK, HALO, PER = 4096, 256, 16
ACCEPT, REFUSE, HOST, LIMIT = "accept", "refuse", "host", "limit"

# verdict: ACCEPT (restate judges the values), REFUSE (both parsers raise), HOST
# (whatever the host parser does: raise, or these values), LIMIT (as ACCEPT on the
# host; the device refuses with LIMIT_MESSAGE). kind: the number
# fault a REFUSE names ("number", "overflow", "range") or None. base: the
# accepted text a mutation was made from.
Case = namedtuple("Case", "name text verdict kind base", defaults=(None, None))


class Refused(ValueError):
    pass


@functools.lru_cache(maxsize=1 << 14)
def serde_number(token):
    s = token[1:] if token.startswith("-") else token
    mant, _, exp = s.replace("E", "e").partition("e")
    ip, _, fp = mant.partition(".")
    sig = int((ip + fp).lstrip("0") or "0")
    if sig >= 1 << 64:
        raise Refused("significand beyond u64")
    e = (int(exp) if exp else 0) - len(fp)
    f = float(sig)
    while True:
        if abs(e) <= 308:
            f = f * float("1e%d" % e) if e >= 0 else f / float("1e%d" % -e)
            break
        if f == 0.0:
            break
        if e >= 0:
            raise Refused("number out of range")
        f /= 1e308
        e += 308
    return -f if token.startswith("-") else f


def _constant(name):
    raise Refused("constant " + name)


def _pairs(pairs):
    seen = set()
    for k, _ in pairs:
        if k in ("m", "u", "v", "d") and k in seen:
            raise Refused("duplicate key " + k)
        seen.add(k)
    return dict(pairs)


def _array(x, matrix):
    rows = x if matrix else [x]
    if not isinstance(rows, list) or (matrix and not rows):
        raise Refused("shape")
    for r in rows:
        if not isinstance(r, list) or any(type(y) is not float for y in r) or len(r) != len(rows[0]):
            raise Refused("shape")
    a = np.array(rows, dtype=np.float64).reshape(len(rows), len(rows[0]))
    return a if matrix else a[0]


def restate(text):
    """{"m", "u", "v", "d"} -> (shape, f64 bits) of a text; Refused / ValueError otherwise."""
    doc = json.loads(text, parse_float=serde_number, parse_int=serde_number, parse_constant=_constant,
                     object_pairs_hook=_pairs)
    if not isinstance(doc, dict) or any(k not in doc for k in "muvd"):
        raise Refused("keys")
    out = {}
    for k in "muvd":
        a = _array(doc[k], k != "d")
        out[k] = (a.shape, np.ascontiguousarray(a).view(np.uint64))
    return out


def accepts(text):
    try:
        restate(text)
        return True
    except (ValueError, RecursionError):
        return False


# ---------------------------------------------------------------- the core
# One accepted document: keys in the order d, v, u, m; an empty d; a key with an
# escaped quote and a depth-1 string value; an unknown member with literals, a
# nested object and a string holding ']', ',' and '\"'; a two-row matrix, -0.0,
# a 19-digit significand, a negative number, a fraction, exponents with e, E, +, -.
_KNOWN = (b'"v": [[-1.5e+3, 2.5E-3],\r\n\t[-0.0, 1234567890123456789]],\n'
          b' "u" : [ [1e5 , 7E+0,0.125] ,[ 4.9e-324, 18446744073709551615, -123.456e-7 ] ],\n'
          b' "m": [[3, -17.25, 1E-05], [9.87654321e-300, 1.7976931348623157e308, -2]]')
CORE_BODY = (b'"d": [],\n "x\\"y": "v]al,\\"ue[",\n'
             b' "note": {"a": [true, false, null, {"b": {"c": 1}}, "s],\\"t", -2.5e-3], "n": null, "f": false},\n'
             b' "pad": "' + b'=' * 150 + b'",\n ' + _KNOWN)
CORE = b"{" + CORE_BODY + b"}"
KNOWN_AT = len(CORE_BODY) - len(_KNOWN)          # v, u, m: the last members of the body

_UNIT = b']1,[\\"}{:e-5.t '


def _string_fill(k):
    s = bytearray((_UNIT * (k // len(_UNIT) + 1))[:k])
    if s.endswith(b"\\"):
        s[-1] = ord("x")
    return bytes(s)


def _blank_fill(k):
    return (b"   \n\t \r\n    " * (k // 12 + 1))[:k]


def place(off, pad_kind, body=CORE_BODY, tail=b"}"):
    """The body behind a pad of the kind, its first byte at offset off."""
    if pad_kind == "string":
        assert off >= 10
        return b'{"p": "' + _string_fill(off - 10) + b'", ' + body + tail
    if pad_kind == "blank":
        assert off >= 1
        return b"{" + _blank_fill(off - 1) + body + tail
    assert pad_kind == "dense" and off >= 13
    key = b'"p"' if off % 2 else b'"pp"'
    j = (off - 8 - len(key)) // 2
    return b"{" + key + b": [" + b"1," * j + b"1], " + body + tail


PAD_KINDS = ("string", "blank", "dense")
SLIDE_LO, SLIDE_HI = CHUNK - HALO - len(CORE_BODY), CHUNK + HALO


def slide(core=CORE_BODY, pad_kind="string", lo=None, hi=None, step=1):
    """(offset, text): the core's first byte at every offset lo..hi, so that each of
    its bytes crosses the chunk seam, both window edges and every thread seam."""
    lo = CHUNK - HALO - len(core) if lo is None else lo
    hi = CHUNK + HALO if hi is None else hi
    for off in range(lo, hi + 1, step):
        yield off, place(off, pad_kind, core)


# ---------------------------------------------------------------- long runs
_TAIL = b'"u": [[1]], "v": [[1]], "d": [1]'


def _straddled(n, first):
    """n bytes of string content, read in pieces that end at content offsets first,
    first + 256: a backslash last of a piece with its quote first of the next; where
    the content ends on a piece, an escaped backslash ends it and the closing quote
    opens the next; where it ends one byte earlier, the closing quote is the last byte
    of the piece, behind an escaped quote."""
    s = bytearray(b"k" * n)
    for edge in (first, first + 256):
        if n > edge:
            s[edge - 1:edge + 1] = b'\\"'
        elif n == edge:
            s[edge - 2:edge] = b"\\\\"
        elif n == edge - 1:
            s[edge - 3:edge - 1] = b'\\"'
    return bytes(s)


def runs():
    for n in (255, 256, 257, 4097):
        b = _blank_fill(n)
        slots = {
            "colon-string": b'{"s":' + b + b'"abc", "m": [[1, 2]], ' + _TAIL + b"}",
            "colon-bracket": b'{"s": "abc", "m":' + b + b"[[1, 2]], " + _TAIL + b"}",
            "number-comma": b'{"s": "abc", "m": [[1' + b + b", 2]], " + _TAIL + b"}",
            "bracket-number": b'{"s": "abc", "m": [[1, 2], [' + b + b"3, 4]], " + _TAIL + b"}",
            "before-key": b'{"s": "abc", "m": [[1, 2]],' + b + _TAIL + b"}",
            "before-close": b'{"s": "abc", "m": [[1, 2]], ' + _TAIL + b + b"}",
            "after-close": b'{"s": "abc", "m": [[1, 2]], ' + _TAIL + b"}" + b,
        }
        for where, text in slots.items():
            yield Case(f"blank{n}-{where}", text, ACCEPT)
    # strings whose backslash escapes straddle the host's 256-byte read-backs. The
    # host path reads forward in 256-byte pieces from the first byte it misses: a key
    # that opens the text is read from byte 2, so its pieces end at content offsets
    # 256 and 512; the value of "s" is read within the pieces that began at byte 2 for
    # its key, and its content begins at byte 7: offsets 251 and 507.
    for what, first, lengths in (("key", 256, (255, 256, 257, 600)), ("value", 251, (250, 251, 252, 255, 256, 257, 600))):
        for n in lengths:
            s = _straddled(n, first)
            if what == "key":
                text = b'{"' + s + b'": 1, "m": [[1, 2]], ' + _TAIL + b"}"
                assert text.index(s) == 2
            else:
                text = b'{"s": "' + s + b'", "m": [[1, 2]], ' + _TAIL + b"}"
                assert text.index(s) == 7 and 7 + first == 2 + 256
            yield Case(f"{what}{n}", text, ACCEPT)
    # backslash runs before a quote, the quote one byte before, on and after the seam
    for r in (1, 2, 3, 4, 5, 255, 256, 257, 258):
        for q in (CHUNK - 1, CHUNK, CHUNK + 1):
            k = q - 7 - r
            s = b"x" * k + b"\\" * r + b'"' + (b'z]"' if r % 2 else b"")
            yield Case(f"backslash{r}-quote{q}", b'{"s": "' + s + b', "m": [[1, 2]], ' + _TAIL + b"}", ACCEPT)


# ---------------------------------------------------------------- number tokens
def _both(tok):
    yield "m00", b'{"m": [[' + tok + b', 2]], "u": [[1]], "v": [[1]], "d": [3]}'
    yield "dlast", b'{"m": [[2]], "u": [[1]], "v": [[1]], "d": [3, ' + tok + b']}'


def _token_list():
    t = [("18446744073709551615", ACCEPT, None), ("18446744073709551616", REFUSE, "overflow"),
         ("1844674407370955161.5", ACCEPT, None), ("1.8446744073709551616", REFUSE, "overflow"),
         ("1.8446744073709551616e-5", REFUSE, "overflow"), ("99999999999999999999", REFUSE, "overflow"),
         ("-18446744073709551616", REFUSE, "overflow")]
    for e in (307, 308, 309, 323, 324, 616, 617, 700):
        for sig in ("1", "7", "-17", "12345678901234567", "1234.5678901234567", "-0.25"):
            fl = len(sig.partition(".")[2])
            for sign in (+1, -1):
                tok = "%se%s%d" % (sig, "-" if sign * e + fl < 0 else "+" if sig == "7" else "", abs(sign * e + fl))
                try:
                    if math.isinf(serde_number(tok)):
                        continue                       # both signs where finite
                    t.append((tok, ACCEPT, None))
                except Refused:
                    t.append((tok, REFUSE, "range"))
    t += [(x, ACCEPT, None) for x in ("0e999", "-0e999", "0.0e400000", "1e-99999999999999999999", "4.9e-324",
                                      "2.5e-324", "-2.5e-324", "2.4e-324", "0", "-0", "-0.0", "0.5E+1")]
    t += [("1e309", REFUSE, "range"), ("1e400000", REFUSE, "range"), ("-1e309", REFUSE, "range"),
          ("0.001e312", REFUSE, "range")]
    t += [("1.8e308", HOST, None), ("-1.8e308", HOST, None)]     # +-inf today; serde_json, we believe, refuses
    t += [("0." + "0" * 300 + "12345", ACCEPT, None), ("-0." + "0" * 300 + "9007199254740993", ACCEPT, None),
          ("0." + "0" * 5000 + "1", ACCEPT, None), ("1.5e" + "0" * 300 + "12", ACCEPT, None),
          ("25E-" + "0" * 300 + "300", ACCEPT, None), ("1e+" + "0" * 300 + "309", REFUSE, "range")]
    t += [(x, REFUSE, "number") for x in ("1.", "1e", "1.e5", "1e-", "1E+", "-1.", "0.e1")]
    return list({x[0]: x for x in t}.values())


def _behind(start, head, tail):
    """head, a string of x, tail: `start` bytes in all."""
    return head + b"x" * (start - len(head) - len(tail)) + tail


def tokens():
    for tok, verdict, kind in _token_list():
        name = tok if len(tok) < 40 else f"{tok[:12]}..{len(tok)}..{tok[-6:]}"
        for where, text in _both(tok.encode()):
            yield Case(f"{name}-{where}", text, verdict, kind)
    # '-', '.', 'e', the exponent sign and the last digit on the last byte of a
    # chunk and on the first byte of the next
    tok = b"-12.5e-3"
    for part, idx in (("minus", 0), ("point", 3), ("e", 5), ("expsign", 6), ("lastdigit", 7)):
        for pos in (CHUNK - 1, CHUNK):
            start = pos - idx
            m = _behind(start, b'{"p": "', b'", "m": [[') + tok + b', 2]], "u": [[1]], "v": [[1]], "d": [3]}'
            d = _behind(start, b'{"m": [[2]], "u": [[1]], "v": [[1]], "p": "', b'", "d": [3, ') + tok + b"]}"
            assert m[pos] == tok[idx] and d[pos] == tok[idx]
            yield Case(f"seam-{part}-{pos}-m00", m, ACCEPT)
            yield Case(f"seam-{part}-{pos}-dlast", d, ACCEPT)
    # a malformed token cut by the seam
    for tok, idx in ((b"1.", 1), (b"1e", 1), (b"1e-", 2)):
        for pos in (CHUNK - 1, CHUNK):
            start = pos - idx
            m = _behind(start, b'{"p": "', b'", "m": [[') + tok + b', 2]], "u": [[1]], "v": [[1]], "d": [3]}'
            assert m[pos] == tok[idx]
            yield Case(f"seam-{tok.decode()}-{pos}", m, REFUSE, "number")


# ---------------------------------------------------------------- fuzz
_EXPS = (0, 1, 5, 22, 23, 200, 291, 292, 307, 308, 309, 323, 324, 340, 400, 616, 617, 700)


def _fuzz_token(rs):
    nd = 20 if rs.random() < 0.1 else rs.randint(1, 19)
    digits = str(rs.randint(1, 9)) + "".join(str(rs.randint(0, 9)) for _ in range(nd - 1))
    tok = "-" if rs.random() < 0.3 else ""
    if rs.random() < 0.5:
        ni = rs.randint(0, nd - 1)
        tok += (digits[:ni] or "0") + "." + digits[ni:]
    else:
        tok += digits
    if rs.random() < 0.25:
        tok += rs.choice("eE") + rs.choice(("", "+", "-", "-")) + str(rs.choice(_EXPS))
    return tok


def _fault(tok):
    try:
        serde_number(tok)
    except Refused as e:
        return "overflow" if "u64" in str(e) else "range"
    return None


def fuzz(seed=20240607, count=2000):
    rs = random.Random(seed)
    for i in range(count):
        t = [_fuzz_token(rs) for _ in range(4)]
        text = '{"m": [[%s, %s]], "u": [[%s]], "v": [[1]], "d": [%s]}' % tuple(t)
        faults = {_fault(x) for x in t} - {None}
        # (the device reports the lowest fault code, the host the first in the text:
        # the kind is compared where a text has one kind of fault)
        yield Case(f"fuzz{i}", text.encode(), REFUSE if faults else ACCEPT, faults.pop() if len(faults) == 1 else None)


# ---------------------------------------------------------------- mutations
def _outside(text):
    """True where a byte lies outside strings (quotes count as inside)."""
    out, ins, esc = [], False, False
    for c in text:
        if ins:
            out.append(False)
            if esc:
                esc = False
            elif c == 0x5C:
                esc = True
            elif c == 0x22:
                ins = False
        else:
            ins = c == 0x22
            out.append(not ins)
    return out


def _near(sites, at):
    after = [s for s in sites if s >= at]
    return after[0] if after else (sites[-1] if sites else None)


def mutations(text, at, known_from=0, exact=False):
    """(name, site, variant) with one defect each: a comma removed, a comma doubled,
    a ']' removed, a ']' added, a digit replaced by 'x', a '.' appended to a number, a
    ':' removed, a key's closing quote removed; and a second "m" member appended. The
    site is byte `at` itself where that byte admits the defect (exact), else the
    nearest site: the first at or after `at`, or the last before it. Brackets and
    quotes change only from known_from on (the members m, u, v, d), so that no
    variant mismatches bracket kinds inside an unknown member. Variants that are
    still valid JSON of the right shape (restate accepts) are skipped."""
    out = _outside(text)
    n = len(text)

    def sites(pred, lo=0):
        if exact:
            return [at] if at >= lo and out[at] and pred(at) else []
        return [i for i in range(lo, n) if out[i] and pred(i)]

    digit = lambda i: 0x30 <= text[i] <= 0x39
    numch = lambda i: i < n and (digit(i) or text[i] in b".eE+-")
    keyq = [i for i in ([at] if exact else range(known_from, n - 1)) if known_from <= i < n - 1 and text[i] == 0x22
            and not out[i] and out[i + 1] and text[i + 1:].lstrip()[:1] == b":"]
    plans = [
        ("comma-removed", _near(sites(lambda i: text[i] == 0x2C), at), lambda i: text[:i] + text[i + 1:]),
        ("comma-doubled", _near(sites(lambda i: text[i] == 0x2C), at), lambda i: text[:i] + b"," + text[i:]),
        ("bracket-removed", _near(sites(lambda i: text[i] == 0x5D, known_from), at), lambda i: text[:i] + text[i + 1:]),
        ("bracket-added", _near(sites(lambda i: text[i] == 0x5D, known_from), at), lambda i: text[:i] + b"]" + text[i:]),
        ("digit-x", _near(sites(digit), at), lambda i: text[:i] + b"x" + text[i + 1:]),
        ("point-appended", _near(sites(lambda i: digit(i) and not numch(i + 1)), at),
         lambda i: text[:i + 1] + b"." + text[i + 1:]),
        ("colon-removed", _near(sites(lambda i: text[i] == 0x3A), at), lambda i: text[:i] + text[i + 1:]),
        ("keyquote-removed", _near(keyq, at), lambda i: text[:i] + text[i + 1:]),
    ]
    if not exact:
        plans.append(("second-m", text.rstrip().rfind(b"}"), lambda i: text[:i] + b', "m": [[2]]' + text[i:]))
    for name, i, make in plans:
        if i is None or i < 0:
            continue
        v = make(i)
        if not accepts(v):
            yield name, i, v


def mutation_cases():
    """One defect on the chunk seam, behind the string pad and the blank pad. "near":
    every 16th placement of the slide, the defect at the nearest site to byte 4096.
    "seam": for every byte of the core that admits a defect, the placement that puts
    it on the seam (even core offsets on byte 4096, the first of chunk 1; odd ones on
    byte 4095, the last of chunk 0). A defect inside m, u, v is refused by both
    parsers (REFUSE); elsewhere the host decides (HOST: it is lenient in unknown
    members). base: the unmutated text."""
    for kind in ("string", "blank"):
        for off, text in slide(pad_kind=kind, step=16):
            for name, i, v in mutations(text, CHUNK, known_from=off + KNOWN_AT):
                inside = i >= off + KNOWN_AT or name == "second-m"
                yield Case(f"{kind}{off}-near-{name}@{i}", v, REFUSE if inside else HOST, None, text)
        for r in range(len(CORE_BODY)):
            at = CHUNK - r % 2
            text = place(at - r, kind)
            for name, i, v in mutations(text, at, known_from=at - r + KNOWN_AT, exact=True):
                yield Case(f"{kind}{at - r}-seam-{name}@{i}", v, REFUSE if r >= KNOWN_AT else HOST, None, text)


# ---------------------------------------------------------------- limits
_MUVD = b'"m": [[1, 2]], ' + _TAIL

LIMIT_MESSAGE = "too many structural irregularities"


def limits():
    # each string inside an array at depth >= 2 is one irregularity: 255 fit the list
    yield Case("strings255", b'{"w": [' + b'"x",' * 255 + b"1], " + _MUVD + b"}", ACCEPT)
    yield Case("strings256", b'{"w": [' + b'"x",' * 256 + b"1], " + _MUVD + b"}", LIMIT)
    for k in (126, 127, 128, 200):
        yield Case(f"nested{k}", b'{"w": ' + b"[" * k + b"7" + b"]" * k + b", " + _MUVD + b"}", ACCEPT)
        yield Case(f"nested{k}-in-m", b'{"w": 1, "m": ' + b"[" * k + b"7" + b"]" * k + b", " + _TAIL + b"}", REFUSE)
    # a chunk of structural bytes only: all 4096 slots of the structural list
    yield Case("brackets", b'{"w": [' + b"[]," * 3000 + b"[]], " + CORE_BODY + b"}", ACCEPT)


# ---------------------------------------------------------------- member values
def members():
    """m, u, v, d given something else than an array of the right nesting (a
    literal or a string holds no number: it must not pass for an empty d), and
    empty rows."""
    for key in ("d", "m"):
        rest = b", ".join(b'"%s": %s' % (k, b"[1]" if k == b"d" else b"[[1]]") for k in (b"m", b"u", b"v", b"d")
                          if k != key.encode())
        for val in (b"null", b"true", b"false", b'"abc"', b"5", b"{}", b'{"a": [1]}', b"[[[1]]]",
                    b"[[1]]" if key == "d" else b"[1]", b"[[]]" if key == "d" else b"[]", b"[[1], []]", b"[[], [1]]"):
            for text in (b'{"%s": %s, ' % (key.encode(), val) + rest + b"}", b"{" + rest + b', "%s": %s}' % (key.encode(), val)):
                yield Case(f"{key}={val.decode()}-{'first' if text[2:3] == key.encode() else 'last'}", text, REFUSE)
    yield Case("m=[[]]", b'{"m": [[]], ' + _TAIL + b"}", ACCEPT)
    yield Case("m=[[],[]]", b'{"m": [[], [ ]], ' + _TAIL + b"}", ACCEPT)
    yield Case("d=[]", b'{"m": [[1]], "u": [[1]], "v": [[1]], "d": [ ]}', ACCEPT)


# ---------------------------------------------------------------- sizes
def _to_length(n, pad_kind="dense"):
    text = place(n - len(CORE_BODY) - 1, pad_kind)
    assert len(text) == n
    return text


def sizes():
    for n in (4095, 4096, 4097, 8192, 8193):
        for kind in PAD_KINDS:
            yield Case(f"length{n}-{kind}", _to_length(n, kind), ACCEPT)
    for r in range(16):
        yield Case(f"residue{r}", _to_length(len(CORE) + 32 + r, "blank"), ACCEPT)
    yield Case("core", CORE, ACCEPT)


BIG_CHUNKS = 1025


def big():
    """1025 chunks (4 MiB + 1 byte) of dense numeric padding, the core at the very
    end: the smallest text at which k_scan1 / k_scan2 give a thread two chunks."""
    return Case("chunks1025", _to_length(1024 * CHUNK + 1, "dense"), ACCEPT)


UNALIGNED = (1, 3, 8, 15)


def unaligned_text():
    return _to_length(2 * CHUNK + 77, "string")


# three texts Python's json reads differently: pinned against the host parser
HOST_ONLY = [
    Case("backslash-m-key", b'{"\\m": [[5]], "u": [[1]], "v": [[1]], "d": [1]}', HOST),
    Case("leading-zeros", b'{"m": [[007]], "u": [[1]], "v": [[1]], "d": [1]}', HOST),
    Case("1.8e308-pair", b'{"m": [[1.8e308, -1.8e308]], "u": [[1]], "v": [[1]], "d": [1]}', HOST),
]

FAMILIES = {"runs": runs, "tokens": tokens, "fuzz": fuzz, "limits": limits, "members": members, "sizes": sizes}
