"""Device ingest (svdw_parse_svd_input_device) on the texts of ingest_cases.py,
which put every kind of byte on every boundary of its design: the 16-byte thread
seam, the 4096-byte chunk seam, the staged window's edges 256 bytes either side,
the host's 256-byte read-backs, more than 1024 chunks, the 2048 / 4096 LDS list
slots and the 255-entry irregularity list. The device equals the plain
restatement (ingest_cases.restate) bit for bit wherever that accepts, and raises
exactly where the host parser does; test_ingest_seams_cpu.py ties the host parser
to the same restatement."""
import time

import numpy as np
import pytest

import halo2_svd041_amd as hs
import ingest_cases as ic

pytestmark = pytest.mark.gpu

# the kind of a number fault: host message -> device message
KINDS = {
    "expected fraction digits": "expected a number",
    "expected exponent digits": "expected a number",
    "significand beyond u64": "significand beyond u64",
    "number out of range": "number out of range",
}
KIND_OF = {"number": ("expected fraction digits", "expected exponent digits"), "overflow": ("significand beyond u64",),
           "range": ("number out of range",)}


@pytest.fixture(scope="module")
def ctx():
    from conftest import have_gpu
    if not have_gpu():                   # (torch initialises the runtime first)
        pytest.skip("no HIP device")
    with hs.Context(device=0, precision_bits=63, lookup_bits=19) as c:
        yield c


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def _equal(dev, want, name):
    """want: {key: (shape, bits)}"""
    for k in "muvd":
        got = dev[k].cpu().numpy()
        assert got.shape == want[k][0], (name, k, got.shape, want[k][0])
        bad = np.nonzero(np.ravel(_bits(got) != want[k][1]))[0]
        assert bad.size == 0, (name, k, bad[:4], np.ravel(got)[bad[:4]])


def _of_host(host):
    return {k: (host[k].shape, _bits(host[k])) for k in "muvd"}


def _accepted(ctx, text, name, src=None):
    _equal(hs.parse_svd_input_device(ctx, text if src is None else src), ic.restate(text), name)


def _refused(ctx, text, name, kind=None):
    with pytest.raises(hs.SvdwError) as host:
        hs.parse_svd_input(text, "serde")
        pytest.fail(f"{name}: the host parser accepted")
    with pytest.raises(hs.SvdwError) as dev:
        hs.parse_svd_input_device(ctx, text)
        pytest.fail(f"{name}: the device parser accepted; host: {host.value}")
    assert dev.value.code == -1, (name, str(dev.value))      # SVDW_EINVAL: a refusal, not a device error
    if kind is not None:                 # one number token is at fault: the same kind of message
        hit = [h for h in KINDS if h in str(host.value)]
        assert hit and hit[0] in KIND_OF[kind], (name, str(host.value))
        assert KINDS[hit[0]] in str(dev.value), (name, str(host.value), str(dev.value))


def _judge(ctx, case):
    if case.verdict == ic.ACCEPT:
        _accepted(ctx, case.text, case.name)
    elif case.verdict == ic.REFUSE:
        _refused(ctx, case.text, case.name, case.kind)
        return False
    elif case.verdict == ic.LIMIT:                  # (the host accepts: test_ingest_seams_cpu.py)
        with pytest.raises(hs.SvdwError, match=ic.LIMIT_MESSAGE):
            hs.parse_svd_input_device(ctx, case.text)
        return False
    else:                                # HOST: raise exactly where the host does, else its values
        try:
            host = hs.parse_svd_input(case.text, "serde")
        except hs.SvdwError:
            _refused(ctx, case.text, case.name)
            return False
        _equal(hs.parse_svd_input_device(ctx, case.text), _of_host(host), case.name)
    return True


def _core_again(ctx, after):
    """a refusal leaves nothing behind (error words, scratch sizes)"""
    _accepted(ctx, ic.CORE, f"the core after {after}")


@pytest.mark.parametrize("kind", ic.PAD_KINDS)
def test_slides(ctx, kind):
    t0 = time.perf_counter()
    n = 0
    for off, text in ic.slide(pad_kind=kind):
        seam = text[ic.CHUNK - 1:ic.CHUNK + 1]
        _accepted(ctx, text, f"{kind} pad, core at {off}, seam bytes {seam!r} (core byte {ic.CHUNK - off})")
        n += 1
    _core_again(ctx, kind)
    print(f"\n{kind} slide: {n} texts, {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("family", ["runs", "tokens", "fuzz", "limits", "members", "sizes"])
def test_family(ctx, family):
    t0 = time.perf_counter()
    cases = list(ic.FAMILIES[family]())
    ok = sum(_judge(ctx, c) for c in cases)
    _core_again(ctx, family)
    print(f"\n{family}: {len(cases)} texts, {ok} accepted, {time.perf_counter() - t0:.2f} s")


def test_mutations(ctx):
    """One defect on the chunk seam: refused exactly where the host refuses, and the
    unmutated neighbour accepted in the same run (refusing everything must not pass)."""
    t0 = time.perf_counter()
    based, refused, n = set(), 0, 0
    for c in ic.mutation_cases():
        if c.base not in based:
            based.add(c.base)
            _accepted(ctx, c.base, c.name + " (unmutated)")
        refused += not _judge(ctx, c)
        n += 1
    assert refused > 0
    _core_again(ctx, "mutations")
    print(f"\nmutations: {n} texts, {refused} refused, {time.perf_counter() - t0:.2f} s")


def test_host_only_texts(ctx):
    for c in ic.HOST_ONLY:
        host = hs.parse_svd_input(c.text, "serde")
        _equal(hs.parse_svd_input_device(ctx, c.text), _of_host(host), c.name)


def test_1025_chunks(ctx):
    """k_scan1 / k_scan2: two chunks per thread, none for the threads past 512."""
    case = ic.big()
    _accepted(ctx, case.text, case.name)
    _core_again(ctx, case.name)


def test_unaligned_base_pointer(ctx):
    """stage()'s 16-byte loads fall back to bytes behind an unaligned pointer."""
    import torch
    text = ic.unaligned_text()
    for j in ic.UNALIGNED:
        t = torch.frombuffer(bytearray(b"\x5d" * j + text), dtype=torch.uint8).to("cuda:0")
        assert t.data_ptr() % 16 == 0
        _accepted(ctx, text, f"{j} junk bytes in front", src=t[j:])
