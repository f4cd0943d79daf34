"""A KZG structured reference string as halo2_proofs' ParamsKZG reads and writes
it: read one, make one on the device as halo2-base's gen_srs does, write one.

Layout (pinned by tests/golden/kzg_bn254_8.srs): u32 k little endian, 2^k x 64 B
`g` (the powers of the secret in G1), 2^k x 64 B `g_lagrange` (the same in the
Lagrange basis of the size-2^k domain), then 2 x 128 B of G2: the generator and
[s] G2. A G1 point is x then y, each a 32-byte little-endian Fq in Montgomery
form: halo2curves' in-memory G1Affine, which is `bases_form="montgomery"` of
Context.commit. A G2 point is x.c0, x.c1, y.c0, y.c1, each such an Fq
(Fq2 = Fq[u] / (u^2 + 1)).

gen_srs(k) of halo2-base reads params/kzg_bn254_{k}.srs or makes it with
ParamsKZG::setup(k, ChaCha20Rng::from_seed(Default::default())): one secret s =
Fr::random(rng), g[i] = [s^i] G, g_lagrange[i] = [l_i(s)] G. default_secret()
derives that s; gen_srs() here runs the 2 * 2^k fixed-base multiplications on
the device (Context.srs_setup); write_srs() adds the G2 half on the host, one
scalar multiplication over Python integers. The golden file is reproduced byte
for byte (tests/test_srs_cpu.py, tests/test_srs_gpu.py).

A ceremony's file has no known secret and fixes k at the ceremony's size:
downsize() is ParamsKZG::downsize, the first 2^k points of g and their Lagrange
form by g_to_lagrange(), an inverse FFT over G1 on the device (Context.g1_fft).
read_srs() keeps the file's G2 bytes and write_srs() writes them back when it
has no secret, so a downsized ceremony file can be written
(tests/test_g1_fft_cpu.py, tests/test_g1_fft_gpu.py).
"""
from __future__ import annotations

import numpy as np

from ._lib import SvdwError

__all__ = ["read_srs", "default_secret", "gen_srs", "write_srs", "g_to_lagrange", "downsize"]

_G2_BYTES = 2 * 128
_Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583
_R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
_MONT = 1 << 256
# The generator of G2 on the twist y^2 = x^3 + 3 / (9 + u), as (c0, c1) pairs (EIP-197's P2).
_G2 = ((10857046999023057135944570762232829481370756359578518086990519993285655852781,
        11559732032986387107991004021392285783925812861821192530917403151452391805634),
       (8495653923123431417604973247489272438418190587263600148770280649306958101930,
        4082367875863433681332203403145435568316851327593401208105741076214120093531))


def read_srs(path) -> dict:
    """{"k", "g", "g_lagrange", "g2"}: the two arrays as [2^k, 64] u8 views of the
    file's bytes and its 256 G2 bytes as they are. Raises SvdwError on a
    truncated file or a k that does not fit the file's length."""
    with open(path, "rb") as f:
        raw = f.read()
    if len(raw) < 4:
        raise SvdwError(-1, f"{path}: truncated SRS (no header)")
    k = int.from_bytes(raw[:4], "little")
    if not 1 <= k <= 28 or len(raw) != 4 + 2 * (64 << k) + _G2_BYTES:
        raise SvdwError(-1, f"{path}: k = {k} does not fit a file of {len(raw)} bytes (truncated or not an SRS)")
    a = np.frombuffer(raw, dtype=np.uint8, count=2 * (64 << k), offset=4).reshape(2, 1 << k, 64)
    return {"k": k, "g": a[0], "g_lagrange": a[1], "g2": raw[-_G2_BYTES:]}


def _chacha20_block0() -> bytes:
    """The first 64 bytes of the ChaCha20 key stream (20 rounds) for the zero
    key, the zero nonce and block counter 0."""
    m = 0xffffffff
    init = [0x61707865, 0x3320646e, 0x79622d32, 0x6b206574] + [0] * 12
    x = list(init)

    def quarter(a, b, c, d):
        for add_to, xor_into, other, rot in ((a, d, b, 16), (c, b, d, 12), (a, d, b, 8), (c, b, d, 7)):
            x[add_to] = (x[add_to] + x[other]) & m
            v = x[xor_into] ^ x[add_to]
            x[xor_into] = ((v << rot) | (v >> (32 - rot))) & m

    for _ in range(10):
        for q in ((0, 4, 8, 12), (1, 5, 9, 13), (2, 6, 10, 14), (3, 7, 11, 15),
                  (0, 5, 10, 15), (1, 6, 11, 12), (2, 7, 8, 13), (3, 4, 9, 14)):
            quarter(*q)
    return b"".join(((a + b) & m).to_bytes(4, "little") for a, b in zip(x, init))


def default_secret() -> int:
    """The secret of halo2-base's gen_srs: Fr::random of
    ChaCha20Rng::from_seed([0; 32]), which reads the stream's first 64 bytes as a
    512-bit little-endian integer and reduces it mod r (Fr::from_u512)."""
    return int.from_bytes(_chacha20_block0(), "little") % _R


# ---- G2 on the host: Fq2 elements are (c0, c1) pairs of ints, points affine pairs of them or None
def _f2_mul(a, b):
    return (a[0] * b[0] - a[1] * b[1]) % _Q, (a[0] * b[1] + a[1] * b[0]) % _Q


def _f2_sub(a, b):
    return (a[0] - b[0]) % _Q, (a[1] - b[1]) % _Q


def _f2_inv(a):
    d = pow(a[0] * a[0] + a[1] * a[1], -1, _Q)
    return a[0] * d % _Q, -a[1] * d % _Q


def _g2_add(p, q):
    if p is None:
        return q
    if q is None:
        return p
    if p[0] == q[0]:
        if p[1] != q[1]:
            return None
        xx = _f2_mul(p[0], p[0])
        lam = _f2_mul((3 * xx[0] % _Q, 3 * xx[1] % _Q), _f2_inv((2 * p[1][0] % _Q, 2 * p[1][1] % _Q)))
    else:
        lam = _f2_mul(_f2_sub(q[1], p[1]), _f2_inv(_f2_sub(q[0], p[0])))
    x = _f2_sub(_f2_sub(_f2_mul(lam, lam), p[0]), q[0])
    return x, _f2_sub(_f2_mul(lam, _f2_sub(p[0], x)), p[1])


def _g2_mul(p, s: int):
    acc = None
    for bit in bin(s % _R)[2:] if s % _R else "":
        acc = _g2_add(acc, acc)
        if bit == "1":
            acc = _g2_add(acc, p)
    return acc


def _g2_bytes(p) -> bytes:
    if p is None:
        return bytes(128)
    return b"".join((c * _MONT % _Q).to_bytes(32, "little") for f in p for c in f)


def _point_array(what: str, a, rows: int) -> bytes:
    if not isinstance(a, np.ndarray):
        a = a.cpu().numpy()                                # a device tensor
    if a.dtype != np.uint8 or a.shape != (rows, 64):
        raise SvdwError(-1, f"{what} must be [2^k, 64] uint8")
    return np.ascontiguousarray(a).tobytes()


def gen_srs(ctx, k: int, s=None) -> dict:
    """{"k", "g", "g_lagrange", "s"}: what halo2-base's gen_srs(k) makes when no
    file exists, for the secret s (None: default_secret()). The arrays are
    [2^k, 64] u8 device tensors in Montgomery form, ready for
    Context.commit_coeffs / commit_lagrange."""
    s = default_secret() if s is None else int(s)
    g, gl, _ = ctx.srs_setup(k, s)
    return {"k": k, "g": g, "g_lagrange": gl, "s": s}


def g_to_lagrange(ctx, g, k=None):
    """ParamsKZG's g_to_lagrange on the device: the Lagrange form of the first
    2^k points of g, a [2^k, 64] u8 device tensor in Montgomery form
    (Context.g1_fft, inverse). g: a [>= 2^k, 64] u8 device tensor or numpy array
    in Montgomery form; k None: all of g, whose length must be a power of two."""
    import torch
    if not isinstance(g, (np.ndarray, torch.Tensor)) or len(g.shape) != 2:
        raise SvdwError(-1, "g must be a [rows, 64] uint8 device tensor or numpy array")
    if k is None:
        k = max(int(g.shape[0]).bit_length() - 1, 0)
        if g.shape[0] != 1 << k:
            raise SvdwError(-1, f"g has {g.shape[0]} points, not a power of two: give k")
    k = int(k)
    if not 1 <= k <= 28:
        raise SvdwError(-2, f"k = {k} is outside 1..28")
    if g.shape[0] < 1 << k:
        raise SvdwError(-2, f"k = {k} needs {1 << k} points, g has {g.shape[0]}")
    g = g[:1 << k]
    if isinstance(g, np.ndarray):                          # (a copy: read_srs's views are read-only)
        g = torch.from_numpy(np.array(g)).to(torch.device("cuda", ctx.device))
    out, _ = ctx.g1_fft(g.contiguous(), k, inverse=True)
    return out


def downsize(ctx, srs: dict, k: int) -> dict:
    """ParamsKZG::downsize(k) of read_srs's or gen_srs's dict: g[:2^k], the
    recomputed g_lagrange (a device tensor) and the new k; "s" and "g2" are
    carried through. Raises SvdwError when k exceeds the dict's k."""
    k = int(k)
    if not 1 <= k <= int(srs["k"]):
        raise SvdwError(-2, f"k = {k} is outside 1..{int(srs['k'])}, the SRS's size")
    out = {key: srs[key] for key in ("s", "g2") if key in srs}
    out.update(k=k, g=srs["g"][:1 << k], g_lagrange=g_to_lagrange(ctx, srs["g"], k))
    return out


def write_srs(path, srs: dict) -> None:
    """Write {"k", "g", "g_lagrange"} and "s" or "g2" (gen_srs's, read_srs's or
    downsize's result; the arrays device tensors or numpy arrays in Montgomery
    form) as ParamsKZG::write does: u32 k, g, g_lagrange, the G2 generator and
    [s] G2. With "s" the G2 half is computed from it; without, the 256 bytes of
    "g2" are written back unchanged (a ceremony's file, whose secret nobody
    has); with neither it raises."""
    k = int(srs["k"])
    if not 1 <= k <= 28:
        raise SvdwError(-2, f"k = {k} is outside 1..28")
    if srs.get("s") is not None:
        s = int(srs["s"])
        if not 0 <= s < _R:
            raise SvdwError(-1, "s must be in [0, r)")
        g2 = None
    elif srs.get("g2") is not None:
        g2 = bytes(srs["g2"])
        if len(g2) != _G2_BYTES:
            raise SvdwError(-1, f"g2 must be the {_G2_BYTES} bytes of two G2 points")
    else:
        raise SvdwError(-1, 'write_srs needs the secret "s" or the G2 bytes "g2"')
    body = _point_array("g", srs["g"], 1 << k) + _point_array("g_lagrange", srs["g_lagrange"], 1 << k)
    if g2 is None:
        g2 = _g2_bytes(_G2) + _g2_bytes(_g2_mul(_G2, s))
    with open(path, "wb") as f:
        f.write(k.to_bytes(4, "little") + body + g2)
