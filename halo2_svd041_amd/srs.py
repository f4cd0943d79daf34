"""Read a KZG structured reference string as halo2_proofs' ParamsKZG writes it.

Layout (pinned by tests/golden/kzg_bn254_8.srs): u32 k little endian, 2^k x 64 B
`g` (the powers of tau in G1), 2^k x 64 B `g_lagrange` (the same in the Lagrange
basis of the size-2^k domain), then 2 x 128 B of G2, which is not parsed. A point
is x then y, each a 32-byte little-endian Fq in Montgomery form: halo2curves'
in-memory G1Affine, which is `bases_form="montgomery"` of Context.commit.
"""
from __future__ import annotations

import numpy as np

from ._lib import SvdwError

__all__ = ["read_srs"]

_G2_BYTES = 2 * 128


def read_srs(path) -> dict:
    """{"k", "g", "g_lagrange"}: the two arrays as [2^k, 64] u8 views of the
    file's bytes. Raises SvdwError on a truncated file or a k that does not fit
    the file's length."""
    with open(path, "rb") as f:
        raw = f.read()
    if len(raw) < 4:
        raise SvdwError(-1, f"{path}: truncated SRS (no header)")
    k = int.from_bytes(raw[:4], "little")
    if not 1 <= k <= 28 or len(raw) != 4 + 2 * (64 << k) + _G2_BYTES:
        raise SvdwError(-1, f"{path}: k = {k} does not fit a file of {len(raw)} bytes (truncated or not an SRS)")
    a = np.frombuffer(raw, dtype=np.uint8, count=2 * (64 << k), offset=4).reshape(2, 1 << k, 64)
    return {"k": k, "g": a[0], "g_lagrange": a[1]}
