"""Host-side mirror of the reference's ZkMatrix / ZkVector / SVD API.

Same names and argument meaning as the Rust reference (src/matrix/mod.rs,
src/svd/mod.rs); every call goes through the C ABI (include/svdw.h) into the
gfx950 kernels. Where the reference panics on a shape mismatch, these raise
`SvdwError(SVDW_EINVAL)`.

    ctx = Context(device=0, precision_bits=63, lookup_bits=19)
    m = ZkMatrix.new(ctx, m_f64); u = ZkMatrix.new(ctx, u_f64); ...
    payload = check_svd_phase0(ctx, m, u, v, d, err_svd, err_u, 30)
    check_svd_phase1(ctx, m, u, v, payload, gamma)
    cells = ctx.advice(0)            # (n, 4) uint64 canonical Fr, like Fr::to_repr
"""
from __future__ import annotations

import collections
import ctypes as ct
from dataclasses import dataclass
from typing import Optional

import numpy as np

from ._lib import (CheckResult, CommitCheck, CommitResult, EqCheck, FixedBaseResult, G1FftResult, G1MulResult, LagrangeCheck, OpenCheck, OpenResult, LookupCheck, LookupProductCheck, LookupProductResult, LookupResult, NttCheck, NttResult, PermutationCyclesResult, PermutationLayout, PermutationMappingCheck, PermutationProductCheck, PermutationProductResult, PhysParams, QuotientArgs, QuotientCheck, QuotientResult, Counts, DivScale, InputDims, KStat, Mat, Params, Payload, Region, Segment, SvdConfig, SvdInfo, SvdOpts, SrsCheck, SrsResult, SvdwError,
                   Vec, check, lib)

P_MOD = 21888242871839275222246405745257275088548364400416034343698204186575808495617

__all__ = ["Context", "ZkMatrix", "ZkVector", "honest_prover_mat_mul", "field_mat_vec_mul",
           "mat_times_diag_mat", "check_mat_diff", "check_mat_id", "check_mat_entries_bounded",
           "check_svd_phase0", "check_svd_phase1", "err_calc", "svd_witness", "svd_decompose", "plan_svd",
           "SvdwError", "SvdPayload", "SvdConfigPy", "P_MOD", "int_to_words", "words_to_int",
           "fr_convert", "quantization", "dequantization", "format_f64_debug", "permutation_constants",
           "commit_plan", "shplonk_queries"]


def int_to_words(x: int) -> np.ndarray:
    x = int(x)
    if x < 0:
        raise ValueError("expected a non-negative integer")
    return np.array([(x >> (64 * i)) & ((1 << 64) - 1) for i in range(4)], dtype=np.uint64)


_M64 = (1 << 64) - 1


def _words_arg(x: int):
    """x mod p as the 4-word little-endian argument of the C calls (a ctypes
    array: no numpy round trip on the per-witness path)."""
    x = int(x) % P_MOD
    return (ct.c_uint64 * 4)(x & _M64, (x >> 64) & _M64, (x >> 128) & _M64, x >> 192)


def _challenge_arg(x: int):
    """A challenge in [0, p) as the 4-word argument; unlike _words_arg it is not
    reduced: a value outside the field is the caller's mistake."""
    x = int(x)
    if not 0 <= x < P_MOD:
        raise SvdwError(-1, "challenge must be in [0, p)")
    return (ct.c_uint64 * 4)(x & _M64, (x >> 64) & _M64, (x >> 128) & _M64, x >> 192)


def words_to_int(w) -> int:
    w = [int(v) for v in w]
    return w[0] | (w[1] << 64) | (w[2] << 128) | (w[3] << 192)


FORMS = {"canonical": 0, "montgomery": 1}


def _form(form) -> int:
    try:
        return FORMS[form]
    except KeyError:
        raise SvdwError(-1, f"unknown form {form!r} (canonical or montgomery)") from None


def fr_convert(values, from_: str, to: str) -> np.ndarray:
    """Field elements between the canonical (Fr::to_repr) and Montgomery
    (halo2curves' in-memory [u64; 4], x * 2^256 mod p) forms on the host
    (svdw_fr_convert): `values` is an (n, 4) uint64 array or a sequence of
    ints; returns (n, 4) uint64. A value >= p raises SVDW_EINVAL."""
    if isinstance(values, np.ndarray):
        a = np.ascontiguousarray(values, dtype=np.uint64).reshape(-1, 4)
    else:
        a = np.array([int_to_words(v) for v in values], dtype=np.uint64).reshape(-1, 4)
    out = np.empty_like(a)
    check(lib().svdw_fr_convert(a.ctypes.data, a.shape[0], _form(from_), _form(to), out.ctypes.data))
    return out


def permutation_constants(k: int):
    """(delta, omega_k) of BN254 Fr as ints: delta = 7^(2^28), omega_k =
    7^((p - 1) / 2^k) generates the 2^k rows (svdw_permutation_constants)."""
    d, w = (ct.c_uint64 * 4)(), (ct.c_uint64 * 4)()
    check(lib().svdw_permutation_constants(k, d, w))
    return words_to_int(d), words_to_int(w)


def commit_plan(k: int) -> tuple:
    """(window_bits, windows) of a size-2^k commitment (svdw_commit_plan)."""
    c, w = ct.c_uint32(), ct.c_uint32()
    lib().svdw_commit_plan(k, ct.byref(c), ct.byref(w))
    return c.value, w.value


def shplonk_queries(k: int, unusable_rows: int, n_gate: int, n_perm: int, chunk_len: int, n_lookup: int, x: int):
    """(set_of, sets): the rotation sets of the SHPLONK opening at x for the
    circuit shape svdw_quotient_args describes, as Context.open_quotient takes
    them. Host only. The columns, in this order: advice [n_gate], selectors
    [n_gate], sigma [n_perm], lookup_input A [n_lookup], lookup_table [n_lookup],
    perm_z [ceil(n_perm / chunk_len)], lookup_z [n_lookup], permuted_input A'
    [n_lookup], permuted_table S' [n_lookup], then the combined h (one column:
    the pieces of h folded by linear_combination). Their rotations: advice
    {0, 1, 2, 3}; selectors, sigma, A, the lookup table, S' and h {0}; a
    permutation Z {0, 1, usable}, the last one {0, 1}; a lookup Z {0, 1}; A'
    {0, -1}. (perm_columns names no polynomial of its own: the v_j are advice
    and lookup input columns, opened once.) Families with
    equal rotations share a set, sets are numbered in the order in which the
    columns first need them, and a point of rotation r is x omega_k^r
    (usable = 2^k - unusable_rows, -1 = 2^k - 1). set_of: one set index per
    column; sets: one list of points (ints) per set."""
    n = 1 << k
    if not 0 < unusable_rows < n:
        raise SvdwError(-2, "shplonk_queries: unusable_rows must be in [1, 2^k)")
    if n_perm and chunk_len < 1:
        raise SvdwError(-1, "shplonk_queries: chunk_len == 0")
    x = int(x)
    if not 0 <= x < P_MOD:
        raise SvdwError(-1, "shplonk_queries: x must be in [0, p)")
    _, w = permutation_constants(k)
    usable = n - unusable_rows
    n_z = -(-n_perm // chunk_len) if n_perm else 0
    families = ([(0, 1, 2, 3)] * n_gate + [(0,)] * (n_gate + n_perm + 2 * n_lookup) + [(0, 1, usable)] * max(n_z - 1, 0)
                + [(0, 1)] * (min(n_z, 1) + n_lookup) + [(0, n - 1)] * n_lookup + [(0,)] * (n_lookup + 1))
    index, set_of = {}, []
    for rot in families:
        set_of.append(index.setdefault(rot, len(index)))
    return set_of, [[x * pow(w, r, P_MOD) % P_MOD for r in rot] for rot in index]


def quantization(x: float, precision_bits: int) -> int:
    """FixedPointChip041::quantization of one f64 (svdw_quantization)."""
    w = (ct.c_uint64 * 4)()
    check(lib().svdw_quantization(float(x), precision_bits, w))
    return words_to_int(w)


def dequantization(value: int, precision_bits: int) -> float:
    """FixedPointChip041::dequantization of one field element
    (svdw_dequantization; parity unpinned, include/svdw.h)."""
    out = ct.c_double()
    check(lib().svdw_dequantization(_words_arg(value), precision_bits, ct.byref(out)))
    return out.value


def format_f64_debug(x: float) -> str:
    """Rust's `{:?}` of an f64: the shortest digits that round-trip, always
    with a fractional part (1.0), exponent form below 1e-5 and from 1e16 on."""
    x = float(x)
    if x != x:
        return "NaN"
    if x in (float("inf"), float("-inf")):
        return "inf" if x > 0 else "-inf"
    sign = "-" if np.signbit(x) else ""
    if x == 0:
        return sign + "0.0"
    import decimal
    _, dig, exp = decimal.Decimal(repr(abs(x))).as_tuple()      # repr: shortest round-trip digits
    digits = "".join(map(str, dig)).lstrip("0")
    stripped = digits.rstrip("0")
    exp += len(digits) - len(stripped)
    digits = stripped
    e10 = len(digits) - 1 + exp                                  # x = d.ddd * 10^e10
    if abs(x) < 1e-5 or abs(x) >= 1e16:
        frac = "." + digits[1:] if len(digits) > 1 else ""
        return f"{sign}{digits[0]}{frac}e{e10}"
    if exp >= 0:
        return sign + digits + "0" * exp + ".0"
    if -exp < len(digits):
        return sign + digits[:exp] + "." + digits[exp:]
    return sign + "0." + "0" * (-exp - len(digits)) + digits


_torch = None


def _torch_mod():
    global _torch
    if _torch is None:
        import torch  # noqa: WPS433
        _torch = torch
    return _torch


def _device_ptr(a) -> Optional[int]:
    """torch CUDA tensor -> device pointer (float64, contiguous) or None."""
    if isinstance(a, np.ndarray):
        return None
    try:
        torch = _torch_mod()
    except ImportError:  # pragma: no cover
        return None
    if isinstance(a, torch.Tensor) and a.is_cuda:
        if a.dtype != torch.float64 or not a.is_contiguous():
            raise SvdwError(-1, "device input must be a contiguous float64 tensor")
        return a.data_ptr()
    return None


def _torch_stream(ctx: "Context") -> int:
    """torch's current stream on the context's device (hipStream_t as int)."""
    t = _torch_mod()
    raw = getattr(t._C, "_cuda_getCurrentRawStream", None)   # no Stream object per call
    if raw is not None:
        return raw(ctx.device)
    return t.cuda.current_stream(ctx.device).cuda_stream


def _after_torch(ctx: "Context") -> None:
    """The engine's streams wait (on the device) for work torch has queued on
    its current stream: tensors it is still writing, memory it still reads."""
    check(lib().svdw_stream_wait(ctx.handle, _torch_stream(ctx)))


def _before_torch(ctx: "Context") -> None:
    """torch's current stream waits for the engine's queued work (its outputs)."""
    check(lib().svdw_stream_signal(ctx.handle, _torch_stream(ctx)))


# svdw_set_option names that change the cell layout (not just the schedule)
LAYOUT_OPTIONS = ("rlc_prefix",)


class Context:
    """One engine context = the phase-0 and phase-1 halo2-base `Context`s of a
    circuit (examples/svd_example.rs:108,181), streams resident on `device`."""

    def __init__(self, device: int = 0, precision_bits: int = 32, lookup_bits: int = 19):
        self.precision_bits = precision_bits
        self.lookup_bits = lookup_bits
        self.device = device
        self._phys = None
        self.last_svd = None
        self.layout_opts = {}
        self._h = ct.c_void_p()
        # device input tensors whose reads may still be queued (include/svdw.h,
        # "Lifetime of device inputs"): id -> [tensor, sequence number of the
        # last call that read it], kept until a completion mark at or after that call
        # has completed, so torch's allocator cannot hand their memory to a
        # tensor written on another stream while a pipelined call still reads it
        self._held = {}
        self._seq = 0
        self._ckpts = collections.deque()      # (call sequence number, svdw_mark ticket)
        p = Params(device, precision_bits, lookup_bits)
        check(lib().svdw_ctx_create(ct.byref(p), ct.byref(self._h)))

    # Per-call completion, at a cost amortised over calls: every HOLD_EVERY-th
    # call that holds inputs records a completion mark (svdw_mark: an event on
    # each of the context's streams, no waits); a held tensor is released once
    # a mark at or after its last reader has completed. At most HOLD_CKPTS
    # marks are pending: beyond that the oldest is waited for. So back-to-back
    # calls on fresh tensors hold the inputs of at most
    # HOLD_EVERY * (HOLD_CKPTS + 1) calls, whatever the device's progress, and
    # each call costs one dict update plus an event query. (The marks replaced
    # a side stream ordered after the context by svdw_stream_signal: with 4
    # hardware queues per process that stream shared one with a context stream,
    # whose next call then waited behind it -- 3.5 % of a 512^2 step.)
    HOLD_EVERY = 8
    HOLD_CKPTS = 4

    def _hold(self, *tensors) -> None:
        """Keep device inputs alive until the calls reading them have run (see _held)."""
        self._seq += 1
        seq = self._seq
        held = self._held
        for t in tensors:
            held[id(t)] = [t, seq]
        ck = self._ckpts
        done = 0
        while ck:
            s0, ticket = ck[0]
            if len(ck) > self.HOLD_CKPTS:
                check(lib().svdw_mark_wait(self._h, ticket))
            else:
                rc = lib().svdw_mark_done(self._h, ticket)
                if rc < 0:
                    check(rc)
                if rc != 1:
                    break
            ck.popleft()
            done = s0
        if done:
            for k in [k for k, (_, s) in held.items() if s <= done]:
                del held[k]
        if seq % self.HOLD_EVERY == 0:
            ticket = ct.c_uint64(0)
            check(lib().svdw_mark(self._h, ct.byref(ticket)))
            ck.append((seq, ticket.value))

    def _release_all(self) -> None:
        self._held.clear()
        self._ckpts.clear()

    def close(self) -> None:
        if self._h:
            lib().svdw_ctx_destroy(self._h)      # (waits for the context's work)
            self._h = ct.c_void_p()
        self._release_all()

    def __del__(self):  # pragma: no cover - best effort
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def handle(self):
        return self._h

    def reset(self) -> None:
        check(lib().svdw_ctx_reset(self._h))     # (synchronises)
        self._release_all()

    def reserve(self, phase: int, advice: int, lookups: int) -> None:
        check(lib().svdw_reserve(self._h, phase, advice, lookups))

    def sync(self) -> None:
        check(lib().svdw_sync(self._h))
        self._release_all()

    def query(self) -> bool:
        """svdw_query: has everything queued on the context completed?"""
        rc = lib().svdw_query(self._h)
        if rc < 0:
            check(rc)
        if rc == 1:
            self._release_all()
        return rc == 1

    def advice_len(self, phase: int) -> int:
        return lib().svdw_advice_len(self._h, phase)

    def lookup_len(self, phase: int) -> int:
        return lib().svdw_lookup_len(self._h, phase)

    def advice_device_ptr(self, phase: int) -> int:
        return lib().svdw_advice_device_ptr(self._h, phase) or 0

    def lookup_device_ptr(self, phase: int) -> int:
        return lib().svdw_lookup_device_ptr(self._h, phase) or 0

    def advice(self, phase: int, off: int = 0, n: Optional[int] = None) -> np.ndarray:
        n = self.advice_len(phase) - off if n is None else n
        out = np.zeros((n, 4), dtype=np.uint64)
        check(lib().svdw_copy_advice(self._h, phase, off, n, out.ctypes.data))
        return out

    def lookups(self, phase: int, off: int = 0, n: Optional[int] = None) -> np.ndarray:
        n = self.lookup_len(phase) - off if n is None else n
        out = np.zeros((n, 4), dtype=np.uint64)
        check(lib().svdw_copy_lookup(self._h, phase, off, n, out.ctypes.data))
        return out

    def cells(self, phase: int, lookup: bool = False, off: int = 0, n: Optional[int] = None,
              form: str = "canonical", device: bool = False):
        """Cells [off, off + n) of a phase's advice (or lookup) stream in `form`
        ("canonical": Fr::to_repr; "montgomery": halo2curves' in-memory
        [u64; 4]), converted on the device. (n, 4) uint64 numpy array
        (svdw_copy_cells), or with device=True a uint8 [n, 32] torch tensor on
        the context's device (svdw_export_cells: queued, no host wait; torch's
        current stream is ordered behind it)."""
        f = _form(form)
        total = self.lookup_len(phase) if lookup else self.advice_len(phase)
        n = total - off if n is None else n
        if n < 0 or off < 0:
            raise SvdwError(-1, "cells: range outside the stream")
        if device:
            torch = _torch_mod()
            out = torch.empty((n, 32), dtype=torch.uint8, device=torch.device("cuda", self.device))
            _after_torch(self)
            check(lib().svdw_export_cells(self._h, phase, int(bool(lookup)), off, n, f, out.data_ptr() or 1))
            _before_torch(self)
            return out
        out = np.zeros((n, 4), dtype=np.uint64)
        check(lib().svdw_copy_cells(self._h, phase, int(bool(lookup)), off, n, f, out.ctypes.data or 1))
        return out

    def set_gemm_impl(self, impl: str) -> None:
        """'mfma' (matrix cores, default) or 'valu' (v_dot4): bit-identical GEMM paths."""
        check(lib().svdw_set_gemm_impl(self._h, {"mfma": 0, "valu": 1}[impl]))

    def set_option(self, name: str, value: int) -> None:
        """Options of svdw_set_option (include/svdw.h). Tuning knobs leave the
        cells bit-identical; the layout options (LAYOUT_OPTIONS) add cells and
        are recorded in `layout_opts`, so a replay of this context's witness
        (collect.plan's dry planner) sees the same layout."""
        check(lib().svdw_set_option(self._h, name.encode(), int(value)))
        if name in LAYOUT_OPTIONS:
            self.layout_opts[name] = int(value)

    def graph_stats(self) -> tuple:
        """(captures, replays) of the captured verify_mul_witness graph
        (svdw_graph_stats; option "graph")."""
        cap, rep = ct.c_uint64(0), ct.c_uint64(0)
        check(lib().svdw_graph_stats(self._h, ct.byref(cap), ct.byref(rep)))
        return cap.value, rep.value

    def set_shard(self, rank: int, world: int) -> None:
        """Row-block sharding of one witness over `world` contexts (svdw_set_shard)."""
        check(lib().svdw_set_shard(self._h, int(rank), int(world)))

    def shard_segments(self) -> list:
        """[(phase, lookup, off, n)] cell ranges this rank is the source of."""
        n = ct.c_uint64()
        check(lib().svdw_shard_segments(self._h, None, 0, ct.byref(n)))
        buf = (Segment * max(n.value, 1))()
        check(lib().svdw_shard_segments(self._h, buf, n.value, ct.byref(n)))
        return [(s.phase, s.lookup, s.off, s.n) for s in buf[:n.value]]

    def layout(self) -> list:
        """Virtual layout of the last witness (svdw_layout): dicts with phase, off,
        n, loff, nl, rows, tag for every appended region, in append order."""
        n = ct.c_uint64()
        check(lib().svdw_layout(self._h, None, 0, ct.byref(n)))
        buf = (Region * max(n.value, 1))()
        check(lib().svdw_layout(self._h, buf, n.value, ct.byref(n)))
        return [{"phase": r.phase, "off": r.off, "n": r.n, "loff": r.loff, "nl": r.nl,
                 "rows": r.rows, "tag": r.tag.decode()} for r in buf[:n.value]]

    def rlc_trace(self) -> Optional[dict]:
        """ctx_rlc of the last svd_witness with rlc_prefix (svdw_rlc_trace;
        parity unpinned): {"cells": (3, 4) uint64, "copies": [(phase, offset)]
        of its two E cells}, or None without the prefix."""
        cells = np.zeros((3, 4), dtype=np.uint64)
        copies = np.zeros(2, dtype=np.uint64)
        n = ct.c_uint32()
        check(lib().svdw_rlc_trace(self._h, cells.ctypes.data, copies.ctypes.data, ct.byref(n)))
        if not n.value:
            return None
        return {"cells": cells, "copies": [(int(c) >> 62, int(c) & ((1 << 62) - 1)) for c in copies]}

    def check_gates(self) -> dict:
        """Device constraint check of the last witness (svdw_check_gates)."""
        r = CheckResult()
        check(lib().svdw_check_gates(self._h, ct.byref(r)))
        return {"gates_checked": r.gates_checked, "gate_failures": r.gate_failures,
                "lookups_checked": r.lookups_checked, "lookup_failures": r.lookup_failures,
                "copies_checked": r.copies_checked, "copy_failures": r.copy_failures}

    def physical_layout(self, k: int, minimum_rows: int = 20) -> dict:
        """Virtual -> physical layout plan of the last witness (svdw_physical_layout)."""
        p = PhysParams()
        check(lib().svdw_physical_layout(self._h, k, minimum_rows, ct.byref(p)))
        self._phys = {"k": p.k, "minimum_rows": p.minimum_rows, "max_rows": p.max_rows,
                "num_advice": list(p.num_advice), "columns_used": list(p.columns_used),
                "num_lookup_advice": list(p.num_lookup_advice), "num_fixed": p.num_fixed,
                "constants": p.constants}
        return dict(self._phys)

    def break_points(self, phase: int) -> list:
        n = ct.c_uint64()
        check(lib().svdw_break_points(self._h, phase, None, 0, ct.byref(n)))
        buf = (ct.c_uint64 * max(n.value, 1))()
        check(lib().svdw_break_points(self._h, phase, buf, n.value, ct.byref(n)))
        return list(buf[:n.value])

    def assign_columns(self, phase: int, device=None, form: str = "canonical"):
        """(advice [cols, 2^k, 32] u8, selectors [cols, 2^k] u8, lookup [nl, 2^k, 32] u8)
        torch tensors on the device, filled by svdw_assign_columns_form: the
        advice and lookup cells in `form` ("canonical" | "montgomery")."""
        import torch
        p = self._phys
        if p is None:
            raise RuntimeError("call physical_layout() after the witness first")
        dev = device or torch.device("cuda", self.device)
        rows = 1 << p["k"]
        nc, nl = p["columns_used"][phase], p["num_lookup_advice"][phase]
        adv = torch.empty((nc, rows, 32), dtype=torch.uint8, device=dev)
        sel = torch.empty((nc, rows), dtype=torch.uint8, device=dev)
        lk = torch.empty((nl, rows, 32), dtype=torch.uint8, device=dev)
        _after_torch(self)
        check(lib().svdw_assign_columns_form(self._h, phase, _form(form), adv.data_ptr() if nc else None,
                                             sel.data_ptr() if nc else None, lk.data_ptr() if nl else None))
        _before_torch(self)
        return adv, sel, lk

    def check_physical(self, phase: int, adv, sel) -> dict:
        r = CheckResult()
        _after_torch(self)
        check(lib().svdw_check_physical(self._h, phase, adv.data_ptr(), sel.data_ptr(), adv.shape[0],
                                        ct.byref(r)))
        return {"gates_checked": r.gates_checked, "gate_failures": r.gate_failures,
                "copies_checked": r.copies_checked, "copy_failures": r.copy_failures}

    def equalities(self, phase: int):
        """Copy-constraint lists of the last witness (svdw_equalities), in assign
        order: copies (n, 3) uint64 [source phase (2: init_rand), source cell,
        destination cell], consts: list of (cell, value int)."""
        nc, nk = ct.c_uint64(), ct.c_uint64()
        check(lib().svdw_equalities(self._h, phase, None, 0, ct.byref(nc), None, 0, ct.byref(nk)))
        cp = np.zeros((max(nc.value, 1), 2), dtype=np.uint64)
        ks = np.zeros((max(nk.value, 1), 5), dtype=np.uint64)
        check(lib().svdw_equalities(self._h, phase, cp.ctypes.data, nc.value, ct.byref(nc),
                                    ks.ctypes.data, nk.value, ct.byref(nk)))
        cp, ks = cp[:nc.value], ks[:nk.value]
        out = np.empty((cp.shape[0], 3), dtype=np.uint64)
        out[:, 0] = cp[:, 0] >> np.uint64(62)
        out[:, 1] = cp[:, 0] & np.uint64((1 << 62) - 1)
        out[:, 2] = cp[:, 1]
        consts = [(int(r[0]), words_to_int(r[1:])) for r in ks]
        return out, consts

    def check_equalities(self, phase: int, columns0=None, columns1=None) -> dict:
        """Device check of the equality records (svdw_check_equalities) on the
        cell streams, or on assigned physical columns (torch tensors)."""
        r = EqCheck()
        p0 = columns0.data_ptr() if columns0 is not None else None
        p1 = columns1.data_ptr() if columns1 is not None else None
        if p0 is not None or p1 is not None:
            _after_torch(self)
        check(lib().svdw_check_equalities(self._h, phase, p0, p1, ct.byref(r)))
        return {"copies_checked": r.copies_checked, "copy_failures": r.copy_failures,
                "consts_checked": r.consts_checked, "const_failures": r.const_failures}

    # ---- lookup argument (include/svdw.h, "lookup argument"; parity unpinned)
    def _lookup_cols(self, phase: int, columns):
        """(pointer, ncols, 2^k, device) of a lookup-argument call's input columns."""
        import torch
        p = self._phys
        if p is None:
            raise RuntimeError("call physical_layout() after the witness first")
        rows = 1 << p["k"]
        if columns is None:
            return None, p["num_lookup_advice"][phase], rows, torch.device("cuda", self.device)
        if (not columns.is_cuda or columns.dtype != torch.uint8 or not columns.is_contiguous()
                or columns.dim() != 3 or tuple(columns.shape[1:]) != (rows, 32)):
            raise SvdwError(-1, "columns must be a contiguous uint8 device tensor [n, 2^k, 32]")
        return (columns.data_ptr() if columns.shape[0] else None), columns.shape[0], rows, columns.device

    def lookup_multiplicities(self, phase: int, unusable_rows: int = 6, columns=None):
        """[nl, 2^lookup_bits] int32 device tensor: how often each table value occurs
        in the usable rows of each lookup column (svdw_lookup_multiplicities).
        columns: None (the lookup stream of `phase` through the physical layout)
        or canonical columns [n, 2^k, 32] u8, e.g. assign_columns(...)[2]."""
        import torch
        ptr, nl, _, dev = self._lookup_cols(phase, columns)
        mult = torch.empty((nl, 1 << self.lookup_bits), dtype=torch.int32, device=dev)
        _after_torch(self)
        check(lib().svdw_lookup_multiplicities(self._h, phase, unusable_rows, ptr, nl,
                                               mult.data_ptr() if nl else None))
        _before_torch(self)
        return mult

    def lookup_permute(self, phase: int, unusable_rows: int = 6, form: str = "canonical", columns=None,
                       out=None):
        """(A', S', result): the permuted input and table columns of the lookup
        argument, [nl, 2^k, 32] u8 device tensors in `form`, rows >= 2^k -
        unusable_rows zero (svdw_lookup_permute). result: columns, usable_rows,
        out_of_table, distinct; with out_of_table > 0 the tensors are left as
        allocated (or as `out` = (A', S') held them)."""
        import torch
        ptr, nl, rows, dev = self._lookup_cols(phase, columns)
        if out is None:
            out = (torch.empty((nl, rows, 32), dtype=torch.uint8, device=dev),
                   torch.empty((nl, rows, 32), dtype=torch.uint8, device=dev))
        a, s = out
        for t in (a, s):
            if (not t.is_cuda or t.dtype != torch.uint8 or not t.is_contiguous()
                    or tuple(t.shape) != (nl, rows, 32)):
                raise SvdwError(-1, "out must be two contiguous uint8 device tensors [n, 2^k, 32]")
        r = LookupResult()
        _after_torch(self)
        check(lib().svdw_lookup_permute(self._h, phase, unusable_rows, _form(form), ptr, nl,
                                        a.data_ptr() if nl else None, s.data_ptr() if nl else None,
                                        ct.byref(r)))
        _before_torch(self)
        return a, s, {"columns": r.columns, "usable_rows": r.usable_rows,
                      "out_of_table": r.out_of_table, "distinct": r.distinct}

    def check_lookup_argument(self, phase: int, permuted_input, permuted_table, unusable_rows: int = 6,
                              form: str = "canonical", columns=None) -> dict:
        """Device check of the lookup argument's constraints on (A', S') in `form`
        (svdw_check_lookup_argument): checked / failure counts of the adjacency,
        multiset and padding conditions."""
        ptr, nl, rows, _ = self._lookup_cols(phase, columns)
        for t in (permuted_input, permuted_table):
            if not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != (nl, rows, 32):
                raise SvdwError(-1, "permuted columns must be contiguous uint8 device tensors [n, 2^k, 32]")
        r = LookupCheck()
        _after_torch(self)
        check(lib().svdw_check_lookup_argument(self._h, phase, unusable_rows, _form(form), ptr, nl,
                                               permuted_input.data_ptr() if nl else None,
                                               permuted_table.data_ptr() if nl else None, ct.byref(r)))
        return {k: getattr(r, k) for k, _ in LookupCheck._fields_}

    def lookup_product(self, phase: int, permuted_input, permuted_table, beta: int, gamma: int,
                       unusable_rows: int = 6, form: str = "canonical", columns=None, out=None):
        """(Z, result): the lookup argument's grand-product column for the
        challenges beta, gamma (ints below p) from (A', S') of lookup_permute in
        the same `form`, a [nl, 2^k, 32] u8 device tensor in that form: Z[0] = 1,
        Z[usable] = 1 for honest columns, rows above zero (svdw_lookup_product).
        result: columns, usable_rows, zero_denominators, final_not_one."""
        import torch
        b, g = _challenge_arg(beta), _challenge_arg(gamma)
        ptr, nl, rows, dev = self._lookup_cols(phase, columns)
        for t in (permuted_input, permuted_table):
            if (not t.is_cuda or t.dtype != torch.uint8 or not t.is_contiguous()
                    or tuple(t.shape) != (nl, rows, 32)):
                raise SvdwError(-1, "permuted columns must be contiguous uint8 device tensors [n, 2^k, 32]")
        if out is None:
            out = torch.empty((nl, rows, 32), dtype=torch.uint8, device=dev)
        if (not out.is_cuda or out.dtype != torch.uint8 or not out.is_contiguous()
                or tuple(out.shape) != (nl, rows, 32)):
            raise SvdwError(-1, "out must be a contiguous uint8 device tensor [n, 2^k, 32]")
        r = LookupProductResult()
        _after_torch(self)
        check(lib().svdw_lookup_product(self._h, phase, unusable_rows, _form(form), ptr, nl,
                                        permuted_input.data_ptr() if nl else None,
                                        permuted_table.data_ptr() if nl else None, b, g,
                                        out.data_ptr() if nl else None, ct.byref(r)))
        _before_torch(self)
        return out, {"columns": r.columns, "usable_rows": r.usable_rows,
                     "zero_denominators": r.zero_denominators, "final_not_one": r.final_not_one}

    def check_lookup_product(self, phase: int, permuted_input, permuted_table, z, beta: int, gamma: int,
                             unusable_rows: int = 6, form: str = "canonical", columns=None) -> dict:
        """Device check of Z in `form` against (A', S'), the input columns and the
        challenges, division-free (svdw_check_lookup_product): checked / failure
        counts of the recurrence, the boundary rows and the padding."""
        b, g = _challenge_arg(beta), _challenge_arg(gamma)
        ptr, nl, rows, _ = self._lookup_cols(phase, columns)
        import torch
        for t in (permuted_input, permuted_table, z):
            if (not t.is_cuda or t.dtype != torch.uint8 or not t.is_contiguous()
                    or tuple(t.shape) != (nl, rows, 32)):
                raise SvdwError(-1, "permuted columns and z must be contiguous uint8 device tensors [n, 2^k, 32]")
        r = LookupProductCheck()
        _after_torch(self)
        check(lib().svdw_check_lookup_product(self._h, phase, unusable_rows, _form(form), ptr, nl,
                                              permuted_input.data_ptr() if nl else None,
                                              permuted_table.data_ptr() if nl else None, b, g,
                                              z.data_ptr() if nl else None, ct.byref(r)))
        return {k: getattr(r, k) for k, _ in LookupProductCheck._fields_}

    # ---- permutation argument (include/svdw.h, "permutation argument"; parity unpinned)
    def permutation_values(self, k: int, mapping=None, first_col: int = 0, ncols: Optional[int] = None,
                           total_cols: Optional[int] = None, form: str = "canonical"):
        """(sigma, out_of_range): [ncols, 2^k, 32] u8 device cells delta^col omega^row
        in `form` (svdw_permutation_values). mapping: an int64 device tensor
        [ncols, 2^k] of col << 32 | row entries, the cell each (column, row) maps
        to, or None for the identity of the columns first_col .. first_col + ncols.
        total_cols defaults to first_col + ncols; an entry outside it or outside
        the 2^k rows is written as zero and counted."""
        import torch
        rows = 1 << k if 0 <= k < 32 else 0
        if mapping is not None:
            if (not mapping.is_cuda or mapping.dtype != torch.int64 or not mapping.is_contiguous()
                    or mapping.dim() != 2 or mapping.shape[1] != rows):
                raise SvdwError(-1, "mapping must be a contiguous int64 device tensor [n, 2^k]")
            if ncols is not None and ncols != mapping.shape[0]:
                raise SvdwError(-1, "ncols differs from the mapping's columns")
            ncols = mapping.shape[0]
        elif ncols is None:
            raise SvdwError(-1, "ncols is required without a mapping")
        if total_cols is None:
            total_cols = first_col + ncols
        dev = mapping.device if mapping is not None else torch.device("cuda", self.device)
        out = torch.empty((ncols, rows, 32), dtype=torch.uint8, device=dev)
        bad = ct.c_uint64()
        _after_torch(self)
        check(lib().svdw_permutation_values(self._h, k, _form(form),
                                            mapping.data_ptr() if mapping is not None and ncols else None,
                                            first_col, ncols, total_cols, out.data_ptr() if ncols else None,
                                            ct.byref(bad)))
        _before_torch(self)
        return out, bad.value

    @staticmethod
    def _column_pointers(what: str, cols, rows: int):
        """(ctypes array of one device pointer per column, count, device) of a
        tensor [n, 2^k, 32] u8 or a list of such tensors, concatenated in order."""
        import torch
        ptrs, dev = [], None
        for t in ([cols] if isinstance(cols, torch.Tensor) else list(cols)):
            if (not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.uint8 or not t.is_contiguous()
                    or t.dim() != 3 or tuple(t.shape[1:]) != (rows, 32)):
                raise SvdwError(-1, f"{what} must be contiguous uint8 device tensors [n, 2^k, 32]")
            dev = dev or t.device
            ptrs += [t.data_ptr() + i * rows * 32 for i in range(t.shape[0])]
        return (ct.c_void_p * max(len(ptrs), 1))(*ptrs), len(ptrs), dev

    def _permutation_args(self, columns, sigma, k: int):
        rows = 1 << k if 0 <= k < 32 else 0
        cp, n, dev = self._column_pointers("columns", columns, rows)
        sp, ns, _ = self._column_pointers("sigma", sigma, rows)
        if n != ns:
            raise SvdwError(-1, "columns and sigma differ in their number of columns")
        return cp, sp, n, rows, dev

    def permutation_product(self, columns, sigma, beta: int, gamma: int, chunk_len: int, k: int,
                            unusable_rows: int = 6, form: str = "canonical", out=None):
        """(Z, result): the permutation argument's grand-product columns for the
        challenges beta, gamma (ints below p), one per set of chunk_len columns, a
        [nsets, 2^k, 32] u8 device tensor in `form`: Z_0[0] = 1, each set starts
        where the one before ended, the last Z[usable] = 1 for an honest sigma,
        rows above zero (svdw_permutation_product). columns, sigma: a tensor
        [n, 2^k, 32] u8 in `form` or a list of such tensors, concatenated in order.
        result: columns, sets, usable_rows, zero_denominators, final_not_one."""
        import torch
        b, g = _challenge_arg(beta), _challenge_arg(gamma)
        cp, sp, n, rows, dev = self._permutation_args(columns, sigma, k)
        nsets = -(-n // chunk_len) if chunk_len > 0 else 0
        if out is None:
            out = torch.empty((nsets, rows, 32), dtype=torch.uint8, device=dev or torch.device("cuda", self.device))
        if (not out.is_cuda or out.dtype != torch.uint8 or not out.is_contiguous()
                or tuple(out.shape) != (nsets, rows, 32)):
            raise SvdwError(-1, "out must be a contiguous uint8 device tensor [nsets, 2^k, 32]")
        r = PermutationProductResult()
        _after_torch(self)
        check(lib().svdw_permutation_product(self._h, k, unusable_rows, _form(form), cp, sp, n, chunk_len, b, g,
                                             out.data_ptr() if nsets else None, ct.byref(r)))
        _before_torch(self)
        return out, {"columns": r.columns, "sets": r.sets, "usable_rows": r.usable_rows,
                     "zero_denominators": r.zero_denominators, "final_not_one": r.final_not_one}

    def check_permutation_product(self, columns, sigma, z, beta: int, gamma: int, chunk_len: int, k: int,
                                  unusable_rows: int = 6, form: str = "canonical") -> dict:
        """Device check of Z in `form` against the columns, sigma and the
        challenges, division-free (svdw_check_permutation_product): checked /
        failure counts of the recurrence, the chain and boundary rows and the
        padding."""
        import torch
        b, g = _challenge_arg(beta), _challenge_arg(gamma)
        cp, sp, n, rows, _ = self._permutation_args(columns, sigma, k)
        nsets = -(-n // chunk_len) if chunk_len > 0 else 0
        if (not isinstance(z, torch.Tensor) or not z.is_cuda or z.dtype != torch.uint8 or not z.is_contiguous()
                or tuple(z.shape) != (nsets, rows, 32)):
            raise SvdwError(-1, "z must be a contiguous uint8 device tensor [nsets, 2^k, 32]")
        r = PermutationProductCheck()
        _after_torch(self)
        check(lib().svdw_check_permutation_product(self._h, k, unusable_rows, _form(form), cp, sp, n, chunk_len,
                                                   b, g, z.data_ptr() if nsets else None, ct.byref(r)))
        return {k_: getattr(r, k_) for k_, _ in PermutationProductCheck._fields_}

    def _cycles_args(self, edges, k: int, total_cols: int):
        """(edge pointer, edge count, 2^k) of a [n, 2] int64 device edge list."""
        import torch
        if (not isinstance(edges, torch.Tensor) or not edges.is_cuda or edges.dtype != torch.int64
                or not edges.is_contiguous() or edges.dim() != 2 or edges.shape[1] != 2):
            raise SvdwError(-1, "edges must be a contiguous int64 device tensor [n, 2]")
        rows = 1 << k if 0 <= k < 32 else 0
        return (edges.data_ptr() if edges.shape[0] else None), edges.shape[0], rows

    def permutation_cycles(self, edges, k: int, total_cols: int, unusable_rows: int = 6, out=None):
        """(mapping, result): sigma's mapping from the copy constraints, an int64
        device tensor [total_cols, 2^k] of col << 32 | row entries, as
        permutation_values takes it (svdw_permutation_cycles): the cells of every
        connected component of the edges over the rows below 2^k -
        unusable_rows, linked in ascending (col, row) into one cycle; every other
        cell maps to itself. edges: an int64 device tensor [n, 2] of col << 32 |
        row cells. result: cells, edges, out_of_range, self_edges, classes,
        linked_cells, largest_class, sort_passes."""
        import torch
        ep, ne, rows = self._cycles_args(edges, k, total_cols)
        if out is None:
            out = torch.empty((total_cols, rows), dtype=torch.int64, device=edges.device)
        if (not out.is_cuda or out.dtype != torch.int64 or not out.is_contiguous()
                or tuple(out.shape) != (total_cols, rows)):
            raise SvdwError(-1, "out must be a contiguous int64 device tensor [total_cols, 2^k]")
        r = PermutationCyclesResult()
        _after_torch(self)
        check(lib().svdw_permutation_cycles(self._h, k, unusable_rows, total_cols, ep, ne,
                                            out.data_ptr() if out.numel() else None, ct.byref(r)))
        _before_torch(self)
        return out, {k_: getattr(r, k_) for k_, _ in PermutationCyclesResult._fields_ if k_ != "_pad"}

    def check_permutation_mapping(self, edges, mapping, k: int, total_cols: int, unusable_rows: int = 6) -> dict:
        """Device check of a mapping against the rule of permutation_cycles and
        the edges (svdw_check_permutation_mapping): cells_checked,
        not_permutation, order_failures, padding_failures, edges_checked,
        edge_failures, cycles."""
        import torch
        ep, ne, rows = self._cycles_args(edges, k, total_cols)
        if (not isinstance(mapping, torch.Tensor) or not mapping.is_cuda or mapping.dtype != torch.int64
                or not mapping.is_contiguous() or tuple(mapping.shape) != (total_cols, rows)):
            raise SvdwError(-1, "mapping must be a contiguous int64 device tensor [total_cols, 2^k]")
        r = PermutationMappingCheck()
        _after_torch(self)
        check(lib().svdw_check_permutation_mapping(self._h, k, unusable_rows, total_cols, ep, ne,
                                                   mapping.data_ptr() if mapping.numel() else None, ct.byref(r)))
        return {k_: getattr(r, k_) for k_, _ in PermutationMappingCheck._fields_}

    def permutation_layout(self) -> dict:
        """The columns and edge counts of the permutation argument of the last
        witness (svdw_permutation_edges without a list; also on a planning
        context): k, advice [2], fixed, external, total_cols, edges, break_edges,
        copy_edges, const_edges, external_edges, constants."""
        lay = PermutationLayout()
        check(lib().svdw_permutation_edges(self._h, None, 0, ct.byref(lay)))
        d = {k_: getattr(lay, k_) for k_, _ in PermutationLayout._fields_}
        d["advice"] = list(lay.advice)
        return d

    def permutation_edges(self):
        """(edges, layout): the copy constraints of the last witness as an int64
        device tensor [n, 2] of col << 32 | row cells over the columns [advice 0,
        advice 1, fixed, external], in the order include/svdw.h gives
        (svdw_permutation_edges), and the layout dict of permutation_layout."""
        import torch
        lay = self.permutation_layout()
        edges = torch.empty((lay["edges"], 2), dtype=torch.int64, device=torch.device("cuda", self.device))
        out = PermutationLayout()
        _after_torch(self)
        check(lib().svdw_permutation_edges(self._h, edges.data_ptr() if lay["edges"] else None, lay["edges"],
                                           ct.byref(out)))
        _before_torch(self)
        return edges, lay

    def assign_fixed(self, form: str = "canonical"):
        """[num_fixed, 2^k, 32] u8 device cells in `form`: the fixed columns that
        hold the witness's constants, placed as permutation_edges places them
        (svdw_assign_fixed; call permutation_edges first)."""
        import torch
        lay = self.permutation_layout()
        out = torch.empty((lay["fixed"], 1 << lay["k"], 32), dtype=torch.uint8, device=torch.device("cuda", self.device))
        _after_torch(self)
        check(lib().svdw_assign_fixed(self._h, _form(form), out.data_ptr() if lay["fixed"] else None))
        _before_torch(self)
        return out

    def witness_sigma(self, unusable_rows: int = 6, form: str = "canonical"):
        """(sigma, mapping, layout): the permutation columns of the last witness
        over [advice 0, advice 1, fixed, external], [total_cols, 2^k, 32] u8 in
        `form`, from permutation_edges, permutation_cycles and
        permutation_values; an edge out of range raises."""
        edges, lay = self.permutation_edges()
        mapping, res = self.permutation_cycles(edges, lay["k"], lay["total_cols"], unusable_rows)
        if res["out_of_range"]:
            raise SvdwError(-2, f"{res['out_of_range']} copy constraints touch a row >= 2^k - unusable_rows")
        sigma, bad = self.permutation_values(lay["k"], mapping, form=form)
        if bad:
            raise SvdwError(-2, "internal: a mapping entry out of range")
        return sigma, mapping, lay

    # ---- domain transforms (include/svdw.h, "domain transforms"; parity unpinned)
    @staticmethod
    def _shift_arg(shift):
        """None, or a shift in [1, p) as the 4-word argument."""
        if shift is None:
            return None
        if int(shift) == 0:
            raise SvdwError(-1, "shift must be in [1, p)")
        return _challenge_arg(shift)

    def _ntt_args(self, columns, k: int, k_in):
        k_in = k if k_in is None else k_in
        rows_in = 1 << k_in if 0 <= k_in < 32 else 0
        rows = 1 << k if 0 <= k < 32 else 0
        cp, n, dev = self._column_pointers("columns", columns, rows_in)
        return k_in, rows, cp, n, dev

    def ntt(self, columns, k: int, k_in: Optional[int] = None, inverse: bool = False, shift: Optional[int] = None,
            form: str = "canonical", out=None):
        """(out, result): the transform of include/svdw.h's "domain transforms"
        (svdw_ntt) of columns of 2^k_in cells (k_in defaults to k) into a
        [n, 2^k, 32] u8 device tensor in `form`, natural order on both sides.
        Forward: out[j] = sum_i in[i] shift^i omega_k^(i j), the input zero from
        row 2^k_in on; inverse: out[i] = shift^i 2^-k sum_j in[j] omega_k^(-i j).
        columns: a tensor [n, 2^k_in, 32] u8 in `form` or a list of such tensors.
        result: columns, passes, rows_in, rows_out."""
        import torch
        sh = self._shift_arg(shift)
        k_in, rows, cp, n, dev = self._ntt_args(columns, k, k_in)
        if out is None:
            out = torch.empty((n, rows, 32), dtype=torch.uint8, device=dev or torch.device("cuda", self.device))
        if (not out.is_cuda or out.dtype != torch.uint8 or not out.is_contiguous()
                or tuple(out.shape) != (n, rows, 32)):
            raise SvdwError(-1, "out must be a contiguous uint8 device tensor [n, 2^k, 32]")
        r = NttResult()
        _after_torch(self)
        check(lib().svdw_ntt(self._h, k_in, k, _form(form), 1 if inverse else 0, sh, cp, n,
                             out.data_ptr() if n else None, ct.byref(r)))
        _before_torch(self)
        return out, {k_: getattr(r, k_) for k_, _ in NttResult._fields_}

    def lagrange_to_coeff(self, columns, k: int, form: str = "canonical", out=None):
        """EvaluationDomain::lagrange_to_coeff of every column."""
        return self.ntt(columns, k, inverse=True, form=form, out=out)

    def coeff_to_lagrange(self, columns, k: int, form: str = "canonical", out=None):
        """EvaluationDomain::coeff_to_lagrange of every column."""
        return self.ntt(columns, k, form=form, out=out)

    def coeff_to_extended(self, columns, k: int, extended_k: int, zeta: int, form: str = "canonical", out=None):
        """EvaluationDomain::coeff_to_extended: 2^k coefficients to 2^extended_k
        evaluations on the coset zeta * <omega_extended_k>; zeta = Fr::ZETA."""
        return self.ntt(columns, extended_k, k_in=k, shift=zeta, form=form, out=out)

    def extended_to_coeff(self, columns, extended_k: int, zeta_inv: int, form: str = "canonical", out=None):
        """EvaluationDomain::extended_to_coeff: 2^extended_k coset evaluations to
        coefficients (the caller keeps the prefix it needs); zeta_inv = ZETA^2."""
        return self.ntt(columns, extended_k, inverse=True, shift=zeta_inv, form=form, out=out)

    def eval_polynomial(self, columns, k: int, points, form: str = "canonical"):
        """[ncols, npoints, 32] u8 device cells in `form`: the polynomials whose
        2^k coefficients the columns hold, at the points (ints in [0, p)), as
        halo2's eval_polynomial (svdw_eval_polynomial)."""
        import torch
        rows = 1 << k if 0 <= k < 32 else 0
        pts = [_challenge_arg(x) for x in points]
        cp, n, dev = self._column_pointers("columns", columns, rows)
        buf = (ct.c_uint64 * max(4 * len(pts), 1))(*[w for p in pts for w in p])
        out = torch.empty((n, len(pts), 32), dtype=torch.uint8, device=dev or torch.device("cuda", self.device))
        _after_torch(self)
        check(lib().svdw_eval_polynomial(self._h, k, _form(form), cp, n, buf, len(pts),
                                         out.data_ptr() if n and pts else None))
        _before_torch(self)
        return out

    def check_ntt(self, columns, out, k: int, k_in: Optional[int] = None, inverse: bool = False,
                  shift: Optional[int] = None, form: str = "canonical", log_samples: int = 10, seed: int = 0) -> dict:
        """Device check of a transform's `out` against its input columns on
        2^log_samples stratified rows per column, by direct evaluation
        (svdw_check_ntt): rows_checked, row_failures, summed over the columns."""
        import torch
        sh = self._shift_arg(shift)
        k_in, rows, cp, n, _ = self._ntt_args(columns, k, k_in)
        if (not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != torch.uint8
                or not out.is_contiguous() or tuple(out.shape) != (n, rows, 32)):
            raise SvdwError(-1, "out must be a contiguous uint8 device tensor [n, 2^k, 32]")
        r = NttCheck()
        _after_torch(self)
        check(lib().svdw_check_ntt(self._h, k_in, k, _form(form), 1 if inverse else 0, sh, cp, n,
                                   out.data_ptr() if n else None, log_samples, seed & _M64, ct.byref(r)))
        return {"rows_checked": r.rows_checked, "row_failures": r.row_failures}

    # ---- what the G1 methods (commitments, the SRS, G1 transforms) share
    @staticmethod
    def _u8_rows(t, width: int) -> bool:                    # a contiguous [., width] u8 device tensor
        import torch
        return (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()
                and t.dim() == 2 and t.shape[1] == width)

    @classmethod
    def _points_tensor(cls, what: str, t, rows: int, at_least: bool = False, shown: Optional[str] = None):
        # shown: the row count as the message names it, where that is not the number
        if not cls._u8_rows(t, 64) or (t.shape[0] < rows if at_least else t.shape[0] != rows):
            raise SvdwError(-1, f"{what} must be a contiguous uint8 device tensor "
                                f"[{'>= ' if at_least else ''}{shown or rows}, 64]")

    @classmethod
    def _cells_tensor(cls, what: str, t):
        if not cls._u8_rows(t, 32):
            raise SvdwError(-1, f"{what} must be a contiguous uint8 device tensor [n, 32]")

    @staticmethod
    def _result(r) -> dict:                                 # a result struct as a dict, without its padding
        return {name: getattr(r, name) for name, _ in r._fields_ if name != "_pad"}

    # ---- commitments (include/svdw.h, "commitments"; parity unpinned)
    def _commit_args(self, columns, bases, k: int):
        rows = 1 << k if 0 <= k < 32 else 0
        cp, n, dev = self._column_pointers("columns", columns, rows)
        self._points_tensor("bases", bases, rows, shown="2^k")
        return cp, n, dev or bases.device

    def commit(self, columns, bases, k: int, form: str = "canonical", bases_form: str = "montgomery", out=None):
        """(points, result): the KZG commitments sum_i s_i P_i of columns of 2^k
        cells in `form` over the 2^k G1 bases (svdw_commit), a [ncols, 64] u8
        device tensor of affine points (x, y; (0, 0) the identity) in bases_form.
        bases: a [2^k, 64] u8 device tensor in bases_form; "montgomery" is what
        srs.read_srs returns. columns: a tensor [n, 2^k, 32] u8 or a list of such
        tensors, so h_coeffs.view(E, 2**k, 32) commits the E pieces of h of
        2^k coefficients each in one call. result: columns, window_bits,
        windows, rows, zero_scalars, identity_bases, identity_outputs."""
        import torch
        cp, n, dev = self._commit_args(columns, bases, k)
        if out is None:
            out = torch.empty((n, 64), dtype=torch.uint8, device=dev)
        self._points_tensor("out", out, n, shown="ncols")
        r = CommitResult()
        _after_torch(self)
        check(lib().svdw_commit(self._h, k, _form(form), _form(bases_form), bases.data_ptr(), cp, n,
                                out.data_ptr() if n else None, ct.byref(r)))
        _before_torch(self)
        return out, self._result(r)

    def commit_lagrange(self, columns, g_lagrange, k: int, form: str = "canonical", out=None):
        """ParamsKZG::commit_lagrange of every column (cells in Lagrange form) on
        the SRS's g_lagrange as read_srs returns it. No blinding term: as far as
        recalled the reference ignores its Blind argument (unpinned)."""
        return self.commit(columns, g_lagrange, k, form=form, out=out)

    def commit_coeffs(self, columns, g, k: int, form: str = "canonical", out=None):
        """ParamsKZG::commit of every column (cells in coefficient form) on the
        SRS's g as read_srs returns it; the blinding note of commit_lagrange holds."""
        return self.commit(columns, g, k, form=form, out=out)

    def check_commit(self, columns, bases, commitments, k: int, form: str = "canonical",
                     bases_form: str = "montgomery") -> dict:
        """Device check of commitments [ncols, 64] u8 in bases_form against the
        columns and the bases, bit-serial and division-free, sharing nothing with
        commit (svdw_check_commit): columns_checked, commit_failures,
        bases_checked, bases_off_curve."""
        cp, n, _ = self._commit_args(columns, bases, k)
        self._points_tensor("commitments", commitments, n, shown="ncols")
        r = CommitCheck()
        _after_torch(self)
        check(lib().svdw_check_commit(self._h, k, _form(form), _form(bases_form), bases.data_ptr(), cp, n,
                                      commitments.data_ptr() if n else None, ct.byref(r)))
        return self._result(r)

    # ---- the SRS (include/svdw.h, "SRS"; parity pinned by the reference's file)
    def fixed_base_mul(self, base, scalars, form: str = "canonical", base_form: str = "montgomery",
                       window_bits: int = 0, out=None):
        """(points, result): [scalars[i]] base for every cell of `scalars`, a
        [n, 32] u8 device tensor in `form` (svdw_fixed_base_mul). base: the 64
        bytes of one affine point in base_form (bytes or a u8 array), (0, 0) the
        identity. points: [n, 64] u8 on the device in base_form; an `out` with
        more than n rows keeps its rows from n on. window_bits: 0 for the
        planned window, or 2..16. result: window_bits, windows, points,
        zero_scalars, identity_outputs."""
        import torch
        f, bf = _form(form), _form(base_form)
        raw = bytes(base) if isinstance(base, (bytes, bytearray)) else np.ascontiguousarray(base, dtype=np.uint8).tobytes()
        if len(raw) != 64:
            raise SvdwError(-1, "base must be the 64 bytes of one affine point")
        self._cells_tensor("scalars", scalars)
        n = scalars.shape[0]
        if out is None:
            out = torch.empty((n, 64), dtype=torch.uint8, device=scalars.device)
        self._points_tensor("out", out, n, at_least=True)
        r = FixedBaseResult()
        _after_torch(self)
        check(lib().svdw_fixed_base_mul(self._h, f, bf, raw, scalars.data_ptr() if n else None,
                                        n, window_bits, out.data_ptr() if n else None, ct.byref(r)))
        _before_torch(self)
        return out, self._result(r)

    def srs_setup(self, k: int, s: int, bases_form: str = "montgomery", g=True, g_lagrange=True):
        """(g, g_lagrange, result): ParamsKZG::setup(k, .) for the secret s (an
        int in [0, p)): g[i] = [s^i] G and g_lagrange[i] = [l_i(s)] G, [2^k, 64] u8
        device tensors in bases_form (svdw_srs_setup). g, g_lagrange: True for a
        new tensor, a tensor to write into, or None to leave that array out (it
        is returned as None). result: k, window_bits, windows, chunks, rows,
        chunk_rows, the zero scalars and identity outputs of either array,
        secret_in_domain."""
        import torch
        sw, bf = _challenge_arg(s), _form(bases_form)
        rows = 1 << k if 0 <= k < 32 else 0
        outs = []
        for what, t in (("g", g), ("g_lagrange", g_lagrange)):
            if t is True:
                t = torch.empty((rows, 64), dtype=torch.uint8, device=torch.device("cuda", self.device))
            elif t is None or t is False:
                t = None
            else:
                self._points_tensor(what, t, rows)
            outs.append(t)
        r = SrsResult()
        _after_torch(self)
        check(lib().svdw_srs_setup(self._h, k, sw, bf, *[t.data_ptr() if t is not None else None
                                                                        for t in outs], ct.byref(r)))
        _before_torch(self)
        return outs[0], outs[1], self._result(r)

    def check_srs(self, g, g_lagrange, k: int, s: int, rho: int, bases_form: str = "montgomery") -> dict:
        """Device check of an SRS's two arrays against its secret s with the
        challenge rho (ints in [0, p)), sharing nothing with srs_setup
        (svdw_check_srs): points_checked, points_off_curve, g_failed,
        lagrange_failed."""
        sw, rw, bf = _challenge_arg(s), _challenge_arg(rho), _form(bases_form)
        rows = 1 << k if 0 <= k < 32 else 0
        self._points_tensor("g", g, rows)
        self._points_tensor("g_lagrange", g_lagrange, rows)
        r = SrsCheck()
        _after_torch(self)
        check(lib().svdw_check_srs(self._h, k, bf, g.data_ptr(), g_lagrange.data_ptr(), sw, rw,
                                   ct.byref(r)))
        return self._result(r)

    # ---- G1 transforms (include/svdw.h, "G1 transforms"; parity pinned by the reference's file)
    def g1_mul(self, points, scalars, form: str = "canonical", bases_form: str = "montgomery", window_bits: int = 0,
               out=None):
        """(out, result): [scalars[i]] points[i], an unrelated scalar times an
        unrelated point per row (svdw_g1_mul). points: a [n, 64] u8 device
        tensor of affine points in bases_form, (0, 0) the identity; scalars: a
        [n, 32] u8 device tensor in `form`. out: [n, 64] u8 on the device in
        bases_form; an `out` with more than n rows keeps its rows from n on.
        window_bits: 0 for the planned window, or 2..6. result: window_bits,
        windows, points, zero_scalars, identity_inputs, identity_outputs."""
        import torch
        f, bf = _form(form), _form(bases_form)
        self._cells_tensor("scalars", scalars)
        n = scalars.shape[0]
        self._points_tensor("points", points, n)
        if out is None:
            out = torch.empty((n, 64), dtype=torch.uint8, device=scalars.device)
        self._points_tensor("out", out, n, at_least=True)
        r = G1MulResult()
        _after_torch(self)
        check(lib().svdw_g1_mul(self._h, f, bf, points.data_ptr() if n else None, scalars.data_ptr() if n else None,
                                n, window_bits, out.data_ptr() if n else None, ct.byref(r)))
        _before_torch(self)
        return out, self._result(r)

    def g1_fft(self, points, k: int, inverse: bool = False, bases_form: str = "montgomery", out=None):
        """(out, result): the FFT over G1 of the 2^k affine points, natural
        order on both sides (svdw_g1_fft): out[i] = sum_j [omega^(i j)] points[j],
        or with inverse=True [2^-k] sum_j [omega^(-i j)] points[j], which is
        ParamsKZG's g_to_lagrange. points, out: [2^k, 64] u8 device tensors in
        bases_form that do not overlap. result: k, stages, window_bits,
        windows, rows, multiplications, identity_inputs, identity_outputs."""
        import torch
        bf = _form(bases_form)
        rows = 1 << k if 0 <= k < 32 else 0
        self._points_tensor("points", points, rows)
        if out is None:
            out = torch.empty((rows, 64), dtype=torch.uint8, device=points.device)
        self._points_tensor("out", out, rows)
        r = G1FftResult()
        _after_torch(self)
        check(lib().svdw_g1_fft(self._h, k, bf, 1 if inverse else 0, points.data_ptr(), out.data_ptr(), ct.byref(r)))
        _before_torch(self)
        return out, self._result(r)

    def check_lagrange(self, g, g_lagrange, k: int, rho: int, bases_form: str = "montgomery") -> dict:
        """Device check that g_lagrange is the Lagrange form of g, with the
        challenge rho (an int in [0, p)) and no secret, sharing nothing with
        g1_fft (svdw_check_lagrange): points_checked, points_off_curve, failed.
        It does not show that g is a sequence of powers (that needs G2 and a
        pairing)."""
        rw, bf = _challenge_arg(rho), _form(bases_form)
        rows = 1 << k if 0 <= k < 32 else 0
        self._points_tensor("g", g, rows)
        self._points_tensor("g_lagrange", g_lagrange, rows)
        r = LagrangeCheck()
        _after_torch(self)
        check(lib().svdw_check_lagrange(self._h, k, bf, g.data_ptr(), g_lagrange.data_ptr(), rw, ct.byref(r)))
        return self._result(r)

    # ---- quotient polynomial (include/svdw.h, "quotient"; parity unpinned)
    _QUOTIENT_FAMILIES = ("advice", "selectors", "perm_columns", "sigma", "perm_z", "lookup_input", "lookup_table",
                          "permuted_input", "permuted_table", "lookup_z")

    def _quotient_args(self, rows: int, k: int, extended_k: int, shift: int, beta: int, gamma: int, y: int,
                       chunk_len: int, unusable_rows: int, form: str, families: dict):
        """(QuotientArgs, what keeps its pointer arrays alive, the columns' device)
        from the keyword arguments of quotient / check_quotient; every column of
        every family has `rows` cells."""
        a = QuotientArgs()
        a.shift, a.beta, a.gamma, a.y = (self._shift_arg(shift), _challenge_arg(beta), _challenge_arg(gamma),
                                         _challenge_arg(y))
        unknown = set(families) - set(self._QUOTIENT_FAMILIES)
        if unknown:
            raise TypeError(f"unknown column family {sorted(unknown)[0]!r}")
        a.k, a.extended_k, a.unusable_rows, a.form, a.chunk_len = k, extended_k, unusable_rows, _form(form), chunk_len
        keep, count, dev = [], {}, None
        for name in self._QUOTIENT_FAMILIES:
            ptrs, count[name], d = self._column_pointers(name, families.get(name, ()), rows)
            dev = dev or d
            keep.append(ptrs)
            setattr(a, name, ct.cast(ptrs, ct.c_void_p))
        if count["advice"] != count["selectors"]:
            raise SvdwError(-1, "advice and selectors differ in their number of columns")
        if count["perm_columns"] != count["sigma"]:
            raise SvdwError(-1, "perm_columns and sigma differ in their number of columns")
        if chunk_len > 0 and count["perm_z"] != -(-count["perm_columns"] // chunk_len):
            raise SvdwError(-1, "perm_z must hold one column per set of chunk_len columns")
        if len({count[f] for f in self._QUOTIENT_FAMILIES[5:]}) != 1:
            raise SvdwError(-1, "the lookup families differ in their number of columns")
        a.n_gate, a.n_perm, a.n_lookup = count["advice"], count["perm_columns"], count["lookup_z"]
        return a, keep, dev

    def quotient(self, k: int, extended_k: int, shift: int, beta: int, gamma: int, y: int, chunk_len: int = 0,
                 unusable_rows: int = 6, form: str = "canonical", out=None, **families):
        """(h_ext, result): the quotient polynomial on the extended domain
        (svdw_quotient), a [1, 2^extended_k, 32] u8 device tensor in `form`: the
        gates, the permutation argument and the lookup arguments folded with
        powers of y in the header's order and divided by X^n - 1. The families
        are keyword arguments named as the struct's fields (advice, selectors;
        perm_columns, sigma, perm_z with chunk_len; lookup_input, lookup_table,
        permuted_input, permuted_table, lookup_z), each a tensor
        [n, 2^extended_k, 32] u8 in `form` or a list of such tensors, already on
        the coset of `shift` (coeff_to_extended); any family may be left out.
        result: gate_expressions, permutation_expressions, lookup_expressions,
        rows, extension, degree."""
        import torch
        rows = 1 << extended_k if 0 <= extended_k < 32 else 0
        a, _keep, dev = self._quotient_args(rows, k, extended_k, shift, beta, gamma, y, chunk_len, unusable_rows, form,
                                           families)
        if out is None:
            out = torch.empty((1, rows, 32), dtype=torch.uint8, device=dev or torch.device("cuda", self.device))
        if (not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != torch.uint8
                or not out.is_contiguous() or tuple(out.shape) != (1, rows, 32)):
            raise SvdwError(-1, "out must be a contiguous uint8 device tensor [1, 2^extended_k, 32]")
        r = QuotientResult()
        _after_torch(self)
        check(lib().svdw_quotient(self._h, ct.byref(a), out.data_ptr(), ct.byref(r)))
        _before_torch(self)
        return out, {k_: getattr(r, k_) for k_, _ in QuotientResult._fields_}

    def check_quotient(self, h_coeffs, x: int, k: int, extended_k: int, shift: int, beta: int, gamma: int, y: int,
                       chunk_len: int = 0, unusable_rows: int = 6, form: str = "canonical", **families) -> dict:
        """The verifier's identity h(x) (x^n - 1) == fold(x) at the point x
        (svdw_check_quotient). The families as for quotient, but every column in
        coefficient form, [n, 2^k, 32] u8; h_coeffs: [1, 2^extended_k, 32] u8, the
        coefficients of h. Returns lhs and rhs as ints, identity_failures (0 or
        1), tail_checked and tail_nonzero (the coefficients of h above
        D (n - 1) - n)."""
        import torch
        xa = _challenge_arg(x)
        rows = 1 << k if 0 <= k < 32 else 0
        a, _keep, _ = self._quotient_args(rows, k, extended_k, shift, beta, gamma, y, chunk_len, unusable_rows, form,
                                         families)
        ext_rows = 1 << extended_k if 0 <= extended_k < 32 else 0
        if h_coeffs is not None and (not isinstance(h_coeffs, torch.Tensor) or not h_coeffs.is_cuda
                                     or h_coeffs.dtype != torch.uint8 or not h_coeffs.is_contiguous()
                                     or tuple(h_coeffs.shape) != (1, ext_rows, 32)):
            raise SvdwError(-1, "h_coeffs must be a contiguous uint8 device tensor [1, 2^extended_k, 32]")
        r = QuotientCheck()
        _after_torch(self)
        check(lib().svdw_check_quotient(self._h, ct.byref(a), h_coeffs.data_ptr() if h_coeffs is not None else None,
                                        xa, ct.byref(r)))
        return {"lhs": words_to_int(r.lhs), "rhs": words_to_int(r.rhs), "identity_failures": r.identity_failures,
                "tail_checked": r.tail_checked, "tail_nonzero": r.tail_nonzero}

    # ---- openings (include/svdw.h, "openings"; parity unpinned)
    def _open_args(self, columns, set_of, sets, k: int):
        """(column pointers, count, set_of, points, npoints, nsets, rows, device)
        of an opening call; of a set's points the first 8 are handed over, its
        count as it is (the C ABI rejects more than 8)."""
        rows = 1 << k if 0 <= k < 32 else 0
        cp, n, dev = self._column_pointers("columns", columns, rows)
        set_of = [int(i) for i in set_of]
        if len(set_of) != n:
            raise SvdwError(-1, "set_of must hold one set index per column")
        if any(not 0 <= i < 1 << 32 for i in set_of):
            raise SvdwError(-1, "set_of out of range")
        sets = [list(s) for s in sets]
        ns = len(sets)
        so = (ct.c_uint32 * max(n, 1))(*set_of)
        npts = (ct.c_uint32 * max(ns, 1))(*[len(s) for s in sets])
        pts = (ct.c_uint64 * max(32 * ns, 1))()
        for i, pset in enumerate(sets):
            for q, x in enumerate(pset[:8]):
                pts[32 * i + 4 * q:32 * i + 4 * q + 4] = list(_challenge_arg(x))
        return cp, n, so, pts, npts, ns, rows, dev

    def _open_cell_tensor(self, what: str, t, rows: int, dev=None):
        import torch
        if t is None:
            return torch.empty((1, rows, 32), dtype=torch.uint8, device=dev or torch.device("cuda", self.device))
        if (not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.uint8 or not t.is_contiguous()
                or tuple(t.shape) != (1, rows, 32)):
            raise SvdwError(-1, f"{what} must be a contiguous uint8 device tensor [1, 2^k, 32]")
        return t

    @staticmethod
    def _open_result(r) -> dict:
        return {"columns": r.columns, "sets": r.sets, "points": r.points, "passes": r.passes, "rows": r.rows,
                "remainder": words_to_int(r.remainder)}

    def open_quotient(self, columns, set_of, sets, y: int, v: int, k: int, form: str = "canonical", out=None):
        """(h1, result): SHPLONK's first quotient polynomial (svdw_open_quotient),
        a [1, 2^k, 32] u8 device tensor of coefficients in `form`. columns: the
        polynomials' 2^k coefficients, a tensor [n, 2^k, 32] u8 in `form` or a list
        of such tensors; set_of: one rotation-set index per column; sets: one list
        of points (ints below p, at most 8, distinct) per set, e.g. from
        shplonk_queries; y, v: the challenges. Per set the columns are folded by
        Horner in y and divided by the set's vanishing polynomial, the quotients
        folded by Horner in v. result: columns, sets, points (|T|), passes, rows,
        remainder (0 here)."""
        cy, cv = _challenge_arg(y), _challenge_arg(v)
        cp, n, so, pts, npts, ns, rows, dev = self._open_args(columns, set_of, sets, k)
        out = self._open_cell_tensor("out", out, rows, dev)
        r = OpenResult()
        _after_torch(self)
        check(lib().svdw_open_quotient(self._h, k, _form(form), cp, n, so, pts, npts, ns, cy, cv, out.data_ptr(),
                                       ct.byref(r)))
        _before_torch(self)
        return out, self._open_result(r)

    def open_linearise(self, columns, set_of, sets, y: int, v: int, u: int, h1, k: int, form: str = "canonical",
                       out=None):
        """(h2, result): SHPLONK's second quotient polynomial (svdw_open_linearise)
        from the arguments of open_quotient, the challenge u and h1 as
        open_quotient returned it: the quotient of G(X) = (Horner in v of c_i
        F_i(X)) - Z_{S_0}(u) h1(X) by (X - u). result["remainder"] is G(u), which
        equals the verifier's constant for an honest h1."""
        cy, cv, cu = _challenge_arg(y), _challenge_arg(v), _challenge_arg(u)
        cp, n, so, pts, npts, ns, rows, dev = self._open_args(columns, set_of, sets, k)
        h1 = self._open_cell_tensor("h1", h1, rows) if h1 is not None else None
        out = self._open_cell_tensor("out", out, rows, dev)
        r = OpenResult()
        _after_torch(self)
        check(lib().svdw_open_linearise(self._h, k, _form(form), cp, n, so, pts, npts, ns, cy, cv, cu,
                                        h1.data_ptr() if h1 is not None else None, out.data_ptr(), ct.byref(r)))
        _before_torch(self)
        return out, self._open_result(r)

    def check_open(self, columns, set_of, sets, y: int, v: int, u: int, h1, h2, t: int, k: int,
                   form: str = "canonical") -> dict:
        """The independent check of h1 and h2 at the point t (svdw_check_open):
        lhs1, rhs1, lhs2, rhs2 and constant as ints, identity1_failures,
        identity2_failures, the counts of the top cells, and evals: per column
        the list of its values at its set's points (what the transcript takes)."""
        cy, cv, cu, ctt = _challenge_arg(y), _challenge_arg(v), _challenge_arg(u), _challenge_arg(t)
        cp, n, so, pts, npts, ns, rows, _ = self._open_args(columns, set_of, sets, k)
        h1 = self._open_cell_tensor("h1", h1, rows) if h1 is not None else None
        h2 = self._open_cell_tensor("h2", h2, rows) if h2 is not None else None
        ev = (ct.c_uint64 * max(32 * n, 1))()
        r = OpenCheck()
        _after_torch(self)
        check(lib().svdw_check_open(self._h, k, _form(form), cp, n, so, pts, npts, ns, cy, cv, cu,
                                    h1.data_ptr() if h1 is not None else None,
                                    h2.data_ptr() if h2 is not None else None, ctt, ev, ct.byref(r)))
        out = {f: words_to_int(getattr(r, f)) for f in ("lhs1", "rhs1", "lhs2", "rhs2", "constant")}
        out.update({f: getattr(r, f) for f, _ in OpenCheck._fields_[5:]})
        sizes = [len(s) for s in sets]
        out["evals"] = [[words_to_int(ev[32 * j + 4 * q:32 * j + 4 * q + 4]) for q in range(sizes[so[j]])]
                        for j in range(n)]
        return out

    def linear_combination(self, columns, scalars, k: int, form: str = "canonical", out=None):
        """sum_j scalars[j] columns[j] as a [1, 2^k, 32] u8 device tensor in `form`
        (svdw_linear_combination): columns a tensor [n, 2^k, 32] u8 or a list of
        such tensors, scalars ints below p. With h_coeffs.view(E, 2**k, 32) and the
        scalars x^(n i) it is the one polynomial create_proof opens for h."""
        rows = 1 << k if 0 <= k < 32 else 0
        sc = [_challenge_arg(x) for x in scalars]
        cp, n, dev = self._column_pointers("columns", columns, rows)
        if len(sc) != n:
            raise SvdwError(-1, "scalars must hold one value per column")
        buf = (ct.c_uint64 * max(4 * n, 1))(*[w for x in sc for w in x])
        out = self._open_cell_tensor("out", out, rows, dev)
        _after_torch(self)
        check(lib().svdw_linear_combination(self._h, k, _form(form), cp, n, buf, out.data_ptr()))
        _before_torch(self)
        return out

    def profile(self, on: bool = True, prefix: str = "") -> None:
        """Record HIP events around kernel launches (names starting with `prefix`)."""
        check(lib().svdw_profile_filter(self._h, prefix.encode()))
        check(lib().svdw_profile_enable(self._h, 1 if on else 0))

    def profile_collect(self) -> list:
        """Per-kernel {name, launches, total_ms, max_ms, bytes, ops}; drops the records."""
        n = ct.c_uint32()
        cap = 256   # distinct kernel names; collect() drops the records, so one call
        buf = (KStat * cap)()
        check(lib().svdw_profile_collect(self._h, buf, cap, ct.byref(n)))
        return [{"name": s.name.decode(), "launches": s.launches, "total_ms": s.total_ms,
                 "max_ms": s.max_ms, "bytes": s.bytes, "ops": s.ops} for s in buf[:min(n.value, cap)]]

    def load_witness(self, value: int, phase: int = 0) -> "ZkVector":
        v = Vec()
        w = int_to_words(int(value) % P_MOD)
        check(lib().svdw_load_witness(self._h, phase, w.ctypes.data, ct.byref(v)))
        return ZkVector(self, v)

    def load_constant(self, value: int, phase: int = 0) -> "ZkVector":
        v = Vec()
        w = int_to_words(int(value) % P_MOD)
        check(lib().svdw_load_constant(self._h, phase, w.ctypes.data, ct.byref(v)))
        return ZkVector(self, v)


def _dequantize(ctx: Context, fn, view, shape, device: bool):
    """fn = svdw_dequantize_mat / _vec of `view` into a new array of `shape`."""
    if device:
        torch = _torch_mod()
        out = torch.empty(shape, dtype=torch.float64, device=torch.device("cuda", ctx.device))
        _after_torch(ctx)
        check(fn(ctx.handle, ct.byref(view), out.data_ptr() or 1, 1))
        _before_torch(ctx)
        return out
    out = np.zeros(shape, dtype=np.float64)
    check(fn(ctx.handle, ct.byref(view), out.ctypes.data or 1, 0))
    return out


class ZkMatrix:
    """src/matrix/mod.rs:219-420: a view (offset + strides) into a phase stream."""

    def __init__(self, ctx: Context, mat: Mat):
        self.ctx = ctx
        self.mat = mat

    @property
    def num_rows(self) -> int:
        return self.mat.rows

    @property
    def num_col(self) -> int:
        return self.mat.cols

    @classmethod
    def new(cls, ctx: Context, matrix, phase: int = 0) -> "ZkMatrix":
        """ZkMatrix::new (src/matrix/mod.rs:230-252)."""
        out = Mat()
        dp = _device_ptr(matrix)
        if dp is not None:
            rows, cols = matrix.shape
            _after_torch(ctx)
            check(lib().svdw_zkmatrix_new(ctx.handle, phase, dp, rows, cols, 1, ct.byref(out)))
            ctx._hold(matrix)
        else:
            a = np.ascontiguousarray(matrix, dtype=np.float64)
            if a.ndim != 2:
                raise SvdwError(-1, "ZkMatrix::new expects a 2-D matrix")
            check(lib().svdw_zkmatrix_new(ctx.handle, phase, a.ctypes.data, a.shape[0],
                                          a.shape[1], 0, ct.byref(out)))
        return cls(ctx, out)

    def transpose_matrix(self) -> "ZkMatrix":
        """ZkMatrix::transpose_matrix (src/matrix/mod.rs:408-419): no cells."""
        out = Mat()
        check(lib().svdw_transpose_matrix(ct.byref(self.mat), ct.byref(out)))
        return ZkMatrix(self.ctx, out)

    @staticmethod
    def verify_mul(ctx: Context, a: "ZkMatrix", b: "ZkMatrix", c_s: "ZkMatrix", init_rand: int,
                   phase: int = 1) -> None:
        """ZkMatrix::verify_mul (src/matrix/mod.rs:299-342)."""
        g = int_to_words(int(init_rand) % P_MOD)
        check(lib().svdw_verify_mul(ctx.handle, phase, ct.byref(a.mat), ct.byref(b.mat),
                                    ct.byref(c_s.mat), g.ctypes.data))

    @staticmethod
    def rescale_matrix(ctx: Context, c_s: "ZkMatrix", shift_bits: int = 0,
                       num_bits: int = 0) -> "ZkMatrix":
        """ZkMatrix::rescale_matrix (src/matrix/mod.rs:354-375). signed_div_scale's
        layout is parity unpinned (include/svdw.h, svdw_div_scale)."""
        out = Mat()
        cfg = DivScale(shift_bits, num_bits)
        check(lib().svdw_rescale_matrix(ctx.handle, ct.byref(c_s.mat), ct.byref(cfg), ct.byref(out)))
        return ZkMatrix(ctx, out)

    def values(self, form: str = "canonical") -> np.ndarray:
        """Cell values (rows, cols, 4) uint64 in `form` (host copy of the view's
        cells alone, gathered on the device: svdw_export_mat)."""
        out = np.zeros((self.mat.rows, self.mat.cols, 4), dtype=np.uint64)
        check(lib().svdw_export_mat(self.ctx.handle, ct.byref(self.mat), _form(form), out.ctypes.data or 1, 0))
        return out

    def dequantize(self, device: bool = False):
        """ZkMatrix::dequantize (src/matrix/mod.rs:257-270): (rows, cols) float64,
        a numpy array or with device=True a torch tensor on the context's
        device (svdw_dequantize_mat; parity unpinned, include/svdw.h)."""
        return _dequantize(self.ctx, lib().svdw_dequantize_mat, self.mat, (self.mat.rows, self.mat.cols), device)

    def print(self, file=None) -> None:
        """ZkMatrix::print (src/matrix/mod.rs:272-284): the dequantized matrix in
        the reference's layout, elements as Rust's {:?}."""
        text = "[\n"
        for row in self.dequantize():
            text += "[\n" + "".join(format_f64_debug(x) + ", " for x in row) + "], \n"
        print(text + "]", file=file)


class ZkVector:
    """src/matrix/mod.rs:19-216."""

    def __init__(self, ctx: Context, vec: Vec):
        self.ctx = ctx
        self.vec = vec

    def size(self) -> int:
        return self.vec.len

    @classmethod
    def new(cls, ctx: Context, v, phase: int = 0) -> "ZkVector":
        """ZkVector::new (src/matrix/mod.rs:29-40)."""
        out = Vec()
        dp = _device_ptr(v)
        if dp is not None:
            _after_torch(ctx)
            check(lib().svdw_zkvector_new(ctx.handle, phase, dp, v.numel(), 1, ct.byref(out)))
            ctx._hold(v)
        else:
            a = np.ascontiguousarray(v, dtype=np.float64).ravel()
            check(lib().svdw_zkvector_new(ctx.handle, phase, a.ctypes.data, a.size, 0,
                                          ct.byref(out)))
        return cls(ctx, out)

    def values(self, form: str = "canonical") -> np.ndarray:
        """Cell values (len, 4) uint64 in `form` (host copy of the view's cells
        alone, gathered on the device: svdw_export_vec)."""
        out = np.zeros((self.vec.len, 4), dtype=np.uint64)
        check(lib().svdw_export_vec(self.ctx.handle, ct.byref(self.vec), _form(form), out.ctypes.data or 1, 0))
        return out

    def dequantize(self, device: bool = False):
        """ZkVector::dequantize (src/matrix/mod.rs:50-56): (len,) float64, a numpy
        array or with device=True a torch tensor (svdw_dequantize_vec)."""
        return _dequantize(self.ctx, lib().svdw_dequantize_vec, self.vec, (self.vec.len,), device)

    def print(self, file=None) -> None:
        """ZkVector::print (src/matrix/mod.rs:61-68)."""
        text = "[\n" + "".join(format_f64_debug(x) + ", \n" for x in self.dequantize())
        print(text + "]", file=file)

    def inner_product(self, x: "ZkVector", phase: int = 0, shift_bits: int = 0,
                      num_bits: int = 0) -> "ZkVector":
        """ZkVector::inner_product (src/matrix/mod.rs:79-106): 1-element vector."""
        out = Vec()
        cfg = DivScale(shift_bits, num_bits)
        check(lib().svdw_zkvector_inner_product(self.ctx.handle, phase, ct.byref(self.vec),
                                                ct.byref(x.vec), ct.byref(cfg), ct.byref(out)))
        return ZkVector(self.ctx, out)

    def _norm_square(self, phase: int = 0, shift_bits: int = 0, num_bits: int = 0) -> "ZkVector":
        """ZkVector::_norm_square (src/matrix/mod.rs:112-119): 1-element vector."""
        out = Vec()
        cfg = DivScale(shift_bits, num_bits)
        check(lib().svdw_zkvector_norm_square(self.ctx.handle, phase, ct.byref(self.vec),
                                              ct.byref(cfg), ct.byref(out)))
        return ZkVector(self.ctx, out)

    def norm(self, phase: int = 0, shift_bits: int = 0, num_bits: int = 0,
             sqrt_bits: int = 0) -> "ZkVector":
        """ZkVector::norm (src/matrix/mod.rs:124-131): qsqrt(_norm_square); qsqrt is
        the parameterised construction of svdw_zkvector_norm (parity unpinned)."""
        out = Vec()
        cfg = DivScale(shift_bits, num_bits)
        check(lib().svdw_zkvector_norm(self.ctx.handle, phase, ct.byref(self.vec), ct.byref(cfg),
                                       sqrt_bits, ct.byref(out)))
        return ZkVector(self.ctx, out)

    def dist(self, x: "ZkVector", phase: int = 0, shift_bits: int = 0, num_bits: int = 0,
             sqrt_bits: int = 0) -> "ZkVector":
        """ZkVector::dist (src/matrix/mod.rs:156-164): qsqrt(_dist_square(x))."""
        out = Vec()
        cfg = DivScale(shift_bits, num_bits)
        check(lib().svdw_zkvector_dist(self.ctx.handle, phase, ct.byref(self.vec), ct.byref(x.vec),
                                       ct.byref(cfg), sqrt_bits, ct.byref(out)))
        return ZkVector(self.ctx, out)

    def _dist_square(self, x: "ZkVector", phase: int = 0, shift_bits: int = 0,
                     num_bits: int = 0) -> "ZkVector":
        """ZkVector::_dist_square (src/matrix/mod.rs:135-148): 1-element vector."""
        out = Vec()
        cfg = DivScale(shift_bits, num_bits)
        check(lib().svdw_zkvector_dist_square(self.ctx.handle, phase, ct.byref(self.vec),
                                              ct.byref(x.vec), ct.byref(cfg), ct.byref(out)))
        return ZkVector(self.ctx, out)

    def mul(self, a: ZkMatrix, phase: int = 0, shift_bits: int = 0,
            num_bits: int = 0) -> "ZkVector":
        """ZkVector::mul (src/matrix/mod.rs:169-182): a . self, rescaled."""
        out = Vec()
        cfg = DivScale(shift_bits, num_bits)
        check(lib().svdw_zkvector_mul(self.ctx.handle, phase, ct.byref(self.vec), ct.byref(a.mat),
                                      ct.byref(cfg), ct.byref(out)))
        return ZkVector(self.ctx, out)

    def entries_less_than(self, max_bits: int) -> None:
        """ZkVector::entries_less_than (src/matrix/mod.rs:185-194)."""
        check(lib().svdw_entries_less_than(self.ctx.handle, ct.byref(self.vec), max_bits))

    def entries_in_desc_order(self, max_bits: int) -> None:
        """ZkVector::entries_in_desc_order (src/matrix/mod.rs:199-215)."""
        check(lib().svdw_entries_in_desc_order(self.ctx.handle, ct.byref(self.vec), max_bits))


def _bound_words(b: int) -> np.ndarray:
    if b < 0 or b >= (1 << 256):
        raise SvdwError(-1, "bound must be a non-negative 256-bit integer")
    return int_to_words(b)


def honest_prover_mat_mul(ctx: Context, a: ZkMatrix, b: ZkMatrix, phase: int = 0) -> ZkMatrix:
    """src/matrix/mod.rs:546-568."""
    out = Mat()
    check(lib().svdw_honest_prover_mat_mul(ctx.handle, phase, ct.byref(a.mat), ct.byref(b.mat),
                                           ct.byref(out)))
    return ZkMatrix(ctx, out)


def field_mat_vec_mul(ctx: Context, a: ZkMatrix, v: ZkVector, phase: int = 0) -> ZkVector:
    """src/matrix/mod.rs:574-599."""
    out = Vec()
    check(lib().svdw_field_mat_vec_mul(ctx.handle, phase, ct.byref(a.mat), ct.byref(v.vec),
                                       ct.byref(out)))
    return ZkVector(ctx, out)


def mat_times_diag_mat(ctx: Context, a: ZkMatrix, v: ZkVector) -> ZkMatrix:
    """src/matrix/mod.rs:610-627."""
    out = Mat()
    check(lib().svdw_mat_times_diag_mat(ctx.handle, ct.byref(a.mat), ct.byref(v.vec),
                                        ct.byref(out)))
    return ZkMatrix(ctx, out)


def check_mat_diff(ctx: Context, a: ZkMatrix, b: ZkMatrix, tol: int) -> None:
    """src/matrix/mod.rs:441-457."""
    check(lib().svdw_check_mat_diff(ctx.handle, ct.byref(a.mat), ct.byref(b.mat),
                                    _bound_words(tol).ctypes.data))


def check_mat_id(ctx: Context, a: ZkMatrix, scalar_id: ZkVector, tol: int) -> None:
    """src/matrix/mod.rs:461-483."""
    check(lib().svdw_check_mat_id(ctx.handle, ct.byref(a.mat), ct.byref(scalar_id.vec),
                                  _bound_words(tol).ctypes.data))


def check_mat_entries_bounded(ctx: Context, a: ZkMatrix, bnd: int) -> None:
    """src/matrix/mod.rs:490-501."""
    check(lib().svdw_check_mat_entries_bounded(ctx.handle, ct.byref(a.mat),
                                               _bound_words(bnd).ctypes.data))


def err_calc(p: int, size: int, max_norm: float, eps_svd: float, eps_u: float):
    """src/svd/mod.rs:155-163."""
    a, b = ct.c_double(), ct.c_double()
    check(lib().svdw_err_calc(p, size, max_norm, eps_svd, eps_u, ct.byref(a), ct.byref(b)))
    return a.value, b.value


@dataclass
class SvdPayload:
    u_t: ZkMatrix
    v_t: ZkMatrix
    m_times_vt: ZkMatrix
    u_times_ut: ZkMatrix
    v_times_vt: ZkMatrix
    raw: Payload


def check_svd_phase0(ctx: Context, m: ZkMatrix, u: ZkMatrix, v: ZkMatrix, d: ZkVector,
                     err_svd: float, err_u: float, max_bits_d: int) -> SvdPayload:
    """src/svd/mod.rs:32-116."""
    pl = Payload()
    check(lib().svdw_check_svd_phase0(ctx.handle, ct.byref(m.mat), ct.byref(u.mat),
                                      ct.byref(v.mat), ct.byref(d.vec), err_svd, err_u,
                                      max_bits_d, ct.byref(pl)))
    return SvdPayload(ZkMatrix(ctx, pl.u_t), ZkMatrix(ctx, pl.v_t), ZkMatrix(ctx, pl.m_times_vt),
                      ZkMatrix(ctx, pl.u_times_ut), ZkMatrix(ctx, pl.v_times_vt), pl)


def check_svd_phase1(ctx: Context, m: ZkMatrix, u: ZkMatrix, v: ZkMatrix, payload: SvdPayload,
                     init_rand: int) -> None:
    """src/svd/mod.rs:127-144."""
    g = int_to_words(int(init_rand) % P_MOD)
    check(lib().svdw_check_svd_phase1(ctx.handle, ct.byref(m.mat), ct.byref(u.mat),
                                      ct.byref(v.mat), ct.byref(payload.raw), g.ctypes.data))


@dataclass
class SvdConfigPy:
    """examples/svd_example.rs:115-118,160."""
    max_norm: float = 100.0
    eps_svd: float = 1e-10
    eps_u: float = 1e-10
    max_bits_d: int = 30

    def c(self) -> SvdConfig:
        return SvdConfig(self.max_norm, self.eps_svd, self.eps_u, self.max_bits_d)


def svd_witness(ctx: Context, m, u, v, d, gamma: int, cfg: SvdConfigPy = SvdConfigPy()) -> dict:
    """Whole witness of examples/svd_example.rs:98-200 (intended one-context
    semantics). Inputs: numpy arrays (host) or contiguous float64 torch CUDA
    tensors on the context's device (then nothing is copied over PCIe)."""
    cfgc = cfg.c()
    cnt = Counts()
    g = _words_arg(gamma)
    dps = [_device_ptr(x) for x in (m, u, v, d)]
    if all(p is not None for p in dps):
        N, M = m.shape
        _after_torch(ctx)
        check(lib().svdw_svd_witness(ctx.handle, *dps, N, M, 1, ct.byref(cfgc), g, ct.byref(cnt)))
        ctx._hold(m, u, v, d)       # pipelined: the stages read them after the call returns
    else:
        arrs = [np.ascontiguousarray(x, dtype=np.float64) for x in (m, u, v, d)]
        N, M = arrs[0].shape
        if arrs[1].shape != (N, N) or arrs[2].shape != (M, M) or arrs[3].size != min(N, M):
            raise SvdwError(-1, "svd_witness: shapes must be m NxM, u NxN, v MxM, d min(N,M)")
        check(lib().svdw_svd_witness(ctx.handle, *[a.ctypes.data for a in arrs], N, M, 0,
                                     ct.byref(cfgc), g, ct.byref(cnt)))
    ctx.last_svd = (int(N), int(M), cfg)        # for collect.plan (shard segment replay)
    return cnt.as_dict()


def svd_decompose(ctx: Context, m, device: bool = False, panel: int = 0, inner: int = 0, max_sweeps: int = 0):
    """(u, d, v, info) with m = u diag(d) v, computed on the device by blocked
    one-sided Jacobi (svdw_svd_decompose; input-creator.py:30 without LAPACK):
    u N x N, d min(N, M), v M x M holding the rows of V^T as numpy's third
    output does. device=False: m is a host array and the outputs are numpy
    arrays. device=True: m is a contiguous float64 torch tensor on the
    context's device (a host array is uploaded first) and the outputs are torch
    tensors there, ready for svd_witness. info: sweeps, converged, completed
    (columns made by completion), rotations, off, pairs and skipped_pairs (panel
    pairs visited, and those whose solve made no rotation)."""
    opts = SvdOpts(panel, inner, max_sweeps)
    info = SvdInfo()
    if device:
        torch = _torch_mod()
        dev = torch.device("cuda", ctx.device)
        if _device_ptr(m) is None:
            m = torch.from_numpy(np.ascontiguousarray(m, dtype=np.float64)).to(dev)
        if m.dim() != 2:
            raise SvdwError(-1, "svd_decompose: m must be a matrix")
        N, M = m.shape
        u = torch.empty((N, N), dtype=torch.float64, device=dev)
        d = torch.empty(min(N, M), dtype=torch.float64, device=dev)
        v = torch.empty((M, M), dtype=torch.float64, device=dev)
        _after_torch(ctx)               # m may still be in flight, the outputs' memory still read, on torch's stream
        check(lib().svdw_svd_decompose(ctx.handle, m.data_ptr(), N, M, 1, ct.byref(opts), u.data_ptr(),
                                       d.data_ptr(), v.data_ptr(), ct.byref(info)))
        _before_torch(ctx)
    else:
        m = np.ascontiguousarray(m, dtype=np.float64)
        if m.ndim != 2:
            raise SvdwError(-1, "svd_decompose: m must be a matrix")
        N, M = m.shape
        u, d, v = np.empty((N, N)), np.empty(min(N, M)), np.empty((M, M))
        check(lib().svdw_svd_decompose(ctx.handle, m.ctypes.data, N, M, 0, ct.byref(opts), u.ctypes.data,
                                       d.ctypes.data, v.ctypes.data, ct.byref(info)))
    return u, d, v, {k: getattr(info, k) for k, _ in info._fields_}


def verify_mul_witness(ctx: Context, a, b, gamma: int) -> dict:
    """The README.md:32-46 recipe in one call (svdw_verify_mul_witness): loads
    of a and b, c_s = a * b in phase 0, verify_mul(a, b, c_s, gamma) in phase 1.
    Inputs: numpy arrays or contiguous float64 torch tensors on the device."""
    cnt = Counts()
    g = _words_arg(gamma)
    dps = [_device_ptr(x) for x in (a, b)]
    if all(p is not None for p in dps):
        (N, K), M = a.shape, b.shape[1]
        if b.shape[0] != K:
            raise SvdwError(-1, "verify_mul_witness: a.num_col != b.num_rows")
        # (the hand-off to torch's stream inside the call, on the state that runs it)
        check(lib().svdw_verify_mul_witness_on(ctx.handle, _torch_stream(ctx), *dps, N, K, M, g, ct.byref(cnt)))
        ctx._hold(a, b)             # lanes: the call still runs beside the next one
    else:
        arrs = [np.ascontiguousarray(x, dtype=np.float64) for x in (a, b)]
        (N, K), M = arrs[0].shape, arrs[1].shape[1]
        if arrs[1].shape[0] != K:
            raise SvdwError(-1, "verify_mul_witness: a.num_col != b.num_rows")
        check(lib().svdw_verify_mul_witness(ctx.handle, arrs[0].ctypes.data, arrs[1].ctypes.data, N, K, M, 0,
                                            g, ct.byref(cnt)))
    return cnt.as_dict()


def parse_svd_input(src, mode: str = "serde") -> dict:
    """Arrays m, u, d, v of the example's input file (data/matrix.in; a path,
    bytes or str), parsed natively like serde_json's default float path
    ("serde", what examples/svd_example.rs:326-330 reads) or correctly rounded
    ("correct"); svdw_parse_svd_input."""
    if isinstance(src, (bytes, bytearray)):
        text = bytes(src)
    elif isinstance(src, str) and src.lstrip().startswith("{"):
        text = src.encode()
    else:
        with open(src, "rb") as fh:
            text = fh.read()
    md = {"serde": 0, "correct": 1}[mode]
    dims = InputDims()
    check(lib().svdw_parse_svd_input(text, len(text), md, ct.byref(dims), None, None, None, None))
    m = np.empty((dims.m_rows, dims.m_cols))
    u = np.empty((dims.u_rows, dims.u_cols))
    v = np.empty((dims.v_rows, dims.v_cols))
    d = np.empty(dims.d_len)
    check(lib().svdw_parse_svd_input(text, len(text), md, ct.byref(dims), m.ctypes.data,
                                     u.ctypes.data, d.ctypes.data, v.ctypes.data))
    return {"m": m, "u": u, "d": d, "v": v}


def parse_svd_input_device(ctx: "Context", src):
    """parse_svd_input on the device (svdw_parse_svd_input_device, serde mode):
    the text (a path, bytes, str, or a uint8 torch tensor already on the
    context's device) is staged to HBM and parsed there; returns device f64
    torch tensors m, u, d, v, ready for svd_witness (on_device)."""
    import torch
    dev = torch.device("cuda", ctx.device)
    if isinstance(src, torch.Tensor):
        t = src.to(dev, dtype=torch.uint8).contiguous()
    else:
        if isinstance(src, (bytes, bytearray)):
            text = bytes(src)
        elif isinstance(src, str) and src.lstrip().startswith("{"):
            text = src.encode()
        else:
            with open(src, "rb") as fh:
                text = fh.read()
        t = torch.frombuffer(bytearray(text), dtype=torch.uint8).to(dev)
    dims = InputDims()
    n = t.numel()
    _after_torch(ctx)                   # the text may still be in flight on torch's stream
    check(lib().svdw_parse_svd_input_device(ctx._h, t.data_ptr(), n, 0, ct.byref(dims),
                                            None, None, None, None))
    out = {"m": torch.empty((dims.m_rows, dims.m_cols), dtype=torch.float64, device=dev),
           "u": torch.empty((dims.u_rows, dims.u_cols), dtype=torch.float64, device=dev),
           "v": torch.empty((dims.v_rows, dims.v_cols), dtype=torch.float64, device=dev),
           "d": torch.empty(dims.d_len, dtype=torch.float64, device=dev)}
    _after_torch(ctx)                   # the outputs' memory may still be read on torch's stream
    check(lib().svdw_parse_svd_input_device(ctx._h, t.data_ptr(), n, 0, ct.byref(dims),
                                            out["m"].data_ptr(), out["u"].data_ptr(),
                                            out["d"].data_ptr(), out["v"].data_ptr()))
    ctx._hold(t)
    _before_torch(ctx)                  # torch kernels reading m, u, d, v run after the parse
    return out


def plan_svd(N: int, M: int, precision_bits: int, lookup_bits: int,
             cfg: SvdConfigPy = SvdConfigPy()) -> dict:
    """Closed-form cell counts (no device)."""
    cfgc = cfg.c()
    cnt = Counts()
    check(lib().svdw_plan_svd(N, M, precision_bits, lookup_bits, ct.byref(cfgc), ct.byref(cnt)))
    return cnt.as_dict()
