"""The domain transforms of include/svdw.h ("domain transforms"; parity with
halo2's EvaluationDomain unpinned), restated literally in Python ints: the
O(n^2) sums straight from the header's formulas, a recursive radix-2 version of
the same for larger sizes, Horner evaluation, and the sampling rule of
svdw_check_ntt. They are the reference of the device's multi-pass transform and
share no schedule with it."""
from permutation_cases import P_MOD, cells_of, omega  # noqa: F401  (cells_of: re-exported)

ZETA = pow(7, (P_MOD - 1) // 3, P_MOD)                       # a cube root of unity, as Fr::ZETA is one
WIDE_SHIFT = 0x2b3f9c1d5e7a8046f1e2d3c4b5a69788796a5b4c3d2e1f0a1b2c3d4e5f607182 % P_MOD


def inv(x: int) -> int:
    return pow(x, P_MOD - 2, P_MOD)


def dft_forward(a, k_in: int, k: int, shift: int = 1) -> list:
    """out[j] = sum_i a[i] shift^i omega_k^(i j), i < 2^k_in, j < 2^k."""
    w, n_in, n = omega(k), 1 << k_in, 1 << k
    b = [a[i] * pow(shift, i, P_MOD) % P_MOD for i in range(n_in)]
    return [sum(b[i] * pow(w, i * j % n, P_MOD) for i in range(n_in)) % P_MOD for j in range(n)]


def dft_inverse(a, k: int, shift: int = 1) -> list:
    """out[i] = shift^i 2^-k sum_j a[j] omega_k^(-i j)."""
    wi, n = inv(omega(k)), 1 << k
    scale = inv(n)
    return [pow(shift, i, P_MOD) * scale % P_MOD * (sum(a[j] * pow(wi, i * j % n, P_MOD) for j in range(n)) % P_MOD)
            % P_MOD for i in range(n)]


def _radix2(a, w: int) -> list:
    n = len(a)
    if n == 1:
        return list(a)
    w2 = w * w % P_MOD
    ev, od = _radix2(a[0::2], w2), _radix2(a[1::2], w2)
    out, t = [0] * n, 1
    for i in range(n // 2):
        x = od[i] * t % P_MOD
        out[i] = (ev[i] + x) % P_MOD
        out[i + n // 2] = (ev[i] - x) % P_MOD
        t = t * w % P_MOD
    return out


def _powers(x: int, n: int) -> list:
    out, t = [1] * n, 1
    for i in range(n):
        out[i] = t
        t = t * x % P_MOD
    return out


def ntt_forward(a, k_in: int, k: int, shift: int = 1) -> list:
    """dft_forward by recursive halving."""
    sp = _powers(shift, 1 << k_in)
    b = [a[i] * sp[i] % P_MOD for i in range(1 << k_in)] + [0] * ((1 << k) - (1 << k_in))
    return _radix2(b, omega(k))


def ntt_inverse(a, k: int, shift: int = 1) -> list:
    """dft_inverse by recursive halving."""
    n = 1 << k
    c = _radix2(list(a), inv(omega(k)))
    scale, sp = inv(n), _powers(shift, n)
    return [c[i] * scale % P_MOD * sp[i] % P_MOD for i in range(n)]


def horner(coeffs, x: int) -> int:
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % P_MOD
    return acc


def sample_rows(k: int, log_samples: int, seed: int) -> list:
    """The rows svdw_check_ntt samples: j_s = s q + ((seed + s 0x9E3779B1) mod q)."""
    q = (1 << k) >> log_samples
    return [s * q + (seed + s * 0x9E3779B1) % q for s in range(1 << log_samples)]


def spikes_forward(spikes, k: int) -> list:
    """The forward transform (shift 1) of a column that is zero but for
    spikes = [(row, value)]: a sum of geometric sequences."""
    n, out = 1 << k, [0] * (1 << k)
    for row, value in spikes:
        step, t = pow(omega(k), row, P_MOD), value
        for j in range(n):
            out[j] = (out[j] + t) % P_MOD
            t = t * step % P_MOD
    return out


def spikes_inverse(spikes, k: int) -> list:
    n, out = 1 << k, [0] * (1 << k)
    for row, value in spikes:
        step, t = pow(inv(omega(k)), row, P_MOD), value * inv(n) % P_MOD
        for i in range(n):
            out[i] = (out[i] + t) % P_MOD
            t = t * step % P_MOD
    return out
