"""The lookup argument's grand-product column Z, restated literally, and the
challenges the lookup-product tests run with.

grand_product is halo2's lookup::prover::Permuted::commit_product as
include/svdw.h restates it (parity unpinned): the per-row fraction with
batch_invert's inv0, then the running product. It is the reference of the
device's prefix / suffix products and shares no arithmetic with them;
recurrence_holds is the division-free form the device checker evaluates."""
P_MOD = 21888242871839275222246405745257275088548364400416034343698204186575808495617

# (beta, gamma): well outside the table; then with the top bits set, so that all
# eight 32-bit words of both are non-zero
CHALLENGES = [
    (0x1234567890abcdef1234567890abcdef, P_MOD - (1 << 200)),
    (P_MOD - 0x0fedcba987654321, (0x30644e72 << 224) | int("9abcdef1" * 7, 16)),
]
assert all(0 <= x < P_MOD for pair in CHALLENGES for x in pair)
assert all((x >> (32 * w)) & 0xffffffff for x in CHALLENGES[1] for w in range(8))


def inv0(x: int) -> int:
    return pow(x, P_MOD - 2, P_MOD) if x else 0


def grand_product(A, T, Ap, Sp, beta, gamma, usable, rows):
    """(Z as a list of `rows` ints, the number of zero denominators)."""
    z = [0] * rows
    z[0] = 1
    zeros = 0
    for r in range(usable):
        den = (Ap[r] + beta) * (Sp[r] + gamma) % P_MOD
        zeros += den == 0
        f = (A[r] + beta) * (T[r] + gamma) % P_MOD * inv0(den) % P_MOD
        z[r + 1] = z[r] * f % P_MOD
    return z, zeros


def recurrence_holds(A, T, Ap, Sp, Z, beta, gamma, usable, rows) -> list:
    """The rows r < usable where Z[r+1] (A'[r]+b)(S'[r]+g) != Z[r] (A[r]+b)(T[r]+g)."""
    return [r for r in range(usable)
            if Z[r + 1] * (Ap[r] + beta) * (Sp[r] + gamma) % P_MOD != Z[r] * (A[r] + beta) * (T[r] + gamma) % P_MOD]
