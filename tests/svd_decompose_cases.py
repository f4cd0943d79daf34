"""The decomposition of svdw_svd_decompose restated in plain numpy, and the
inputs the CPU and GPU tests share.

restate(m, panel, inner, max_sweeps) follows the device algorithm step for
step: G = m (N <= M) or m^T (N > M), R x C, W = I (C x C); columns in panels of
b, the panel count padded to an even number with zero columns; a sweep is the
round-robin tournament over panel pairs; per pair the Gram matrix H = S^T S of
the 2b columns, `inner` cyclic Jacobi sweeps on H in the 2b x 2b tournament
order accumulating J, with the two skip rules, then S <- S J and the W columns
alike; a sweep without a rotation ends it. Then the stable sort by norm, d, the
normalised R x R factor, completion of the columns that cannot be normalised.
The device sums its Gram matrices in another order (matrix-core tiles, row
chunks), so the figures agree in kind, not in bits.

Row chunks on the device: a Gram block takes 64 rows of G (R of them) and an
apply block 64 rows of G stacked on W (R + C of them). 130 x 96 and 96 x 130
have R = 96 (two Gram chunks, the second half full), C = 130 (W's rows end two
rows into a chunk of their own) and R + C = 226 (four apply chunks, the last
one partial), so every chunked loop runs more than once and ends inside a chunk.
"""
import numpy as np

EPS = 2.0 ** -52
DEFAULT_PANEL, DEFAULT_INNER, DEFAULT_MAX_SWEEPS = 8, 2, 40


def recipe(N, M, seed):
    """conftest.gen_svd_input's matrix (input-creator.py:23-29), without the LAPACK call."""
    rs = np.random.RandomState(seed)
    m = rs.uniform(-10, 10, size=(N, M))
    return m / np.linalg.norm(m, ord=2) * rs.uniform(1, 100)


def _orthogonal(n, seed):
    q, r = np.linalg.qr(np.random.RandomState(seed).standard_normal((n, n)))
    return q * np.sign(np.diag(r))


def tournament(n, step):
    """The n / 2 disjoint pairs (i < j) of step `step` (0 .. n - 2) of the round robin over n (even) players."""
    w = n - 1
    pairs = [(step % w, n - 1)]
    for k in range(1, n // 2):
        a, b = (step + k) % w, (step - k + w) % w
        pairs.append((min(a, b), max(a, b)))
    return pairs


def solve_block(H, inner, tiny):
    """`inner` cyclic sweeps on the symmetric H; returns J, the rotations applied, the largest relative
    off-diagonal entry met."""
    n = H.shape[0]
    H = H.copy()
    J = np.eye(n)
    rot, off = 0, 0.0
    for _ in range(inner):
        before = rot
        for step in range(n - 1):
            for i, j in tournament(n, step):
                hii, hjj, hij = H[i, i], H[j, j], H[i, j]
                if min(hii, hjj) <= tiny:
                    continue
                off = max(off, abs(hij) / np.sqrt(hii * hjj))
                if hij * hij <= EPS * EPS * hii * hjj:
                    continue
                z = (hjj - hii) / (2.0 * hij)
                t = (1.0 if z >= 0 else -1.0) / (abs(z) + np.sqrt(1.0 + z * z))
                c = 1.0 / np.sqrt(1.0 + t * t)
                s = c * t
                for X in (H, J):                                # X <- X Jr
                    xi, xj = X[:, i].copy(), X[:, j].copy()
                    X[:, i], X[:, j] = c * xi - s * xj, s * xi + c * xj
                hi, hj = H[i, :].copy(), H[j, :].copy()         # H <- Jr^T H
                H[i, :], H[j, :] = c * hi - s * hj, s * hi + c * hj
                H[i, j] = H[j, i] = 0.0
                rot += 1
        if rot == before:
            break
    return J, rot, off


def complete(Q, missing):
    """Columns `missing` of the square Q from unit vectors, orthogonalised twice (modified Gram-Schmidt)
    against every other column; a unit vector that keeps 1 / (2 R) of its square is taken, and the search
    goes on from the one after it, wrapping: a column costs O(R^2) per try."""
    R = Q.shape[0]
    gone = set(missing)
    have = [Q[:, j].copy() for j in range(R) if j not in gone]
    k = 0
    for j in missing:
        for _ in range(R):
            x = np.zeros(R)
            x[k] = 1.0
            k = (k + 1) % R
            for _ in range(2):
                for q in have:
                    x -= np.dot(q, x) * q
            nn = np.dot(x, x)
            if nn >= 1.0 / (2 * R):
                Q[:, j] = x / np.sqrt(nn)
                have.append(Q[:, j].copy())
                break


def restate(m, panel=0, inner=0, max_sweeps=0):
    """(u, d, v, info) as svd_decompose returns them."""
    b = panel or DEFAULT_PANEL
    inner = inner or DEFAULT_INNER
    max_sweeps = max_sweeps or DEFAULT_MAX_SWEEPS
    m = np.asarray(m, dtype=np.float64)
    N, M = m.shape
    G = (m if N <= M else m.T).copy()
    R, C = G.shape
    P = -(-C // b)
    P += P & 1
    A = np.zeros((R + C, P * b))                                # G stacked on W, padded columns zero
    A[:R, :C] = G
    A[R:, :C] = np.eye(C)
    tiny = (EPS * np.linalg.norm(m)) ** 2
    sweeps = rotations = converged = skipped = 0
    off = 0.0
    while sweeps < max_sweeps:
        sweeps += 1
        rot, off = 0, 0.0
        for step in range(P - 1):
            for p, q in tournament(P, step):
                cols = np.r_[p * b:(p + 1) * b, q * b:(q + 1) * b]
                S = A[:R, cols]
                J, r, o = solve_block(S.T @ S, inner, tiny)
                off = max(off, o)
                if r:
                    A[:, cols] = A[:, cols] @ J
                    rot += r
                else:
                    skipped += 1
        rotations += rot
        if rot == 0:
            converged = 1
            break
    norms = np.sqrt(np.sum(A[:R, :C] ** 2, axis=0))
    order = np.argsort(-norms, kind="stable")
    d = norms[order[:R]]
    floor = C * EPS * d[0]
    missing = [j for j in range(R) if d[j] <= floor]
    Q = np.zeros((R, R))
    for j in range(R):
        if d[j] > floor:
            Q[:, j] = A[:R, order[j]] / d[j]
    complete(Q, missing)
    Wf = A[R:, order]
    u, v = (Q, Wf.T) if N <= M else (Wf, Q.T)
    info = {"sweeps": sweeps, "converged": converged, "completed": len(missing), "rotations": rotations,
            "off": off, "pairs": sweeps * (P - 1) * (P // 2), "skipped_pairs": skipped}
    return np.ascontiguousarray(u), d, np.ascontiguousarray(v), info


def residuals(m, u, d, v):
    """R1 = max|u d - m v^T| (zero-padded for N < M as check_svd_phase0 pads), R2 = max|u u^T - I|,
    R3 = max|v v^T - I|."""
    N, M = m.shape
    ud = np.zeros((N, M))
    k = min(N, M)
    ud[:, :k] = u[:, :k] * d[None, :k]
    r1 = np.max(np.abs(ud - m @ v.T))
    r2 = np.max(np.abs(u @ u.T - np.eye(N)))
    r3 = np.max(np.abs(v @ v.T - np.eye(M)))
    return r1, r2, r3


def d_error(m, d):
    ref = np.linalg.svd(m, compute_uv=False)
    return float(np.max(np.abs(d - ref)) / ref[0]) if ref[0] > 0 else float(np.max(np.abs(d)))


def _special():
    rs = np.random.RandomState(77)
    rank1 = np.outer(rs.uniform(-1, 1, 5), rs.uniform(-1, 1, 4)) * 7.0
    graded = np.diag(10.0 ** -np.arange(13.0)) @ _orthogonal(13, 5)
    return [("zero4", np.zeros((4, 4)), 4), ("rank1_5x4", rank1, 3), ("ones4x6", np.ones((4, 6)), 3),
            ("3I5", 3.0 * np.eye(5), 0), ("orth12", _orthogonal(12, 3), 0), ("graded13", graded, 0)]


# (name, matrix, panel, inner, completed, is a recipe input)
RECIPE_SHAPES = [(1, 1), (1, 5), (5, 1), (2, 3), (16, 16), (17, 17), (33, 70), (70, 33), (130, 96), (96, 130)]
RECTANGULAR = {"1x5", "5x1", "2x3", "33x70", "70x33", "130x96", "96x130"}


def cases():
    out = []
    for N, M in RECIPE_SHAPES:
        out.append((f"{N}x{M}", recipe(N, M, 100 + N + M), 0, 0, 0, True))
    m64 = recipe(64, 64, 164)
    for b in (1, 4, 8):
        for inner in (1, 2):
            out.append((f"64x64_b{b}_i{inner}", m64, b, inner, 0, True))
    for name, mat, completed in _special():
        out.append((name, mat, 0, 0, completed, False))
    return out


CASES = cases()
CASE_IDS = [c[0] for c in CASES]
_restated = {}


def restated(name):
    """The restatement's result on case `name`, computed once."""
    if name not in _restated:
        _, m, b, inner, _, _ = CASES[CASE_IDS.index(name)]
        _restated[name] = restate(m, b, inner)
    return _restated[name]
