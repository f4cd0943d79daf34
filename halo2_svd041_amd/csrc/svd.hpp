// The singular value decomposition on the device (svd.hip): m (N x M, f64) to
// u, d, v by the blocked one-sided (Hestenes) Jacobi method, so that a witness
// needs no host linear algebra (input-creator.py:30 calls LAPACK for it).
//
// With R = min(N, M), C = max(N, M) the method works on G = m (N <= M) or m^T
// (N > M), R x C, and carries W = I (C x C): columns of G and W are rotated
// together, G <- G J, W <- W J, until the columns of G are mutually orthogonal.
// Their norms, sorted, are d; the normalised columns the R x R factor; W the
// C x C factor, its trailing C - R columns the null space.
//
// Storage: one array A of Cp columns of L = R + C rows each, column-contiguous
// (A[col * L + row]): rows [0, R) are G's, rows [R, L) W's, so one launch
// rotates both. Cp = P b: the columns in P panels of b (1, 4 or 8), P padded to
// an even number with zero columns. A zero column has zero Gram entries, a
// rotation with h_ij == 0 is skipped, and a skipped pair is the identity in J:
// padded columns stay exactly zero.
//
// A sweep is the round-robin tournament over the P panels: P - 1 steps of P / 2
// disjoint pairs (svd_pair). A step is two launches on the context's stream:
//
//  k_svd_gram    block (pair, y): the partial Gram matrix of the pair's 2b
//                columns over rows [64 y, 64 y + 64) of G, to gram[pair][y][256].
//                b = 8: one v_mfma_f64_16x16x4_f64 tile per wave, each wave 16
//                rows as 4 steps of k = 4 (A and B operand are the same value,
//                S[row][col = lane & 15]); the four waves' tiles are summed in
//                wave order through LDS. b = 1, 4: thread (i, j) runs an fma
//                loop over the 64 rows. No floating-point atomics anywhere:
//                the partial matrices are summed in y order by their readers
//  k_svd_rotate  block (pair, y): sums the pair's partial Gram matrices in y
//                order into H (LDS), solves it (below) into J, and, unless the
//                solve made no rotation, applies J to rows [64 y, 64 y + 64) of
//                the pair's columns of A in place. b = 8: per wave one
//                16-row tile, D^T = J^T S^T as four v_mfma_f64_16x16x4_f64 over
//                k = 16: a lane's four results are four columns at its one row,
//                and the 16 lanes of lane & 15 hold 16 consecutive rows of a
//                column, so a store writes 128 contiguous bytes per column;
//                b = 1, 4: a thread per (row, column group), fma loops.
//                Every block of a pair redoes the solve: it is deterministic, so
//                all get the same J, and a kernel of its own would add a launch
//                per step where launches already cost as much as the data.
//                Block y = 0 adds the pair's rotations to the sweep's counter
//                (an integer atomic), or one to the sweep's count of pairs
//                whose solve made no rotation, and folds the largest relative
//                off-diagonal entry it met into the sweep's maximum
//
// The solve: `inner` cyclic Jacobi sweeps on the 2b x 2b H in the 2b-player
// tournament order, b disjoint rotations at once: lane k < b decides its pair
// (i, j), skipped when min(h_ii, h_jj) <= (eps |m|_F)^2 or h_ij^2 <= eps^2 h_ii
// h_jj (eps = 2^-52), else z = (h_jj - h_ii) / (2 h_ij), t = sign(z) / (|z| +
// sqrt(1 + z^2)), c = 1 / sqrt(1 + t^2), s = c t; then all (2b)^2 threads update
// H <- Jr^T H Jr and J <- J Jr, and h_ij is set to zero.
//
// A sweep without a rotation ends the iteration; the host reads the sweep's
// counters (24 bytes through pinned memory) once per sweep.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace svdw {

static constexpr unsigned kSvdThreads = 256;               // every kernel's block: 4 waves, (2 * 8)^2 threads
static constexpr uint32_t kSvdRows = 64;                   // rows of a Gram block and of an apply block
static constexpr uint32_t kSvdGramCells = 256;             // a partial Gram matrix's cells, whatever b

// The device words of a call (8 bytes each).
struct SvdWords {
    unsigned long long nonfinite;                          // entries of m that are NaN or infinite
    unsigned long long rotations;                          // of the running sweep
    unsigned long long off_bits;                           // the sweep's largest |h_ij| / sqrt(h_ii h_jj), as bits
    unsigned long long skipped;                            // the sweep's pairs whose solve made no rotation
    double tiny;                                           // (eps |m|_F)^2
};

struct SvdArgs {
    double* A;                                             // [Cp][L]
    double* gram;                                          // [P / 2][gram_chunks][256]
    double* norms;                                         // [Cp]: column norms of G, partial squares while loading
    SvdWords* words;
    uint32_t R, C, L, b, P, inner, gram_chunks, apply_chunks;
};

// The pair of step `step` (0 .. P - 2) with index k (0 .. P / 2 - 1) of the round robin over P (even): p < q.
__host__ __device__ inline void svd_pair(uint32_t P, uint32_t step, uint32_t k, uint32_t* p, uint32_t* q) {
    const uint32_t w = P - 1;
    uint32_t a, b;
    if (k == 0) {
        a = step % w;
        b = P - 1;
    } else {
        a = (step + k) % w;
        b = (step + w - k) % w;
    }
    *p = a < b ? a : b;
    *q = a < b ? b : a;
}

// A <- [G; I] from m (N x M row-major), padded columns zero; norms[j] = sum of squares of column j of G;
// words->nonfinite counts the entries that are not finite.
hipError_t launch_svd_load(const SvdArgs& a, const double* m, uint32_t N, uint32_t M, hipStream_t st);
// words->tiny from the norms (one block, fixed order).
hipError_t launch_svd_tiny(const SvdArgs& a, hipStream_t st);
hipError_t launch_svd_gram(const SvdArgs& a, uint32_t step, hipStream_t st);
hipError_t launch_svd_rotate(const SvdArgs& a, uint32_t step, hipStream_t st);
// norms[j] = |column j of G| for j < Cp.
hipError_t launch_svd_norms(const SvdArgs& a, hipStream_t st);
// u, d, v from A by the sorted order perm[0 .. C): a column whose norm is <= floor is written as zeros.
hipError_t launch_svd_write(const SvdArgs& a, const uint32_t* perm, uint32_t N, uint32_t M, double floor, double* u,
                            double* d, double* v, hipStream_t st);

}  // namespace svdw
