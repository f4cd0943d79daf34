// Fr number-theoretic transforms of columns on the device (ntt.hip): halo2's
// EvaluationDomain conversions lagrange_to_coeff, coeff_to_lagrange,
// coeff_to_extended and extended_to_coeff as one transform, eval_polynomial for
// a batch, and a checker by direct evaluation. Restated from memory (PARITY
// UNPINNED, include/svdw.h). With N = 2^k, omega = omega_k, natural order on
// both sides:
//
//   forward  b[i] = in[i] shift^i (i < 2^k_in, zero above),  out[j] = sum_i b[i] omega^(i j)
//   inverse  c[i] = 2^-k sum_j in[j] omega^(-i j),           out[i] = c[i] shift^i
//
// The transform is a Stockham autosort in P = ceil(k / 10) passes over global
// memory, pass i of radix r = 2^b_i (the b_i split k evenly). With s the product
// of the radices before it, n = N / s, m = n / r, and t = q + s p (q < s, p < m)
// one of N / r butterflies,
//
//   y[q + s (r p + i)] = omega_n^(p i) * sum_{j < r} x[t + (N / r) j] omega_r^(i j),   i < r
//
// so a pass always gathers at the one stride N / r and scatters runs at stride
// s, and after the last pass (n = r, no factor) y is the transform in natural
// order. A block takes c = min(2^10, N) / r consecutive t: a tile of r c <= 2^10
// cells, c consecutive cells per gathered row, and on the first pass (s = 1) one
// contiguous run of r c cells written. The r-point sums are radix-2
// decimation-in-frequency stages in LDS; the bit reversal they leave is undone
// by the address the output loop reads, and the last stage (twiddle 1) is folded
// into that read.
//
// Powers of 2^256 (R), phi = 1 for canonical and R for Montgomery cells: a cell
// is x phi and the transform is linear, so every constant is held as c R,
// mont_mul(x phi, c R) = c x phi, sums keep phi, and nothing is converted on
// load or store, in either form. The constants:
//
//   tw    omega_1024^(+-j) R, j < 512: the stage twiddle omega_(2 hh)^u is entry
//         u (512 / hh), one table for every k and radix, one per direction
//   w     the domain's omega_k table (pow_table.hpp): the factor between passes is
//         omega_N^e, e = s p i < N (inverse: N - e), one mont_mul to form, one to apply
//   f     per call, the table of shift^i R, the inverse's 2^-k its top factor: on
//         the first pass's load (forward) or the last pass's store (inverse);
//         without a shift the inverse multiplies by the constant 2^-k R and the
//         forward by nothing. No pass of their own.
//
// LDS layout: word-planar, sh[w][slot], the eight words of a cell in eight
// planes of 1024 dwords (32 KiB). Lanes at consecutive positions then read
// consecutive banks with ds_read_b32, where cells kept whole (32 B apart) would
// put a wave's 16-byte accesses on 8 of the 64 banks each. The slot is the
// position with its bits 5..9 folded onto bits 0..4 (XOR): positions that differ
// only above bit 4, which is what the bit-reversed read of the output loop and
// the gathers of the late stages touch, land on different banks, and a run of
// 32 consecutive positions still does.
//
// As grand_product.hpp asks: loops over stages, butterflies and cells stay
// rolled (#pragma unroll 1, one inlined mont_mul per use), no register arrays
// under a runtime index, 64-bit row indices.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pow_table.hpp"                                    // Fr, PowTable

namespace svdw {

static constexpr uint32_t kNttLogTile = 10;                // a tile is at most 2^10 cells
static constexpr unsigned kNttThreads = 256;
static constexpr uint32_t kNttEvalRun = 256;               // coefficients per thread of k_ntt_eval at the most

// Global-memory passes of a size-2^k transform, and the radix bits of pass i.
inline uint32_t ntt_passes(uint32_t k) { return k ? (k + kNttLogTile - 1) / kNttLogTile : 1; }
inline uint32_t ntt_pass_bits(uint32_t k, uint32_t i) {
    const uint32_t P = ntt_passes(k);
    return k / P + (i < k % P ? 1u : 0u);
}

// One pass. cols: the ncols column pointers of the first pass (device table),
// else null and src the ncols x 2^k cells of the pass before. post: 0 nothing,
// 1 the constant fc, 2 the table f, on the stored cell of the last pass; pre: f
// on the loaded cell (first pass).
struct NttPass {
    const Fr* const* cols;
    const Fr* src;
    Fr* dst;
    const Fr* tw;
    PowTable w, f;
    Fr fc;
    uint32_t k, kin, b, ls, ncols;
    uint32_t inverse, last, pre, post;
};
hipError_t launch_ntt_pass(const NttPass& a, hipStream_t st);

// Blocks per (column, point) of k_ntt_eval over n coefficients, and its run.
inline uint32_t ntt_eval_run(uint64_t n) {
    const uint64_t per = (n + kNttThreads - 1) / kNttThreads;
    return (uint32_t)(per < kNttEvalRun ? (per ? per : 1) : kNttEvalRun);
}
inline uint32_t ntt_eval_blocks(uint64_t n) {
    const uint64_t chunk = (uint64_t)kNttThreads * ntt_eval_run(n);
    return (uint32_t)((n + chunk - 1) / chunk);
}
// part[(col * npoints + q) * ntt_eval_blocks(n) + block] = the block's share of
// sum_i coeffs_col[i] x_q^i (cells in the coefficients' form), pts[q] = x_q R.
// npoints <= 65535 per launch.
hipError_t launch_ntt_eval(const Fr* const* cols, const Fr* src, uint64_t n, uint32_t ncols, const Fr* pts,
                           uint32_t npoints, Fr* part, hipStream_t st);
// out[col * out_stride + q] = the sum of the (col, q) partials.
hipError_t launch_ntt_eval_sum(const Fr* part, uint32_t nblocks, uint32_t ncols, uint32_t npoints, uint64_t out_stride,
                               Fr* out, hipStream_t st);
// The sampled row of sample s: q = 2^(k - log_samples) rows per stratum.
__host__ __device__ inline uint64_t ntt_sample_row(uint32_t k, uint32_t log_samples, uint64_t seed, uint64_t s) {
    const uint64_t q = 1ull << (k - log_samples);
    return s * q + ((seed + s * 0x9E3779B1ull) & (q - 1));
}
// vals[col * nsamp + i] against cell ntt_sample_row(s0 + i) of column col (cols
// or src as above, 2^k cells each): cnt[0] += rows, cnt[1] += rows that differ.
hipError_t launch_ntt_compare(const Fr* const* cols, const Fr* src, uint32_t k, uint32_t log_samples, uint64_t seed,
                              uint64_t s0, uint32_t nsamp, uint32_t ncols, const Fr* vals, unsigned long long* cnt,
                              hipStream_t st);

}  // namespace svdw
