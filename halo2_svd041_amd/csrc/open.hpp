// The SHPLONK opening's polynomial work on the device (open.hip): linear
// combinations of coefficient columns and the division of a polynomial by
// (X - s), dropping the remainder. The rule the entries build from them (fold
// per rotation set, quotient per set, h1, the linearisation G and h2) is
// include/svdw.h's, "openings"; restated from memory, PARITY UNPINNED.
//
//  k_open_fold   out[r] = sum_j c_j col_j[r] (+ c_acc acc[r]) over a device table
//                of column pointers and per-column scalars; the scalars carry
//                the Horner powers (y^e for F_i; c_i v^e y^e' for G), so one
//                kernel serves the fold per set, G and svdw_linear_combination
//
// Division by (X - s) of a[0..n) is the affine suffix scan
//
//   q[i] = sum_{j > i} a[j] s^(j - i - 1),   remainder a[0] + s q[0] = a(s),
//
// in the shape of grand_product.hpp:
//
//  k_open_tiles  T[t] = sum_l a[t kOpenTile + l] s^l: the value of tile t at its
//                first coefficient; one wave per tile, a Horner in s^64 per lane
//                over its strided (coalesced) coefficients, times s^lane, summed
//                over the lanes
//  k_open_carry  C[t] = sum_{u > t} T[u] S^(u - t - 1), S = s^kOpenTile: the same
//                scan over the tile totals, in place, one block, kOpenCarryCap
//                totals per round, one per thread; with more than one round a
//                thread's totals are consecutive (a run: Horner down it, the
//                block scan over the runs, down it again), as gp_run does
//  k_open_write  the tile again: a thread's kOpenItems consecutive coefficients by
//                Horner, a block scan of (value, s^len) pairs seeded with C[t]
//                (every run has the same length, so the pair's second half is
//                one squaring per scan step for the whole block), then the
//                thread's q by synthetic division from what enters above it.
//                Stores q, or out <- out v + q for the last division of a set
//                (h1 <- h1 v + Q_i without a pass of its own); tile 0 hands out
//                the remainder. out may be a: a thread reads its own cells
//                before it writes them, and no other thread's.
//
// Powers of s come from a per-point table (PowTable, pow_table.hpp) over
// 2^open_pow_bits(k) exponents: one mont_mul to form, one to apply, no chains of
// multiplications per thread. s = 0 and s = 1 are ordinary points of it (0^0 = 1).
//
// Powers of R = 2^256 as ntt.hpp explains: a cell is x phi, every constant is
// held as c R, mont_mul(x phi, c R) = c x phi, sums keep phi: nothing is
// converted on load or store and the kernels do not know the form.
//
// As grand_product.hpp asks: loops around mont_mul stay rolled, no register
// array under a runtime index, 64-bit row indices, no scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pow_table.hpp"                                    // Fr, PowTable

namespace svdw {

static constexpr uint32_t kOpenLogTile = 9;
static constexpr uint32_t kOpenTile = 512;                     // coefficients per tile
static constexpr unsigned kOpenThreads = 128, kOpenWaves = kOpenThreads / 64;
static constexpr unsigned kOpenItems = 4;                      // consecutive coefficients per thread of k_open_write
static constexpr uint32_t kOpenCarryCap = 128;                 // tile totals per round of k_open_carry: one per thread
static constexpr unsigned kOpenFoldThreads = 256, kOpenFoldBlocks = 8192;   // k_open_fold: a grid-stride loop over rows
static_assert(kOpenTile == kOpenThreads * kOpenItems && kOpenTile == 1u << kOpenLogTile, "tile");
static_assert(kOpenCarryCap == kOpenThreads, "one total per thread and round");

inline uint64_t open_tiles(uint64_t n) { return (n + kOpenTile - 1) / kOpenTile; }
// The exponents a point's table covers for 2^k coefficients: 2^open_pow_bits(k).
inline uint32_t open_pow_bits(uint32_t k) { return k < kOpenLogTile ? kOpenLogTile : k; }

// out[r] = sum_{j < ncols} sc[j] cols[j][r] + (acc ? cacc acc[r] : 0), r < n.
// cols, sc: device tables; sc[j] and cacc as c R.
hipError_t launch_open_fold(const Fr* const* cols, const Fr* sc, uint32_t ncols, const Fr* acc, const Fr& cacc,
                            uint64_t n, Fr* out, hipStream_t st);
// tot[t] = the value of tile t of a[0..n) at its first coefficient, t < open_tiles(n).
hipError_t launch_open_tiles(const Fr* a, uint64_t n, const PowTable& pw, Fr* tot, hipStream_t st);
// In place: tot[t] becomes the carry of tile t, what the tiles above it are worth
// at its end.
hipError_t launch_open_carry(Fr* tot, uint64_t nt, const PowTable& pw, hipStream_t st);
// out[0..n) = the quotient of a by (X - s), or out v + it with v (as v R) given;
// carry: launch_open_carry's, null for a single tile. rem, if given, gets a(s).
hipError_t launch_open_write(const Fr* a, uint64_t n, const PowTable& pw, const Fr* carry, const Fr* v, Fr* out,
                             Fr* rem, hipStream_t st);

}  // namespace svdw
