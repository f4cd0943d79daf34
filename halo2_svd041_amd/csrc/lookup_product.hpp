// The lookup argument's grand-product column Z on the device
// (lookup_product.hip): halo2's lookup::prover::Permuted::commit_product for
// RangeChip's table, restated from memory (PARITY UNPINNED, include/svdw.h).
// With N[r] = (A[r] + beta)(T[r] + gamma), D[r] = (A'[r] + beta)(S'[r] + gamma)
// over the usable rows (a zero D[r] enters as D = 1, N = 0: ff's batch_invert
// leaves a zero zero),
//
//   Z[i] = prod_{r < i} N[r] * prod_{r >= i} D[r] * (prod_r D[r])^-1,
//
// a prefix product, a suffix product and one inversion per column: the passes
// of grand_product.hpp (profiled as k_lp_tiles, k_lp_write, k_lp_check) over
// this argument's leaf, with one carry kernel between tiles and write:
//
//  k_lp_carry   one block per column: exclusive prefix (N) and suffix (D) of
//               the tile products, the inverse, Z[usable] against 1
//
// Factors are multiplied with mont_mul in whatever power of 2^256 the form
// hands them over in (canonical cells: 2^-256 per factor pair, Montgomery
// cells: 2^256), the same for N and D; products are combined as a tree whose
// neutral element is 2^256 mod p, so every Z[i] and the column's product of D
// carry one and the same power, which the inverse cancels. No cell is
// converted on load and none on store.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fr.hpp"
#include "grand_product.hpp"
#include "lookup.hpp"

namespace svdw {

// The challenges as the kernels add them: to the canonical input column (b0,
// g0), to the permuted columns in their form (bx, gx), to T 2^512 (g2 = gamma
// 2^512, t2 = 2^544: one CIOS round of a row index by t2 is T 2^512);
// one = 2^256 mod p.
struct LpChal {
    Fr b0, g0, bx, gx, g2, t2, one;
};
// What the row kernels read: the input columns (src), the permuted columns A',
// S' (pin, ptab: ncols x rows cells in `form`, device memory), the challenges.
struct LpArgs {
    LkSrc src;
    const Fr *pin, *ptab;
    LpChal ch;
    uint32_t ncols, lb;
    uint64_t rows, usable;
};

// tp[(c * ntiles + t) * 2 + {0, 1}] = the products of N, of D over tile t of
// column c; cnt[0] += rows with a zero denominator.
hipError_t launch_lp_tiles(const LpArgs& a, int form, Fr* tp, unsigned long long* cnt, hipStream_t st);
// tp in place: the carries k_lp_write multiplies in; cnt[1] += columns with Z[usable] != 1.
hipError_t launch_lp_carry(const LpArgs& a, int form, Fr* tp, unsigned long long* cnt, hipStream_t st);
// z (ncols x rows cells in `form`): rows [0, usable] the product, rows above zero.
hipError_t launch_lp_write(const LpArgs& a, int form, const Fr* tp, Fr* z, hipStream_t st);
// cnt[0..1] += recurrence rows checked / failed, cnt[2..3] += boundary rows,
// cnt[4..5] += padding cells.
hipError_t launch_lp_check(const LpArgs& a, int form, const Fr* z, unsigned long long* cnt, hipStream_t st);

}  // namespace svdw

