// The lookup argument's grand-product column Z on the device
// (lookup_product.hip): halo2's lookup::prover::Permuted::commit_product for
// RangeChip's table, restated from memory (PARITY UNPINNED, include/svdw.h).
// With N[r] = (A[r] + beta)(T[r] + gamma), D[r] = (A'[r] + beta)(S'[r] + gamma)
// over the usable rows (a zero D[r] enters as D = 1, N = 0: ff's batch_invert
// leaves a zero zero),
//
//   Z[i] = prod_{r < i} N[r] * prod_{r >= i} D[r] * (prod_r D[r])^-1,
//
// a prefix product, a suffix product and one inversion per column:
//
//  k_lp_tiles   the products of N and of D over each tile of kLpTile rows
//  k_lp_carry   one block per column: exclusive prefix (N) and suffix (D) of
//               the tile products, the inverse, Z[usable] against 1
//  k_lp_write   the tile again: local prefix / suffix products, a block scan,
//               Z written in `form`
//  k_lp_check   the division-free recurrence, the boundary rows and the padding
//               (shares no scan and no inversion with the three above)
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
#include "lookup.hpp"

namespace svdw {

static constexpr uint32_t kLpTile = 1024;   // rows per tile
inline uint64_t lp_tiles(uint64_t rows) { return (rows + kLpTile - 1) / kLpTile; }

// The challenges as the kernels add them: to the canonical input column (b0,
// g0), to the permuted columns in their form (bx, gx), to T 2^512 (g2 = gamma
// 2^512, t2 = 2^544: one CIOS round of a row index by t2 is T 2^512);
// one = 2^256 mod p.
struct LpChal {
    Fr b0, g0, bx, gx, g2, t2, one;
};

// tp[(c * ntiles + t) * 2 + {0, 1}] = the products of N, of D over tile t of
// column c; cnt[0] += rows with a zero denominator.
hipError_t launch_lp_tiles(const LkSrc& src, const Fr* pin, const Fr* ptab, const LpChal& ch, int form,
                           uint32_t ncols, uint64_t rows, uint64_t usable, uint32_t lb, Fr* tp,
                           unsigned long long* cnt, hipStream_t st);
// tp in place: the carries k_lp_write multiplies in; cnt[1] += columns with Z[usable] != 1.
hipError_t launch_lp_carry(Fr* tp, const LpChal& ch, int form, uint32_t ncols, uint64_t rows, unsigned long long* cnt,
                           hipStream_t st);
// z (ncols x rows cells in `form`): rows [0, usable] the product, rows above zero.
hipError_t launch_lp_write(const LkSrc& src, const Fr* pin, const Fr* ptab, const LpChal& ch, int form,
                           uint32_t ncols, uint64_t rows, uint64_t usable, uint32_t lb, const Fr* tp, Fr* z,
                           hipStream_t st);
// cnt[0..1] += recurrence rows checked / failed, cnt[2..3] += boundary rows,
// cnt[4..5] += padding cells.
hipError_t launch_lp_check(const LkSrc& src, const Fr* pin, const Fr* ptab, const Fr* z, const LpChal& ch, int form,
                           uint32_t ncols, uint64_t rows, uint64_t usable, uint32_t lb, unsigned long long* cnt,
                           hipStream_t st);

}  // namespace svdw
