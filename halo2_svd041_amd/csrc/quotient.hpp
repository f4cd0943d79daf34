// The quotient polynomial on the extended domain (quotient.hip): halo2's
// evaluate_h for halo2-base's vertical gate, the permutation argument and the
// lookup arguments, folded with powers of y and divided by X^n - 1. Restated
// from memory (PARITY UNPINNED); include/svdw.h ("quotient") has the rule and the
// order of the expressions. N = 2^ek rows, E = 2^le = N / n.
//
// A thread owns one extended row j. A rotation by r rows of the original domain
// is the same column at row (j + r E) mod N: the lanes of a wave still read
// consecutive cells. The fold is a Horner chain in y, h <- h y + e.
//
// Powers of 2^256 (R), phi = 1 for canonical and R for Montgomery cells: a cell
// is x phi and h is kept as h phi. The expressions mix degrees, so a canonical
// cell cannot ride through as in the transforms; what is fixed instead:
//
//   a multiplier that is a constant or one of the engine's own columns (y, beta,
//   X_j, l_0, l_last, l_active, the divisor's inverse) is held as c R:
//   mont_mul(c R, x phi) = c x phi in either form, nothing to convert;
//   an addend that is a constant (gamma, beta, 1) is held as c phi;
//   a product of two cell-derived values converts one operand first,
//   mont_mul(mont_mul(x, R^2), y) = x y: that one extra multiplication per
//   cell-by-cell product is what the canonical form pays (Montgomery: none).
//
// Multiplications (mont_mul) per row, Montgomery form, + those the canonical
// form adds:
//
//   a gate                   3   (+2)   a1 a2, q (..), the fold
//   the permutation          2          X_j R from the omega_e table (pow_table.hpp)
//                                       and the shift (once per row)
//                          + 5   (+1)   l_0 (1 - Z_0), l_last Z (Z - 1), two folds
//                          + 2          per set after the first: the chain and its fold
//                          + 2          per set: l_active (..) and its fold
//                          + 4   (+2)   per column: beta sigma_j, (beta delta^j) X_j
//                                       and the two running products
//   a lookup argument       16   (+6)   2 + 3 + 6 + 2 + 3 for its five expressions
//   the division             1          by the table of E inverses
//
// quotient_muls below is this count; the l columns cost three loads, not
// multiplications. As grand_product.hpp asks: every loop over a family's
// columns stays rolled (#pragma unroll 1), row indices are 64-bit, nothing is
// indexed at run time in registers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pow_table.hpp"                                    // Fr, PowTable

namespace svdw {

static constexpr unsigned kQuotientThreads = 256;

struct QuotientArgs {
    // device table of column pointers, N cells each in the cells' form:
    // advice[ng], selectors[ng], v[np], sigma[np], Z[nsets], then A, T, A', S', Z
    // of the lookups, [nl] each
    const Fr* const* ptrs;
    const Fr* bd;                       // beta delta^j phi, j < np
    PowTable w;                         // the omega_e table of the extended domain
    const Fr* inv;                      // (shift^n (omega_e^n)^i - 1)^-1 R, i < E
    const Fr *l0, *llast, *lact;        // N cells each, l(X_j) R
    Fr* out;                            // N cells, h_ext phi
    Fr y, beta, shift;                  // c R
    Fr gamma, betaf, one;               // c phi
    uint32_t ek, le, ng, np, chunk, nsets, nl;
    uint64_t usable;
};
// form: kFormCanonical / kFormMontgomery of the cells and of out.
hipError_t launch_quotient(const QuotientArgs& a, int form, hipStream_t st);
inline uint64_t quotient_muls(uint32_t ng, uint32_t np, uint32_t nsets, uint32_t nl, bool canonical) {
    uint64_t m = (uint64_t)ng * (canonical ? 5 : 3) + (uint64_t)nl * (canonical ? 22 : 16) + 1;
    if (np) m += 2 + (canonical ? 6 : 5) + 2 * (uint64_t)(nsets - 1) + 2 * (uint64_t)nsets +
                 (uint64_t)np * (canonical ? 6 : 4);
    return m;
}

// out[0 .. 3 n): the Lagrange columns of l_0, l_last, l_active over n rows, the
// ones as `one`.
hipError_t launch_quotient_basis(Fr* out, uint64_t n, uint64_t usable, const Fr& one, hipStream_t st);
// cnt[0] += the cells of h[from, N), cnt[1] += those that are not zero.
hipError_t launch_quotient_tail(const Fr* h, uint64_t from, uint64_t N, unsigned long long* cnt, hipStream_t st);

}  // namespace svdw
