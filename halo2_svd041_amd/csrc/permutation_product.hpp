// The permutation (copy-constraint) argument's grand-product columns Z on the
// device (permutation_product.hip): halo2's permutation::prover::Argument::commit,
// restated from memory (PARITY UNPINNED, include/svdw.h). The ncols columns are
// cut into sets of chunk columns; with, over the usable rows,
//
//   N_s[r] = prod_{j in set s} (v_j[r] + beta delta^j omega^r + gamma)
//   D_s[r] = prod_{j in set s} (v_j[r] + beta sigma_j[r] + gamma)
//
// (a zero D_s[r] enters as D = 1, N = 0: ff's batch_invert leaves a zero zero),
//
//   Z_s[i] = start_s * prod_{r < i} N_s[r] * prod_{r >= i} D_s[r] * (prod_r D_s[r])^-1
//   start_0 = 1,  start_{s+1} = start_s * prod_r N_s[r] * (prod_r D_s[r])^-1 = Z_s[usable]
//
// a prefix product, a suffix product and one inversion per set, the sets of one
// call in the same launches (a set per blockIdx.y): the passes of
// grand_product.hpp (profiled as k_pp_tiles, k_pp_write, k_pp_check) over this
// argument's leaf, with a carry stage of three kernels between tiles and write,
// as only it sees the chain, and
//
//  k_pp_totals  one block per set: exclusive prefix (N) and suffix (D) of the
//               tile products per thread, the set's totals, the inverse
//  k_pp_chain   one thread: the nsets starts, each folded into its set's
//               inverse; the last Z[usable] against 1
//  k_pp_fold    one block per set: the tile carries k_pp_write multiplies in
//  k_pp_values  sigma cells delta^col omega^row from a (col, row) mapping
//
// Powers of 2^256 (R), phi = 1 for canonical and R for Montgomery cells: a cell
// is x phi. beta sigma_j is mont_mul(sigma phi, beta R) = beta sigma phi, the
// identity term mont_mul(omega^r R, beta delta^j phi) = beta delta^j omega^r phi,
// gamma is added as gamma phi: every factor is its value times phi, in both
// forms, and nothing is converted on load or store. Products are mont_mul trees
// whose neutral element is R, so a leaf of m factors is R (phi / R)^m times its
// value, the same for N_s and D_s (both have the set's m factors, a shorter
// last set included), and every Z_s[i] and the set's product of D carry one and
// the same power, which the set's inverse cancels. The starts are kept as
// start R and meet the inverse in one mont_mul.
//
// omega^r comes from the domain's omega_k table (PowTable, pow_table.hpp), one
// mont_mul per row, shared by the set's columns; k_pp_check takes the table for
// a thread's first row only and steps by omega^(its grid stride) from there.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "grand_product.hpp"
#include "pow_table.hpp"                                    // Fr, PowTable

namespace svdw {

// What the row kernels read, all in device memory. cols / sig: ncols column
// base pointers each; bd[j] = beta delta^j phi; w the omega_k table of the
// rows' k. bR = beta R, g = gamma phi, one = R.
struct PpArgs {
    const Fr* const* cols;
    const Fr* const* sig;
    const Fr* bd;
    PowTable w;
    uint32_t ncols, chunk, nsets;
    uint64_t rows, usable;
    Fr bR, g, one;
};
inline uint32_t pp_sets(uint32_t ncols, uint32_t chunk) { return (ncols + chunk - 1) / chunk; }
// Cells of scratch behind tp: per set kGpThreads x 2 thread carries, 2 set values.
inline uint64_t pp_scratch_cells(uint32_t nsets, uint64_t rows) {
    return (uint64_t)nsets * (2 * gp_tiles(rows) + 2 * kGpThreads + 2);
}

// tp[(s * ntiles + t) * 2 + {0, 1}] = the products of N_s, of D_s over tile t;
// cnt[0] += rows with a zero denominator.
hipError_t launch_pp_tiles(const PpArgs& a, int form, Fr* tp, unsigned long long* cnt, hipStream_t st);
// The carry stage (xs, sv: the scratch behind tp). Totals: xs = each thread's
// carries over its run of tiles, sv = per set the factor to the next start and
// the inverse. Chain: sv = per set the start and the inverse times the start;
// cnt[1] += 1 if the last set's Z[usable] != 1. Fold: tp in place, the carries
// k_pp_write multiplies in.
hipError_t launch_pp_totals(const PpArgs& a, int form, const Fr* tp, Fr* xs, Fr* sv, hipStream_t st);
hipError_t launch_pp_chain(const PpArgs& a, Fr* sv, unsigned long long* cnt, hipStream_t st);
hipError_t launch_pp_fold(const PpArgs& a, int form, Fr* tp, const Fr* xs, const Fr* sv, hipStream_t st);
// z (nsets x rows cells in `form`): rows [0, usable] the product, rows above zero.
hipError_t launch_pp_write(const PpArgs& a, int form, const Fr* tp, Fr* z, hipStream_t st);
// cnt[0..1] += recurrence rows checked / failed, cnt[2..3] += boundary rows,
// cnt[4..5] += padding cells. wstep = omega^(grid stride of the launch) R, from
// pp_check_stride.
uint64_t pp_check_stride(uint64_t rows);
hipError_t launch_pp_check(const PpArgs& a, int form, const Fr* z, const Fr& wstep, unsigned long long* cnt,
                           hipStream_t st);
// out (ncols x rows cells in `form`): delta^col omega^row of mapping[i] =
// col << 32 | row, or of (first_col + i / rows, i % rows) without a mapping;
// dl[c] = delta^c phi for c < total_cols, w the rows' omega table. An entry with
// col >= total_cols or row >= rows is written as zero; cnt[0] += those.
hipError_t launch_pp_values(const uint64_t* mapping, const Fr* dl, const PowTable& w, uint32_t first_col,
                            uint32_t ncols, uint32_t total_cols, uint64_t rows, Fr* out, unsigned long long* cnt,
                            hipStream_t st);

}  // namespace svdw
