// A KZG structured reference string on the device (srs.hip): multiples of one
// fixed BN254 G1 base (g1.hpp) by n unrelated scalars, and the two scalar
// columns ParamsKZG::setup multiplies the generator by, s^i and l_i(s).
//
// Fixed-base multiplication with signed c-bit digits (g1_signed_digits,
// g1_mul.hpp): a scalar, as a canonical integer below r < 2^254, is cut into
// W = ceil(255 / c) digits d_w in (-2^(c-1), 2^(c-1)] with carry (no carry
// leaves the top window). The base is known, so every digit's multiple is
// looked up, not accumulated: the table
//
//   T[w][d - 1] = [d 2^(c w)] base,  1 <= d <= B = 2^(c-1),  w < W
//
// holds W B affine Montgomery points, and out[i] = sum_w sign(d_w) T[w][|d_w| - 1]
// is at most W mixed adds (a negative digit adds the entry with y -> q - y; a
// zero digit adds nothing). No doubling is left in the multiplication itself.
//
//  k_fb_windows   thread w < W: P_w = [2^(c w)] base by c w doublings, affine,
//                 into T[w][0]
//  k_fb_table     a thread per (w, d): [d] P_w by double-and-add over the bits
//                 of d (at most kCommitMaxBits of each), one inversion to
//                 affine. The table is built once per (base, c) and kept on the
//                 context (SrsState, engine_internal.hpp)
//  k_fb_mul       the multiplication. A block of kFbThreads threads owns
//                 kFbThreads kFbGroup consecutive outputs; thread t takes
//                 outputs t, t + kFbThreads, ... of them (the scalars and the
//                 results stay coalesced), one at a time:
//                   forward   the W gathered mixed adds into an XYZZ accumulator
//                             in registers; the accumulator goes to acc[i], the
//                             running product of the ZZZ so far to pre[i]
//                   invert    one fq_inv of the product of the group's ZZZ
//                   backward  1 / ZZZ_i = inv pre[i], inv <- inv ZZZ_i, then
//                             1 / ZZ = (ZZ / ZZZ)^2, x = X / ZZ, y = Y / ZZZ
//                             (g1_affine_shared_inv, g1_mul.hpp)
//                 An identity accumulator (ZZZ = 0) takes no part in the product
//                 and is written as (0, 0). One launch may serve two arrays
//                 (FbMul::split): the setup multiplies both columns of a piece
//                 at once. A wave lives for its 8 outputs, about 4 ms, and the
//                 kernel's 132 VGPRs allow 3 waves per SIMD, 3072 on the device:
//                 a launch runs in rounds of 3072 waves (1.5 M outputs) and ends
//                 in a round that is partly empty, so fewer, larger launches
//                 are faster (2^20 rows: 7.9 ms in one launch, 9.8 ms in two).
//
// The inversion is shared PER THREAD (Montgomery's trick over the kFbGroup
// outputs of one thread), not per wave: a thread's outputs meet only in its own
// registers, so no LDS, no barrier and no lane exchange is needed, and the
// ragged end of a call needs no care beyond i < n. fq_inv costs 512 products
// (it squares and multiplies at every bit of q - 2), so an output costs
//
//   10 W  (adds)  +  1 (prefix)  +  2 (backward)  +  4 (to affine)  +  512 / kFbGroup
//
// products: 220 + 7 + 64 = 291 at c = 12, against 220 + 4 + 512 = 736 with an
// inversion per output. A larger group shares more but leaves fewer threads:
// at 2^20 outputs kFbGroup = 8 still gives 2^17 threads, two waves per SIMD.
// acc and pre are global scratch of the call (kFbRowBytes per output), private
// to the thread between the two passes.
//
// fb_plan picks c: the table must stay resident in one XCD's 4 MiB L2
// (W B 64 B: 2.75 MiB at c = 12, 5 MiB at c = 13), and below that the c with the
// fewest products, 10 W per output and about 800 per table entry.
//
// The scalar columns of the setup, for rows [i0, i0 + m) of a size-2^k domain,
// in Montgomery form:
//
//  k_srs_powers    s^i from the two-level table of s (pow_table.hpp)
//  k_srs_lagrange  l_i(s) = (s^n - 1) omega^i / (n (s - omega^i)): omega^i from the
//                  domain's table, the m inverses by Montgomery's trick over Fr,
//                  one fr inversion per thread and kSrsInvGroup rows (the prefix
//                  products wait in the output column itself). When s lies in
//                  the domain (s^n = 1) the quotient is 0 / 0 and the column is
//                  the indicator of s = omega^i instead.
//
// As g1.hpp and commit.hpp ask: loops over points stay rolled, no register
// array is indexed at run time (the digits shift the scalar down), row indices
// are 64-bit, and exactly n points are written. The base and the outputs change
// form through g1.hpp's g1_affine_to_mont and g1_affine_to_form alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "commit.hpp"
#include "pow_table.hpp"

namespace svdw {

static constexpr unsigned kFbThreads = 64;                 // one wave per block
static constexpr uint32_t kFbGroup = 8;                    // outputs per thread: they share one Fq inversion
static constexpr uint32_t kFbMaxTableBits = 12;            // the planned window at the most (the table stays in L2)
static constexpr uint64_t kFbRowBytes = sizeof(G1Xyzz) + sizeof(Fq);   // acc and pre of one output
static constexpr uint32_t kSrsInvGroup = 8;                // rows per thread of k_srs_lagrange: one Fr inversion
static constexpr unsigned kSrsThreads = 64;

inline uint32_t fb_windows(uint32_t c) { return (255 + c - 1) / c; }
// The window of a call: its bits c and W = fb_windows(c).
struct G1Window {
    uint32_t c, W;
};
inline uint64_t fb_table_points(uint32_t c) { return (uint64_t)fb_windows(c) << (c - 1); }
// The window of n outputs: the c in [2, kFbMaxTableBits] with the fewest
// products, 10 W per output and 800 per table entry (an inversion and a
// double-and-add); the smallest c among equal costs.
inline uint32_t fb_plan(uint64_t n) {
    uint32_t best = 2;
    double cost = 0;
    for (uint32_t c = 2; c <= kFbMaxTableBits; ++c) {
        const double v = 10.0 * fb_windows(c) * (double)n + 800.0 * (double)fb_table_points(c);
        if (c == 2 || v < cost) {
            cost = v;
            best = c;
        }
    }
    return best;
}

// table[w B + d - 1] = [d 2^(c w)] base (Montgomery affine), base given in base_form.
hipError_t launch_fb_table(G1Affine base, int base_form, uint32_t c, G1Affine* table, hipStream_t st);

struct FbMul {
    const G1Affine* table;                                 // fb_table_points(c) points
    const Fr* scalars;                                     // n cells in `form`
    G1Affine* out;                                         // outputs [0, split) in base_form
    G1Affine* out2;                                        // outputs [split, n), from out2[0] on (split == n: unused)
    G1Xyzz* acc;                                           // n accumulators (scratch)
    Fq* pre;                                               // n prefix products (scratch)
    unsigned long long* cnt;                               // [0] zero scalars, [1] identity outputs; [2], [3]: of out2
    uint64_t n, split;
    uint32_t c, W;
    int form, base_form;
};
hipError_t launch_fb_mul(const FbMul& a, hipStream_t st);

// out[j] = s^(i0 + j) R for j < m; pw: the table of s over k bits (device view).
hipError_t launch_srs_powers(PowTable pw, uint64_t i0, uint64_t m, Fr* out, hipStream_t st);
// out[j] = l_(i0 + j)(s) R for j < m. sR = s R; coef = (s^n - 1) / n R; dom: the
// domain's omega_k table (device view); in_domain: s^n = 1, the indicator column.
hipError_t launch_srs_lagrange(PowTable dom, Fr sR, Fr coef, bool in_domain, uint64_t i0, uint64_t m, Fr* out,
                               hipStream_t st);

}  // namespace svdw
