// Transforms over BN254 G1 on the device (g1_fft.hip): the multiplication of n
// unrelated points by n unrelated scalars, and on top of it the radix-2 FFT
// over the group that ParamsKZG's g_to_lagrange is (an inverse FFT of the SRS's
// g), which is what `downsize` of a ceremony file needs.
//
// Variable-base multiplication with signed c-bit digits (g1_signed_digits,
// g1_mul.hpp): a scalar, as a canonical integer below r < 2^254, is cut into
// W = ceil(255 / c) digits d_w in (-2^(c-1), 2^(c-1)] with carry. Neither side
// is known ahead, so every point gets a table of its own and the doublings stay:
//
//  k_g1_table   thread i: T[d - 1][i] = [d] P_i for 1 <= d <= B = 2^(c-1), in
//               XYZZ, by B - 1 complete adds in one rolled loop. The table is
//               global scratch laid out [d][i], so a wave's entries of one d are
//               contiguous
//  k_g1_mul     thread i: the W digits go to LDS (a byte each, |d| and the sign;
//               W bytes x 64 lanes <= 8 KiB per block), because they are made
//               bottom up, carries included, and walked top down. Then per
//               window c doublings and one complete add of T[|d| - 1][i], y
//               negated for a negative digit; a zero digit adds nothing. Every
//               lane doubles c times per window whatever its digits, so a wave
//               diverges on zero digits only. The product goes to dst
//  k_g1_butterfly  a stage's (a + p, a - p) over the working array, p the
//               product k_g1_mul left, both adds in one rolled loop. A kernel of
//               its own: inside k_g1_mul it cost 256 VGPRs and 224 B of scratch
//               per lane, apart it costs a 128 B store and load per butterfly
//  k_g1_affine  XYZZ -> affine, k_fb_mul's forward / invert / backward without
//               the adds: a thread takes kFbGroup points (srs.hpp), multiplies
//               their ZZZ up, inverts once (fq_inv) and walks back by the same
//               step (g1_affine_shared_inv, g1_mul.hpp). The prefix products
//               wait in the output points themselves, so there is no scratch.
//               An identity (ZZ = 0) takes no part and is written (0, 0)
//
// A multiplication costs 9 c W (doublings) + 14 W (adds, a few less for zero
// digits) + 14 (B - 1) (table) field products: 4110, 3527, 3298, 3219, 3358 at
// c = 2 .. 6. g1_plan takes the cheapest c <= kG1PlanBits = 4 whose scratch,
// (B + 1) 128 B per point (table and accumulator), leaves a piece of 2^17 points
// (the device's 1024 SIMDs at two waves each) under the cap (the option
// "commit_scratch_mib"). c = 5 has 2.4 % fewer products and twice the table:
// measured, a 2^20 transform takes 368 ms at c = 4 and 433 ms at
// c = 5, whose stages no longer fit the default cap in one piece, and a 2^16
// transform 54.8 against 53.2 ms. 5 and 6 stay available as window_bits.
//
// The transform, out[i] = sum_j [omega^(+-i j)] in[j], natural order both sides,
// decimation in time over a working array of n = 2^k XYZZ points:
//
//  k_g1_fft_first  bit reversal and stage 0 in one: thread t reads the affine
//                  in[rev(t)] and in[rev(t) + n / 2] (rev over k - 1 bits) and
//                  writes a + b, a - b (mixed adds); the twiddle is 1
//  stage s < k     butterflies t < n / 2 on (ia, ia + 2^s), ia = (t >> s) 2^(s+1)
//                  + j, j = t mod 2^s, twiddle omega^(+-j 2^(k-1-s)) from the
//                  domain's table (pow_table.hpp), canonical for its digits:
//                  k_g1_table, k_g1_mul and k_g1_butterfly over pieces of
//                  butterflies under the cap. j = 0 (twiddle 1) multiplies
//                  nothing. Stages are not fused: a stage moves 256 B per
//                  butterfly and multiplies for some 3,000 field products
//  inverse         the last stage folds 2^-k in, [c] a +- [c w] b: one pass of
//                  k_g1_mul that scales the a half in place, then the
//                  stage with c w for w and nothing skipped; n / 2 more
//                  multiplications than forward, where a scaling pass costs n.
//                  At k = 1 the first stage is the last: both sums are scaled
//  k_g1_affine     the working array to `out`
//
// so k n / 2 - n + 1 multiplications forward and k n / 2 - n / 2 + 2 inverse
// (counted on the device, G1Mul::cnt[3]).
//
// As g1.hpp asks: each law is instantiated once per kernel in a rolled loop,
// no register array is indexed at run time (the digits wait in LDS, the table
// in global memory), indices are 64-bit, exactly n points are written. Points
// change form through g1.hpp's g1_affine_to_mont and g1_affine_to_form alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "commit.hpp"
#include "pow_table.hpp"
#include "srs.hpp"

namespace svdw {

static constexpr unsigned kG1Threads = 64;                 // one wave per block: its digits are 64 W bytes of LDS
static constexpr uint32_t kG1MaxBits = 6;                  // window bits at the most (|d| <= 32 and the sign in a byte)
static constexpr uint32_t kG1PlanBits = 4;                 // the planned window at the most
static constexpr uint32_t kG1MaxWindows = 128;             // fb_windows(2)
static constexpr uint64_t kG1PlanPoints = 131072;          // g1_plan: the points a piece should hold at the least
static constexpr uint32_t kG1Linear = 62;                  // G1Mul::shift of a point array taken in order

// Scratch bytes per point: the B table entries and the accumulator.
inline uint64_t g1_point_bytes(uint32_t c) { return ((1ull << (c - 1)) + 1) * sizeof(G1Xyzz); }
// Field products of one multiplication: doublings, W adds, the table's adds.
inline uint32_t g1_mul_products(uint32_t c) {
    return 9 * c * fb_windows(c) + 14 * fb_windows(c) + 14 * ((1u << (c - 1)) - 1);
}
// The window: the cheapest c in [2, kG1PlanBits] among those whose scratch for
// kG1PlanPoints points fits cap_bytes, the smallest c among equal costs; 2 when
// none fits.
inline uint32_t g1_plan(uint64_t cap_bytes) {
    uint32_t best = 2;
    for (uint32_t c = 3; c <= kG1PlanBits; ++c)
        if (g1_point_bytes(c) * kG1PlanPoints <= cap_bytes && g1_mul_products(c) < g1_mul_products(best)) best = c;
    return best;
}

// One piece of multiplications: items t in [t0, t0 + m) of a call.
//   point   src is affine (points, in bases_form) or XYZZ (work); item t's point
//           is element idx(t) = ((t >> shift) << (shift + 1)) + (t & (2^shift - 1))
//           + offset: t itself for shift = kG1Linear, offset = 0, and a stage's b
//           for shift = s, offset = 2^s
//   scalar  scalars[t] in `form` (twiddle == 0), or factor * omega^e from the
//           domain's table, e = (t & tw_mask) << tw_shift and n - e for the
//           inverse; skip_one: e == 0 is not multiplied (the point is the result)
//   result  dst[dst_linear ? t - t0 : idx(t)]; launch_g1_butterfly then writes
//           the sum and the difference of work[idx(t) - offset] and dst[t - t0]
//           (a skipped item: work[idx(t)]) to work[idx(t) - offset], work[idx(t)]
struct G1Mul {
    const G1Affine* points;
    G1Xyzz* work;
    const Fr* scalars;
    G1Xyzz* table;                                         // [B][m]
    G1Xyzz* dst;
    PowTable dom;
    Fr factor;                                             // Montgomery
    unsigned long long* cnt;                               // [0] zero scalars, [1] identity inputs, [3] multiplications
    uint64_t t0, m, offset, tw_mask, n;
    uint32_t shift, tw_shift, c, W;
    int form, bases_form, twiddle, inverse, has_factor, skip_one, dst_linear;
};
hipError_t launch_g1_table(const G1Mul& a, hipStream_t st);
hipError_t launch_g1_mul(const G1Mul& a, hipStream_t st);
hipError_t launch_g1_butterfly(const G1Mul& a, hipStream_t st);
// out[i] = src[i] as an affine point in bases_form for i < n; cnt[2] += identities.
hipError_t launch_g1_affine(const G1Xyzz* src, uint64_t n, int bases_form, G1Affine* out, unsigned long long* cnt,
                            hipStream_t st);
// work[2 t], work[2 t + 1] = in[rev(t)] +- in[rev(t) + n / 2] for t < n / 2 = 2^(k-1); cnt[1] += identity inputs.
hipError_t launch_g1_fft_first(const G1Affine* in, uint32_t k, int bases_form, G1Xyzz* work, unsigned long long* cnt,
                               hipStream_t st);

}  // namespace svdw
