// What the G1 scalar-multiplication kernels share (commit.hip, srs.hip,
// g1_fft.hip): the signed-digit recoder of a scalar and one backward step of the
// inversion shared over XYZZ accumulators. The form rule of affine points
// (g1_affine_to_mont, g1_affine_to_form) is g1.hpp's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fr.hpp"
#include "g1.hpp"

namespace svdw {

// The signed c-bit digits of s, a canonical integer below r < 2^254:
// emit(window, |d_w|, d_w < 0) for every window w < W, zero digits included,
// with s = sum_w d_w 2^(c w). A window's c bits plus the carry from below give
// d in [0, 2^c]; d > 2^(c-1) becomes d - 2^c and carries one up, so d_w lies in
// (-2^(c-1), 2^(c-1)]. W c >= 255 leaves no carry out of the top window. The
// scalar is shifted down c bits per window, so no word of it is indexed at run
// time (a register array under a runtime index goes to scratch).
template <class Emit>
__device__ __forceinline__ void g1_signed_digits(Fr s, uint32_t c, uint32_t W, Emit&& emit) {
    const uint32_t full = 1u << c, half = full >> 1;
    uint32_t carry = 0;
#pragma unroll 1
    for (uint32_t w = 0; w < W; ++w) {
        const uint32_t d = (s.w[0] & (full - 1)) + carry;
#pragma unroll
        for (int i = 0; i < 7; ++i) s.w[i] = (s.w[i] >> c) | (s.w[i + 1] << (32 - c));
        s.w[7] >>= c;
        carry = d > half;
        emit(w, carry ? full - d : d, carry);
    }
}

// One backward step of Montgomery's trick over the ZZZ of non-identity
// accumulators: inv holds 1 / (ZZZ_0 .. ZZZ_i) and prefix ZZZ_0 .. ZZZ_(i-1), so
// 1 / ZZZ_i = inv prefix and inv <- inv ZZZ_i; then 1 / ZZ = (ZZ / ZZZ)^2,
// x = X / ZZ, y = Y / ZZZ. The affine point of acc in `form`.
__device__ __forceinline__ G1Affine g1_affine_shared_inv(const G1Xyzz& acc, const Fq& prefix, Fq& inv, int form) {
    const Fq i3 = fq_mul(inv, prefix);
    inv = fq_mul(inv, acc.zzz);
    const Fq i2 = fq_sqr(fq_mul(acc.zz, i3));
    G1Affine r;
    r.x = fq_mul(acc.x, i2);
    r.y = fq_mul(acc.y, i3);
    return g1_affine_to_form(r, form);
}

inline unsigned blocks_of(uint64_t n, uint64_t per) { return (unsigned)((n + per - 1) / per); }

}  // namespace svdw
