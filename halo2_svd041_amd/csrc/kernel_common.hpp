// Device helpers shared by kernels.hip and gemm.hip: reading an operand view
// and the 9-word reduction mod p. (ld_fr, st_fr and quantize_fr: export.hpp,
// shared with the read-out kernels.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fr.hpp"
#include "prog.hpp"
#include "export.hpp"

namespace svdw {

__device__ __forceinline__ double f64_scale(const DView& v) { return ldexp(1.0, (int)v._r0); }
// X(i, j) of a view; `pad` is the value outside the view (K[v.pad_k]).
__device__ __forceinline__ Fr view_load(const DView v, const Fr pad, uint32_t i, uint32_t j) {
    if (v.mode == VIEW_DIAG) return (i == j) ? ld_fr(v.ptr) : pad;
    if (v.mode == VIEW_F64) {
        if (i < v.rows && j < v.cols)
            return quantize_fr(reinterpret_cast<const double*>(v.ptr)[(int64_t)i * v.rs + (int64_t)j * v.cs],
                               f64_scale(v));
        return pad;
    }
    if (i < v.rows && j < v.cols) return ld_fr(v.ptr + (int64_t)i * v.rs + (int64_t)j * v.cs);
    return pad;
}

// x mod p for a 9-word x < 2^270
__device__ __forceinline__ Fr reduce9(const uint32_t (&x)[9]) {
    const double two32 = 4294967296.0;
    // 1 / (p / 2^192): quotient estimate within 2 of floor(x / p) (x < 2^270)
    constexpr double inv_pd = 1.0 / (((double)0x30644e72u * 4294967296.0 + (double)0xe131a029u) +
                                     (double)0xb85045b6u / 4294967296.0);
    const double xd = ((double)x[8] * two32 + (double)x[7]) * two32 + (double)x[6];
    const double qd = floor(xd * inv_pd) - 1.0;
    const uint32_t q = qd > 0.0 ? (uint32_t)qd : 0u;
    Fr r;
    uint32_t carry = 0, br = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint64_t pr = (uint64_t)q * p_word(i) + carry;   // v_mad_u64_u32
        carry = (uint32_t)(pr >> 32);
        r.w[i] = subb32(x[i], (uint32_t)pr, br);
    }
    // x - q p < 3p < 2^256: the ninth word is gone; two conditional subtractions
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        Fr t;
        const uint32_t b = sub_p(t, r);
#pragma unroll
        for (int i = 0; i < 8; ++i) r.w[i] = b ? r.w[i] : t.w[i];
    }
    return r;
}

}  // namespace svdw
