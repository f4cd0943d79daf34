// Read-out of witness cells in the form a consumer holds them (export.hip):
//
//  k_export<FORM>  cells of a contiguous stream range or of a strided view,
//                  written dense: canonical (a gather) or Montgomery
//                  (x * 2^256 mod p, halo2curves' in-memory Fr([u64; 4]))
//  k_dequantize    the same addressing, one f64 per cell
//                  (FixedPointChip041::dequantization, parity unpinned)
//
// and the per-value arithmetic shared by host and device: the cell load /
// store, ZkMatrix::new's quantization and the dequantization.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "fr.hpp"

namespace svdw {

// ----------------------------------------------------------------- helpers
__device__ __forceinline__ Fr ld_fr(const Fr* p) {
    const uint4* q = reinterpret_cast<const uint4*>(p);
    uint4 a = q[0], b = q[1];
    Fr r;
    r.w[0] = a.x; r.w[1] = a.y; r.w[2] = a.z; r.w[3] = a.w;
    r.w[4] = b.x; r.w[5] = b.y; r.w[6] = b.z; r.w[7] = b.w;
    return r;
}
__device__ __forceinline__ void st_fr(Fr* p, const Fr& v) {
    uint4* q = reinterpret_cast<uint4*>(p);
    q[0] = make_uint4(v.w[0], v.w[1], v.w[2], v.w[3]);
    q[1] = make_uint4(v.w[4], v.w[5], v.w[6], v.w[7]);
}
// ZkMatrix::new's quantization of one f64 (quantize_body's arithmetic):
// x_q = round_half_away(|x| 2^P) as u128 (saturating, NaN -> 0), sign(x) < 0
// (incl. -0.0) -> p - x_q.
SVDW_HD Fr quantize_fr(double x, double scale) {
    const bool neg = signbit(x) && !isnan(x);
    const double s = round(fabs(x) * scale);
    Fr q = fr_zero();
    if (s >= 340282366920938463463374607431768211456.0) {
        q.w[0] = q.w[1] = q.w[2] = q.w[3] = 0xffffffffu;
    } else if (s > 0.0) {
        const uint64_t bits = __builtin_bit_cast(uint64_t, s);
        const int e = (int)((bits >> 52) & 0x7ff) - 1075;
        const uint64_t mant = (bits & 0xfffffffffffffull) | (1ull << 52);
        const unsigned __int128 v = e >= 0 ? ((unsigned __int128)mant << e) : (unsigned __int128)(mant >> -e);
        q.w[0] = (uint32_t)v; q.w[1] = (uint32_t)(v >> 32);
        q.w[2] = (uint32_t)(v >> 64); q.w[3] = (uint32_t)(v >> 96);
    }
    return neg ? fr_sub(fr_zero(), q) : q;
}

// (hi 2^64 + lo) as f64, round to nearest even (Rust's `u128 as f64`). There is
// no u128 conversion on the device, and (double)hi 2^64 + (double)lo rounds
// twice: instead the top 64 bits with the bits shifted out OR-ed into bit 0 as
// a sticky bit -- 64 >= 53 + 2, so the one u64 conversion rounds as the full
// value would -- scaled back by an exact power of two.
SVDW_HD double u128_to_f64(uint64_t hi, uint64_t lo) {
    if (!hi) return (double)lo;
    const int sh = 64 - __builtin_clzll(hi);             // 1..64: bits above the low word
    uint64_t top, lost;
    if (sh == 64) {
        top = hi;
        lost = lo;
    } else {
        top = (hi << (64 - sh)) | (lo >> sh);
        lost = lo << (64 - sh);
    }
    top |= lost ? 1u : 0u;
    const double scale = __builtin_bit_cast(double, (uint64_t)(1023 + sh) << 52);   // 2^sh
    return (double)top * scale;
}
// FixedPointChip041::dequantization of one cell for PRECISION_BITS = P (1..63);
// PARITY UNPINNED (the chip's source is not available, include/svdw.h): x is
// negative iff x > (p - 1) / 2 (signed_bits' convention); m = the low 128 bits
// of |x|; S = 2^P; the result is +-((m / S as f64) + (m % S as f64) / (S as f64)),
// every `as f64` rounding to nearest even and the sum one f64 addition. 0 -> +0.0.
SVDW_HD double dequantize_fr(const Fr& x, uint32_t P) {
    Fr n, d;
    sub256(n, fr_p(), x);                                 // p - x
    const bool neg = sub256(d, n, x) != 0;                // p - x < x
    const uint64_t m0 = neg ? ((uint64_t)n.w[1] << 32 | n.w[0]) : ((uint64_t)x.w[1] << 32 | x.w[0]);
    const uint64_t m1 = neg ? ((uint64_t)n.w[3] << 32 | n.w[2]) : ((uint64_t)x.w[3] << 32 | x.w[2]);
    const uint64_t qlo = (m0 >> P) | (m1 << (64 - P)), qhi = m1 >> P;      // m / S
    const uint64_t rem = m0 & ((1ull << P) - 1);                           // m % S
    const double inv = __builtin_bit_cast(double, (uint64_t)(1023 - (int)P) << 52);   // 1 / S, exact
    const double r = u128_to_f64(qhi, qlo) + (double)rem * inv;
    return neg ? -r : r;
}

// ---------------------------------------------------------------- launches
static constexpr int kFormCanonical = 0, kFormMontgomery = 1;   // SVDW_FORM_* (include/svdw.h)

// Source cells of an export: cell k < n is src[off + i rs + j cs] with
// i = (k0 + k) / cols, j = (k0 + k) % cols (k0: a chunk of a larger view starts
// there). cols == 0: the contiguous range src[off + k].
struct ExportSrc {
    const Fr* src;
    uint64_t off, n, k0;
    int64_t rs, cs;
    uint32_t cols;
};
// dst[k] = cell k in `form`, then `pad` zero cells (column padding rows).
hipError_t launch_export(const ExportSrc& s, int form, Fr* dst, uint64_t pad, hipStream_t st);
// dst[k] = dequantize_fr(cell k, P).
hipError_t launch_dequantize(const ExportSrc& s, uint32_t P, double* dst, hipStream_t st);

}  // namespace svdw
