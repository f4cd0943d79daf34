// The two-level power table of the prover kernels: the powers b^e of one field
// element over e < 2^bits in 2^h + 2^(bits - h) cells instead of 2^bits,
//
//   b^e R = hi[e >> h] * lo[e & (2^h - 1)],   h = pow_split(bits) = ceil(bits / 2),
//
// with lo[i] = b^i R for i < 2^h and hi[i] = top b^(i 2^h) for i < 2^(bits - h),
// hi contiguous behind lo. top = R gives the plain powers; any other top rides
// on every power (the inverse transform's 2^-k on its shift's). One mont_mul
// forms a power and one applies it. The domain's omega_k tables (one per k on the
// context, prover.cpp), a transform's shift and an opening's points all use it.
#pragma once
#include "export.hpp"                                       // ld_fr

namespace svdw {

struct PowTable {
    const Fr *lo, *hi;
    uint32_t h, bits;
};
inline uint32_t pow_split(uint32_t bits) { return (bits + 1) / 2; }
inline size_t pow_table_cells(uint32_t bits) { return ((size_t)1 << pow_split(bits)) + ((size_t)1 << (bits / 2)); }
// The table of pow_table_cells(bits) cells at base, host or device.
inline PowTable pow_table_view(const Fr* base, uint32_t bits) {
    return PowTable{base, base + ((size_t)1 << pow_split(bits)), pow_split(bits), bits};
}
// The cells of base bR (b R) with the top factor `top`, on the host.
inline void pow_table_fill(const Fr& bR, const Fr& top, uint32_t bits, Fr* out) {
    const uint32_t h = pow_split(bits);
    const size_t nlo = (size_t)1 << h, nhi = (size_t)1 << (bits - h);
    out[0] = fr_one_mont();
    for (size_t i = 1; i < nlo; ++i) out[i] = mont_mul(out[i - 1], bR);
    const Fr bh = mont_mul(out[nlo - 1], bR);
    out[nlo] = top;
    for (size_t i = 1; i < nhi; ++i) out[nlo + i] = mont_mul(out[nlo + i - 1], bh);
}
// What a launch refuses: a table that is not the view of `bits` exponents.
inline bool pow_table_bad(const PowTable& t, uint32_t bits) {
    return !t.lo || !t.hi || t.bits != bits || t.h != pow_split(bits);
}
// top b^e R for e < 2^bits: a host view on the host, a device view on the device.
// The upper level is the first operand; mont_mul commutes, so the order changes no
// bit. t by value: a kernel that picks one of two tables then selects loaded
// pointers (global loads); a selected reference into its arguments gave flat loads.
SVDW_HD Fr pow_at(const PowTable t, uint64_t e) {
    const Fr *hi = t.hi + (e >> t.h), *lo = t.lo + (e & ((1ull << t.h) - 1));
#if defined(__HIP_DEVICE_COMPILE__)
    return mont_mul(ld_fr(hi), ld_fr(lo));
#else
    return mont_mul(*hi, *lo);
#endif
}

}  // namespace svdw
