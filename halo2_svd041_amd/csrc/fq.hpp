// BN254 base field Fq for host and gfx950 device code: the coordinates of G1.
//
// Representation as Fr's (fr.hpp): 8 x u32 little-endian limbs, the same CIOS
// Montgomery product over the words of q. A coordinate in Montgomery form
// (x * 2^256 mod q) is byte-identical to halo2curves' in-memory Fq, which is
// what an SRS file holds. Sums and differences are form-agnostic; products here
// are Montgomery products, so curve arithmetic (g1.hpp) runs on Montgomery
// coordinates throughout and converts, if asked, on load and store only.
//
// The carry primitives (addc32, subb32, mac32) are fr.hpp's; nothing there
// changes. Every constant below is derived from q at compile time and pinned
// by a static_assert.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fr.hpp"

namespace svdw {

struct alignas(16) Fq {
    uint32_t w[8];
};

// q = 21888242871839275222246405745257275088696311157297823662689037894645226208583
#define SVDW_Q_WORDS 0xd87cfd47u, 0x3c208c16u, 0x6871ca8du, 0x97816a91u, \
                     0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u
// R = 2^256 mod q (the Montgomery form of 1) and R^2 mod q
#define SVDW_QR1_WORDS 0xc58f0d9du, 0xd35d438du, 0xf5c70b3du, 0x0a78eb28u, \
                       0x7879462cu, 0x666ea36fu, 0x9a07df2fu, 0x0e0a77c1u
#define SVDW_QR2_WORDS 0x538afa89u, 0xf32cfc5bu, 0xd44501fbu, 0xb5e71911u, \
                       0x0a417ff6u, 0x47ab1effu, 0xcab8351fu, 0x06d89f71u
static constexpr uint32_t kQinv32 = 0xe4866389u;   // -q^-1 mod 2^32

namespace fq_pin {
struct W8 {
    uint32_t w[8];
};
// 2^e mod q by e doublings of 1, each reduced by one conditional subtraction.
constexpr W8 pow2_mod_q(int e) {
    constexpr uint32_t Q[8] = {SVDW_Q_WORDS};
    W8 x{};
    x.w[0] = 1;
    for (int s = 0; s < e; ++s) {
        uint32_t top = x.w[7] >> 31;
        for (int i = 7; i > 0; --i) x.w[i] = (x.w[i] << 1) | (x.w[i - 1] >> 31);
        x.w[0] <<= 1;
        W8 d{};
        uint64_t br = 0;
        for (int i = 0; i < 8; ++i) {
            const uint64_t t = (uint64_t)x.w[i] - Q[i] - br;
            d.w[i] = (uint32_t)t;
            br = (t >> 63) & 1;
        }
        if (top || !br) x = d;
    }
    return x;
}
constexpr bool same(const W8& a, const uint32_t (&b)[8]) {
    for (int i = 0; i < 8; ++i)
        if (a.w[i] != b[i]) return false;
    return true;
}
constexpr uint32_t kQ[8] = {SVDW_Q_WORDS};
constexpr uint32_t kR1[8] = {SVDW_QR1_WORDS};
constexpr uint32_t kR2[8] = {SVDW_QR2_WORDS};
static_assert((uint32_t)(kQ[0] * kQinv32) == 0xffffffffu, "q * qinv == -1 mod 2^32");
static_assert(same(pow2_mod_q(256), kR1), "R == 2^256 mod q");
static_assert(same(pow2_mod_q(512), kR2), "R^2 == 2^512 mod q");
static_assert((kQ[7] >> 30) == 0, "q < 2^254: the CIOS rounds need 2 q < 2^256");
}  // namespace fq_pin

SVDW_HD uint32_t q_word(int i) {
    constexpr uint32_t Q[8] = {SVDW_Q_WORDS};
    return Q[i];
}
SVDW_HD Fq fq_zero() {
    Fq r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.w[i] = 0;
    return r;
}
// The Montgomery form of 1.
SVDW_HD Fq fq_one() {
    Fq r;
    constexpr uint32_t R1[8] = {SVDW_QR1_WORDS};
#pragma unroll
    for (int i = 0; i < 8; ++i) r.w[i] = R1[i];
    return r;
}
SVDW_HD Fq fq_r2() {
    Fq r;
    constexpr uint32_t R2[8] = {SVDW_QR2_WORDS};
#pragma unroll
    for (int i = 0; i < 8; ++i) r.w[i] = R2[i];
    return r;
}
SVDW_HD bool fq_is_zero(const Fq& a) {
    uint32_t x = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) x |= a.w[i];
    return x == 0;
}
SVDW_HD bool fq_eq(const Fq& a, const Fq& b) {
    uint32_t x = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) x |= a.w[i] ^ b.w[i];
    return x == 0;
}
// r = a - q over 256 bits; returns borrow.
SVDW_HD uint32_t sub_q(Fq& r, const Fq& a) {
    uint32_t br = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.w[i] = subb32(a.w[i], q_word(i), br);
    return br;
}
SVDW_HD bool fq_reduced(const Fq& a) {
    Fq t;
    return sub_q(t, a) != 0;
}
// Modular add / sub / negate (inputs < q, output < q), in either form.
SVDW_HD Fq fq_add(const Fq& a, const Fq& b) {
    Fq s, t, r;
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) s.w[i] = addc32(a.w[i], b.w[i], c);
    const uint32_t br = sub_q(t, s);                       // a + b < 2^255: no carry out
    const bool use_t = !br;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.w[i] = use_t ? t.w[i] : s.w[i];
    return r;
}
SVDW_HD Fq fq_sub(const Fq& a, const Fq& b) {
    Fq d, t, r;
    uint32_t br = 0, c = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) d.w[i] = subb32(a.w[i], b.w[i], br);
#pragma unroll
    for (int i = 0; i < 8; ++i) t.w[i] = addc32(d.w[i], q_word(i), c);
#pragma unroll
    for (int i = 0; i < 8; ++i) r.w[i] = br ? t.w[i] : d.w[i];
    return r;
}
SVDW_HD Fq fq_neg(const Fq& a) { return fq_sub(fq_zero(), a); }
SVDW_HD Fq fq_dbl(const Fq& a) { return fq_add(a, a); }

// Montgomery product a * b * 2^-256 mod q (CIOS over 32-bit limbs, as fr.hpp's
// mont_mul_rounds<8>). Output < q for inputs < q.
SVDW_HD Fq fq_mul(const Fq& a, const Fq& b) {
    uint32_t t[10];
#pragma unroll
    for (int i = 0; i < 10; ++i) t[i] = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        uint32_t c = 0, cy = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) t[j] = mac32(a.w[j], b.w[i], t[j], c);
        t[8] = addc32(t[8], c, cy);
        t[9] = cy;
        const uint32_t m = t[0] * kQinv32;
        c = 0;
        (void)mac32(m, q_word(0), t[0], c);                // low word cancels
#pragma unroll
        for (int j = 1; j < 8; ++j) t[j - 1] = mac32(m, q_word(j), t[j], c);
        cy = 0;
        t[7] = addc32(t[8], c, cy);
        t[8] = t[9] + cy;
    }
    Fq r, s;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.w[i] = t[i];
    const uint32_t br = sub_q(s, r);
    const bool use_s = t[8] | (br ^ 1u);
#pragma unroll
    for (int i = 0; i < 8; ++i) r.w[i] = use_s ? s.w[i] : r.w[i];
    return r;
}
SVDW_HD Fq fq_sqr(const Fq& a) { return fq_mul(a, a); }
SVDW_HD Fq fq_to_mont(const Fq& a) { return fq_mul(a, fq_r2()); }
SVDW_HD Fq fq_from_mont(const Fq& a) {
    Fq one = fq_zero();
    one.w[0] = 1;
    return fq_mul(a, one);
}
// a^-1 = a^(q - 2) for a Montgomery a, Montgomery out; 0 -> 0. The loops stay
// rolled: two inlined products in all.
SVDW_HD Fq fq_inv(const Fq& a) {
    Fq r = fq_one();
#pragma unroll 1
    for (int wi = 7; wi >= 0; --wi) {
        // select chain instead of a table under wi: a runtime index would spill to scratch
        uint32_t word = q_word(0) - 2u;                    // q - 2: no borrow, the low word is 0x...47
#pragma unroll
        for (int k = 1; k < 8; ++k) word = (wi == k) ? q_word(k) : word;
#pragma unroll 1
        for (int b = 31; b >= 0; --b) {
            r = fq_mul(r, r);
            const Fq ra = fq_mul(r, a);
            const bool bit = (word >> b) & 1;
#pragma unroll
            for (int i = 0; i < 8; ++i) r.w[i] = bit ? ra.w[i] : r.w[i];
        }
    }
    return r;
}

}  // namespace svdw
