// BN254 G1 (y^2 = x^3 + 3 over Fq) for host and gfx950 device code.
//
// Affine points are (x, y) with (0, 0) the identity, as halo2curves' G1Affine
// (the curve has no point with x = y = 0). Accumulators are extended Jacobian
// "XYZZ": x = X / ZZ, y = Y / ZZZ with ZZ^3 = ZZZ^2, ZZ = 0 the identity. All
// coordinates are Montgomery Fq (fq.hpp).
//
// The three laws are the EFD's add-2008-s (full, 14 products), madd-2008-s
// (mixed, 10) and dbl-2008-s-1 (9) for a = 0, made complete: an identity on
// either side, equal points (the add falls through to the double) and opposite
// points (the identity) are ordinary inputs. G1 has odd order, so no point
// has y = 0 and the double needs no case of its own; it maps ZZ = 0 to ZZ = 0.
//
// As grand_product.hpp and ntt.hpp ask: callers keep their loops over points
// rolled (#pragma unroll 1 around these inlined laws), and nothing here indexes
// a register array at run time.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fq.hpp"

namespace svdw {

struct alignas(16) G1Affine {
    Fq x, y;
};
struct alignas(16) G1Xyzz {
    Fq x, y, zz, zzz;
};

SVDW_HD bool g1_affine_is_identity(const G1Affine& p) { return fq_is_zero(p.x) && fq_is_zero(p.y); }
SVDW_HD bool g1_is_identity(const G1Xyzz& p) { return fq_is_zero(p.zz); }
SVDW_HD G1Xyzz g1_identity() {
    G1Xyzz r;
    r.x = r.y = r.zz = r.zzz = fq_zero();
    return r;
}
SVDW_HD G1Xyzz g1_from_affine(const G1Affine& p) {
    G1Xyzz r;
    const bool id = g1_affine_is_identity(p);
    r.x = p.x;
    r.y = p.y;
    r.zz = r.zzz = id ? fq_zero() : fq_one();
    return r;
}
// The form of an affine point's coordinates as the entries pass it (bases_form,
// base_form): 0 canonical Fq, anything else Montgomery. These two state the
// rule for every reader and writer of points. (0, 0) stays (0, 0) either way,
// so the identity is the same bytes in both forms.
SVDW_HD G1Affine g1_affine_to_mont(G1Affine p, int form) {
    if (form == 0) {
        p.x = fq_to_mont(p.x);
        p.y = fq_to_mont(p.y);
    }
    return p;
}
SVDW_HD G1Affine g1_affine_to_form(G1Affine p, int form) {
    if (form == 0) {
        p.x = fq_from_mont(p.x);
        p.y = fq_from_mont(p.y);
    }
    return p;
}
SVDW_HD G1Affine g1_affine_neg(const G1Affine& p) {
    G1Affine r;
    r.x = p.x;
    r.y = fq_neg(p.y);                                     // q - 0 folds back to 0: the identity stays (0, 0)
    return r;
}
SVDW_HD G1Xyzz g1_neg(const G1Xyzz& p) {
    G1Xyzz r = p;
    r.y = fq_neg(p.y);
    return r;
}
// y^2 == x^3 + 3 (Montgomery coordinates); the identity is not on the curve.
SVDW_HD bool g1_on_curve(const G1Affine& p) {
    const Fq one = fq_one();
    const Fq three = fq_add(fq_add(one, one), one);
    const Fq rhs = fq_add(fq_mul(fq_sqr(p.x), p.x), three);
    return fq_eq(fq_sqr(p.y), rhs);
}

// 2 p (dbl-2008-s-1, a = 0).
SVDW_HD G1Xyzz g1_double(const G1Xyzz& p) {
    const Fq u = fq_dbl(p.y);
    const Fq v = fq_sqr(u);
    const Fq w = fq_mul(u, v);
    const Fq s = fq_mul(p.x, v);
    const Fq xx = fq_sqr(p.x);
    const Fq m = fq_add(fq_dbl(xx), xx);
    G1Xyzz r;
    r.x = fq_sub(fq_sqr(m), fq_dbl(s));
    r.y = fq_sub(fq_mul(m, fq_sub(s, r.x)), fq_mul(w, p.y));
    r.zz = fq_mul(v, p.zz);
    r.zzz = fq_mul(w, p.zzz);
    return r;
}
// The common tail of both adds: the sum from U1 = X1 ZZ2, S1 = Y1 ZZZ2, the
// differences P = U2 - U1, R = S2 - S1 (P != 0) and zz = ZZ1 ZZ2, zzz = ZZZ1 ZZZ2.
SVDW_HD G1Xyzz g1_add_tail(const Fq& u1, const Fq& s1, const Fq& p, const Fq& r, const Fq& zz, const Fq& zzz) {
    const Fq pp = fq_sqr(p);
    const Fq ppp = fq_mul(p, pp);
    const Fq q = fq_mul(u1, pp);
    G1Xyzz o;
    o.x = fq_sub(fq_sub(fq_sqr(r), ppp), fq_dbl(q));
    o.y = fq_sub(fq_mul(r, fq_sub(q, o.x)), fq_mul(s1, ppp));
    o.zz = fq_mul(zz, pp);
    o.zzz = fq_mul(zzz, ppp);
    return o;
}
// a + b for an affine b (madd-2008-s), complete.
SVDW_HD G1Xyzz g1_add_mixed(const G1Xyzz& a, const G1Affine& b) {
    if (g1_affine_is_identity(b)) return a;
    if (g1_is_identity(a)) return g1_from_affine(b);
    const Fq p = fq_sub(fq_mul(b.x, a.zz), a.x);
    const Fq r = fq_sub(fq_mul(b.y, a.zzz), a.y);
    if (fq_is_zero(p)) return fq_is_zero(r) ? g1_double(a) : g1_identity();
    return g1_add_tail(a.x, a.y, p, r, a.zz, a.zzz);
}
// a + b (add-2008-s), complete.
SVDW_HD G1Xyzz g1_add(const G1Xyzz& a, const G1Xyzz& b) {
    if (g1_is_identity(b)) return a;
    if (g1_is_identity(a)) return b;
    const Fq u1 = fq_mul(a.x, b.zz);
    const Fq s1 = fq_mul(a.y, b.zzz);
    const Fq p = fq_sub(fq_mul(b.x, a.zz), u1);
    const Fq r = fq_sub(fq_mul(b.y, a.zzz), s1);
    if (fq_is_zero(p)) return fq_is_zero(r) ? g1_double(a) : g1_identity();
    return g1_add_tail(u1, s1, p, r, fq_mul(a.zz, b.zz), fq_mul(a.zzz, b.zzz));
}
// The affine point of p with one inversion: 1 / ZZ = (ZZ / ZZZ)^2.
SVDW_HD G1Affine g1_to_affine(const G1Xyzz& p) {
    G1Affine r;
    if (g1_is_identity(p)) {
        r.x = r.y = fq_zero();
        return r;
    }
    const Fq i3 = fq_inv(p.zzz);
    const Fq i2 = fq_sqr(fq_mul(p.zz, i3));
    r.x = fq_mul(p.x, i2);
    r.y = fq_mul(p.y, i3);
    return r;
}
// a == the affine b, cross-multiplied (no division).
SVDW_HD bool g1_eq_affine(const G1Xyzz& a, const G1Affine& b) {
    const bool ia = g1_is_identity(a), ib = g1_affine_is_identity(b);
    if (ia || ib) return ia && ib;
    return fq_eq(fq_mul(b.x, a.zz), a.x) && fq_eq(fq_mul(b.y, a.zzz), a.y);
}

}  // namespace svdw
