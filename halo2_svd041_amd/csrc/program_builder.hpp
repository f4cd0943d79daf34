// The symbolic program builder of the witness engine (engine.cpp, which alone
// includes this): host big integers for the range checks' bounds, and PB, which
// replays the reference's gadgets into a stage's cell program. It knows nothing
// of the context.
#pragma once

// ------------------------------------------------------- host big integers
// Unsigned 256-bit integers (BigUint bounds of the range checks).
struct BigU {
    Fr v;
};
static BigU big_from_words(const uint64_t w[4]) { return BigU{fr_raw_words(w)}; }
static BigU big_from_u128(unsigned __int128 x) {
    BigU b;
    b.v = fr_zero();
    for (int i = 0; i < 4; ++i) b.v.w[i] = (uint32_t)(x >> (32 * i));
    return b;
}
static int big_bits(const BigU& b) {
    for (int i = 7; i >= 0; --i)
        if (b.v.w[i]) return 32 * i + 32 - __builtin_clz(b.v.w[i]);
    return 0;
}
static bool big_is_zero(const BigU& b) { return big_bits(b) == 0; }
static BigU big_pow2(uint32_t k) {     // k < 256
    BigU b;
    b.v = fr_zero();
    b.v.w[k / 32] = 1u << (k % 32);
    return b;
}
static BigU big_add_u32(const BigU& a, uint32_t s) {
    BigU r;
    Fr t = fr_from_u64(s);
    if (add256(r.v, a.v, t)) fail(SVDW_ERANGE, "bound overflows 256 bits");
    return r;
}
static BigU big_sub_u32(const BigU& a, uint32_t s) {
    BigU r;
    Fr t = fr_from_u64(s);
    if (sub256(r.v, a.v, t)) fail(SVDW_EINVAL, "bound underflow (bound must be >= 1)");
    return r;
}
static BigU big_shl1(const BigU& a) {
    BigU r;
    if (a.v.w[7] >> 31) fail(SVDW_ERANGE, "bound overflows 256 bits");
    for (int i = 7; i > 0; --i) r.v.w[i] = (a.v.w[i] << 1) | (a.v.w[i - 1] >> 31);
    r.v.w[0] = a.v.w[0] << 1;
    return r;
}
// biguint_to_fe: value mod p.
static Fr big_to_fr(const BigU& b) {
    Fr x = b.v, t;
    while (!sub256(t, x, fr_p())) x = t;   // at most a few subtractions (< 2^256)
    return x;
}
static Fr pow2_fr(uint32_t k) {
    Fr x = fr_from_u64(1);
    for (uint32_t i = 0; i < k; ++i) x = fr_add(x, x);
    return x;
}

// ------------------------------------------------------- program builder
// Replays halo2-base 0.4.1 gadgets on symbolic per-element values
// (SURVEY.md Appendix A); produces the micro-ops, cell and lookup slot ops.
struct PB {
    StageArgs a;
    uint32_t lb;
    // What MockProver checks on an element's C cells (svdw_check_gates), as
    // check words (kernels.hpp CHK_*): the offsets where halo2-base's
    // assign_region enables a basic gate a + b*c = d, and the copy constraints
    // -- a value's later cells against its first cell, a loaded value's first
    // cell against its source cell (view), range_check's last running sum
    // against the checked value (RangeChip::range_check's constrain_equal).
    std::vector<uint32_t> chk;
    // halo2-base's equality records of an element's cells (svdw_equalities), in
    // assign order: a Constant cell's (cell, value), an Existing cell's (source
    // cell, cell), range_check's constrain_equal(a, last running sum) -- as eq
    // words (kernels.hpp EQ_*): a constant slot, an earlier cell of the element,
    // the element's cell of a view (RegionChecks::esrc), or an external cell
    std::vector<uint32_t> eq;
    int kext = -1;            // constant slot holding an external cell's value (init_rand)
    bool vsrc[kMaxViews] = {true, true};   // false: the view holds values produced here
    static constexpr int EQ_AUTO = -1, EQ_WIT = -2;
    bool kconst = true;       // its constant-source cells are halo2-base Constants
    int8_t vload[kMaxV];      // view a value was loaded from (-1: computed)
    int16_t fullc[kMaxV];     // first cell holding the value in full (-1: none)
    void gate(uint32_t at) { chk.push_back(chk_gate(at)); }
    void copy_of(uint8_t v, uint32_t at) {    // cell `at` must equal value v's cell
        if (fullc[v] >= 0) chk.push_back(chk_copy((uint32_t)fullc[v], at));
        else if (vload[v] >= 0) chk.push_back(chk_view((uint32_t)vload[v], at));
    }
    explicit PB(uint32_t lookup_bits) : lb(lookup_bits) {
        memset(&a, 0, sizeof(a));
        memset(vload, -1, sizeof vload);
        for (auto& f : fullc) f = -1;
    }

    uint8_t newv() {
        if (a.nv >= (uint32_t)kMaxV) fail(SVDW_ERANGE, "stage needs too many element values");
        return (uint8_t)a.nv++;
    }
    uint8_t kidx(const Fr& c) {
        for (uint32_t k = 0; k < a.nk; ++k)
            if (fr_eq(a.K[k], c)) return (uint8_t)k;
        if (a.nk >= (uint32_t)kMaxK) fail(SVDW_ERANGE, "stage needs too many constants");
        a.K[a.nk] = c;
        return (uint8_t)a.nk++;
    }
    uint8_t K(const Fr& c) { return KSRC + kidx(c); }
    uint8_t K(uint64_t c) { return K(fr_from_u64(c)); }
    void op(uint8_t code, uint8_t dst, uint8_t x, uint8_t y, uint16_t p0 = 0, uint16_t p1 = 0) {
        if (a.nmo >= (uint32_t)kMaxMicro) fail(SVDW_ERANGE, "stage needs too many micro-ops");
        a.mo[a.nmo++] = MicroOp{code, dst, x, y, p0, p1};
    }
    static SlotOp slot(uint8_t src, uint32_t lo, uint32_t nbits) {
        if (nbits >= 256) nbits = 0;
        return SlotOp{src, (uint8_t)lo, (uint8_t)nbits, 0};
    }
    // cell `at` holds a copy of value v (QuantumCell::Existing of v's cell)
    void eq_of_value(uint8_t v, uint32_t at) {
        if (vload[v] >= 0 && vsrc[vload[v]]) eq.push_back(eq_word(EQ_VIEW, (uint32_t)vload[v], at));
        else if (fullc[v] >= 0) eq.push_back(eq_word(EQ_LOCAL, (uint32_t)fullc[v], at));
    }
    // eqk: EQ_AUTO -- a Constant for a constant slot (kconst), the external cell
    // for kext, an Existing copy for a value's full cell seen before (or loaded
    // from a source view), else a Witness; EQ_WIT: a Witness; >= 0: an Existing
    // copy of the element's cell eqk (range_check's last limb)
    void cell(uint8_t src, uint32_t lo = 0, uint32_t nbits = 0, int eqk = EQ_AUTO) {
        if (a.C >= (uint32_t)kMaxAdv) fail(SVDW_ERANGE, "stage has too many cells per element (raise lookup_bits)");
        const SlotOp s = slot(src, lo, nbits);
        if (eqk >= 0) {
            eq.push_back(eq_word(EQ_LOCAL, (uint32_t)eqk, a.C));
        } else if (eqk == EQ_AUTO) {
            if (src >= KSRC) {
                const int k = src - KSRC;
                if (k == kext) eq.push_back(eq_word(EQ_EXT, 0, a.C));
                else if (kconst) eq.push_back(eq_word(EQ_CONST, (uint32_t)k, a.C));
            } else if (s.lo == 0 && s.nbits == 0) {
                eq_of_value(src, a.C);
            }
        }
        if (src < KSRC && s.lo == 0 && s.nbits == 0) {      // the value itself: a copy or its first cell
            copy_of(src, a.C);
            if (fullc[src] < 0) fullc[src] = (int16_t)a.C;
        }
        a.adv[a.C++] = s;
    }
    void look(uint8_t src, uint32_t lo = 0, uint32_t nbits = 0) {
        if (a.L >= (uint32_t)kMaxLk) fail(SVDW_ERANGE, "stage has too many lookups per element (raise lookup_bits)");
        a.lk[a.L++] = slot(src, lo, nbits);
    }
    // --- element values
    uint8_t load(int view_idx) {
        uint8_t v = newv();
        op(MO_LOAD, v, (uint8_t)view_idx, 0);
        vload[v] = (int8_t)view_idx;
        return v;
    }
    uint8_t addk(uint8_t x, const Fr& k) {
        uint8_t t = newv();
        op(MO_ADDK, t, x, kidx(k));
        return t;
    }
    // --- GateChip
    uint8_t g_add_k(uint8_t x, const Fr& k) {       // add(x, Constant(k)): [x, k, 1, x+k]
        uint8_t t = addk(x, k);
        gate(a.C);
        cell(x); cell(K(k)); cell(K(1)); cell(t);
        return t;
    }
    uint8_t g_sub_k(uint8_t x, const Fr& k) {       // sub(x, Constant(k)): [x-k, k, 1, x]
        uint8_t d = addk(x, fr_neg(k));
        gate(a.C);
        cell(d); cell(K(k)); cell(K(1)); cell(x);
        return d;
    }
    uint8_t g_sub(uint8_t x, uint8_t y) {           // sub: [x-y, y, 1, x]
        uint8_t d = newv();
        op(MO_SUB, d, x, y);
        gate(a.C);
        cell(d); cell(y); cell(K(1)); cell(x);
        return d;
    }
    uint8_t g_mul(uint8_t x, uint8_t y) {           // mul: [0, x, y, x*y]
        uint8_t m = newv();
        op(MO_MUL, m, x, y);
        gate(a.C);
        cell(K(0)); cell(x); cell(y); cell(m);
        return m;
    }
    void g_is_equal(uint8_t x, uint8_t y) {         // sub + is_zero: 12 cells
        uint8_t d = g_sub(x, y);
        uint8_t z = newv();
        uint8_t inv = newv();
        (void)inv;
        op(MO_ISZERO, z, d, 0);
        gate(a.C);
        gate(a.C + 4);
        cell(z); cell(d); cell((uint8_t)(z + 1)); cell(K(1));
        cell(K(0)); cell(d); cell(z); cell(K(0));
    }
    // --- RangeChip::range_check
    void range_check(uint8_t v, uint32_t bits) {
        if (bits == 0) return;    // assert_is_const(a, 0): no cells
        if (bits > 254 + lb) fail(SVDW_ERANGE, "range_check bits too large");
        const uint32_t n = (bits + lb - 1) / lb, rem = bits % lb;
        uint8_t lsrc = v;
        uint32_t llo = 0, lnb = 0;
        int lastc = EQ_AUTO;                        // the last limb's cell (n > 1)
        if (n == 1) {
            look(v);
        } else {
            for (uint32_t i = 0; i < n; ++i) {
                const uint32_t lo = i * lb;
                uint8_t src = v;
                uint32_t slo = lo, snb = lb;
                if (lo >= 256) { src = K(0); slo = 0; snb = 0; }
                if (i == 0) {
                    lastc = (int)a.C;
                    cell(src, slo, snb, EQ_WIT);   // limbs are witnesses
                } else {
                    gate(a.C - 1);                  // [s_(i-1), l_i, 2^(i lb), s_i]
                    lastc = (int)a.C;
                    cell(src, slo, snb, EQ_WIT);
                    cell(K(pow2_fr(lo)));
                    cell(v, 0, (i + 1) * lb, EQ_WIT);   // running sum = v mod 2^((i+1) lb)
                    if (i + 1 == n && n * lb < 256) copy_of(v, a.C - 1);   // constrain_equal(a, sum)
                    if (i + 1 == n) eq_of_value(v, a.C - 1);
                }
                look(src, slo, snb);
                lsrc = src; llo = slo; lnb = snb;
            }
        }
        if (rem == 1) {                             // assert_bit: [0, l, l, l]
            gate(a.C);
            cell(K(0)); cell(lsrc, llo, lnb, lastc); cell(lsrc, llo, lnb, lastc); cell(lsrc, llo, lnb, lastc);
        } else if (rem > 1) {                       // mul(last, 2^(lb-rem)), looked up
            const uint32_t sh = lb - rem;
            uint8_t m = newv();
            if (n == 1) op(MO_FDBL, m, v, (uint8_t)sh);
            else if ((n - 1) * lb >= 256) op(MO_ADDK, m, v, kidx(fr_zero()));   // unreachable in practice
            else op(MO_LIMBSHL, m, v, (uint8_t)sh, (uint16_t)((n - 1) * lb), (uint16_t)lb);
            gate(a.C);
            cell(K(0)); cell(lsrc, llo, lnb, lastc); cell(K(pow2_fr(sh))); cell(m);
            look(m);
        }
    }
    // --- RangeChip::check_less_than(a, Constant(b), bits)
    void check_less_than_k(uint8_t x, const BigU& b, uint32_t bits) {
        Fr pw = pow2_fr(bits), bf = big_to_fr(b);
        uint8_t t3 = addk(x, pw);                  // a + 2^bits
        uint8_t t2 = addk(t3, fr_neg(bf));         // a + 2^bits - b
        gate(a.C);
        gate(a.C + 3);
        cell(t2); cell(K(bf)); cell(K(1)); cell(t3); cell(K(fr_neg(pw))); cell(K(1)); cell(x);
        range_check(t2, bits);
    }
    void check_big_less_than_safe(uint8_t x, const BigU& bnd) {
        uint32_t rb = (big_bits(bnd) + lb - 1) / lb * lb;
        range_check(x, rb);
        check_less_than_k(x, bnd, rb);
    }
    // RangeChip::div_mod(t, 2^p, nb) [ext halo2-base 0.4.1]: [r, 2^p, q, t], then
    // check_big_less_than_safe(q, 2^nb / 2^p + 1), check_big_less_than_safe(r, 2^p)
    uint8_t div_mod_pow2(uint8_t t, uint32_t p, uint32_t nb) {
        uint8_t q = newv();
        op(MO_SHR, q, t, 0, (uint16_t)p);
        uint8_t r = newv();
        op(MO_LIMBSHL, r, t, 0, 0, (uint16_t)p);
        gate(a.C);
        cell(r); cell(K(pow2_fr(p))); cell(q); cell(t);
        check_big_less_than_safe(q, big_add_u32(big_pow2(nb - p), 1));
        check_big_less_than_safe(r, big_pow2(p));
        return q;
    }
    // FixedPointChip041::signed_div_scale, parameterised (oracle/pyoracle.py
    // signed_div_scale; chip source unavailable, parity unpinned): add 2^s,
    // div_mod by 2^p on nb bits, subtract 2^(s-p). Returns the quotient value.
    uint8_t signed_div_scale(uint8_t x, uint32_t p, uint32_t s, uint32_t nb) {
        uint8_t t = g_add_k(x, pow2_fr(s));
        uint8_t q = div_mod_pow2(t, p, nb);
        return g_sub_k(q, pow2_fr(s - p));
    }
    // FixedPointChip041::qsqrt (ZkVector::norm / dist, src/matrix/mod.rs:124-131,
    // 156-164), parameterised (the chip's source is unavailable: PARITY UNPINNED;
    // oracle/pyoracle.py qsqrt): y = floor(sqrt(a 2^P)) for a fixed-point a in
    // [0, 2^nbits), as load_witness(y) with range_check(y, ny), t = mul(a, 2^P),
    // d = sub(t, mul(y, y)) and f = sub(mul(y, 2), d), both range-checked on nd
    // bits: 0 <= t - y^2 <= 2y, i.e. y^2 <= t < (y + 1)^2.
    uint8_t qsqrt(uint8_t x, uint32_t p, uint32_t nbits) {
        const uint32_t ny = (nbits + p + 1) / 2 + 1, nd = ny + 1;
        uint8_t t = newv();
        op(MO_FDBL, t, x, (uint8_t)p);                   // a 2^P (< 2^254: an integer)
        uint8_t y = newv();
        op(MO_ISQRT, y, t, 0);
        cell(y);                                          // load_witness(y)
        range_check(y, ny);
        gate(a.C);
        cell(K(0)); cell(x); cell(K(pow2_fr(p))); cell(t);   // mul(a, 2^P)
        uint8_t y2 = g_mul(y, y);
        uint8_t d = g_sub(t, y2);
        range_check(d, nd);
        uint8_t e = newv();
        op(MO_FDBL, e, y, 1);
        gate(a.C);
        cell(K(0)); cell(y); cell(K(2)); cell(e);          // mul(y, 2)
        uint8_t f = g_sub(e, d);
        range_check(f, nd);
        return y;
    }
    // check_abs_less_than (src/matrix/mod.rs:425-435)
    void check_abs_less_than(uint8_t x, const BigU& bnd) {
        if (big_is_zero(bnd)) fail(SVDW_EINVAL, "check_abs_less_than: bound must be >= 1");
        BigU nb = big_sub_u32(big_shl1(bnd), 1);
        uint8_t t = g_add_k(x, big_to_fr(big_sub_u32(bnd, 1)));
        check_big_less_than_safe(t, nb);
    }
};
