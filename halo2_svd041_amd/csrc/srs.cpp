// The SRS calls of the C ABI (include/svdw.h, "SRS"; kernels: srs.hip):
// svdw_fixed_base_mul, svdw_srs_setup and svdw_check_srs. Like prover.cpp's
// entries each checks its arguments in the order the header documents, takes
// its counters from the context's staged scratch (stage, engine_internal.hpp)
// and queues its kernels on the context's stream. Of the context this file
// uses the stream, the profiler, sync, ensure_buf, the staged scratch, the
// domain's table (domain_table, prover.cpp) and its own SrsState.
#include <string.h>

#include <algorithm>

#include "engine_internal.hpp"
#include "srs.hpp"

// A scalar argument: four words, canonical.
static Fr srs_scalar(const std::string& f, const char* name, const uint64_t w[4]) {
    const Fr x = fr_raw_words(w);
    REQUIRE(fr_reduced(x), f + ": " + name + " must be below p");
    return x;
}
// The base as Montgomery affine.
static G1Affine fb_base_mont(const std::string& f, const void* base, int base_form) {
    G1Affine p;
    memcpy(&p, base, sizeof p);
    REQUIRE(fq_reduced(p.x) && fq_reduced(p.y), f + ": a base coordinate is not below q");
    p = g1_affine_to_mont(p, base_form);
    REQUIRE(g1_affine_is_identity(p) || g1_on_curve(p), f + ": the base is not on the curve");
    return p;
}
static G1Window fb_window(uint32_t window_bits, uint64_t n) {
    const uint32_t c = window_bits ? window_bits : fb_plan(n ? n : 1);
    return G1Window{c, fb_windows(c)};
}
// The context's table of (base, c), the base given as Montgomery affine: built
// on the stream on first use, in the slot whose turn it is.
static const G1Affine* fb_table(svdw_ctx* c, const G1Affine& base, uint32_t cb) {
    SrsState& s = c->srs;
    for (SrsState::Table& t : s.table)
        if (t.buf.p && t.c == cb && t.base_form == SVDW_FORM_MONTGOMERY && !memcmp(t.base, &base, sizeof base))
            return (const G1Affine*)t.buf.p;
    SrsState::Table& t = s.table[s.next];
    s.next = (s.next + 1) % (uint32_t)(sizeof s.table / sizeof s.table[0]);
    t.c = 0;
    ensure_buf(c, t.buf, fb_table_points(cb) * sizeof(G1Affine));
    profiled(c, "k_fb_table", 64.0 * (double)fb_table_points(cb), [&] {
        return launch_fb_table(base, SVDW_FORM_MONTGOMERY, cb, (G1Affine*)t.buf.p, c->st);
    });
    memcpy(t.base, &base, sizeof base);
    t.base_form = SVDW_FORM_MONTGOMERY;
    t.c = cb;
    return (const G1Affine*)t.buf.p;
}
// out[i] = [scalars[i]] base for i < split and out2[i - split] for the rest of the n,
// through acc and pre (n entries each).
static void fb_mul(svdw_ctx* c, const G1Affine* table, G1Window w, const Fr* scalars, uint64_t n, int form,
                   int out_form, G1Affine* out, G1Xyzz* acc, Fq* pre, unsigned long long* cnt,
                   G1Affine* out2 = nullptr, uint64_t split = ~0ull) {
    FbMul a{};
    a.table = table;
    a.scalars = scalars;
    a.out = out;
    a.out2 = out2;
    a.acc = acc;
    a.pre = pre;
    a.cnt = cnt;
    a.n = n;
    a.split = std::min(split, n);
    a.c = w.c;
    a.W = w.W;
    a.form = form;
    a.base_form = out_form;
    profiled(c, "k_fb_mul", (32.0 + 64.0 + 2.0 * kFbRowBytes) * (double)n, [&] { return launch_fb_mul(a, c->st); });
}

int svdw_fixed_base_mul(svdw_ctx* c, int form, int base_form, const void* base, const void* scalars, uint64_t n,
                        uint32_t window_bits, void* out, svdw_fixed_base_result* result) {
    return guarded([&] {
        const std::string f = "svdw_fixed_base_mul";
        REQUIRE(c && base && result, "null argument");
        check_form(form);
        check_form(base_form);
        const G1Affine b = fb_base_mont(f, base, base_form);
        if (window_bits == 1 || window_bits > kCommitMaxBits) fail(SVDW_ERANGE, f + ": window_bits must be 0 or in [2, 16]");
        need_device(c, f);
        memset(result, 0, sizeof *result);
        const G1Window w = fb_window(window_bits, n);
        result->window_bits = w.c;
        result->windows = w.W;
        result->points = n;
        if (!n) return;
        REQUIRE(scalars && out, "null argument");
        const uintptr_t o0 = (uintptr_t)out, i0 = (uintptr_t)scalars;
        need_apart(f, "out", o0, o0 + n * sizeof(G1Affine), "the scalars", i0, i0 + n * sizeof(Fr));
        sync(c);
        const uint64_t rows = std::min<uint64_t>(std::max<uint64_t>(scratch_cap(c) / kFbRowBytes, 1), n);
        ensure_buf(c, c->srs.ws, rows * kFbRowBytes);
        G1Xyzz* acc = (G1Xyzz*)c->srs.ws.p;
        Fq* pre = (Fq*)(acc + rows);
        const G1Affine* table = fb_table(c, b, w.c);
        const Staged d = stage_counters(c);
        for (uint64_t r0 = 0; r0 < n; r0 += rows)
            fb_mul(c, table, w, (const Fr*)scalars + r0, std::min(rows, n - r0), form, base_form, (G1Affine*)out + r0,
                   acc, pre, d.cnt);
        unsigned long long h[2];
        read_counters(c, d.cnt, h, 2);
        result->zero_scalars = h[0];
        result->identity_outputs = h[1];
    });
}

int svdw_srs_setup(svdw_ctx* c, uint32_t k, const uint64_t s[4], int bases_form, void* g, void* g_lagrange,
                   svdw_srs_result* result) {
    return guarded([&] {
        const std::string f = "svdw_srs_setup";
        REQUIRE(c && s && result, "null argument");
        check_form(bases_form);
        const Fr sc = srs_scalar(f, "s", s);
        need_k(f, k);
        need_device(c, f);
        const uint64_t n = 1ull << k;
        if (g && g_lagrange) {
            const uintptr_t a0 = (uintptr_t)g, b0 = (uintptr_t)g_lagrange, len = n * sizeof(G1Affine);
            need_apart(f, "g", a0, a0 + len, "g_lagrange", b0, b0 + len);
        }
        memset(result, 0, sizeof *result);
        const uint32_t arrays = (g ? 1 : 0) + (g_lagrange ? 1 : 0);
        const uint64_t outputs = n * arrays;
        const G1Window w = fb_window(0, outputs);
        const uint64_t per = std::max(arrays, 1u) * (kFbRowBytes + sizeof(Fr));   // a row of every array asked for
        const uint64_t rows = std::min<uint64_t>(
            c->opt.srs_chunk_rows ? c->opt.srs_chunk_rows : std::max<uint64_t>(scratch_cap(c) / per, 1), n);
        // s^n by k squarings: the secret is in the domain when it is 1
        const Fr sR = fr_to_mont(sc), one = fr_one_mont();
        Fr snR = sR;
        for (uint32_t i = 0; i < k; ++i) snR = mont_mul(snR, snR);
        const bool in_domain = fr_eq(snR, one);
        result->k = k;
        result->window_bits = w.c;
        result->windows = w.W;
        result->rows = n;
        result->chunk_rows = rows;
        result->chunks = (uint32_t)((n + rows - 1) / rows);
        result->secret_in_domain = in_domain;
        if (!outputs) return;
        sync(c);
        const Fr coef = mont_mul(fr_sub(snR, one), fr_to_mont(fr_inv(fr_from_u64(n))));   // (s^n - 1) / n R
        ensure_buf(c, c->srs.ws, rows * per);
        G1Xyzz* acc = (G1Xyzz*)c->srs.ws.p;                // the scratch of `arrays` rows per row of a piece
        Fq* pre = (Fq*)(acc + arrays * rows);
        Fr* col = (Fr*)(pre + arrays * rows);
        G1Affine gen;                                      // G = (1, 2)
        gen.x = fq_one();
        gen.y = fq_dbl(gen.x);
        const G1Affine* table = fb_table(c, gen, w.c);
        const PowTable dom = domain_table(c, k).dev;
        // the staged cells: the two-level table of s over the rows
        const Staged d = stage(c, nullptr, 0, nullptr, 0, g ? pow_table_cells(k) : 0, 0, [&](Fr* t) {
            if (g) pow_table_fill(sR, one, k, t);
        });
        const PowTable pw = pow_table_view(d.cells, k);
        // per piece: the columns side by side, s^i then l_i(s), and one multiplication over both (a launch ends in
        // a tail of waves that run alone, so the fewer launches the better)
        for (uint64_t r0 = 0; r0 < n; r0 += rows) {
            const uint64_t m = std::min(rows, n - r0);
            Fr* lcol = g ? col + m : col;
            G1Affine *og = g ? (G1Affine*)g + r0 : nullptr, *ol = g_lagrange ? (G1Affine*)g_lagrange + r0 : nullptr;
            if (g) profiled(c, "k_srs_powers", 32.0 * (double)m, [&] { return launch_srs_powers(pw, r0, m, col, c->st); });
            if (g_lagrange)
                profiled(c, "k_srs_lagrange", 96.0 * (double)m,
                         [&] { return launch_srs_lagrange(dom, sR, coef, in_domain, r0, m, lcol, c->st); });
            if (g) fb_mul(c, table, w, col, arrays * m, SVDW_FORM_MONTGOMERY, bases_form, og, acc, pre, d.cnt, ol, m);
            else fb_mul(c, table, w, col, m, SVDW_FORM_MONTGOMERY, bases_form, ol, acc, pre, d.cnt + 2);
        }
        unsigned long long h[4];
        read_counters(c, d.cnt, h, 4);
        result->g_zero_scalars = h[0];
        result->g_identity_outputs = h[1];
        result->lagrange_zero_scalars = h[2];
        result->lagrange_identity_outputs = h[3];
    });
}

// [x] G by double-and-add over the 254 bits of the canonical x, on the host.
static G1Xyzz srs_host_mul(const Fr& x) {
    G1Affine gen;
    gen.x = fq_one();
    gen.y = fq_dbl(gen.x);
    G1Xyzz acc = g1_identity();
    for (int bit = (int)kCommitScalarBits - 1; bit >= 0; --bit) {
        acc = g1_double(acc);
        if ((x.w[bit >> 5] >> (bit & 31)) & 1) acc = g1_add_mixed(acc, gen);
    }
    return acc;
}
// The point as read from the device equals acc.
static bool srs_same(const G1Xyzz& acc, const G1Affine& p, int bases_form) {
    return fq_reduced(p.x) && fq_reduced(p.y) && g1_eq_affine(acc, g1_affine_to_mont(p, bases_form));
}

int svdw_check_srs(svdw_ctx* c, uint32_t k, int bases_form, const void* g, const void* g_lagrange,
                   const uint64_t s[4], const uint64_t rho[4], svdw_srs_check* result) {
    return guarded([&] {
        const std::string f = "svdw_check_srs";
        REQUIRE(c && s && rho && result, "null argument");
        check_form(bases_form);
        const Fr sc = srs_scalar(f, "s", s), rc = srs_scalar(f, "rho", rho);
        need_k(f, k);
        need_device(c, f);
        REQUIRE(g && g_lagrange, "null argument");
        memset(result, 0, sizeof *result);
        sync(c);
        const uint64_t n = 1ull << k;
        // every point on the curve
        {
            const Staged d = stage_counters(c);
            for (const void* arr : {g, g_lagrange})
                profiled(c, "k_commit_check_bases", 64.0 * (double)n, [&] {
                    return launch_commit_check_bases((const G1Affine*)arr, n, bases_form, d.cnt, c->st);
                });
            unsigned long long h[4];
            read_counters(c, d.cnt, h, 4);
            result->points_checked = h[2];
            result->points_off_curve = h[3];
        }
        // the column rho^i (Montgomery), its coefficients, the two sums and the value at s
        ensure_buf(c, c->srs.ws, (2 * n + 1) * sizeof(Fr) + 2 * sizeof(G1Affine));
        G1Affine* sums = (G1Affine*)c->srs.ws.p;
        Fr *col = (Fr*)(sums + 2), *coeffs = col + n, *value = coeffs + n;
        const Fr rR = fr_to_mont(rc), one = fr_one_mont();
        {
            const Staged d = stage(c, nullptr, 0, nullptr, 0, pow_table_cells(k), 0,
                                   [&](Fr* t) { pow_table_fill(rR, one, k, t); });
            profiled(c, "k_srs_powers", 32.0 * (double)n,
                     [&] { return launch_srs_powers(pow_table_view(d.cells, k), 0, n, col, c->st); });
        }
        const void* colp = col;
        const void* coefp = coeffs;
        svdw_commit_result cr;
        nested(svdw_commit(c, k, SVDW_FORM_MONTGOMERY, bases_form, g, &colp, 1, sums, &cr));
        nested(svdw_commit(c, k, SVDW_FORM_MONTGOMERY, bases_form, g_lagrange, &colp, 1, sums + 1, &cr));
        svdw_ntt_result nr;
        nested(svdw_ntt(c, k, k, SVDW_FORM_MONTGOMERY, 1, nullptr, &colp, 1, coeffs, &nr));
        nested(svdw_eval_polynomial(c, k, SVDW_FORM_MONTGOMERY, &coefp, 1, s, 1, value));
        G1Affine hs[2];
        Fr hv;
        hipck(hipMemcpyAsync(hs, sums, sizeof hs, hipMemcpyDeviceToHost, c->st), "D2H");
        hipck(hipMemcpyAsync(&hv, value, sizeof hv, hipMemcpyDeviceToHost, c->st), "D2H");
        sync(c);
        // ((rho s)^n - 1) / (rho s - 1), n when rho s = 1
        const Fr xR = mont_mul(rR, fr_to_mont(sc));
        Fr xnR = xR;
        for (uint32_t i = 0; i < k; ++i) xnR = mont_mul(xnR, xnR);
        const Fr geo = fr_eq(xR, one) ? fr_from_u64(n)   // (a R) * b * R^-1: canonical
                                      : mont_mul(fr_sub(xnR, one), fr_inv(fr_from_mont(fr_sub(xR, one))));
        result->g_failed = !srs_same(srs_host_mul(geo), hs[0], bases_form);
        result->lagrange_failed = !srs_same(srs_host_mul(fr_from_mont(hv)), hs[1], bases_form);
    });
}
