// The G1 transform calls of the C ABI (include/svdw.h, "G1 transforms";
// kernels: g1_fft.hip): svdw_g1_mul, svdw_g1_fft and svdw_check_lagrange. Like
// srs.cpp's entries each checks its arguments in the order the header
// documents, takes its counters from the context's staged scratch and queues
// its kernels on the context's stream. Of the context this file uses the
// stream, the profiler, sync, ensure_buf, the staged scratch, the domain's
// table (domain_table, prover.cpp) and its own G1FftState.
#include <string.h>

#include <algorithm>

#include "engine_internal.hpp"
#include "g1_fft.hpp"

static G1Window g1_window(const svdw_ctx* c, uint32_t window_bits) {
    const uint32_t cb = window_bits ? window_bits : g1_plan(scratch_cap(c));
    return G1Window{cb, fb_windows(cb)};
}
// The `items` multiplications a describes, in pieces whose tables and
// accumulators stay under the cap: the table, the multiplication, then
// after(a) of the piece (a.t0, a.m and, for a linear dst, a.dst are the piece's).
template <class After>
static void g1_pieces(svdw_ctx* c, G1Mul a, uint64_t items, After&& after) {
    const uint64_t per = g1_point_bytes(a.c);
    const uint64_t rows = std::min<uint64_t>(std::max<uint64_t>(scratch_cap(c) / per, 1), items);
    ensure_buf(c, c->g1fft.ws, rows * per);
    G1Xyzz* acc = (G1Xyzz*)c->g1fft.ws.p;
    a.table = acc + rows;
    if (a.dst_linear) a.dst = acc;
    for (uint64_t t0 = 0; t0 < items; t0 += rows) {
        a.t0 = t0;
        a.m = std::min(rows, items - t0);
        profiled(c, "k_g1_table", (double)per * (double)a.m, [&] { return launch_g1_table(a, c->st); });
        profiled(c, "k_g1_mul", (128.0 * a.W + 160.0) * (double)a.m, [&] { return launch_g1_mul(a, c->st); });
        after(a);
    }
}
static void g1_affine(svdw_ctx* c, const G1Xyzz* src, uint64_t n, int bases_form, G1Affine* out,
                      unsigned long long* cnt) {
    profiled(c, "k_g1_affine", (128.0 + 3 * 64.0) * (double)n,
             [&] { return launch_g1_affine(src, n, bases_form, out, cnt, c->st); });
}

int svdw_g1_mul(svdw_ctx* c, int form, int bases_form, const void* points, const void* scalars, uint64_t n,
                uint32_t window_bits, void* out, svdw_g1_mul_result* result) {
    return guarded([&] {
        const std::string f = "svdw_g1_mul";
        REQUIRE(c && result, "null argument");
        check_form(form);
        check_form(bases_form);
        if (window_bits == 1 || window_bits > kG1MaxBits) fail(SVDW_ERANGE, f + ": window_bits must be 0 or in [2, 6]");
        need_device(c, f);
        memset(result, 0, sizeof *result);
        const G1Window w = g1_window(c, window_bits);
        result->window_bits = w.c;
        result->windows = w.W;
        result->points = n;
        if (!n) return;
        REQUIRE(points && scalars && out, "null argument");
        const uintptr_t o0 = (uintptr_t)out, o1 = o0 + n * sizeof(G1Affine), p0 = (uintptr_t)points,
                        s0 = (uintptr_t)scalars;
        need_apart(f, "out", o0, o1, "the points", p0, p0 + n * sizeof(G1Affine));
        need_apart(f, "out", o0, o1, "the scalars", s0, s0 + n * sizeof(Fr));
        sync(c);
        G1Mul a{};
        a.points = (const G1Affine*)points;
        a.scalars = (const Fr*)scalars;
        a.form = form;
        a.bases_form = bases_form;
        a.shift = kG1Linear;
        a.dst_linear = 1;
        a.c = w.c;
        a.W = w.W;
        ensure_buf(c, c->g1fft.ws, std::min<uint64_t>(scratch_cap(c), n * g1_point_bytes(w.c)));   // ahead of the counters
        const Staged d = stage_counters(c);
        a.cnt = d.cnt;
        g1_pieces(c, a, n, [&](const G1Mul& p) { g1_affine(c, p.dst, p.m, bases_form, (G1Affine*)out + p.t0, d.cnt); });
        unsigned long long h[4];
        read_counters(c, d.cnt, h, 4);
        result->zero_scalars = h[0];
        result->identity_inputs = h[1];
        result->identity_outputs = h[2];
    });
}

int svdw_g1_fft(svdw_ctx* c, uint32_t k, int bases_form, int inverse, const void* points, void* out,
                svdw_g1_fft_result* result) {
    return guarded([&] {
        const std::string f = "svdw_g1_fft";
        REQUIRE(c && result, "null argument");
        check_form(bases_form);
        need_k(f, k);
        need_device(c, f);
        REQUIRE(points && out, "null argument");
        const uint64_t n = 1ull << k, half = n >> 1;
        const uintptr_t o0 = (uintptr_t)out, p0 = (uintptr_t)points, len = n * sizeof(G1Affine);
        need_apart(f, "out", o0, o0 + len, "the points", p0, p0 + len);
        memset(result, 0, sizeof *result);
        const G1Window w = g1_window(c, c->opt.g1_window_bits);
        result->k = result->stages = k;
        result->window_bits = w.c;
        result->windows = w.W;
        result->rows = n;
        sync(c);
        // everything that may allocate comes ahead of the first launch
        ensure_buf(c, c->g1fft.work, n * sizeof(G1Xyzz));
        ensure_buf(c, c->g1fft.ws, std::min<uint64_t>(scratch_cap(c), half * g1_point_bytes(w.c)));
        const PowTable dom = domain_table(c, k).dev;
        G1Xyzz* work = (G1Xyzz*)c->g1fft.work.p;
        const Staged d = stage_counters(c);
        profiled(c, "k_g1_fft_first", 256.0 * (double)half,
                 [&] { return launch_g1_fft_first((const G1Affine*)points, k, bases_form, work, d.cnt, c->st); });
        G1Mul base{};
        base.work = work;
        base.dom = dom;
        base.factor = fr_to_mont(fr_inv(fr_from_u64(n)));  // 2^-k R
        base.cnt = d.cnt;
        base.n = n;
        base.twiddle = 1;
        base.inverse = inverse ? 1 : 0;
        base.c = w.c;
        base.W = w.W;
        // [2^-k] of the first `items` points of the working array, in place
        const auto scale = [&](uint64_t items) {
            G1Mul a = base;
            a.shift = kG1Linear;
            a.has_factor = 1;
            a.dst = work;
            g1_pieces(c, a, items, [](const G1Mul&) {});
        };
        for (uint32_t s = 1; s < k; ++s) {
            const bool last = inverse && s == k - 1;
            if (last) scale(half);                         // the a of the last stage are the lower half
            G1Mul a = base;
            a.shift = s;
            a.offset = 1ull << s;
            a.tw_mask = a.offset - 1;
            a.tw_shift = k - 1 - s;
            a.has_factor = last;
            a.skip_one = !last;
            a.dst_linear = 1;
            g1_pieces(c, a, half, [&](const G1Mul& p) {
                profiled(c, "k_g1_butterfly", 5 * 128.0 * (double)p.m, [&] { return launch_g1_butterfly(p, c->st); });
            });
        }
        if (inverse && k == 1) scale(n);                   // the first stage was the last
        g1_affine(c, work, n, bases_form, (G1Affine*)out, d.cnt);
        unsigned long long h[4];
        read_counters(c, d.cnt, h, 4);
        result->identity_inputs = h[1];
        result->identity_outputs = h[2];
        result->multiplications = h[3];
    });
}

int svdw_check_lagrange(svdw_ctx* c, uint32_t k, int bases_form, const void* g, const void* g_lagrange,
                        const uint64_t rho[4], svdw_lagrange_check* result) {
    return guarded([&] {
        const std::string f = "svdw_check_lagrange";
        REQUIRE(c && rho && result, "null argument");
        check_form(bases_form);
        const Fr rc = fr_raw_words(rho);
        REQUIRE(fr_reduced(rc), f + ": rho must be below p");
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
        // the column rho^i (Montgomery), its coefficients and the two sums
        ensure_buf(c, c->g1fft.ws, 2 * n * sizeof(Fr) + 2 * sizeof(G1Affine));
        G1Affine* sums = (G1Affine*)c->g1fft.ws.p;
        Fr *col = (Fr*)(sums + 2), *coeffs = col + n;
        const Fr rR = fr_to_mont(rc), one = fr_one_mont();
        {
            const Staged d = stage(c, nullptr, 0, nullptr, 0, pow_table_cells(k), 0,
                                   [&](Fr* t) { pow_table_fill(rR, one, k, t); });
            profiled(c, "k_srs_powers", 32.0 * (double)n,
                     [&] { return launch_srs_powers(pow_table_view(d.cells, k), 0, n, col, c->st); });
        }
        const void* colp = col;
        const void* coefp = coeffs;
        svdw_ntt_result nr;
        nested(svdw_ntt(c, k, k, SVDW_FORM_MONTGOMERY, 1, nullptr, &colp, 1, coeffs, &nr));
        svdw_commit_result cr;
        nested(svdw_commit(c, k, SVDW_FORM_MONTGOMERY, bases_form, g, &coefp, 1, sums, &cr));
        nested(svdw_commit(c, k, SVDW_FORM_MONTGOMERY, bases_form, g_lagrange, &colp, 1, sums + 1, &cr));
        G1Affine hs[2];
        hipck(hipMemcpyAsync(hs, sums, sizeof hs, hipMemcpyDeviceToHost, c->st), "D2H");
        sync(c);
        // both are affine points with coordinates below q in the same form: equal points are equal bytes
        result->failed = memcmp(&hs[0], &hs[1], sizeof hs[0]) != 0;
    });
}
