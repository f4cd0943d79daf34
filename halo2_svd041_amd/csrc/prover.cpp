// The prover calls of the C ABI (include/svdw.h) on an assigned witness: the
// lookup argument, the grand products of the lookup and permutation arguments,
// the transforms, the commitments, the quotient and the opening. Each entry
// checks its arguments in the order include/svdw.h documents, stages what its
// kernels read in the context's staged scratch (stage, engine_internal.hpp) and
// queues the kernels on the context's stream. The context (svdw_ctx,
// engine_internal.hpp) is engine.cpp's: of it this file uses the stream, the
// profiler, sync, ensure_buf, the staged scratch, its own ProverState and the
// few facts its argument checks read.
#include <string.h>

#include <algorithm>

#include "engine_internal.hpp"
#include "export.hpp"                                       // ld_fr, st_fr of grand_product.hpp
#include "lookup.hpp"
#include "lookup_product.hpp"
#include "permutation_product.hpp"
#include "permutation_cycles.hpp"
#include "ntt.hpp"
#include "commit.hpp"
#include "quotient.hpp"
#include "open.hpp"

// (The argument checks the families share, need_k and the like: engine_internal.hpp.)
// ---- lookup argument: multiplicities, permuted columns, their check (lookup.hpp)
namespace {
struct LkArgs {
    uint32_t lb = 0;
    uint64_t rows = 0, usable = 0;
    LkSrc src{};
};
}  // namespace
// The argument checks the three entries share. False: no columns, nothing to do.
static bool lk_args(svdw_ctx* c, const char* fn, uint32_t phase, uint32_t unusable_rows, const void* columns,
                    uint32_t ncols, LkArgs* a) {
    const std::string f(fn);
    REQUIRE(c && phase < 2, "bad argument");
    need_device(c, f);
    REQUIRE(!sharded(c), f + ": the lookup stream of a row-sharded context is partial");
    const svdw_ctx::Phys& P = c->phys;
    REQUIRE(P.valid, f + ": call svdw_physical_layout after the witness");
    if (P.k > 31) fail(SVDW_ERANGE, f + ": k > 31");
    REQUIRE(unusable_rows <= P.min_rows, f + ": unusable_rows exceeds the layout's minimum_rows "
                                             "(an assigned row would be a blinding row)");
    const uint64_t TL = c->ph[phase].nl, nl = (TL + P.R - 1) / P.R;
    REQUIRE(columns || ncols == nl, f + ": ncols differs from num_lookup_advice of the phase");
    a->lb = c->LB;
    a->rows = 1ull << P.k;
    a->usable = a->rows - unusable_rows;
    if (a->lb > 31 || (1ull << a->lb) > a->usable)
        fail(SVDW_ERANGE, f + ": the 2^lookup_bits table does not fit the usable rows (not enough rows: raise k)");
    need_columns(f, ncols);
    a->src = columns ? LkSrc{(const Fr*)columns, a->rows, a->rows, (uint64_t)ncols * a->rows}
                     : LkSrc{c->ph[phase].lk, P.R, P.R, TL};
    return ncols != 0;
}
int svdw_lookup_multiplicities(svdw_ctx* c, uint32_t phase, uint32_t unusable_rows, const void* columns,
                               uint32_t ncols, uint32_t* mult) {
    return guarded([&] {
        LkArgs a;
        if (!lk_args(c, "svdw_lookup_multiplicities", phase, unusable_rows, columns, ncols, &a)) return;
        REQUIRE(mult, "null output");
        sync(c);
        unsigned long long* oot = stage_counters(c).cnt;
        hipck(hipMemsetAsync(mult, 0, ((size_t)ncols << a.lb) * sizeof(uint32_t), c->st), "hipMemsetAsync");
        profiled(c, "k_lk_hist", 32.0 * ncols * a.usable,
                 [&] { return launch_lk_hist(a.src, SVDW_FORM_CANONICAL, ncols, a.usable, a.lb, mult, oot, c->st); });
        hipck(hipStreamSynchronize(c->st), "hipStreamSynchronize");
    });
}
int svdw_lookup_permute(svdw_ctx* c, uint32_t phase, uint32_t unusable_rows, int form, const void* columns,
                        uint32_t ncols, void* permuted_input, void* permuted_table, svdw_lookup_result* result) {
    return guarded([&] {
        REQUIRE(result, "null argument");
        check_form(form);
        LkArgs a;
        const bool any = lk_args(c, "svdw_lookup_permute", phase, unusable_rows, columns, ncols, &a);
        memset(result, 0, sizeof *result);
        result->usable_rows = a.usable;
        if (!any) return;
        REQUIRE(permuted_input && permuted_table, "null output");
        sync(c);
        const uint64_t B = 1ull << a.lb, nblk = lk_scan_blocks(B), bins = (uint64_t)ncols * B;
        const Staged d = stage_counters(c, (4 * bins + 2 * ncols * nblk + ncols) * sizeof(uint32_t),
                                        bins * sizeof(uint32_t));   // the histogram starts at zero
        LkScratch s;
        s.cnt = (uint32_t*)d.free;
        s.start = s.cnt + bins;
        s.pincl = s.start + bins;
        s.absent = s.pincl + bins;
        s.bsum = s.absent + bins;
        s.tot = s.bsum + 2 * ncols * nblk;
        profiled(c, "k_lk_hist", 32.0 * ncols * a.usable, [&] {
            return launch_lk_hist(a.src, SVDW_FORM_CANONICAL, ncols, a.usable, a.lb, s.cnt, d.cnt, c->st);
        });
        unsigned long long bad = 0;
        read_counters(c, d.cnt, &bad, 1);
        result->columns = ncols;
        result->out_of_table = bad;
        if (bad) return;                                    // ConstraintSystemFailure: the outputs stay as they are
        profiled(c, "k_lk_scan", 20.0 * bins, [&] { return launch_lk_scans(s, ncols, a.lb, c->st); });
        profiled(c, "k_lk_fill", 64.0 * ncols * a.rows, [&] {
            return launch_lk_fill(s, ncols, a.rows, a.usable, a.lb, form, (Fr*)permuted_input, (Fr*)permuted_table,
                                  c->st);
        });
        std::vector<uint32_t> tot(ncols);
        hipck(hipMemcpyAsync(tot.data(), s.tot, ncols * sizeof(uint32_t), hipMemcpyDeviceToHost, c->st), "D2H");
        hipck(hipStreamSynchronize(c->st), "hipStreamSynchronize");
        for (uint32_t t : tot) result->distinct += t;
    });
}
int svdw_check_lookup_argument(svdw_ctx* c, uint32_t phase, uint32_t unusable_rows, int form, const void* columns,
                               uint32_t ncols, const void* permuted_input, const void* permuted_table,
                               svdw_lookup_check* result) {
    return guarded([&] {
        REQUIRE(result, "null argument");
        check_form(form);
        LkArgs a;
        const bool any = lk_args(c, "svdw_check_lookup_argument", phase, unusable_rows, columns, ncols, &a);
        memset(result, 0, sizeof *result);
        if (!any) return;
        REQUIRE(permuted_input && permuted_table, "null argument");
        sync(c);
        const uint64_t bins = (uint64_t)ncols << a.lb;
        const Staged d = stage_counters(c, 3 * bins * sizeof(uint32_t), 3 * bins * sizeof(uint32_t));
        unsigned long long* cnt = d.cnt;                   // [0..3] rows, [4..5] bins, [8] cells outside the table
        uint32_t *ha = (uint32_t*)d.free, *hpin = ha + bins, *htab = hpin + bins;
        const uint64_t cells = (uint64_t)ncols * a.rows;
        {
            ProfScope ps(c, c->st, "k_lk_hist:check", 32.0 * ncols * 3 * a.usable, 0);
            hipck(launch_lk_hist(a.src, SVDW_FORM_CANONICAL, ncols, a.usable, a.lb, ha, cnt + 8, c->st), "k_lk_hist");
            hipck(launch_lk_hist(LkSrc{(const Fr*)permuted_input, a.rows, a.rows, cells}, form, ncols, a.usable,
                                 a.lb, hpin, cnt + 8, c->st), "k_lk_hist");
            hipck(launch_lk_hist(LkSrc{(const Fr*)permuted_table, a.rows, a.rows, cells}, form, ncols, a.usable,
                                 a.lb, htab, cnt + 8, c->st), "k_lk_hist");
            hipck(launch_lk_compare(ha, hpin, htab, ncols, a.usable, a.lb, cnt + 4, c->st), "k_lk_compare");
        }
        profiled(c, "k_lk_adjacent", 64.0 * ncols * a.rows, [&] {
            return launch_lk_adjacent((const Fr*)permuted_input, (const Fr*)permuted_table, ncols, a.rows, a.usable,
                                      cnt, c->st);
        });
        unsigned long long h[9];
        read_counters(c, cnt, h, 9);
        result->adjacency_checked = h[0];
        result->adjacency_failures = h[1];
        result->padding_checked = h[2];
        result->padding_failures = h[3];
        result->multiset_checked = h[4];
        result->multiset_failures = h[5] + h[8];           // a cell outside the table is in no bin
    });
}
// ---- the grand products Z and their checks (grand_product.hpp)
// What the lookup's and the permutation's entries check first, in this order:
// the form, beta and gamma (to b, g), a row for Z[usable].
static void gp_challenges(const char* fn, int form, const uint64_t beta[4], const uint64_t gamma[4],
                          uint32_t unusable_rows, Fr* b, Fr* g) {
    const std::string f(fn);
    REQUIRE(beta && gamma, "null argument");
    check_form(form);
    *b = fr_raw_words(beta);
    *g = fr_raw_words(gamma);
    REQUIRE(fr_reduced(*b) && fr_reduced(*g), f + ": beta or gamma >= p");
    if (!unusable_rows) fail(SVDW_ERANGE, f + ": unusable_rows == 0 leaves no row for Z[usable]");
}
// The six counters of a check kernel into either argument's check result.
template <class Check>
static void gp_check_result(svdw_ctx* c, const unsigned long long* cnt, Check* result) {
    unsigned long long h[6];
    read_counters(c, cnt, h, 6);
    result->recurrence_checked = h[0];
    result->recurrence_failures = h[1];
    result->boundary_checked = h[2];
    result->boundary_failures = h[3];
    result->padding_checked = h[4];
    result->padding_failures = h[5];
}
// ---- lookup argument: the grand product Z and its check (lookup_product.hpp)
// The argument checks of both entries and what the kernels read (a->usable also
// without columns); false: no columns, nothing to do.
static bool lp_args(svdw_ctx* c, const char* fn, uint32_t phase, uint32_t unusable_rows, int form, const void* columns,
                    uint32_t ncols, const void* permuted_input, const void* permuted_table, const uint64_t beta[4],
                    const uint64_t gamma[4], LpArgs* a) {
    Fr b, g;
    gp_challenges(fn, form, beta, gamma, unusable_rows, &b, &g);
    LkArgs lk;
    const bool any = lk_args(c, fn, phase, unusable_rows, columns, ncols, &lk);
    const bool mont = form == SVDW_FORM_MONTGOMERY;
    a->src = lk.src;
    a->pin = (const Fr*)permuted_input;
    a->ptab = (const Fr*)permuted_table;
    a->ncols = ncols;
    a->lb = lk.lb;
    a->rows = lk.rows;
    a->usable = lk.usable;
    a->ch.b0 = b;
    a->ch.g0 = g;
    a->ch.bx = mont ? fr_to_mont(b) : b;
    a->ch.gx = mont ? fr_to_mont(g) : g;
    a->ch.g2 = fr_to_mont(fr_to_mont(g));
    a->ch.t2 = fr_to_mont(fr_to_mont(fr_from_u64(1ull << 32)));
    a->ch.one = fr_one_mont();
    return any;
}
int svdw_lookup_product(svdw_ctx* c, uint32_t phase, uint32_t unusable_rows, int form, const void* columns,
                        uint32_t ncols, const void* permuted_input, const void* permuted_table,
                        const uint64_t beta[4], const uint64_t gamma[4], void* z, svdw_lookup_product_result* result) {
    return guarded([&] {
        REQUIRE(result, "null argument");
        LpArgs a;
        const bool any = lp_args(c, "svdw_lookup_product", phase, unusable_rows, form, columns, ncols, permuted_input,
                                 permuted_table, beta, gamma, &a);
        memset(result, 0, sizeof *result);
        result->usable_rows = a.usable;
        if (!any) return;
        REQUIRE(permuted_input && permuted_table && z, "null argument");
        sync(c);
        const uint64_t nt = gp_tiles(a.rows);
        const Staged d = stage_counters(c, 2 * ncols * nt * sizeof(Fr));
        unsigned long long* cnt = d.cnt;                   // [0] zero denominators, [1] columns with Z[usable] != 1
        Fr* tp = (Fr*)d.free;
        const double cells = (double)ncols * a.usable;
        profiled(c, "k_lp_tiles", 96.0 * cells, [&] { return launch_lp_tiles(a, form, tp, cnt, c->st); });
        profiled(c, "k_lp_carry", 128.0 * ncols * nt, [&] { return launch_lp_carry(a, form, tp, cnt, c->st); });
        profiled(c, "k_lp_write", 96.0 * cells + 32.0 * ncols * a.rows,
                 [&] { return launch_lp_write(a, form, tp, (Fr*)z, c->st); });
        unsigned long long h[2];
        read_counters(c, cnt, h, 2);
        result->columns = ncols;
        result->zero_denominators = h[0];
        result->final_not_one = h[1];
    });
}
int svdw_check_lookup_product(svdw_ctx* c, uint32_t phase, uint32_t unusable_rows, int form, const void* columns,
                              uint32_t ncols, const void* permuted_input, const void* permuted_table,
                              const uint64_t beta[4], const uint64_t gamma[4], const void* z,
                              svdw_lookup_product_check* result) {
    return guarded([&] {
        REQUIRE(result, "null argument");
        LpArgs a;
        const bool any = lp_args(c, "svdw_check_lookup_product", phase, unusable_rows, form, columns, ncols,
                                 permuted_input, permuted_table, beta, gamma, &a);
        memset(result, 0, sizeof *result);
        if (!any) return;
        REQUIRE(permuted_input && permuted_table && z, "null argument");
        sync(c);
        unsigned long long* cnt = stage_counters(c).cnt;
        profiled(c, "k_lp_check", 96.0 * ncols * a.usable + 32.0 * ncols * a.rows,
                 [&] { return launch_lp_check(a, form, (const Fr*)z, cnt, c->st); });
        gp_check_result(c, cnt, result);
    });
}
// ---- permutation argument: sigma values, the grand products Z and their check
// (permutation_product.hpp)
namespace {
struct DomainConsts {
    Fr delta, omega28;                                     // canonical
};
struct PpDev {
    PpArgs a{};
    unsigned long long* cnt = nullptr;
    Fr *sv = nullptr, *xs = nullptr, *tp = nullptr;
};
}  // namespace
// The evaluation domain, for every family from here on.
// delta = 7^(2^28) and omega_28 = 7^((p - 1) / 2^28), as halo2curves derives them.
static const DomainConsts& domain_consts() {
    static const DomainConsts k = [] {
        Fr e = fr_p();
        e.w[0] -= 1;
        for (int i = 0; i < 8; ++i) e.w[i] = (e.w[i] >> 28) | (i < 7 ? e.w[i + 1] << 4 : 0u);
        const Fr g = fr_to_mont(fr_from_u64(7));
        Fr w = fr_one_mont(), d = g;
        for (int i = 255; i >= 0; --i) {
            w = mont_mul(w, w);
            if ((e.w[i >> 5] >> (i & 31)) & 1) w = mont_mul(w, g);
        }
        for (int i = 0; i < 28; ++i) d = mont_mul(d, d);
        return DomainConsts{fr_from_mont(d), fr_from_mont(w)};
    }();
    return k;
}
// omega_k R for 1 <= k <= 28.
static Fr domain_omega_mont(uint32_t k) {
    Fr w = fr_to_mont(domain_consts().omega28);
    for (uint32_t i = k; i < 28; ++i) w = mont_mul(w, w);
    return w;
}
// The context's slot of omega_k's table (pow_table.hpp), host and device views: filled and uploaded on the first
// use of k, never again. The upload is ordered on the stream before the caller's kernels; the slot keeps its source.
const ProverState::DomainSlot& domain_table(svdw_ctx* c, uint32_t k) {   // (srs.cpp reads it too)
    ProverState::DomainSlot& s = c->prover.domain[k];
    if (!s.buf.p) {
        s.cells.resize(pow_table_cells(k));
        pow_table_fill(domain_omega_mont(k), fr_one_mont(), k, s.cells.data());
        ensure_buf(c, s.buf, s.cells.size() * sizeof(Fr));
        hipck(hipMemcpyAsync(s.buf.p, s.cells.data(), s.cells.size() * sizeof(Fr), hipMemcpyHostToDevice, c->st), "H2D");
        s.host = pow_table_view(s.cells.data(), k);
        s.dev = pow_table_view((const Fr*)s.buf.p, k);
    }
    return s;
}
// x delta^j phi for j < n (phi = 1 canonical, R Montgomery), x canonical.
static void pp_delta_powers(const Fr& x, int form, uint32_t n, Fr* out) {
    const Fr dm = fr_to_mont(domain_consts().delta);
    Fr v = form == SVDW_FORM_MONTGOMERY ? fr_to_mont(x) : x;
    for (uint32_t j = 0; j < n; ++j) {
        out[j] = v;
        v = mont_mul(v, dm);
    }
}
int svdw_permutation_constants(uint32_t k, uint64_t delta[4], uint64_t omega[4]) {
    return guarded([&] {
        REQUIRE(delta && omega, "null argument");
        need_k("svdw_permutation_constants", k);
        fr_store_words(domain_consts().delta, delta);
        fr_store_words(fr_from_mont(domain_omega_mont(k)), omega);
    });
}
int svdw_permutation_values(svdw_ctx* c, uint32_t k, int form, const uint64_t* mapping, uint32_t first_col,
                            uint32_t ncols, uint32_t total_cols, void* out, uint64_t* out_of_range) {
    return guarded([&] {
        REQUIRE(c && out_of_range, "null argument");
        check_form(form);
        need_k("svdw_permutation_values", k);
        need_device(c, "svdw_permutation_values");
        need_columns("svdw_permutation_values", std::max(ncols, total_cols));
        *out_of_range = 0;
        if (!ncols) return;
        REQUIRE(out, "null output");
        sync(c);
        const PowTable w = domain_table(c, k).dev;
        // the staged cells: delta^j phi for j < total_cols (one cell at least)
        const Staged d = stage(c, nullptr, 0, nullptr, 0, std::max(total_cols, 1u), 0,
                               [&](Fr* t) { pp_delta_powers(fr_from_u64(1), form, total_cols, t); });
        profiled(c, "k_pp_values", (mapping ? 40.0 : 32.0) * ncols * (double)(1ull << k), [&] {
            return launch_pp_values(mapping, d.cells, w, first_col, ncols, total_cols, 1ull << k, (Fr*)out, d.cnt,
                                    c->st);
        });
        unsigned long long bad = 0;
        read_counters(c, d.cnt, &bad, 1);
        *out_of_range = bad;
    });
}
// The argument checks of both entries, in the order include/svdw.h gives, and
// what the kernels read on the device; false: no columns, nothing to do.
static bool pp_args(svdw_ctx* c, const char* fn, uint32_t k, uint32_t unusable_rows, int form,
                    const void* const* columns, const void* const* sigma, uint32_t ncols, uint32_t chunk_len,
                    const uint64_t beta[4], const uint64_t gamma[4], const void* z, bool scratch, PpDev* d) {
    const std::string f(fn);
    REQUIRE(c, "null argument");
    Fr b, g;
    gp_challenges(fn, form, beta, gamma, unusable_rows, &b, &g);
    const uint64_t rows = k < 63 ? 1ull << k : ~0ull;
    if (unusable_rows >= rows) fail(SVDW_ERANGE, f + ": unusable_rows leaves no usable row");
    REQUIRE(chunk_len, f + ": chunk_len == 0");
    need_k(f, k);
    need_device(c, f);
    PpArgs& a = d->a;
    a.rows = rows;
    a.usable = rows - unusable_rows;
    a.ncols = ncols;
    a.chunk = chunk_len;
    a.nsets = ncols ? pp_sets(ncols, chunk_len) : 0;
    if (!ncols) return false;
    need_columns(f, ncols);
    REQUIRE(columns && sigma && z, "null argument");
    for (uint32_t j = 0; j < ncols; ++j) {
        need_pointer(f, columns[j]);
        need_pointer(f, sigma[j]);
    }
    sync(c);
    const bool mont = form == SVDW_FORM_MONTGOMERY;
    a.w = domain_table(c, k).dev;
    a.bR = fr_to_mont(b);
    a.g = mont ? fr_to_mont(g) : g;
    a.one = fr_one_mont();
    // the staged cells: beta delta^j phi for j < ncols
    const uint64_t cells = scratch ? pp_scratch_cells(a.nsets, rows) : 0;
    const Staged s = stage(c, columns, ncols, sigma, ncols, ncols, cells * sizeof(Fr),
                           [&](Fr* t) { pp_delta_powers(b, form, ncols, t); });
    d->cnt = s.cnt;
    a.cols = s.ptrs;
    a.sig = a.cols + ncols;
    a.bd = s.cells;
    d->sv = (Fr*)s.free;
    d->xs = d->sv + 2 * (uint64_t)a.nsets;
    d->tp = d->xs + 2 * (uint64_t)kGpThreads * a.nsets;
    return true;
}
int svdw_permutation_product(svdw_ctx* c, uint32_t k, uint32_t unusable_rows, int form, const void* const* columns,
                             const void* const* sigma, uint32_t ncols, uint32_t chunk_len, const uint64_t beta[4],
                             const uint64_t gamma[4], void* z, svdw_permutation_product_result* result) {
    return guarded([&] {
        REQUIRE(result, "null argument");
        PpDev d;
        const bool any = pp_args(c, "svdw_permutation_product", k, unusable_rows, form, columns, sigma, ncols,
                                 chunk_len, beta, gamma, z, true, &d);
        memset(result, 0, sizeof *result);
        result->usable_rows = d.a.usable;
        if (!any) return;
        const PpArgs& a = d.a;
        const double cells = (double)ncols * a.usable, nt = (double)gp_tiles(a.rows);
        profiled(c, "k_pp_tiles", 64.0 * cells, [&] { return launch_pp_tiles(a, form, d.tp, d.cnt, c->st); });
        profiled(c, "k_pp_totals", 64.0 * a.nsets * nt,
                 [&] { return launch_pp_totals(a, form, d.tp, d.xs, d.sv, c->st); });
        profiled(c, "k_pp_chain", 128.0 * a.nsets, [&] { return launch_pp_chain(a, d.sv, d.cnt, c->st); });
        profiled(c, "k_pp_fold", 128.0 * a.nsets * nt,
                 [&] { return launch_pp_fold(a, form, d.tp, d.xs, d.sv, c->st); });
        profiled(c, "k_pp_write", 64.0 * cells + 32.0 * a.nsets * a.rows,
                 [&] { return launch_pp_write(a, form, d.tp, (Fr*)z, c->st); });
        unsigned long long h[2];
        read_counters(c, d.cnt, h, 2);
        result->columns = ncols;
        result->sets = a.nsets;
        result->zero_denominators = h[0];
        result->final_not_one = (uint32_t)h[1];
    });
}
int svdw_check_permutation_product(svdw_ctx* c, uint32_t k, uint32_t unusable_rows, int form,
                                   const void* const* columns, const void* const* sigma, uint32_t ncols,
                                   uint32_t chunk_len, const uint64_t beta[4], const uint64_t gamma[4], const void* z,
                                   svdw_permutation_product_check* result) {
    return guarded([&] {
        REQUIRE(result, "null argument");
        PpDev d;
        const bool any = pp_args(c, "svdw_check_permutation_product", k, unusable_rows, form, columns, sigma, ncols,
                                 chunk_len, beta, gamma, z, false, &d);
        memset(result, 0, sizeof *result);
        if (!any) return;
        const PpArgs& a = d.a;
        const Fr wstep = fr_to_mont(fr_pow_u64(fr_from_mont(domain_omega_mont(k)), pp_check_stride(a.rows)));
        profiled(c, "k_pp_check", 64.0 * ncols * a.usable + 32.0 * a.nsets * a.rows,
                 [&] { return launch_pp_check(a, form, (const Fr*)z, wstep, d.cnt, c->st); });
        gp_check_result(c, d.cnt, result);
    });
}
// ---- permutation argument: sigma's mapping from the copy constraints and its
// check (permutation_cycles.hpp)
// The argument checks of both entries, in the order include/svdw.h gives; false:
// no columns, nothing to do.
static bool pc_args(svdw_ctx* c, const char* fn, uint32_t k, uint32_t unusable_rows, uint32_t total_cols,
                    const uint64_t* edges, uint64_t n_edges, const uint64_t* mapping, bool writes, PcShape* s) {
    const std::string f(fn);
    REQUIRE(c, "null argument");
    need_k(f, k);
    const uint64_t rows = 1ull << k;
    if (unusable_rows >= rows) fail(SVDW_ERANGE, f + ": unusable_rows leaves no usable row");
    need_device(c, f);
    need_columns(f, total_cols);
    const uint64_t cells = (uint64_t)total_cols << k;
    if (cells > (1ull << 32)) fail(SVDW_ERANGE, f + ": total_cols << k above 2^32 (cell ids are 32-bit)");
    if (n_edges > (1ull << 59)) fail(SVDW_ERANGE, f + ": n_edges above 2^59");
    *s = PcShape{k, total_cols, rows, rows - unusable_rows, cells};
    if (!total_cols) return false;
    REQUIRE(mapping && (edges || !n_edges), "null argument");
    const uintptr_t o0 = (uintptr_t)mapping, e0 = (uintptr_t)edges;
    if (writes && n_edges) need_apart(f, "mapping", o0, o0 + cells * 8, "the edges", e0, e0 + n_edges * 16);
    return true;
}
static size_t pc_pad(size_t bytes) { return (bytes + 127) / 128 * 128; }
int svdw_permutation_cycles(svdw_ctx* c, uint32_t k, uint32_t unusable_rows, uint32_t total_cols,
                            const uint64_t* edges, uint64_t n_edges, uint64_t* mapping,
                            svdw_permutation_cycles_result* result) {
    return guarded([&] {
        REQUIRE(result, "null argument");
        PcShape s{};
        const bool any =
            pc_args(c, "svdw_permutation_cycles", k, unusable_rows, total_cols, edges, n_edges, mapping, true, &s);
        memset(result, 0, sizeof *result);
        result->cells = s.cells;
        result->edges = n_edges;
        result->sort_passes = pc_sort_passes(s.cells);
        if (!any) return;
        sync(c);
        const uint64_t n = s.cells, nt = pc_tiles(n);
        // the flags (zeroed with the counters), the tile sums, the parents
        const size_t o_bsum = pc_pad(n), o_parent = o_bsum + pc_pad(nt * 8);
        const Staged d = stage_counters(c, o_parent + n * 4, pc_pad(n));
        unsigned long long* cnt = d.cnt;   // [0] out of range, [1] self edges, [2] members, [3] classes, [4] largest
        uint8_t* flag = (uint8_t*)d.free;
        uint64_t* bsum = (uint64_t*)(d.free + o_bsum);
        uint32_t* parent = (uint32_t*)(d.free + o_parent);
        const double dn = (double)n, de = (double)n_edges;
        profiled(c, "k_pc_init", 4.0 * dn, [&] { return launch_pc_init(s, parent, c->st); });
        profiled(c, "k_pc_union", 16.0 * de, [&] { return launch_pc_union(s, edges, n_edges, parent, cnt, c->st); });
        profiled(c, "k_pc_flatten", 8.0 * dn, [&] { return launch_pc_flatten(s, parent, c->st); });
        profiled(c, "k_pc_flag", 5.0 * dn, [&] { return launch_pc_flag(s, parent, flag, c->st); });
        profiled(c, "k_pc_scan", 5.0 * dn, [&] { return launch_pc_member_scan(s, parent, flag, bsum, cnt + 2, c->st); });
        unsigned long long h[5];
        read_counters(c, cnt, h, 3);
        const uint64_t m = h[2];
        REQUIRE(m <= n, "internal: more linked cells than cells");
        if (m) {
            // two (key, val) pairs of arrays, the digit table of one pass and its tile sums
            const uint64_t nblk = pc_sort_blocks(m);
            const size_t o_arr = pc_pad(m * 4), o_hist = 4 * o_arr, o_bs2 = o_hist + pc_pad(256 * nblk * 4);
            DBuf& ws = c->prover.cycles_ws;
            ensure_buf(c, ws, o_bs2 + pc_tiles(256 * nblk) * 8);
            char* w = (char*)ws.p;
            uint32_t *key = (uint32_t*)w, *val = (uint32_t*)(w + o_arr), *key2 = (uint32_t*)(w + 2 * o_arr),
                     *val2 = (uint32_t*)(w + 3 * o_arr);
            const double dm = (double)m;
            profiled(c, "k_pc_compact", 5.0 * dn + 12.0 * dm,
                     [&] { return launch_pc_compact(s, parent, flag, bsum, m, key, val, c->st); });
            for (uint32_t p = 0; p < result->sort_passes; ++p) {
                profiled(c, "k_pc_sort", 24.0 * dm, [&] {
                    return launch_pc_sort_pass(key, val, m, 8 * p, (uint32_t*)(w + o_hist), (uint64_t*)(w + o_bs2),
                                               key2, val2, c->st);
                });
                std::swap(key, key2);
                std::swap(val, val2);
            }
            profiled(c, "k_pc_link", 16.0 * dm, [&] { return launch_pc_link(s, key, val, m, mapping, cnt + 3, c->st); });
        }
        profiled(c, "k_pc_identity", 5.0 * dn + 8.0 * (dn - (double)m),
                 [&] { return launch_pc_identity(s, parent, flag, mapping, c->st); });
        read_counters(c, cnt, h, 5);
        result->out_of_range = h[0];
        result->self_edges = h[1];
        result->linked_cells = m;
        result->classes = h[3];
        result->largest_class = h[4];
    });
}
int svdw_check_permutation_mapping(svdw_ctx* c, uint32_t k, uint32_t unusable_rows, uint32_t total_cols,
                                   const uint64_t* edges, uint64_t n_edges, const uint64_t* mapping,
                                   svdw_permutation_mapping_check* result) {
    return guarded([&] {
        REQUIRE(result, "null argument");
        PcShape s{};
        const bool any = pc_args(c, "svdw_check_permutation_mapping", k, unusable_rows, total_cols, edges, n_edges,
                                 mapping, false, &s);
        memset(result, 0, sizeof *result);
        if (!any) return;
        sync(c);
        const uint64_t n = s.cells;
        // hit counts and descents (zeroed with the counters), then the two buffers of (next, min) pairs
        const size_t o_desc = pc_pad(n * 4), o_nm = 2 * o_desc, o_nm2 = o_nm + pc_pad(n * 8);
        const Staged d = stage_counters(c, o_nm2 + n * 8, o_nm);
        unsigned long long* cnt = d.cnt;   // [0] bad entries, [1] padding, [2] hits != 1, [3] cycles, [4] order,
                                           // [5] edges, [6] edge failures
        uint32_t *hit = (uint32_t*)d.free, *desc = (uint32_t*)(d.free + o_desc);
        uint2 *nm = (uint2*)(d.free + o_nm), *nm2 = (uint2*)(d.free + o_nm2);
        const double dn = (double)n;
        profiled(c, "k_pm_hits", 20.0 * dn, [&] { return launch_pm_hits(s, mapping, hit, nm, cnt, c->st); });
        uint32_t rounds = 0;
        while ((1ull << rounds) < n) ++rounds;
        for (uint32_t r = 0; r < rounds; ++r) {
            profiled(c, "k_pm_double", 24.0 * dn, [&] { return launch_pm_double(s, nm, nm2, c->st); });
            std::swap(nm, nm2);
        }
        profiled(c, "k_pm_descents", 24.0 * dn,
                 [&] { return launch_pm_descents(s, mapping, hit, nm, desc, cnt + 2, c->st); });
        profiled(c, "k_pm_cycles", 20.0 * dn, [&] { return launch_pm_cycles(s, mapping, nm, desc, cnt + 3, c->st); });
        profiled(c, "k_pm_edges", 24.0 * (double)n_edges,
                 [&] { return launch_pm_edges(s, edges, n_edges, nm, cnt + 5, c->st); });
        unsigned long long h[7];
        read_counters(c, cnt, h, 7);
        result->cells_checked = n;
        result->not_permutation = h[0] + h[2];
        result->padding_failures = h[1];
        result->cycles = h[3];
        result->order_failures = h[4];
        result->edges_checked = h[5];
        result->edge_failures = h[6];
    });
}
// ---- transforms between Lagrange, coefficient and extended form, evaluation at
// points and the transform's check (ntt.hpp)
namespace {
struct NttCall {
    uint32_t k_in = 0, k = 0, ncols = 0;
    int form = 0, inverse = 0;
    bool shifted = false;
    Fr shift;                                              // canonical
};
}  // namespace
// The argument checks of svdw_ntt and svdw_check_ntt (log_samples: the latter's,
// else 0), in the order include/svdw.h gives; false: no columns, nothing to do.
static bool ntt_args(svdw_ctx* c, const char* fn, uint32_t k_in, uint32_t k, int form, int inverse,
                     const uint64_t shift[4], const void* const* in, uint32_t ncols, const void* out,
                     uint32_t log_samples, NttCall* a) {
    const std::string f(fn);
    REQUIRE(c, "null argument");
    check_form(form);
    const Fr one = fr_from_u64(1), s = shift ? fr_raw_words(shift) : one;
    REQUIRE(fr_reduced(s) && !fr_is_zero(s), f + ": shift >= p or shift == 0");
    REQUIRE(inverse == 0 || inverse == 1, f + ": inverse must be 0 or 1");
    need_k(f, k);
    if (k_in < 1 || k_in > k) fail(SVDW_ERANGE, f + ": k_in must be in [1, k]");
    if (inverse && k_in != k) fail(SVDW_ERANGE, f + ": an inverse transform needs k_in == k");
    if (log_samples > k) fail(SVDW_ERANGE, f + ": log_samples must be in [0, k]");
    need_device(c, f);
    *a = NttCall{k_in, k, ncols, form, inverse, !fr_eq(s, one), s};
    if (!ncols) return false;
    need_columns(f, ncols);
    REQUIRE(in && out, "null argument");
    const uintptr_t o0 = (uintptr_t)out, o1 = o0 + (((uintptr_t)ncols << k) * sizeof(Fr));
    for (uint32_t j = 0; j < ncols; ++j) {
        need_pointer(f, in[j]);
        const uintptr_t i0 = (uintptr_t)in[j];
        need_apart(f, "out", o0, o1, "an input column", i0, i0 + (((uintptr_t)1 << k_in) * sizeof(Fr)));
    }
    return true;
}
// The stage twiddles on the device, the same for every k and made once:
// omega_1024^j R, then omega_1024^-j R, for j < 512.
static const Fr* ntt_twiddles(svdw_ctx* c) {
    DBuf& b = c->prover.ntt_tw;
    if (b.p) return (const Fr*)b.p;
    std::vector<Fr> t(1024, fr_one_mont());
    const Fr w10 = domain_omega_mont(10);
    for (size_t j = 1; j < 512; ++j) t[j] = mont_mul(t[j - 1], w10);
    for (size_t j = 1; j < 512; ++j) t[512 + j] = fr_neg(t[512 - j]);   // omega^-j = -omega^(512 - j)
    ensure_buf(c, b, t.size() * sizeof(Fr));
    hipck(hipMemcpyAsync(b.p, t.data(), t.size() * sizeof(Fr), hipMemcpyHostToDevice, c->st), "H2D");
    hipck(hipStreamSynchronize(c->st), "hipStreamSynchronize");   // t goes away
    return (const Fr*)b.p;
}
uint32_t svdw_ntt_passes(uint32_t k) { return ntt_passes(k); }
// The transform of a checked call with columns: in (a.ncols pointers) to out.
static void ntt_run(svdw_ctx* c, const NttCall& a, const void* const* in, void* out) {
    sync(c);
    const uint32_t k = a.k, k_in = a.k_in, ncols = a.ncols;
    const int inverse = a.inverse;
    const uint32_t P = ntt_passes(k), kk = inverse ? k : k_in;
    const uint64_t N = 1ull << k;
    const Fr* tw = ntt_twiddles(c);
    const PowTable w = domain_table(c, k).dev;
    const Fr scale = inverse ? fr_to_mont(fr_inv(fr_from_u64(N))) : fr_one_mont();   // 2^-k R
    const size_t fcells = a.shifted ? pow_table_cells(kk) : 0;
    if (P > 1) ensure_buf(c, c->prover.ntt_tmp, (size_t)ncols * N * sizeof(Fr));   // the buffer between passes
    // the staged cells: the table of the shift's powers over the input's rows, the scale its top factor
    const Staged d = stage(c, in, ncols, nullptr, 0, fcells, 0, [&](Fr* t) {
        if (a.shifted) pow_table_fill(fr_to_mont(a.shift), scale, kk, t);
    });
    Fr* tmp = (Fr*)c->prover.ntt_tmp.p;
    uint32_t ls = 0;
    for (uint32_t i = 0; i < P; ++i) {
        NttPass p{};
        p.cols = i ? nullptr : d.ptrs;
        // the buffers alternate so that the last pass writes out
        p.src = i ? ((P - i) % 2 ? tmp : (const Fr*)out) : nullptr;
        p.dst = (P - 1 - i) % 2 ? tmp : (Fr*)out;
        p.tw = tw + (inverse ? 512 : 0);
        p.w = w;
        if (a.shifted) p.f = pow_table_view(d.cells, kk);
        p.fc = scale;
        p.k = k;
        p.kin = i ? k : k_in;
        p.b = ntt_pass_bits(k, i);
        p.ls = ls;
        p.ncols = ncols;
        p.inverse = (uint32_t)inverse;
        p.last = i + 1 == P;
        p.pre = !inverse && a.shifted && i == 0;
        p.post = inverse && p.last ? (a.shifted ? 2u : 1u) : 0u;
        ls += p.b;
        const char* label = i == 0 ? "k_ntt_pass1" : i == 1 ? "k_ntt_pass2" : "k_ntt_pass3";
        profiled(c, label, 32.0 * ncols * ((double)(1ull << p.kin) + (double)N),
                 [&] { return launch_ntt_pass(p, c->st); });
    }
}
int svdw_ntt(svdw_ctx* c, uint32_t k_in, uint32_t k, int form, int inverse, const uint64_t shift[4],
             const void* const* in, uint32_t ncols, void* out, svdw_ntt_result* result) {
    return guarded([&] {
        REQUIRE(result, "null argument");
        NttCall a;
        const bool any = ntt_args(c, "svdw_ntt", k_in, k, form, inverse, shift, in, ncols, out, 0, &a);
        memset(result, 0, sizeof *result);
        result->passes = ntt_passes(k);
        result->rows_in = 1ull << k_in;
        result->rows_out = 1ull << k;
        if (!any) return;
        ntt_run(c, a, in, out);
        result->columns = ncols;
    });
}
// The evaluations of ncols polynomials of n coefficients (cols or src, as the
// kernels take them) at the npoints points dpts (device, x R), in chunks of at
// most `chunk` points through part; then(q0, nq), if given, after each chunk's sums.
template <class Then = void (*)(uint64_t, uint32_t)>
static void ntt_eval_chunks(svdw_ctx* c, const Fr* const* cols, const Fr* src, uint64_t n, uint32_t ncols,
                            const Fr* dpts, uint64_t npoints, uint32_t chunk, Fr* part, uint64_t out_stride, Fr* out,
                            bool advance_out, Then&& then = [](uint64_t, uint32_t) {}) {
    const uint32_t nb = ntt_eval_blocks(n);
    for (uint64_t q0 = 0; q0 < npoints; q0 += chunk) {
        const uint32_t nq = (uint32_t)std::min<uint64_t>(chunk, npoints - q0);
        profiled(c, "k_ntt_eval", 32.0 * ncols * (double)n * nq,
                 [&] { return launch_ntt_eval(cols, src, n, ncols, dpts + q0, nq, part, c->st); });
        profiled(c, "k_ntt_eval_sum", 32.0 * ncols * (double)nq * (nb + 1), [&] {
            return launch_ntt_eval_sum(part, nb, ncols, nq, out_stride, out + (advance_out ? q0 : 0), c->st);
        });
        then(q0, nq);
    }
}
static constexpr uint32_t kNttPointChunk = 32768;          // points per launch of k_ntt_eval
int svdw_eval_polynomial(svdw_ctx* c, uint32_t k, int form, const void* const* coeffs, uint32_t ncols,
                         const uint64_t* points, uint32_t npoints, void* out) {
    return guarded([&] {
        const std::string f("svdw_eval_polynomial");
        REQUIRE(c && (points || !npoints), "null argument");
        check_form(form);
        for (uint32_t q = 0; q < npoints; ++q)
            REQUIRE(fr_reduced(fr_raw_words(points + 4 * (size_t)q)), f + ": point >= p");
        need_k(f, k);
        need_device(c, f);
        if (!ncols || !npoints) return;
        need_columns(f, ncols);
        REQUIRE(coeffs && out, "null argument");
        for (uint32_t j = 0; j < ncols; ++j) need_pointer(f, coeffs[j]);
        sync(c);
        const uint64_t n = 1ull << k;
        const uint32_t chunk = std::min(npoints, kNttPointChunk);
        const size_t part = (size_t)ncols * chunk * ntt_eval_blocks(n) * sizeof(Fr);
        const Staged d = stage(c, coeffs, ncols, nullptr, 0, npoints, part, [&](Fr* t) {
            for (uint32_t q = 0; q < npoints; ++q) t[q] = fr_to_mont(fr_raw_words(points + 4 * (size_t)q));
        });
        ntt_eval_chunks(c, d.ptrs, nullptr, n, ncols, d.cells, npoints, chunk, (Fr*)d.free, npoints, (Fr*)out, true);
    });
}
int svdw_check_ntt(svdw_ctx* c, uint32_t k_in, uint32_t k, int form, int inverse, const uint64_t shift[4],
                   const void* const* in, uint32_t ncols, const void* out, uint32_t log_samples, uint64_t seed,
                   svdw_ntt_check* result) {
    return guarded([&] {
        REQUIRE(result, "null argument");
        NttCall a;
        const bool any = ntt_args(c, "svdw_check_ntt", k_in, k, form, inverse, shift, in, ncols, out, log_samples, &a);
        memset(result, 0, sizeof *result);
        if (!any) return;
        sync(c);
        // the points: shift omega^j (forward), omega^j / shift (inverse), as x R
        const PowTable w = domain_table(c, k).host;
        const uint64_t S = 1ull << log_samples, n = 1ull << (inverse ? k : k_in);
        const Fr sR = fr_to_mont(inverse ? fr_inv(a.shift) : a.shift);
        const uint32_t chunk = (uint32_t)std::min<uint64_t>(S, kNttPointChunk);
        const size_t vals = (size_t)ncols * chunk * sizeof(Fr), part = vals * ntt_eval_blocks(n);
        const Staged d = stage(c, in, ncols, nullptr, 0, S, vals + part, [&](Fr* t) {
            for (uint64_t s = 0; s < S; ++s) {
                t[s] = mont_mul(pow_at(w, ntt_sample_row(k, log_samples, seed, s)), sR);
            }
        });
        Fr* dv = (Fr*)d.free;
        // forward: the input's polynomial against the cells of out; inverse: the other way round
        const Fr* const* pcols = inverse ? nullptr : d.ptrs;
        const Fr* psrc = inverse ? (const Fr*)out : nullptr;
        ntt_eval_chunks(c, pcols, psrc, n, ncols, d.cells, S, chunk, dv + (size_t)ncols * chunk, chunk, dv, false,
                        [&](uint64_t s0, uint32_t ns) {       // ns == chunk: both are powers of two
                            profiled(c, "k_ntt_compare", 64.0 * ncols * ns, [&] {
                                return launch_ntt_compare(inverse ? d.ptrs : nullptr,
                                                          inverse ? nullptr : (const Fr*)out, k, log_samples, seed,
                                                          s0, ns, ncols, dv, d.cnt, c->st);
                            });
                        });
        unsigned long long hc[2];
        read_counters(c, d.cnt, hc, 2);
        result->rows_checked = hc[0];
        result->row_failures = hc[1];
    });
}
// ---- KZG commitments of columns: the multi-scalar multiplication and its
// bit-serial check (commit.hpp)
// A batch's workspace stays under the option "commit_scratch_mib" (1 GiB by
// default: the order of ntt_tmp for 8 columns of 2^22 rows) unless one task
// alone needs more. The kernels between the sort and the window sums are
// latency-bound per batch, so fewer, larger batches are faster.
// The argument checks of svdw_commit and svdw_check_commit, in the order
// include/svdw.h gives; false: no columns, nothing to do.
static bool commit_args(svdw_ctx* c, const char* fn, uint32_t k, int form, int bases_form, const void* bases,
                        const void* const* cols, uint32_t ncols, const void* out, bool writes) {
    const std::string f(fn);
    REQUIRE(c, "null argument");
    check_form(form);
    check_form(bases_form);
    need_k(f, k);
    need_device(c, f);
    if (!ncols) return false;
    need_columns(f, ncols);
    REQUIRE(bases && cols && out, "null argument");
    const uintptr_t o0 = (uintptr_t)out, o1 = o0 + (uintptr_t)ncols * sizeof(G1Affine);
    const uintptr_t b0 = (uintptr_t)bases, b1 = b0 + (((uintptr_t)1 << k) * sizeof(G1Affine));
    if (writes) need_apart(f, "out", o0, o1, "the bases", b0, b1);
    for (uint32_t j = 0; j < ncols; ++j) {
        need_pointer(f, cols[j]);
        const uintptr_t i0 = (uintptr_t)cols[j];
        if (writes) need_apart(f, "out", o0, o1, "an input column", i0, i0 + (((uintptr_t)1 << k) * sizeof(Fr)));
    }
    return true;
}
void svdw_commit_plan(uint32_t k, uint32_t* window_bits, uint32_t* windows) {
    uint32_t c = 0, W = 0;
    commit_plan(k < 1 ? 1 : k > 28 ? 28 : k, &c, &W);
    if (window_bits) *window_bits = c;
    if (windows) *windows = W;
}
int svdw_commit(svdw_ctx* c, uint32_t k, int form, int bases_form, const void* bases, const void* const* cols,
                uint32_t ncols, void* out, svdw_commit_result* result) {
    return guarded([&] {
        REQUIRE(result, "null argument");
        const bool any = commit_args(c, "svdw_commit", k, form, bases_form, bases, cols, ncols, out, true);
        memset(result, 0, sizeof *result);
        commit_plan(k, &result->window_bits, &result->windows);
        if (c->opt.commit_window_bits) {                   // the tuning override
            result->window_bits = c->opt.commit_window_bits;
            result->windows = (255 + result->window_bits - 1) / result->window_bits;
        }
        result->rows = 1ull << k;
        if (!any) return;
        sync(c);
        const uint32_t cb = result->window_bits, W = result->windows;
        const uint64_t n = 1ull << k, B = 1ull << (cb - 1), tasks = (uint64_t)ncols * W;
        const uint64_t per = commit_task_bytes(n, B), cap = scratch_cap(c);
        const uint32_t T = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(cap / per, 1),
                                                        std::min<uint64_t>(tasks, 65535));
        // the call's window sums, then the arrays of one batch, each from a 128-byte boundary
        size_t off = 0;
        auto take = [&](size_t bytes) {
            const size_t at = off;
            off += (bytes + 127) / 128 * 128;
            return at;
        };
        const size_t o_win = take(tasks * sizeof(G1Xyzz)), o_slots = take(T * commit_slots_all(n) * sizeof(G1Xyzz)),
                     o_bkt = take(T * B * sizeof(G1Xyzz)), o_chk = take(T * commit_chunks(B) * sizeof(G1Xyzz)),
                     o_sorted = take(T * n * sizeof(uint32_t)), o_cur = take(T * B * sizeof(uint32_t)),
                     o_start = take(T * (B + 1) * sizeof(uint32_t));
        DBuf& wsb = c->prover.commit_ws;
        ensure_buf(c, wsb, off);
        char* ws = (char*)wsb.p;
        const Staged d = stage(c, cols, ncols, nullptr, 0, 0, 0, [](Fr*) {});
        CommitBatch a{};
        a.cols = d.ptrs;
        a.bases = (const G1Affine*)bases;
        a.windows = (G1Xyzz*)(ws + o_win);
        a.slots = (G1Xyzz*)(ws + o_slots);
        a.buckets = (G1Xyzz*)(ws + o_bkt);
        a.chunks = (G1Xyzz*)(ws + o_chk);
        a.sorted = (uint32_t*)(ws + o_sorted);
        a.cursor = (uint32_t*)(ws + o_cur);
        a.start = (uint32_t*)(ws + o_start);
        a.cnt = d.cnt;
        a.k = k;
        a.c = cb;
        a.W = W;
        a.ncols = ncols;
        a.form = form;
        a.bases_form = bases_form;
        for (uint64_t g0 = 0; g0 < tasks; g0 += T) {
            a.g0 = (uint32_t)g0;
            a.T = (uint32_t)std::min<uint64_t>(T, tasks - g0);
            profiled(c, "k_commit_batch", (32.0 + 64.0) * a.T * (double)n,
                     [&] { return launch_commit_batch(a, c->st); });
        }
        profiled(c, "k_commit_horner", 128.0 * tasks, [&] {
            return launch_commit_horner(a.windows, ncols, cb, W, bases_form, (G1Affine*)out, d.cnt, c->st);
        });
        unsigned long long h[3];
        read_counters(c, d.cnt, h, 3);
        result->columns = ncols;
        result->zero_scalars = h[0];
        result->identity_bases = h[1];
        result->identity_outputs = h[2];
    });
}
int svdw_check_commit(svdw_ctx* c, uint32_t k, int form, int bases_form, const void* bases, const void* const* cols,
                      uint32_t ncols, const void* commitments, svdw_commit_check* result) {
    return guarded([&] {
        REQUIRE(result, "null argument");
        const bool any =
            commit_args(c, "svdw_check_commit", k, form, bases_form, bases, cols, ncols, commitments, false);
        memset(result, 0, sizeof *result);
        if (!any) return;
        sync(c);
        const uint64_t n = 1ull << k;
        const size_t per = (size_t)kCommitScalarBits * commit_check_blocks(n) * sizeof(G1Xyzz);
        const uint32_t chunk = (uint32_t)std::min<size_t>(std::max<size_t>(((size_t)64 << 20) / per, 1), ncols);   // 64 MiB of partials
        const Staged d = stage(c, cols, ncols, nullptr, 0, 0, chunk * per, [](Fr*) {});
        unsigned long long* cnt = d.cnt;                   // [0..1] columns, [2..3] bases
        profiled(c, "k_commit_check_bases", 64.0 * (double)n,
                 [&] { return launch_commit_check_bases((const G1Affine*)bases, n, bases_form, cnt, c->st); });
        for (uint32_t c0 = 0; c0 < ncols; c0 += chunk) {
            const uint32_t nc = std::min(chunk, ncols - c0);
            profiled(c, "k_commit_check", 254.0 * nc * (double)n * 32.0, [&] {
                return launch_commit_check(d.ptrs, (const G1Affine*)bases, (const G1Affine*)commitments, k, c0, nc,
                                           form, bases_form, (G1Xyzz*)d.free, cnt, c->st);
            });
        }
        unsigned long long h[4];
        read_counters(c, cnt, h, 4);
        result->columns_checked = h[0];
        result->commit_failures = h[1];
        result->bases_checked = h[2];
        result->bases_off_curve = h[3];
    });
}
// A probe of the mixed-add rate: `threads` threads each add one affine point
// `reps` times into a register-resident accumulator; the seconds of the launch.
int svdw_commit_add_probe(svdw_ctx* c, const void* points, uint32_t npoints, uint64_t threads, uint32_t reps,
                          double* seconds) {
    return guarded([&] {
        REQUIRE(c && points && seconds && npoints && threads && reps, "null argument");
        need_device(c, "svdw_commit_add_probe");
        sync(c);
        DBuf& ws = c->prover.commit_ws;
        ensure_buf(c, ws, threads * sizeof(G1Xyzz));
        hipEvent_t e0, e1;
        hipck(hipEventCreate(&e0), "hipEventCreate");
        hipck(hipEventCreate(&e1), "hipEventCreate");
        hipck(hipEventRecord(e0, c->st), "hipEventRecord");
        const hipError_t le = launch_commit_add_probe((const G1Affine*)points, npoints, threads, reps,
                                                      (G1Xyzz*)ws.p, c->st);
        hipError_t re = hipEventRecord(e1, c->st);
        if (re == hipSuccess) re = hipEventSynchronize(e1);
        float ms = 0;
        if (re == hipSuccess) re = hipEventElapsedTime(&ms, e0, e1);
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        hipck(le, "k_commit_add_probe");
        hipck(re, "hipEventElapsedTime");
        *seconds = ms * 1e-3;
    });
}
// ---- the quotient polynomial on the extended domain and the verifier's identity
// at a point (quotient.hpp)
namespace {
struct QCall {
    Fr shift, beta, gamma, y, x;                           // canonical
    uint32_t k = 0, ek = 0, le = 0, D = 0, nsets = 0;
    uint64_t n = 0, N = 0, usable = 0;
    std::vector<const void*> ptrs;                         // every column, in the order QuotientArgs::ptrs gives
};
}  // namespace
// The argument checks of svdw_quotient and svdw_check_quotient (x: the latter's,
// else null; out: the former's), in the order include/svdw.h gives; false: no
// family, nothing to do.
static bool q_args(svdw_ctx* c, const char* fn, const svdw_quotient_args* a, const void* out, const uint64_t* x,
                   QCall* q) {
    const std::string f(fn);
    REQUIRE(c && a, "null argument");
    check_form(a->form);
    q->shift = fr_raw_words(a->shift);
    q->beta = fr_raw_words(a->beta);
    q->gamma = fr_raw_words(a->gamma);
    q->y = fr_raw_words(a->y);
    q->x = x ? fr_raw_words(x) : fr_zero();
    REQUIRE(fr_reduced(q->shift) && !fr_is_zero(q->shift), f + ": shift >= p or shift == 0");
    REQUIRE(fr_reduced(q->beta) && fr_reduced(q->gamma) && fr_reduced(q->y) && fr_reduced(q->x),
            f + ": beta, gamma, y or x >= p");
    const uint64_t rows = a->k < 63 ? 1ull << a->k : ~0ull;
    if (!a->unusable_rows || a->unusable_rows >= rows) fail(SVDW_ERANGE, f + ": unusable_rows must be in [1, 2^k)");
    REQUIRE(a->chunk_len || !a->n_perm, f + ": chunk_len == 0");
    need_k(f, a->k);
    if (a->extended_k < a->k || a->extended_k > 28) fail(SVDW_ERANGE, f + ": extended_k must be in [k, 28]");
    q->k = a->k;
    q->ek = a->extended_k;
    q->le = q->ek - q->k;
    q->n = rows;
    q->N = 1ull << q->ek;
    q->usable = rows - a->unusable_rows;
    q->nsets = a->n_perm ? pp_sets(a->n_perm, a->chunk_len) : 0;
    q->D = std::max({a->n_gate ? 3u : 0u, a->n_lookup ? 4u : 0u,
                     a->n_perm ? 2u + std::min(a->chunk_len, a->n_perm) : 0u});
    if (q->D > (1ull << q->le) + 1) fail(SVDW_ERANGE, f + ": the degree does not fit the extended domain (D > E + 1)");
    {
        Fr t = fr_to_mont(q->shift);                       // shift^N == 1: shift^n is an E-th root of unity
        for (uint32_t i = 0; i < q->ek; ++i) t = mont_mul(t, t);
        REQUIRE(!fr_eq(t, fr_one_mont()), f + ": shift^n is an E-th root of unity (a zero divisor)");
    }
    need_device(c, f);
    need_columns(f, std::max({a->n_gate, a->n_perm, a->n_lookup}), " in a family");
    if (!a->n_gate && !a->n_perm && !a->n_lookup) return false;
    REQUIRE(out || x, "null argument");
    const struct {
        const void* const* p;
        uint32_t n;
    } fam[] = {{a->advice, a->n_gate},          {a->selectors, a->n_gate},       {a->perm_columns, a->n_perm},
               {a->sigma, a->n_perm},           {a->perm_z, q->nsets},           {a->lookup_input, a->n_lookup},
               {a->lookup_table, a->n_lookup},  {a->permuted_input, a->n_lookup}, {a->permuted_table, a->n_lookup},
               {a->lookup_z, a->n_lookup}};
    for (const auto& fm : fam) {
        REQUIRE(fm.p || !fm.n, "null argument");
        for (uint32_t j = 0; j < fm.n; ++j) {
            need_pointer(f, fm.p[j]);
            q->ptrs.push_back(fm.p[j]);
        }
    }
    if (out) {
        const uintptr_t o0 = (uintptr_t)out, o1 = o0 + q->N * sizeof(Fr);
        for (const void* p : q->ptrs) {
            need_apart(f, "h_ext", o0, o1, "an input column", (uintptr_t)p, (uintptr_t)p + q->N * sizeof(Fr));
        }
    }
    return true;
}
// The extended columns of l_0, l_last, l_active (R form, 3 x N cells) for the
// call's key: three Lagrange columns through the engine's own inverse and coset
// transforms, kept on the context until the key changes.
static const Fr* q_basis(svdw_ctx* c, const QCall& q, uint32_t unusable_rows) {
    ProverState& ps = c->prover;
    const size_t need = 3 * q.N * sizeof(Fr);
    if (ps.basis.cap >= need && ps.basis_k == q.k && ps.basis_ek == q.ek && ps.basis_unusable == unusable_rows &&
        fr_eq(ps.basis_shift, q.shift))
        return (const Fr*)ps.basis.p;
    ps.basis_k = 0;                                        // no key while the columns are rebuilt
    ensure_buf(c, ps.basis, need);
    ensure_buf(c, ps.basis_tmp, 6 * q.n * sizeof(Fr));
    Fr *lag = (Fr*)ps.basis_tmp.p, *cf = lag + 3 * q.n;
    profiled(c, "k_quotient_basis", 96.0 * q.n, [&] {
        return launch_quotient_basis(lag, q.n, q.usable, fr_one_mont(), c->st);
    });
    const void* in[3] = {lag, lag + q.n, lag + 2 * q.n};
    const void* mid[3] = {cf, cf + q.n, cf + 2 * q.n};
    const Fr one = fr_from_u64(1);                         // to coefficients, then onto the extended coset
    ntt_run(c, NttCall{q.k, q.k, 3, SVDW_FORM_MONTGOMERY, 1, false, one}, in, cf);
    ntt_run(c, NttCall{q.k, q.ek, 3, SVDW_FORM_MONTGOMERY, 0, !fr_eq(q.shift, one), q.shift}, mid, ps.basis.p);
    ps.basis_k = q.k;
    ps.basis_ek = q.ek;
    ps.basis_unusable = unusable_rows;
    ps.basis_shift = q.shift;
    return (const Fr*)ps.basis.p;
}
int svdw_quotient(svdw_ctx* c, const svdw_quotient_args* args, void* h_ext, svdw_quotient_result* result) {
    return guarded([&] {
        REQUIRE(result, "null argument");
        QCall q;
        const bool any = q_args(c, "svdw_quotient", args, h_ext, nullptr, &q);
        memset(result, 0, sizeof *result);
        result->rows = q.N;
        result->extension = 1u << q.le;
        result->degree = q.D;
        if (!any) return;
        REQUIRE(h_ext, "null output");
        sync(c);
        const bool mont = args->form == SVDW_FORM_MONTGOMERY;
        const uint32_t ng = args->n_gate, np = args->n_perm, nl = args->n_lookup, E = 1u << q.le;
        const Fr* l = (np | nl) ? q_basis(c, q, args->unusable_rows) : nullptr;
        const Fr one = fr_one_mont();
        // the staged cells: beta delta^j phi for j < np, then the E inverses of the divisor as c R
        const Staged d = stage(c, q.ptrs.data(), (uint32_t)q.ptrs.size(), nullptr, 0, (size_t)np + E, 0, [&](Fr* t) {
            pp_delta_powers(q.beta, args->form, np, t);
            Fr* inv = t + np;
            Fr sn = fr_to_mont(q.shift), wn = domain_omega_mont(q.ek);   // shift^n R, omega_e^n R
            for (uint32_t i = 0; i < q.k; ++i) {
                sn = mont_mul(sn, sn);
                wn = mont_mul(wn, wn);
            }
            // batch inversion: prefix products, one inverse, back substitution
            std::vector<Fr> dv(E), pre(E);
            Fr acc = one;
            for (uint32_t i = 0; i < E; ++i) {
                dv[i] = fr_sub(sn, one);                   // (shift^n omega_e^(n i) - 1) R, not zero (q_args)
                pre[i] = acc;
                acc = mont_mul(acc, dv[i]);
                sn = mont_mul(sn, wn);
            }
            Fr ia = fr_to_mont(fr_to_mont(fr_inv(acc)));    // acc = P R: (P R)^-1 R^2 = P^-1 R
            for (uint32_t i = E; i-- > 0;) {
                inv[i] = mont_mul(ia, pre[i]);
                ia = mont_mul(ia, dv[i]);
            }
        });
        QuotientArgs a{};
        a.ptrs = d.ptrs;
        a.bd = d.cells;
        a.inv = d.cells + np;
        a.w = domain_table(c, q.ek).dev;
        a.l0 = l;
        a.llast = l ? l + q.N : nullptr;
        a.lact = l ? l + 2 * q.N : nullptr;
        a.out = (Fr*)h_ext;
        a.y = fr_to_mont(q.y);
        a.beta = fr_to_mont(q.beta);
        a.shift = fr_to_mont(q.shift);
        a.gamma = mont ? fr_to_mont(q.gamma) : q.gamma;
        a.betaf = mont ? a.beta : q.beta;
        a.one = mont ? one : fr_from_u64(1);
        a.ek = q.ek;
        a.le = q.le;
        a.ng = ng;
        a.np = np;
        a.chunk = args->chunk_len;
        a.nsets = q.nsets;
        a.nl = nl;
        a.usable = q.usable;
        const double cols = 5.0 * ng + 2.0 * np + 3.0 * q.nsets + 7.0 * nl + ((np | nl) ? 3.0 : 0.0) + 1.0;
        profiled(c, "k_quotient", 32.0 * cols * (double)q.N, [&] { return launch_quotient(a, args->form, c->st); });
        result->gate_expressions = ng;
        result->permutation_expressions = np ? 1 + 2 * (uint64_t)q.nsets : 0;
        result->lookup_expressions = 5 * (uint64_t)nl;
    });
}
// l_i(x) R for x^n != 1: omega^i (x^n - 1) / (n (x - omega^i)); t = (x^n - 1) / n as t R.
static Fr q_lagrange_at(const Fr& xR, const Fr& wiR, const Fr& tR) {
    const Fr inv = fr_to_mont(fr_inv(fr_from_mont(fr_sub(xR, wiR))));
    return mont_mul(mont_mul(wiR, tR), inv);
}
int svdw_check_quotient(svdw_ctx* c, const svdw_quotient_args* args, const void* h_coeffs, const uint64_t x[4],
                        svdw_quotient_check* result) {
    return guarded([&] {
        REQUIRE(result && x, "null argument");
        QCall q;
        const bool any = q_args(c, "svdw_check_quotient", args, nullptr, x, &q);
        memset(result, 0, sizeof *result);
        if (!any) return;
        REQUIRE(h_coeffs, "null argument");
        sync(c);
        const bool mont = args->form == SVDW_FORM_MONTGOMERY;
        const uint32_t ng = args->n_gate, np = args->n_perm, nl = args->n_lookup, ns = q.nsets;
        const Fr one = fr_one_mont();
        // the points x omega^r R, r in {0, 1, 2, 3, -1, usable}
        constexpr uint32_t kPts = 6;
        const Fr xR = fr_to_mont(q.x), w = domain_omega_mont(q.k);
        const Fr wu = fr_to_mont(fr_pow_u64(fr_from_mont(w), q.usable)), wm = fr_to_mont(fr_pow_u64(fr_from_mont(w), q.n - 1));
        const Fr w2 = mont_mul(w, w);
        const Fr pts[kPts] = {xR, mont_mul(xR, w), mont_mul(xR, w2), mont_mul(xR, mont_mul(w2, w)), mont_mul(xR, wm),
                              mont_mul(xR, wu)};
        // every column at every point, in chunks of columns; the values as v R
        const size_t total = q.ptrs.size();
        std::vector<Fr> vals(total * kPts);
        constexpr size_t kColChunk = 16384;
        for (size_t c0 = 0; c0 < total; c0 += kColChunk) {
            const uint32_t nc = (uint32_t)std::min(kColChunk, total - c0);
            const size_t part = (size_t)nc * kPts * ntt_eval_blocks(q.n) * sizeof(Fr), outb = (size_t)nc * kPts * sizeof(Fr);
            const Staged d = stage(c, q.ptrs.data() + c0, nc, nullptr, 0, kPts, part + outb, [&](Fr* t) {
                for (uint32_t i = 0; i < kPts; ++i) t[i] = pts[i];
            });
            Fr* dout = (Fr*)(d.free + part);
            ntt_eval_chunks(c, d.ptrs, nullptr, q.n, nc, d.cells, kPts, kPts, (Fr*)d.free, kPts, dout, true);
            hipck(hipMemcpyAsync(vals.data() + c0 * kPts, dout, outb, hipMemcpyDeviceToHost, c->st), "D2H");
            hipck(hipStreamSynchronize(c->st), "hipStreamSynchronize");
        }
        // h at x, and its tail counted on the device
        Fr hx;
        unsigned long long tail[2];
        {
            const size_t part = (size_t)ntt_eval_blocks(q.N) * sizeof(Fr);
            const Staged d = stage(c, &h_coeffs, 1, nullptr, 0, 1, part + sizeof(Fr), [&](Fr* t) { t[0] = xR; });
            Fr* dout = (Fr*)(d.free + part);
            ntt_eval_chunks(c, d.ptrs, nullptr, q.N, 1, d.cells, 1, 1, (Fr*)d.free, 1, dout, true);
            const uint64_t from = (uint64_t)q.D * (q.n - 1) + 1 - q.n;   // D >= 2: not negative
            profiled(c, "k_quotient_tail", 32.0 * (double)(q.N - from),
                     [&] { return launch_quotient_tail((const Fr*)h_coeffs, from, q.N, d.cnt, c->st); });
            hipck(hipMemcpyAsync(&hx, dout, sizeof(Fr), hipMemcpyDeviceToHost, c->st), "D2H");
            read_counters(c, d.cnt, tail, 2);
        }
        if (!mont) {
            for (Fr& v : vals) v = fr_to_mont(v);
            hx = fr_to_mont(hx);
        }
        // l_0, l_last, l_active at x by the closed form
        Fr xn = xR;
        for (uint32_t i = 0; i < q.k; ++i) xn = mont_mul(xn, xn);
        const Fr xn1 = fr_sub(xn, one);
        Fr l0, ll, la = one;
        {
            const bool on_domain = fr_is_zero(xn1);       // x = omega^i: l_i(x) = 1 there and 0 elsewhere
            const Fr t = mont_mul(xn1, fr_to_mont(fr_inv(fr_from_u64(q.n))));
            l0 = on_domain ? (fr_eq(xR, one) ? one : fr_zero()) : q_lagrange_at(xR, one, t);
            ll = fr_zero();
            Fr wi = wu;
            for (uint64_t i = q.usable; i < q.n; ++i) {
                const Fr li = on_domain ? (fr_eq(xR, wi) ? one : fr_zero()) : q_lagrange_at(xR, wi, t);
                if (i == q.usable) ll = li;
                la = fr_sub(la, li);
                wi = mont_mul(wi, w);
            }
        }
        // the fold, include/svdw.h's list in its order
        const Fr b = fr_to_mont(q.beta), g = fr_to_mont(q.gamma), y = fr_to_mont(q.y);
        const uint32_t fam_cols[10] = {ng, ng, np, np, ns, nl, nl, nl, nl, nl};
        size_t base[10] = {0};                             // a family's first column among q.ptrs
        for (int i = 1; i < 10; ++i) base[i] = base[i - 1] + fam_cols[i - 1];
        enum { ADV, SEL, PV, SIG, PZ, LA, LT, LAP, LSP, LZ };
        enum { X0, X1, X2, X3, XM, XU };
        auto val = [&](int fam, size_t i, int pt) { return vals[(base[fam] + i) * kPts + pt]; };
        Fr h = fr_zero();
        auto push = [&](const Fr& e) { h = fr_add(mont_mul(h, y), e); };
        for (uint32_t i = 0; i < ng; ++i)
            push(mont_mul(val(SEL, i, X0),
                          fr_sub(fr_add(val(ADV, i, X0), mont_mul(val(ADV, i, X1), val(ADV, i, X2))), val(ADV, i, X3))));
        if (np) {
            push(mont_mul(l0, fr_sub(one, val(PZ, 0, X0))));
            const Fr zl = val(PZ, ns - 1, X0);
            push(mont_mul(ll, fr_sub(mont_mul(zl, zl), zl)));
            for (uint32_t s = 1; s < ns; ++s) push(mont_mul(l0, fr_sub(val(PZ, s, X0), val(PZ, s - 1, XU))));
            Fr bd = b;                                     // beta delta^j R
            const Fr dl = fr_to_mont(domain_consts().delta);
            for (uint32_t s = 0; s < ns; ++s) {
                Fr left = val(PZ, s, X1), right = val(PZ, s, X0);
                for (uint32_t j = s * args->chunk_len; j < std::min<uint64_t>((uint64_t)(s + 1) * args->chunk_len, np); ++j) {
                    const Fr v = fr_add(val(PV, j, X0), g);
                    left = mont_mul(left, fr_add(v, mont_mul(b, val(SIG, j, X0))));
                    right = mont_mul(right, fr_add(v, mont_mul(bd, xR)));
                    bd = mont_mul(bd, dl);
                }
                push(mont_mul(la, fr_sub(left, right)));
            }
        }
        for (uint32_t i = 0; i < nl; ++i) {
            const Fr z = val(LZ, i, X0), ap = val(LAP, i, X0), sp = val(LSP, i, X0);
            push(mont_mul(l0, fr_sub(one, z)));
            push(mont_mul(ll, fr_sub(mont_mul(z, z), z)));
            const Fr left = mont_mul(val(LZ, i, X1), mont_mul(fr_add(ap, b), fr_add(sp, g)));
            const Fr right = mont_mul(z, mont_mul(fr_add(val(LA, i, X0), b), fr_add(val(LT, i, X0), g)));
            push(mont_mul(la, fr_sub(left, right)));
            const Fr d = fr_sub(ap, sp);
            push(mont_mul(l0, d));
            push(mont_mul(la, mont_mul(d, fr_sub(ap, val(LAP, i, XM)))));
        }
        const Fr lhs = fr_from_mont(mont_mul(hx, xn1)), rhs = fr_from_mont(h);
        fr_store_words(lhs, result->lhs);
        fr_store_words(rhs, result->rhs);
        result->identity_failures = !fr_eq(lhs, rhs);
        result->tail_checked = tail[0];
        result->tail_nonzero = tail[1];
    });
}
// ---- the SHPLONK opening: h1, h2, their check and the linear combination (open.hpp)
namespace {
struct OpenCall {
    uint32_t k = 0, ncols = 0, nsets = 0, passes = 0, minpts = 8;
    uint64_t n = 0;
    Fr y, v, u, t;                                         // x R
    std::vector<std::vector<Fr>> S;                        // the sets' points, x R
    std::vector<Fr> T;                                     // their union, x R, in the order of first appearance
    std::vector<uint32_t> first;                           // set i's columns: slots [first[i], first[i + 1])
    std::vector<uint32_t> col;                             // the column index of a slot: index order within a set
    std::vector<const void*> ptrs;                         // the columns by slot
};
}  // namespace
// Host field arithmetic on x R.
static Fr om_inv(const Fr& xR) { return fr_to_mont(fr_inv(fr_from_mont(xR))); }
static bool om_in(const std::vector<Fr>& set, const Fr& x) {
    return std::any_of(set.begin(), set.end(), [&](const Fr& s) { return fr_eq(s, x); });
}
// prod over the points s of `of` that are not in `without` of (x - s), as R-form.
static Fr om_vanish(const std::vector<Fr>& of, const std::vector<Fr>* without, const Fr& xR) {
    Fr z = fr_one_mont();
    for (const Fr& s : of)
        if (!without || !om_in(*without, s)) z = mont_mul(z, fr_sub(xR, s));
    return z;
}
// The argument checks of the three opening entries (u, t: null where the entry
// has none; out0, out1: the outputs, h1: the input of linearise), in the order
// include/svdw.h gives; false: no columns, nothing to do.
static bool open_args(svdw_ctx* c, const char* fn, uint32_t k, int form, const void* const* cols, uint32_t ncols,
                      const uint32_t* set_of, const uint64_t* points, const uint32_t* npoints, uint32_t nsets,
                      const uint64_t* y, const uint64_t* v, const uint64_t* u, bool has_u, const uint64_t* t,
                      bool has_t, const void* h1, const void* h2, bool h1_is_out, bool h2_is_out, OpenCall* q) {
    const std::string f(fn);
    REQUIRE(c && y && v && (u || !has_u) && (t || !has_t), "null argument");
    REQUIRE((set_of || !ncols) && ((points && npoints) || !nsets), "null argument");
    check_form(form);
    const Fr zero = fr_zero();
    const Fr ch[4] = {fr_raw_words(y), fr_raw_words(v), has_u ? fr_raw_words(u) : zero, has_t ? fr_raw_words(t) : zero};
    REQUIRE(fr_reduced(ch[0]) && fr_reduced(ch[1]) && fr_reduced(ch[2]) && fr_reduced(ch[3]),
            f + ": y, v, u or t >= p");
    const uint32_t ns = std::min(nsets, 256u);             // of more sets (refused below) the first 256 are looked at
    q->S.assign(ns, {});
    for (uint32_t i = 0; i < ns; ++i)
        for (uint32_t j = 0; j < std::min(npoints[i], 8u); ++j) {
            const Fr s = fr_raw_words(points + 4 * (8 * (size_t)i + j));
            REQUIRE(fr_reduced(s), f + ": a point >= p");
            q->S[i].push_back(fr_to_mont(s));
        }
    for (const auto& s : q->S)
        for (size_t a = 0; a < s.size(); ++a)
            for (size_t b = 0; b < a; ++b) REQUIRE(!fr_eq(s[a], s[b]), f + ": two equal points in a set");
    std::vector<uint32_t> count(ns, 0);
    for (uint32_t j = 0; j < ncols; ++j) {
        REQUIRE(set_of[j] < nsets, f + ": set_of out of range");
        if (set_of[j] < ns) ++count[set_of[j]];
    }
    for (uint32_t i = 0; i < ns && ncols; ++i) REQUIRE(count[i], f + ": a set without a polynomial");
    for (const auto& s : q->S)
        for (const Fr& x : s)
            if (!om_in(q->T, x)) q->T.push_back(x);
    q->y = fr_to_mont(ch[0]);
    q->v = fr_to_mont(ch[1]);
    q->u = fr_to_mont(ch[2]);
    q->t = fr_to_mont(ch[3]);
    REQUIRE(!has_u || !om_in(q->T, q->u), f + ": u is one of the points");
    need_k(f, k);
    need_device(c, f);
    q->k = k;
    q->n = 1ull << k;
    q->ncols = ncols;
    q->nsets = nsets;
    if (!ncols) return false;
    need_columns(f, ncols);
    if (nsets < 1 || nsets > 255) fail(SVDW_ERANGE, f + ": nsets must be in [1, 255]");
    for (uint32_t i = 0; i < nsets; ++i) {
        if (npoints[i] < 1 || npoints[i] > 8) fail(SVDW_ERANGE, f + ": npoints must be in [1, 8]");
        q->passes += npoints[i];
        q->minpts = std::min(q->minpts, npoints[i]);
    }
    REQUIRE(cols && h1 && (h2 || !has_u), "null argument");
    for (uint32_t j = 0; j < ncols; ++j) need_pointer(f, cols[j]);
    const uintptr_t bytes = (uintptr_t)q->n * sizeof(Fr), a1 = (uintptr_t)h1, a2 = (uintptr_t)h2;
    for (uint32_t j = 0; j < ncols; ++j) {
        const uintptr_t i0 = (uintptr_t)cols[j];
        if (h1_is_out) need_apart(f, "h1_out", a1, a1 + bytes, "an input column", i0, i0 + bytes);
        if (h2_is_out) need_apart(f, "h2_out", a2, a2 + bytes, "an input column", i0, i0 + bytes);
    }
    if (h2_is_out) need_apart(f, "h2_out", a2, a2 + bytes, "h1", a1, a1 + bytes);
    q->first.assign(nsets + 1, 0);
    for (uint32_t i = 0; i < nsets; ++i) q->first[i + 1] = q->first[i] + count[i];
    std::vector<uint32_t> at(q->first.begin(), q->first.end() - 1);
    q->col.resize(ncols);
    q->ptrs.resize(ncols);
    for (uint32_t j = 0; j < ncols; ++j) {
        const uint32_t slot = at[set_of[j]]++;
        q->col[slot] = j;
        q->ptrs[slot] = cols[j];
    }
    return true;
}
// The slots' scalars of the fold per set: y^(m - 1 - pos) R for position pos of a set's m columns.
static void open_fold_scalars(const OpenCall& q, Fr* sc) {
    for (uint32_t i = 0; i < q.nsets; ++i) {
        Fr p = fr_one_mont();
        for (uint32_t s = q.first[i + 1]; s-- > q.first[i];) {
            sc[s] = p;
            p = mont_mul(p, q.y);
        }
    }
}
// c_i v^(nsets - 1 - i) R per set, c_i = Z_{T \ S_i}(at) / Z_{T \ S_0}(at) (norm) or Z_{T \ S_i}(at).
static std::vector<Fr> open_set_weights(const OpenCall& q, const Fr& at, bool norm) {
    std::vector<Fr> w(q.nsets);
    const Fr z0i = norm ? om_inv(om_vanish(q.T, &q.S[0], at)) : fr_one_mont();
    Fr p = fr_one_mont();
    for (uint32_t i = q.nsets; i-- > 0;) {
        w[i] = mont_mul(mont_mul(om_vanish(q.T, &q.S[i], at), z0i), p);
        p = mont_mul(p, q.v);
    }
    return w;
}
// One division of a[0..n) by (X - s) on the stream: out = the quotient, or out v + it.
static void open_divide(svdw_ctx* c, const Fr* a, uint64_t n, const PowTable& pw, Fr* tot, const Fr* v, Fr* out,
                        Fr* rem) {
    const uint64_t nt = open_tiles(n);
    if (nt > 1) {
        profiled(c, "k_open_tiles", 32.0 * (double)n, [&] { return launch_open_tiles(a, n, pw, tot, c->st); });
        profiled(c, "k_open_carry", 64.0 * (double)nt, [&] { return launch_open_carry(tot, nt, pw, c->st); });
    }
    profiled(c, "k_open_write", (v ? 96.0 : 64.0) * (double)n,
             [&] { return launch_open_write(a, n, pw, nt > 1 ? tot : nullptr, v, out, rem, c->st); });
}
static void open_result(const OpenCall& q, uint32_t passes, svdw_open_result* r) {
    memset(r, 0, sizeof *r);
    r->rows = q.n;
    if (!q.ncols) return;
    r->columns = q.ncols;
    r->sets = q.nsets;
    r->points = (uint32_t)q.T.size();
    r->passes = passes;
}
int svdw_open_quotient(svdw_ctx* c, uint32_t k, int form, const void* const* cols, uint32_t ncols,
                       const uint32_t* set_of, const uint64_t* points, const uint32_t* npoints, uint32_t nsets,
                       const uint64_t y[4], const uint64_t v[4], void* h1_out, svdw_open_result* result) {
    return guarded([&] {
        REQUIRE(result, "null argument");
        OpenCall q;
        const bool any = open_args(c, "svdw_open_quotient", k, form, cols, ncols, set_of, points, npoints, nsets, y, v,
                                   nullptr, false, nullptr, false, h1_out, nullptr, true, false, &q);
        open_result(q, q.passes, result);
        if (!any) return;
        sync(c);
        const uint64_t n = q.n, nt = open_tiles(n);
        const uint32_t pb = open_pow_bits(k), tc = (uint32_t)pow_table_cells(pb);
        // the staged cells: the slots' scalars, then a power table per point in the order of the divisions
        const Staged d = stage(c, q.ptrs.data(), ncols, nullptr, 0, ncols + q.passes * tc, (n + nt) * sizeof(Fr),
                               [&](Fr* t) {
                                   open_fold_scalars(q, t);
                                   Fr* tab = t + ncols;
                                   for (const auto& s : q.S)
                                       for (const Fr& x : s) {
                                           pow_table_fill(x, fr_one_mont(), pb, tab);
                                           tab += tc;
                                       }
                               });
        Fr *F = (Fr*)d.free, *tot = F + n;
        const Fr* tab = d.cells + ncols;
        for (uint32_t i = 0; i < nsets; ++i) {
            const uint32_t m = q.first[i + 1] - q.first[i];
            profiled(c, "k_open_fold", 32.0 * (m + 1) * (double)n, [&] {
                return launch_open_fold(d.ptrs + q.first[i], d.cells + q.first[i], m, nullptr, fr_zero(), n, F, c->st);
            });
            for (size_t p = 0; p < q.S[i].size(); ++p, tab += tc) {
                const bool last = p + 1 == q.S[i].size();   // h1 <- h1 v + Q_i; set 0 starts h1
                open_divide(c, F, n, pow_table_view(tab, pb), tot, last && i ? &q.v : nullptr, last ? (Fr*)h1_out : F,
                            nullptr);
            }
        }
    });
}
// The slots' scalars of G: c_i v^(nsets - 1 - i) y^(m - 1 - pos) R.
static void open_g_scalars(const OpenCall& q, Fr* sc) {
    open_fold_scalars(q, sc);
    const std::vector<Fr> w = open_set_weights(q, q.u, true);
    for (uint32_t i = 0; i < q.nsets; ++i)
        for (uint32_t s = q.first[i]; s < q.first[i + 1]; ++s) sc[s] = mont_mul(sc[s], w[i]);
}
int svdw_open_linearise(svdw_ctx* c, uint32_t k, int form, const void* const* cols, uint32_t ncols,
                        const uint32_t* set_of, const uint64_t* points, const uint32_t* npoints, uint32_t nsets,
                        const uint64_t y[4], const uint64_t v[4], const uint64_t u[4], const void* h1, void* h2_out,
                        svdw_open_result* result) {
    return guarded([&] {
        REQUIRE(result, "null argument");
        OpenCall q;
        const bool any = open_args(c, "svdw_open_linearise", k, form, cols, ncols, set_of, points, npoints, nsets, y,
                                   v, u, true, nullptr, false, h1, h2_out, false, true, &q);
        open_result(q, 1, result);
        if (!any) return;
        sync(c);
        const uint64_t n = q.n, nt = open_tiles(n);
        const uint32_t pb = open_pow_bits(k), tc = (uint32_t)pow_table_cells(pb);
        // the staged cells: the slots' scalars of G, then the power table of u
        const Staged d = stage(c, q.ptrs.data(), ncols, nullptr, 0, ncols + tc, nt * sizeof(Fr), [&](Fr* t) {
            open_g_scalars(q, t);
            pow_table_fill(q.u, fr_one_mont(), pb, t + ncols);
        });
        const Fr cacc = fr_neg(om_vanish(q.S[0], nullptr, q.u));   // -Z_{S_0}(u) R
        Fr *G = (Fr*)h2_out, *rem = (Fr*)d.cnt;            // G is built in h2_out and divided in place
        profiled(c, "k_open_fold", 32.0 * (ncols + 2) * (double)n, [&] {
            return launch_open_fold(d.ptrs, d.cells, ncols, (const Fr*)h1, cacc, n, G, c->st);
        });
        open_divide(c, G, n, pow_table_view(d.cells + ncols, pb), (Fr*)d.free, nullptr, G, rem);
        Fr r;
        hipck(hipMemcpyAsync(&r, rem, sizeof r, hipMemcpyDeviceToHost, c->st), "D2H");
        hipck(hipStreamSynchronize(c->st), "hipStreamSynchronize");
        fr_store_words(form == SVDW_FORM_MONTGOMERY ? fr_from_mont(r) : r, result->remainder);
    });
}
int svdw_check_open(svdw_ctx* c, uint32_t k, int form, const void* const* cols, uint32_t ncols,
                    const uint32_t* set_of, const uint64_t* points, const uint32_t* npoints, uint32_t nsets,
                    const uint64_t y[4], const uint64_t v[4], const uint64_t u[4], const void* h1, const void* h2,
                    const uint64_t t[4], uint64_t* evals_out, svdw_open_check* result) {
    return guarded([&] {
        REQUIRE(result, "null argument");
        OpenCall q;
        const bool any = open_args(c, "svdw_check_open", k, form, cols, ncols, set_of, points, npoints, nsets, y, v, u,
                                   true, t, true, h1, h2, false, false, &q);
        memset(result, 0, sizeof *result);
        if (!any) return;
        REQUIRE(evals_out, "null argument");
        sync(c);
        const bool mont = form == SVDW_FORM_MONTGOMERY;
        const uint64_t n = q.n;
        const Fr one = fr_one_mont();
        // points[0..np) R then t R at the nc columns ptrs: nc x (np + 1) values, as x R
        auto evaluate = [&](const void* const* ptrs, uint32_t nc, const Fr* pts, uint32_t np, Fr* vals) {
            const uint32_t nq = np + 1;
            const size_t part = (size_t)nc * nq * ntt_eval_blocks(n) * sizeof(Fr), outb = (size_t)nc * nq * sizeof(Fr);
            const Staged d = stage(c, ptrs, nc, nullptr, 0, nq, part + outb, [&](Fr* cells) {
                for (uint32_t i = 0; i < np; ++i) cells[i] = pts[i];
                cells[np] = q.t;
            });
            Fr* dout = (Fr*)(d.free + part);
            ntt_eval_chunks(c, d.ptrs, nullptr, n, nc, d.cells, nq, nq, (Fr*)d.free, nq, dout, true);
            hipck(hipMemcpyAsync(vals, dout, outb, hipMemcpyDeviceToHost, c->st), "D2H");
            hipck(hipStreamSynchronize(c->st), "hipStreamSynchronize");
            if (!mont)
                for (size_t i = 0; i < (size_t)nc * nq; ++i) vals[i] = fr_to_mont(vals[i]);
        };
        memset(evals_out, 0, (size_t)ncols * 8 * 4 * sizeof(uint64_t));
        // per set: F_i at its points and at t (folded with y), then r_i at t and at u by Lagrange
        std::vector<Fr> Ft(nsets), rt(nsets), ru(nsets), vals;
        for (uint32_t i = 0; i < nsets; ++i) {
            const std::vector<Fr>& S = q.S[i];
            const uint32_t m = q.first[i + 1] - q.first[i], np = (uint32_t)S.size(), nq = np + 1;
            vals.resize((size_t)m * nq);
            evaluate(q.ptrs.data() + q.first[i], m, S.data(), np, vals.data());
            std::vector<Fr> F(nq, fr_zero());
            for (uint32_t s = 0; s < m; ++s)
                for (uint32_t p = 0; p < nq; ++p) {
                    const Fr& e = vals[(size_t)s * nq + p];
                    F[p] = fr_add(mont_mul(F[p], q.y), e);
                    if (p < np) fr_store_words(fr_from_mont(e), evals_out + 4 * (8 * (size_t)q.col[q.first[i] + s] + p));
                }
            Ft[i] = F[np];
            rt[i] = ru[i] = fr_zero();
            for (uint32_t a = 0; a < np; ++a) {
                Fr den = one, nt_ = one, nu = one;
                for (uint32_t b = 0; b < np; ++b) {
                    if (b == a) continue;
                    den = mont_mul(den, fr_sub(S[a], S[b]));
                    nt_ = mont_mul(nt_, fr_sub(q.t, S[b]));
                    nu = mont_mul(nu, fr_sub(q.u, S[b]));
                }
                const Fr w = mont_mul(F[a], om_inv(den));
                rt[i] = fr_add(rt[i], mont_mul(w, nt_));
                ru[i] = fr_add(ru[i], mont_mul(w, nu));
            }
        }
        Fr ht[4];                                           // h1(t), its slot for t twice, h2(t)
        {
            const void* hp[2] = {h1, h2};
            evaluate(hp, 2, nullptr, 0, ht);
        }
        const Fr h1t = ht[0], h2t = ht[1];
        // identity 1
        const std::vector<Fr> wt = open_set_weights(q, q.t, false), wu = open_set_weights(q, q.u, true);
        Fr rhs1 = fr_zero(), gt = fr_zero(), cst = fr_zero();
        for (uint32_t i = 0; i < nsets; ++i) {
            rhs1 = fr_add(rhs1, mont_mul(wt[i], fr_sub(Ft[i], rt[i])));
            gt = fr_add(gt, mont_mul(wu[i], Ft[i]));
            cst = fr_add(cst, mont_mul(wu[i], ru[i]));
        }
        const Fr lhs1 = mont_mul(h1t, om_vanish(q.T, nullptr, q.t));
        // identity 2
        gt = fr_sub(gt, mont_mul(om_vanish(q.S[0], nullptr, q.u), h1t));
        const Fr lhs2 = fr_sub(gt, cst), rhs2 = mont_mul(h2t, fr_sub(q.t, q.u));
        fr_store_words(fr_from_mont(lhs1), result->lhs1);
        fr_store_words(fr_from_mont(rhs1), result->rhs1);
        fr_store_words(fr_from_mont(lhs2), result->lhs2);
        fr_store_words(fr_from_mont(rhs2), result->rhs2);
        fr_store_words(fr_from_mont(cst), result->constant);
        result->identity1_failures = !fr_eq(lhs1, rhs1);
        result->identity2_failures = !fr_eq(lhs2, rhs2);
        // the top cells
        const uint64_t top = std::min<uint64_t>(q.minpts, n);
        Fr cells[9];
        hipck(hipMemcpyAsync(cells, (const Fr*)h1 + (n - top), top * sizeof(Fr), hipMemcpyDeviceToHost, c->st), "D2H");
        hipck(hipMemcpyAsync(cells + 8, (const Fr*)h2 + (n - 1), sizeof(Fr), hipMemcpyDeviceToHost, c->st), "D2H");
        hipck(hipStreamSynchronize(c->st), "hipStreamSynchronize");
        result->h1_top_checked = top;
        for (uint64_t i = 0; i < top; ++i) result->h1_top_nonzero += !fr_is_zero(cells[i]);
        result->h2_top_checked = 1;
        result->h2_top_nonzero = !fr_is_zero(cells[8]);
    });
}
int svdw_linear_combination(svdw_ctx* c, uint32_t k, int form, const void* const* cols, uint32_t ncols,
                            const uint64_t* scalars, void* out) {
    return guarded([&] {
        const std::string f("svdw_linear_combination");
        REQUIRE(c && (scalars || !ncols), "null argument");
        check_form(form);
        for (uint32_t j = 0; j < ncols; ++j)
            REQUIRE(fr_reduced(fr_raw_words(scalars + 4 * (size_t)j)), f + ": scalar >= p");
        need_k(f, k);
        need_device(c, f);
        if (!ncols) return;
        need_columns(f, ncols);
        REQUIRE(cols && out, "null argument");
        const uint64_t n = 1ull << k;
        const uintptr_t bytes = (uintptr_t)n * sizeof(Fr), o0 = (uintptr_t)out;
        for (uint32_t j = 0; j < ncols; ++j) need_pointer(f, cols[j]);
        for (uint32_t j = 0; j < ncols; ++j)
            need_apart(f, "out", o0, o0 + bytes, "an input column", (uintptr_t)cols[j], (uintptr_t)cols[j] + bytes);
        sync(c);
        const Staged d = stage(c, cols, ncols, nullptr, 0, ncols, 0, [&](Fr* t) {
            for (uint32_t j = 0; j < ncols; ++j) t[j] = fr_to_mont(fr_raw_words(scalars + 4 * (size_t)j));
        });
        profiled(c, "k_open_fold", 32.0 * (ncols + 1) * (double)n, [&] {
            return launch_open_fold(d.ptrs, d.cells, ncols, nullptr, fr_zero(), n, (Fr*)out, c->st);
        });
    });
}
