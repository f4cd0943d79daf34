// Read-out (export.hpp): cells copied to the host or exported to device memory,
// canonical, Montgomery or dequantized, and the host Fr helpers of the C ABI.
#include <math.h>

#include "engine_internal.hpp"
#include "export.hpp"

extern "C" {

static int copy_cells(svdw_ctx* c, uint32_t phase, uint64_t off, uint64_t n, uint64_t* out, bool lk) {
    return guarded([&] {
        REQUIRE(c && phase < 2 && out, "bad argument");
        REQUIRE(!c->dry, "planning context has no cells");
        const Stream& s = c->ph[phase];
        REQUIRE(off + n <= (lk ? s.nl : s.n), "copy range outside the stream");
        if (!n) return;
        settle(c);
        hipck(hipMemcpyAsync(out, (lk ? s.lk : s.adv) + off, n * sizeof(Fr), hipMemcpyDeviceToHost,
                             c->st), "D2H");
        sync(c);
    });
}
int svdw_copy_advice(svdw_ctx* c, uint32_t phase, uint64_t off, uint64_t n, uint64_t* out) {
    return copy_cells(c, phase, off, n, out, false);
}
int svdw_copy_lookup(svdw_ctx* c, uint32_t phase, uint64_t off, uint64_t n, uint64_t* out) {
    return copy_cells(c, phase, off, n, out, true);
}

// ------------------------------------------------------------- read-out
// Cells in the form the consumer holds them (export.hpp): a stream range or a
// view, canonical or Montgomery, or dequantized to f64; into device memory
// (queued, no host wait) or host memory (staged through bounded scratch).
static constexpr size_t kExportChunk = 64ull << 20;       // bytes of cells per staging half
static hipEvent_t export_event(svdw_ctx* c, int i) {
    if (!c->exp.ev[i])
        hipck(hipEventCreateWithFlags(&c->exp.ev[i], hipEventDisableTiming), "hipEventCreate");
    return c->exp.ev[i];
}
// The cell stream behind everything queued on the context so far: a pipelined
// witness's tail (settle) and whatever a call left on the side streams.
static void export_join(svdw_ctx* c) {
    settle(c);
    flush_batch(c, c->st);
    int i = 4;
    for (hipStream_t t : {c->st2, c->st3}) {
        const hipEvent_t e = export_event(c, i++);
        if (!t || t == c->st) continue;
        flush_batch(c, t);
        hipck(hipEventRecord(e, t), "hipEventRecord");
        hipck(hipStreamWaitEvent(c->st, e, 0), "hipStreamWaitEvent");
    }
}
static ExportSrc range_src(svdw_ctx* c, uint32_t phase, int lookup, uint64_t off, uint64_t n) {
    REQUIRE(phase < 2, "phase must be 0 or 1");
    REQUIRE(!c->dry, "planning context has no cells");
    const Stream& s = c->ph[phase];
    const uint64_t len = lookup ? s.nl : s.n;
    REQUIRE(off <= len && n <= len - off, "export range outside the stream");
    return ExportSrc{lookup ? s.lk : s.adv, off, n, 0, 0, 0, 0};
}
static ExportSrc view_src(svdw_ctx* c, const svdw_mat& m) {
    REQUIRE(!c->dry, "planning context has no cells");
    check_mat(c, m);
    return ExportSrc{c->ph[m.phase].adv, m.off, (uint64_t)m.rows * m.cols, 0, m.rs, m.cs, m.cols};
}
// cells [k0, k0 + cnt) of s
static ExportSrc sub_src(const ExportSrc& s, uint64_t k0, uint64_t cnt) {
    ExportSrc r = s;
    r.n = cnt;
    if (s.cols) r.k0 = s.k0 + k0;
    else r.off = s.off + k0;
    return r;
}
// conv(sub, dev): queue the conversion of `sub` into device memory dev on st;
// esz: bytes per converted cell. Into device memory in one launch; into host
// memory in chunks through the two staging halves, chunk k + 1's conversion (st)
// beside chunk k's copy (st2), then waits.
static void export_run(svdw_ctx* c, const ExportSrc& s, size_t esz, void* dst, bool on_device,
                       const std::function<void(const ExportSrc&, void*)>& conv) {
    if (!s.n) return;
    if (on_device) {
        export_join(c);
        conv(s, dst);
        return;
    }
    const uint64_t chunk = kExportChunk / sizeof(Fr);      // cells per half
    for (int h = 0; h < (s.n > chunk ? 2 : 1); ++h)        // (allocating synchronises: first)
        ensure_buf(c, c->exp.half[h], (size_t)std::min(s.n, chunk) * esz);
    export_join(c);
    const hipStream_t cp = c->st2 && c->st2 != c->st ? c->st2 : c->st;
    uint64_t k0 = 0;
    for (uint64_t i = 0; k0 < s.n; ++i, k0 += chunk) {
        const int h = (int)(i & 1);
        const uint64_t cnt = std::min(chunk, s.n - k0);
        if (i >= 2) hipck(hipStreamWaitEvent(c->st, export_event(c, 2 + h), 0), "hipStreamWaitEvent");
        conv(sub_src(s, k0, cnt), c->exp.half[h].p);
        hipck(hipEventRecord(export_event(c, h), c->st), "hipEventRecord");
        hipck(hipStreamWaitEvent(cp, export_event(c, h), 0), "hipStreamWaitEvent");
        hipck(hipMemcpyAsync((char*)dst + k0 * esz, c->exp.half[h].p, cnt * esz, hipMemcpyDeviceToHost, cp), "D2H");
        hipck(hipEventRecord(export_event(c, 2 + h), cp), "hipEventRecord");
    }
    sync(c);
}
static void export_cells_to(svdw_ctx* c, const ExportSrc& s, int form, void* dst, bool on_device) {
    if (!on_device && form == SVDW_FORM_CANONICAL && !s.cols) {   // straight from the stream
        if (!s.n) return;
        export_join(c);
        hipck(hipMemcpyAsync(dst, s.src + s.off, s.n * sizeof(Fr), hipMemcpyDeviceToHost, c->st), "D2H");
        sync(c);
        return;
    }
    export_run(c, s, sizeof(Fr), dst, on_device, [&](const ExportSrc& sub, void* dev) {
        ProfScope ps(c, c->st, form == SVDW_FORM_MONTGOMERY ? "k_export_mont" : "k_export", 64.0 * (double)sub.n, 0);
        hipck(launch_export(sub, form, (Fr*)dev, 0, c->st), "k_export");
    });
}
static void dequantize_to(svdw_ctx* c, const ExportSrc& s, double* dst, bool on_device) {
    export_run(c, s, sizeof(double), dst, on_device, [&](const ExportSrc& sub, void* dev) {
        ProfScope ps(c, c->st, "k_dequantize", 40.0 * (double)sub.n, 0);
        hipck(launch_dequantize(sub, c->P, (double*)dev, c->st), "k_dequantize");
    });
}
int svdw_export_cells(svdw_ctx* c, uint32_t phase, int lookup, uint64_t off, uint64_t n, int form, void* dst) {
    return guarded([&] {
        REQUIRE(c && dst, "null argument");
        check_form(form);
        export_cells_to(c, range_src(c, phase, lookup, off, n), form, dst, true);
    });
}
int svdw_copy_cells(svdw_ctx* c, uint32_t phase, int lookup, uint64_t off, uint64_t n, int form, uint64_t* out) {
    return guarded([&] {
        REQUIRE(c && out, "null argument");
        check_form(form);
        export_cells_to(c, range_src(c, phase, lookup, off, n), form, out, false);
    });
}
int svdw_export_mat(svdw_ctx* c, const svdw_mat* a, int form, void* dst, int on_device) {
    return guarded([&] {
        REQUIRE(c && a && dst, "null argument");
        check_form(form);
        export_cells_to(c, view_src(c, *a), form, dst, on_device != 0);
    });
}
int svdw_export_vec(svdw_ctx* c, const svdw_vec* v, int form, void* dst, int on_device) {
    return guarded([&] {
        REQUIRE(c && v && dst, "null argument");
        check_form(form);
        export_cells_to(c, view_src(c, mat_of_vec(*v)), form, dst, on_device != 0);
    });
}
int svdw_dequantize_mat(svdw_ctx* c, const svdw_mat* a, double* out, int on_device) {
    return guarded([&] {
        REQUIRE(c && a && out, "null argument");
        dequantize_to(c, view_src(c, *a), out, on_device != 0);
    });
}
int svdw_dequantize_vec(svdw_ctx* c, const svdw_vec* v, double* out, int on_device) {
    return guarded([&] {
        REQUIRE(c && v && out, "null argument");
        dequantize_to(c, view_src(c, mat_of_vec(*v)), out, on_device != 0);
    });
}
// Host helpers (fr.hpp / export.hpp on the host, no context, no GPU).
int svdw_fr_convert(const uint64_t* in, uint64_t n, int from, int to, uint64_t* out) {
    return guarded([&] {
        REQUIRE(n == 0 || (in && out), "null argument");
        check_form(from);
        check_form(to);
        for (uint64_t i = 0; i < n; ++i)
            REQUIRE(fr_reduced(fr_raw_words(in + 4 * i)), "svdw_fr_convert: input value >= p");
        for (uint64_t i = 0; i < n; ++i) {
            Fr x = fr_raw_words(in + 4 * i);
            if (from != to) x = to == SVDW_FORM_MONTGOMERY ? fr_to_mont(x) : fr_from_mont(x);
            fr_store_words(x, out + 4 * i);
        }
    });
}
int svdw_quantization(double x, uint32_t precision_bits, uint64_t out[4]) {
    return guarded([&] {
        REQUIRE(out, "null argument");
        if (precision_bits < 1 || precision_bits > 63) fail(SVDW_ERANGE, "precision_bits must be in [1, 63]");
        fr_store_words(quantize_fr(x, ldexp(1.0, (int)precision_bits)), out);
    });
}
int svdw_dequantization(const uint64_t value[4], uint32_t precision_bits, double* out) {
    return guarded([&] {
        REQUIRE(value && out, "null argument");
        if (precision_bits < 1 || precision_bits > 63) fail(SVDW_ERANGE, "precision_bits must be in [1, 63]");
        const Fr x = fr_raw_words(value);
        REQUIRE(fr_reduced(x), "svdw_dequantization: value >= p");
        *out = dequantize_fr(x, precision_bits);
    });
}

}  // extern "C"
