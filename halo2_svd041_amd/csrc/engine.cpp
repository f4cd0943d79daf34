// The witness engine of the SVD-verify library and its C ABI entries
// (include/svdw.h): cell-stream memory, views, stage launches and batches, the
// checker's notes, the reference functions and their entries. The program
// builder is in program_builder.hpp (this file alone includes it), the two
// witness calls and the captured graph in witness.cpp. The context's
// lifetime, lanes, options, stream hand-off, marks and profiling are in
// context.cpp, read-out in export.cpp, text ingest in ingest.cpp, the exact
// product in gemm.cpp, the calls on a finished witness (checker, physical
// layout, equality records, edge list) in circuit.cpp, the prover calls (lookup
// argument, grand products, transforms, commitments, quotient, opening) in
// prover.cpp; engine_internal.hpp holds what the files share, the definition of
// svdw_ctx included.
//
// Each reference function (src/matrix/mod.rs, src/svd/mod.rs) becomes:
//   1. a data-independent cell program built on the host by replaying the
//      halo2-base gadget sequence symbolically (PB below), and
//   2. one launch of the generic stage kernel over the elements, or the
//      dedicated GEMM / inner-product-row kernels.
// Offsets in the per-phase streams are known at enqueue time, so all work is
// asynchronous on the context's HIP stream. A context created with
// device = -1 is a "dry" planner: identical control flow, no device work,
// which is how svdw_plan_svd gets exact closed-form counts.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "engine_internal.hpp"

#include "program_builder.hpp"

Fr fr_from_words(const uint64_t w[4]) { return big_to_fr(big_from_words(w)); }


// ---------------------- stream dependencies, bit bounds, cell-stream memory
// debug logs (read once: getenv scans the environment)
static bool env_flag(const char* name) { const char* v = getenv(name); return v && *v && *v != '0'; }
static const bool g_batch_log = env_flag("SVDW_BATCH_LOG");
static const bool g_stage_log = env_flag("SVDW_STAGE_LOG");
// Dependency recorded on `from`; `to` waits for it (cross-stream dependency).
// The returned handle is waited on later with dep_wait. (Round 4 measured the
// alternative of stream values, hipStreamWriteValue32 / hipStreamWaitValue32,
// once its flag initialisation was ordered: the suite passed, but 512^2 went
// 0.417 -> 0.444 ms and 1024^2 2.078 -> 2.100 ms, 8-way ranks unchanged --
// HIP runs those waits and writes as kernels of their own -- so it was removed.)
hipEvent_t stream_dep(svdw_ctx* c, hipStream_t from, hipStream_t to) {
    if (c->vmg.linear) {                                   // one stream: order is implicit
        flush_batch(c, from);
        return c->lin_ev;
    }
    if (c->dep_next == c->deps.size()) {
        hipEvent_t e;
        // same-device consumer only: agent-scope release, no system-scope writeback
        hipck(hipEventCreateWithFlags(&e, hipEventDisableTiming | hipEventReleaseToDevice),
              "hipEventCreate");
        c->deps.push_back(e);
    }
    hipEvent_t e = c->deps[c->dep_next++];
    flush_batch(c, from);
    if (g_batch_log) fprintf(stderr, "dep %p -> %p\n", (void*)from, (void*)to);
    hipck(hipEventRecord(e, from), "hipEventRecord");
    if (to) hipck(hipStreamWaitEvent(to, e, 0), "hipStreamWaitEvent");
    return e;
}
// `s` waits for a dependency stream_dep returned (or any other event)
void dep_wait(svdw_ctx* c, hipStream_t s, hipEvent_t e) {
    if (c->vmg.linear && e == c->lin_ev) return;
    hipck(hipStreamWaitEvent(s, e, 0), "hipStreamWaitEvent");
}
// (Round 4 removed "gemm_priority", a high-priority second stream at 512 <=
// max(N, M) < 1024: +2 % in round 2's tools/ab.py runs, but bench.py at 512^2
// P=32 measured 0.68 ms with it and 0.41 ms without -- the stream created
// mid-run shares a hardware queue with the cell stream, GPU_MAX_HW_QUEUES = 4.)
static bool same_cells(const svdw_mat& a, const svdw_mat& b) {
    if (a.phase != b.phase || a.off != b.off) return false;
    return (a.rows == b.rows && a.cols == b.cols && a.rs == b.rs && a.cs == b.cs) ||
           (a.rows == b.cols && a.cols == b.rows && a.rs == b.cs && a.cs == b.rs);
}
static void reg_bits(svdw_ctx* c, const svdw_mat& m, uint32_t bits) {
    if (bits == ~0u) return;
    for (auto& r : c->wit.mbits)
        if (same_cells(r.m, m)) { r.bits = bits; return; }
    c->wit.mbits.push_back({m, bits});
}
static uint32_t bits_of(const svdw_ctx* c, const svdw_mat& m) {
    for (auto& r : c->wit.mbits)
        if (same_cells(r.m, m)) return r.bits;
    for (auto& p : c->wit.prods)
        if (same_cells(p.cs, m)) {
            const uint32_t ba = bits_of(c, p.a), bb = bits_of(c, p.b);
            if (ba != ~0u && bb != ~0u) return ba + bb + p.lk;
        }
    return ~0u;
}
static void fetch_bits(svdw_ctx* c) {
    if (!c->bits_pending) return;
    hipck(hipEventSynchronize(c->ev_bits), "hipEventSynchronize");
    // the words are final once the event has fired: read them now (no copy is
    // queued on st per witness, the device-side consumers read the words directly)
    hipck(hipMemcpy(c->hbits, c->wit.dbitw, 3 * sizeof(uint32_t), hipMemcpyDeviceToHost), "D2H");
    c->bits_pending = false;
    for (int i = 0; i < 3; ++i) {
        c->qbits[i] = c->hbits[i];
        reg_bits(c, c->qmat[i], c->qbits[i]);
    }
}
void host_mark(svdw_ctx* c, const char* what) {
    if (!c->opt.host_trace || c->dry) return;
    const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - c->ht0).count();
    fprintf(stderr, "[svdw host] %9.1f us  %s\n", us, what);
}
static void own(svdw_ctx* c, uint32_t phase, bool lookup, uint64_t off, uint64_t n) {
    if (sharded(c) && n) c->owned.push_back({phase, lookup ? 1u : 0u, off, n});
}
// Write rate of the stage kernel's store pattern over `cells` cells at buf: a
// stage of 61 constant cells per element (no loads, no micro-ops), one warm and
// one timed launch on the cell stream.
static double stage_store_rate(svdw_ctx* c, Fr* buf, uint64_t cells) {
    StageArgs a;
    memset(&a, 0, sizeof a);
    const uint32_t C = 61;
    const uint64_t ne = std::min<uint64_t>(cells / C, 1ull << 26);
    if (ne < 1024) return 0.0;
    a.out_adv = buf;
    a.e_begin = 0;
    a.e_end = (uint32_t)ne;
    a.cols = 1;
    a.C = C;
    a.nv = 1;
    a.nk = 1;
    a.flags = c->opt.stage_flags;
    a.cdiv_magic = (uint32_t)(((1ull << 32) + C - 1) / C);
    for (uint32_t k = 0; k < C; ++k) a.adv[k] = SlotOp{(uint8_t)KSRC, (uint8_t)(8 * (k % 8)), 0, 0};
    a.K[0] = fr_from_u64(0x9e3779b97f4a7c15ull);
    hipEvent_t e0, e1;
    hipck(hipEventCreate(&e0), "hipEventCreate");
    hipck(hipEventCreate(&e1), "hipEventCreate");
    hipck(launch_stage(a, c->st), "k_stage (placement probe)");
    hipck(hipEventRecord(e0, c->st), "hipEventRecord");
    hipck(launch_stage(a, c->st), "k_stage (placement probe)");
    hipck(hipEventRecord(e1, c->st), "hipEventRecord");
    hipck(hipEventSynchronize(e1), "hipEventSynchronize");
    float ms = 0;
    hipck(hipEventElapsedTime(&ms, e0, e1), "hipEventElapsedTime");
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return ms > 0 ? 32.0 * C * ne / (ms * 1e-3) : 0.0;
}
// A new cell stream of >= 256 MiB with "place_trials" k > 1 (default 6): k
// buffers are allocated side by side (so they lie in different places of HBM),
// the stage store pattern is timed on each, and the fastest is kept. The same
// witness runs 1.73-2.03 ms per step depending on where its streams lie, and a
// fresh process's first placement is a slow one (fresh
// bench.py processes at 1024^2, one box: 2.010-2.014 ms without trials,
// 1.848-1.861 with 3, 1.721-1.767 with 6, tools/r6/r6pt3.sh).
// The trials need k times the stream in free memory (fewer when it is short:
// none at 4096^2) and a few ms once per allocation.
static Fr* place_cells(svdw_ctx* c, uint64_t cells) {
    const uint64_t bytes = cells * sizeof(Fr);
    int k = c->opt.place_trials;
    if (k > 1 && bytes >= (256ull << 20)) {
        size_t fr = 0, tot = 0;
        if (hipMemGetInfo(&fr, &tot) != hipSuccess) fr = 0;
        while (k > 1 && (double)k * bytes > 0.5 * (double)fr) --k;
    }
    Fr* best = nullptr;
    if (k <= 1 || bytes < (256ull << 20)) {
        if (hipMalloc((void**)&best, bytes) != hipSuccess) return nullptr;
        return best;
    }
    sync(c);
    std::vector<Fr*> cand;
    double br = -1.0;
    for (int i = 0; i < k; ++i) {
        Fr* p = nullptr;
        if (hipMalloc((void**)&p, bytes) != hipSuccess) break;
        cand.push_back(p);
        const double r = stage_store_rate(c, p, cells);
        if (c->opt.host_trace) fprintf(stderr, "place_cells: %.2f GB candidate %d at %p: %.3f TB/s\n", bytes / 1e9, i,
                                   (void*)p, r / 1e12);
        if (r > br) {
            br = r;
            best = p;
        }
    }
    for (Fr* p : cand)
        if (p != best) hipck(hipFree(p), "hipFree");
    return best;
}
void grow(svdw_ctx* c, Fr*& ptr, uint64_t used, uint64_t& cap, uint64_t need) {
    if (c->dry || need <= cap) return;
    REQUIRE(!c->vmg.capturing, "internal: allocation during graph capture");
    ++c->epoch;
    uint64_t ncap = std::max(need, cap + cap / 2);
    Fr* np = ptr ? nullptr : place_cells(c, ncap);
    if (!np && hipMalloc((void**)&np, ncap * sizeof(Fr)) != hipSuccess)
        fail(SVDW_ENOMEM, "device allocation failed (cell stream of " + std::to_string(ncap) + " cells)");
    if (ptr) {
        hipck(hipMemcpyAsync(np, ptr, used * sizeof(Fr), hipMemcpyDeviceToDevice, c->st), "copy");
        sync(c);
        hipck(hipFree(ptr), "hipFree");
    }
    ptr = np;
    cap = ncap;
}
// Append n advice and nl lookup cells to a phase; returns their offsets.
// Every cell region of a witness is appended here, in the reference's order;
// the layout table (svdw_layout) records what each region is: the gadget /
// function that appends it and its rows (row-parallel regions hold `rows`
// equal runs of cells).
void append(svdw_ctx* c, uint32_t phase, uint64_t n, uint64_t nl, uint64_t* off, uint64_t* loff, const char* tag,
            uint64_t rows) {
    REQUIRE(phase < 2, "phase must be 0 or 1");
    settle(c);
    Stream& s = c->ph[phase];
    c->phys.valid = false;
    grow(c, s.adv, s.n, s.cap, s.n + n);
    grow(c, s.lk, s.nl, s.lcap, s.nl + nl);
    *off = s.n;
    if (loff) *loff = s.nl;
    svdw_region r;
    memset(&r, 0, sizeof r);
    r.phase = phase;
    r.off = s.n;
    r.n = n;
    r.loff = s.nl;
    r.nl = nl;
    r.rows = rows ? rows : 1;
    snprintf(r.tag, sizeof r.tag, "%s", tag);
    c->wit.layout.push_back(r);
    c->wit.layout_chk.emplace_back();
    s.n += n;
    s.nl += nl;
}

// Device pointers into the cell streams (views) are taken while a gadget is
// being built; a stream reallocation in between would leave them pointing at
// the freed buffer. Every ABI entry point that appends after taking a view
// therefore runs through here: the streams are sized first from a dry replay of
// fn (layouts are data independent), so nothing reallocates inside the call;
// then fn runs on the context, and its result is returned.
template <class F>
static auto run_sized(svdw_ctx* c, F&& fn) {
    if (!c->dry) {
        PlanCtx plan(c->P, c->LB, c);
        fn(&plan);
        for (int p = 0; p < 2; ++p) {
            grow(c, c->ph[p].adv, c->ph[p].n, c->ph[p].cap, plan.ph[p].n);
            grow(c, c->ph[p].lk, c->ph[p].nl, c->ph[p].lcap, plan.ph[p].nl);
        }
    }
    return fn(c);
}

// --------------------------------------------------------------- views
// A dry context has no streams: its views carry a placeholder pointer that
// view_source decodes to (phase, offset) (never dereferenced: nothing launches).
static constexpr uintptr_t kDryBase = (uintptr_t)1 << 44;
static const Fr* dry_ptr(uint32_t phase, uint64_t off) {
    return reinterpret_cast<const Fr*>(kDryBase * (phase + 1) + off * sizeof(Fr));
}
// rows x cols values at ptr with strides rs, cs, as a strided view
static DView ptr_view(const Fr* ptr, uint32_t rows, uint32_t cols, int64_t rs, int64_t cs) {
    DView v;
    memset(&v, 0, sizeof v);
    v.ptr = ptr;
    v.rs = rs;
    v.cs = cs;
    v.rows = rows;
    v.cols = cols;
    v.mode = VIEW_STRIDED;
    return v;
}
DView view_of(svdw_ctx* c, const svdw_mat& m) {
    return ptr_view(c->dry ? dry_ptr(m.phase, m.off) : cellp(c, m.phase, m.off), m.rows, m.cols, m.rs, m.cs);
}
// The lowest and highest cell of a strided view, counted from its cell 0 (signed strides, in cells).
struct Span { int64_t lo, hi; };
static Span view_span(const DView& v) {
    const int64_t dr = (int64_t)(v.rows ? v.rows - 1 : 0) * v.rs, dc = (int64_t)(v.cols ? v.cols - 1 : 0) * v.cs;
    return {std::min<int64_t>(dr, 0) + std::min<int64_t>(dc, 0), std::max<int64_t>(dr, 0) + std::max<int64_t>(dc, 0)};
}
// A launch's view of loaded cells whose f64 source is registered for this call
// (f64reg): the same elements read from the f64 input and quantized in the
// kernel (VIEW_F64), so the launch does not wait for k_quantize_multi. The
// checker's copies of the views (note_gates) stay cell views.
static DView f64_view(const svdw_ctx* c, const DView& v) {
    if (!c->opt.f64_views || c->call.f64reg.empty() || v.mode != VIEW_STRIDED || !v.ptr || !v.rows || !v.cols) return v;
    const Span sp = view_span(v);
    for (const auto& r : c->call.f64reg) {
        const Fr* base = c->ph[r.phase].adv + r.off;
        const int64_t o = v.ptr - base;
        if (o + sp.lo < 0 || o + sp.hi >= (int64_t)r.n) continue;
        DView f = v;
        f.ptr = reinterpret_cast<const Fr*>(r.x + o);
        f.mode = VIEW_F64;
        f._r0 = (uint8_t)c->P;
        return f;
    }
    return v;
}

// ------------------------------------------------------- stage launches
// A stage of nelem elements in rows of `cols` (0: 1): its R rows, and those of this rank.
struct StageRows { uint64_t cw, R, r0, r1; };
static StageRows stage_rows(const svdw_ctx* c, uint32_t nelem, uint32_t cols) {
    StageRows s{cols ? cols : 1u, 0, 0, 0};
    s.R = nelem / s.cw;
    shard_rows(c, s.R, &s.r0, &s.r1);
    return s;
}
// Appends the stage's cells for `nelem` elements; returns the advice offset.
// Launch a stage whose cells were appended at (off, loff) earlier.
static void stage_launch(svdw_ctx* c, uint32_t phase, PB& pb, uint32_t nelem, uint32_t cols,
                         uint64_t off, uint64_t loff, const char* tag) {
    StageArgs a = pb.a;
    uint32_t eb = 0, ee = nelem;
    const StageRows sr = stage_rows(c, nelem, cols);
    if (sharded(c) && sr.R > 1) {                         // single cells: every rank
        eb = (uint32_t)(sr.r0 * sr.cw);
        ee = (uint32_t)(sr.r1 * sr.cw);
    }
    if (g_stage_log) {
        uint32_t nmul = 0;
        for (uint32_t i = 0; i < a.nmo; ++i) nmul += a.mo[i].op == MO_MUL;
        const int sid = c->st == c->st_cell ? 1 : c->st == c->st2 ? 2 : c->st == c->st3 ? 3 : 0;
        fprintf(stderr, "stage %-28s elems %8u C %3u L %3u nv %2u nmo %2u muls %u nk %u  s%d\n", tag, ee - eb,
                a.C, a.L, a.nv, a.nmo, nmul, a.nk, sid);
        if (getenv("SVDW_STAGE_LOG")[0] == '2') {        // the slot ops too: (src lo nbits) per cell
            fprintf(stderr, "  slots");
            for (uint32_t k = 0; k < a.C + a.L; ++k) {
                const SlotOp& o = k < a.C ? a.adv[k] : a.lk[k - a.C];
                fprintf(stderr, " %u:%u:%u", o.src, o.lo, o.nbits);
            }
            fprintf(stderr, "\n");
        }
    }
    if (c->dry || ee <= eb) return;
    a.out_adv = cellp(c, phase, off);
    a.out_lk = a.L ? c->ph[phase].lk + loff : nullptr;
    for (int k = 0; k < kMaxViews; ++k) a.view[k] = f64_view(c, a.view[k]);
    a.e_begin = eb;
    a.e_end = ee;
    a.cols = cols ? cols : 1;
    a.flags = c->opt.stage_flags;
    // small blocks overlap better with concurrent work, but a stage with field
    // multiplications / inversions keeps one element per thread of a full block
    bool heavy = false;
    for (uint32_t i = 0; i < a.nmo; ++i)
        heavy |= a.mo[i].op == MO_MUL || a.mo[i].op == MO_ISZERO || a.mo[i].op == MO_POWK;
    a.E = heavy ? kStageElems : c->opt.stage_elems;
    // keep the block's LDS (element values) within 64 KiB: fewer elements per
    // block for stages with many values (signed_div_scale)
    while (a.E > 64 && stage_lds_bytes(a.nv ? a.nv : 1, a.E, a.C + a.L) > 65536) a.E -= 64;
    // 32-bit magics for fastdiv (divisor 1 is handled in the kernel)
    auto magic = [](uint64_t d) -> uint32_t { return d > 1 ? (uint32_t)(((1ull << 32) + d - 1) / d) : 0; };
    a.cdiv_magic = magic(a.C);
    a.ldiv_magic = magic(a.L);
    uint32_t loads = 0;
    for (uint32_t i = 0; i < a.nmo; ++i) loads += a.mo[i].op == MO_LOAD;
    const double bytes = 32.0 * (ee - eb) * ((double)a.C + a.L + loads);
    for (auto& b : c->batches) {
        if (b.st != c->st || !stage_multi_fits(a)) continue;
        // does this stage read cells that pending stage q writes?
        auto reads = [&](const svdw_ctx::Pending& q) {
            const char* w0 = reinterpret_cast<const char*>(q.a.out_adv);
            const char* w1 = w0 + sizeof(Fr) * (uint64_t)q.a.e_end * q.a.C;
            for (int k = 0; k < kMaxViews; ++k) {
                const DView& v = a.view[k];
                if (!v.ptr || v.mode == VIEW_DIAGK) continue;
                const Span sp = view_span(v);
                const char* p = reinterpret_cast<const char*>(v.ptr);
                if (p + sp.lo * (int64_t)sizeof(Fr) < w1 && p + (sp.hi + 1) * (int64_t)sizeof(Fr) > w0) return true;
            }
            return false;
        };
        size_t g = 0;                                     // after the last group it depends on
        for (size_t k = 0; k < b.groups.size(); ++k)
            for (const auto& q : b.groups[k])
                if (reads(q)) g = k + 1;
        if (c->call.stage_front && g == 0)                     // a launch of its own, ahead of the batch
            b.groups.insert(b.groups.begin(), std::vector<svdw_ctx::Pending>{});
        else if (g == b.groups.size())
            b.groups.emplace_back();
        b.groups[g].push_back({a, std::string("k_stage:") + tag, bytes});
        b.last = g;
        return;
    }
    {
        ProfScope ps(c, c->st, std::string("k_stage:") + tag, bytes, 0, false, true);
        const StageArgs* one = &a;
        hipck(launch_stage_multi(&one, 1, c->st), "k_stage");
    }
}
// Issue a stream's pending batched stages (k_stage_multi; one program: k_stage).
// waiter: after the group holding the latest stage, `waiter` waits for s there
// (it needs that stage and what came before on s, not the later groups: those
// hold stages queued earlier that depend on other pending ones).
// then_wait: s waits for this event before the groups after that point.
void flush_batch(svdw_ctx* c, hipStream_t s, hipStream_t waiter, hipEvent_t then_wait) {
    for (auto& b : c->batches) {
        if (b.st != s || b.groups.empty()) continue;
        std::vector<std::vector<svdw_ctx::Pending>> groups;
        groups.swap(b.groups);               // (cleared before launching: no re-entry)
        const size_t upto = b.last;
        for (size_t gi = 0; gi < groups.size(); ++gi) {
            const auto& grp = groups[gi];
            if (gi == upto + 1 && waiter) {
                stream_dep(c, s, waiter);
                waiter = nullptr;
                if (then_wait) dep_wait(c, s, then_wait);
            }
            if (grp.empty()) continue;
            std::vector<const StageArgs*> ps;
            double bytes = 0;
            for (const auto& q : grp) {
                ps.push_back(&q.a);
                bytes += q.bytes;
            }
            const std::string name = grp.size() == 1 ? grp[0].name : "k_stage:multi";
            if (g_batch_log) {
                fprintf(stderr, "batch stream %p group %zu/%zu (last %zu):", (void*)s, gi, groups.size(), upto);
                for (const auto& q : grp) fprintf(stderr, " %s", q.name.c_str());
                fprintf(stderr, "\n");
            }
            ProfScope pr(c, s, name, bytes, 0, true, true);
            hipck(launch_stage_multi(ps.data(), (int)ps.size(), s), "k_stage_multi");
        }
    }
    if (waiter) stream_dep(c, s, waiter);
}
// RAII: stage launches on the current stream between construction and end()
// are batched (k_stage_multi); nested scopes on the same stream join the outer
// one. Without end() (an exception) the pending stages are dropped.
struct BatchScope {
    svdw_ctx* c;
    hipStream_t st = nullptr;
    bool mine = false;
    explicit BatchScope(svdw_ctx* cc, hipStream_t on = nullptr) : c(cc) {
        if (c->dry || !c->opt.stage_batch) return;
        if (!on) on = c->st;
        for (auto& b : c->batches)
            if (b.st == on) return;
        st = on;
        c->batches.push_back({st, {}});
        mine = true;
    }
    void end() {
        if (!mine) return;
        flush_batch(c, st);
        close();
    }
    void close() {
        for (size_t i = 0; i < c->batches.size(); ++i)
            if (c->batches[i].st == st) { c->batches.erase(c->batches.begin() + i); break; }
        mine = false;
    }
    ~BatchScope() { if (mine) close(); }
};
// shard ownership of a stage's cells: this rank's rows (single cells: the last rank)
static void stage_own(svdw_ctx* c, uint32_t phase, const PB& pb, uint32_t nelem, uint32_t cols,
                      uint64_t off, uint64_t loff) {
    const StageRows s = stage_rows(c, nelem, cols);
    own(c, phase, false, off + s.r0 * s.cw * pb.a.C, (s.r1 - s.r0) * s.cw * pb.a.C);
    own(c, phase, true, loff + s.r0 * s.cw * pb.a.L, (s.r1 - s.r0) * s.cw * pb.a.L);
}
static void note_const(svdw_ctx* c, const Fr& v) {
    std::array<uint32_t, 8> w;
    for (int i = 0; i < 8; ++i) w[i] = v.w[i];
    c->wit.consts.insert(w);
}
// the last appended region is `nelem` copies of pb's program: record its gates
// (views: the source cells as (phase, offset), strided views into the cell
// streams only -- the streams may move before the check)
// (phase, offset) of a view's cell 0 in the cell streams (dry placeholders too)
static bool view_source(const svdw_ctx* c, const Fr* ptr, uint32_t* phase, uint64_t* off) {
    if (!ptr) return false;
    if (c->dry) {
        const uintptr_t x = reinterpret_cast<uintptr_t>(ptr);
        if (x < kDryBase || x >= 3 * kDryBase) return false;
        *phase = (uint32_t)(x / kDryBase - 1);
        *off = (x % kDryBase) / sizeof(Fr);
        return true;
    }
    for (uint32_t p = 0; p < 2; ++p) {
        const Fr* base = c->ph[p].adv;
        if (base && ptr >= base && ptr < base + c->ph[p].n) {
            *phase = p;
            *off = (uint64_t)(ptr - base);
            return true;
        }
    }
    return false;
}
// equality source of a matrix / a vector chain (RegionChecks::EqSrc)
static RegionChecks::EqSrc eqsrc_mat(const svdw_mat& m) {
    RegionChecks::EqSrc e;
    e.kind = EQS_MAT;
    e.phase = m.phase; e.off = m.off; e.rs = m.rs; e.cs = m.cs; e.rows = m.rows; e.cols = m.cols;
    return e;
}
static RegionChecks::EqSrc eqsrc_chain(uint32_t first_phase, uint64_t first, uint32_t phase,
                                       uint64_t base, int64_t stride) {
    RegionChecks::EqSrc e;
    e.kind = EQS_CHAIN;
    e.first_phase = first_phase; e.first = first; e.phase = phase; e.off = base; e.rs = stride;
    return e;
}
static RegionChecks::EqSrc eqsrc_vec(const svdw_vec& v) {   // cells v.off + t v.stride
    return eqsrc_chain(v.phase, v.off, v.phase, v.off + v.stride, v.stride);
}
static void note_gates(svdw_ctx* c, const PB& pb, uint32_t cols = 1, size_t reg = ~size_t(0)) {
    RegionChecks& r = reg == ~size_t(0) ? c->wit.layout_chk.back() : c->wit.layout_chk.at(reg);
    r.eq = pb.eq;
    r.eqk.assign(pb.a.K, pb.a.K + pb.a.nk);
    // the loaded values' source cells: for the equality records (dry placeholders
    // too), and for the checker (device contexts only: it reads the cells)
    for (int k = 0; k < kMaxViews; ++k) {
        const DView& v = pb.a.view[k];
        uint32_t ph;
        uint64_t off;
        r.src[k].phase = -1;
        if (v.mode != VIEW_STRIDED || !view_source(c, v.ptr, &ph, &off)) continue;
        r.esrc[k] = eqsrc_mat(svdw_mat{ph, v.rows, v.cols, off, v.rs, v.cs});
        if (!c->dry) r.src[k] = RegionChecks::Src{(int)ph, off, v.rs, v.cs, v.rows, v.cols};
    }
    if (pb.kconst)
        for (uint32_t q = 0; q < pb.a.C; ++q)
            if (pb.a.adv[q].src >= KSRC && pb.a.adv[q].src - KSRC != pb.kext)
                note_const(c, pb.a.K[pb.a.adv[q].src - KSRC]);
    r.words = pb.chk;
    r.unit = pb.a.C;
    r.cols = cols ? cols : 1;
    // a view word whose source is not in the streams (host-known constants,
    // the gamma powers buffer) is dropped
    std::vector<uint32_t> keep;
    for (uint32_t w : r.words)
        if (chk_kind(w) != CHK_VIEW || r.src[chk_a(w)].phase >= 0) keep.push_back(w);
    r.words.swap(keep);
}
static uint64_t run_stage(svdw_ctx* c, uint32_t phase, PB& pb, uint32_t nelem, uint32_t cols,
                          const char* tag, uint64_t* loff_out = nullptr) {
    uint64_t off = 0, loff = 0;
    append(c, phase, (uint64_t)nelem * pb.a.C, (uint64_t)nelem * pb.a.L, &off, &loff, tag,
           cols ? nelem / cols : nelem);
    note_gates(c, pb, cols);
    stage_own(c, phase, pb, nelem, cols, off, loff);
    if (loff_out) *loff_out = loff;
    stage_launch(c, phase, pb, nelem, cols, off, loff, tag);
    return off;
}
svdw_vec put_cell(svdw_ctx* c, uint32_t phase, const Fr& v, bool constant) {
    PB pb(c->LB);                                          // load_witness / load_constant
    pb.kconst = constant;
    pb.cell(pb.K(v));
    // Inside svd_witness (products queued ahead), a one-cell launch on the cell
    // stream would wait for a free CU behind the scans on st2 (15-35 us on the
    // critical path); it depends on nothing, so it goes on st2 itself (never
    // back onto the cell stream: with st and st2 exchanged, as for a pipelined
    // witness's diff and ids, it stays where it is).
    const bool aside = c->call.prelaunched && !c->dry && c->st2 != c->st_cell;
    OnStream on(c, aside ? &c->st2 : nullptr);
    const uint64_t off = run_stage(c, phase, pb, 1, 1, "load_cell");
    return svdw_vec{phase, 1, off, 1};
}

// ----------------------------------------------------- reference functions
// qs: collect the quantization into one k_quantize_multi launch (device inputs
// only) instead of launching it here.
// own_rows_only (row-sharded svd_witness, m): quantize only this rank's rows,
// the only rows of the matrix any of its stages read.
// own_rows_cols (row-sharded svd_witness, square u and v, b.g from the f64
// inputs): store only this rank's rows and its column block, the cells its
// stages (bounds, u.d, the a and b = X^T scans) read; the bit-length maxima
// still cover the whole matrix (the GEMM's B operand).
svdw_mat zkmatrix_new(svdw_ctx* c, uint32_t phase, const double* data, uint32_t rows, uint32_t cols, bool on_device,
                      unsigned* blockmax, QuantSegs* qs, bool own_rows_only, bool own_rows_cols) {
    REQUIRE(rows >= 1 && cols >= 1, "ZkMatrix::new: empty matrix");
    REQUIRE(data || c->dry, "null data");
    uint64_t n = (uint64_t)rows * cols, off;
    append(c, phase, n, 0, &off, nullptr, "load", rows);
    uint64_t q0 = 0, r0, r1;                              // first quantized value; this rank's rows
    shard_rows(c, rows, &r0, &r1);
    if (own_rows_only && sharded(c) && on_device && qs) {
        q0 = r0 * cols;
        n = (r1 - r0) * cols;
    }
    if (!c->dry && n) {
        const double* src = data + q0;
        if (!on_device) {
            ensure_buf(c, c->f64in, n * sizeof(double));
            hipck(hipMemcpyAsync(c->f64in.p, data, n * sizeof(double), hipMemcpyHostToDevice, c->st),
                  "H2D");
            src = (const double*)c->f64in.p;
        }
        if (qs && on_device && qs->nseg < (uint32_t)kMaxQuantSegs) {
            const uint32_t k = qs->nseg++;
            qs->in[k] = src;
            qs->out[k] = cellp(c, phase, off + q0);
            qs->blockmax[k] = blockmax;
            qs->n[k] = n;
            qs->keep[k] = QuantKeep{0, 0, 0, 0, 0};
            if (own_rows_cols && sharded(c) && rows == cols)
                qs->keep[k] = QuantKeep{cols, (uint32_t)r0, (uint32_t)r1, (uint32_t)r0, (uint32_t)r1};
            const uint32_t pb = qs->per_block ? qs->per_block : kQuantPerBlock;
            qs->blk0[k + 1] = qs->blk0[k] + (uint32_t)((n + pb - 1) / pb);
        } else {
            ProfScope ps(c, c->st, "k_quantize", 40.0 * n, 0);
            hipck(launch_quantize(src, n, cellp(c, phase, off), (int)c->P, blockmax, c->st),
                  "k_quantize");
        }
    }
    // (every rank quantizes all of it: operands of the products)
    own(c, phase, false, off + r0 * cols, (r1 - r0) * cols);
    return svdw_mat{phase, rows, cols, off, (int64_t)cols, 1};
}

// ZkVector::entries_less_than
static void entries_less_than(svdw_ctx* c, const svdw_vec& d, uint32_t bits) {
    PB pb(c->LB);
    pb.a.view[0] = view_of(c, mat_of_vec(d));
    pb.range_check(pb.load(0), bits);
    run_stage(c, d.phase, pb, d.len, 1, "entries_less_than");
}
// ZkVector::entries_in_desc_order: all qsub(d_i, d_{i+1}) first, then range checks.
static void entries_in_desc_order(svdw_ctx* c, const svdw_vec& d, uint32_t bits) {
    REQUIRE(d.len >= 1, "entries_in_desc_order: empty vector");   // reference: 0..len-1 underflow
    if (d.len == 1) return;
    uint32_t n = d.len - 1;
    PB sb(c->LB);
    svdw_vec d1 = d;
    d1.off = d.off + d.stride;
    d1.len = n;
    svdw_vec d0 = d;
    d0.len = n;
    sb.a.view[0] = view_of(c, mat_of_vec(d0));
    sb.a.view[1] = view_of(c, mat_of_vec(d1));
    uint8_t x = sb.load(0), y = sb.load(1);
    sb.g_sub(x, y);
    uint64_t soff = run_stage(c, d.phase, sb, n, 1, "desc_order_sub");
    PB rb(c->LB);
    rb.a.view[0] = view_of(c, mat_of_vec(svdw_vec{d.phase, n, soff, 4}));
    rb.range_check(rb.load(0), bits);
    run_stage(c, d.phase, rb, n, 1, "desc_order_range");
}
static void check_mat_entries_bounded(svdw_ctx* c, const svdw_mat& a, const BigU& bnd) {
    PB pb(c->LB);
    pb.a.view[0] = view_of(c, a);
    pb.check_abs_less_than(pb.load(0), bnd);
    run_stage(c, a.phase, pb, a.rows * a.cols, a.cols, "check_mat_entries_bounded");
}
// check_mat_diff on arbitrary views (a may be zero-padded, b may be diagonal).
// a cell of the streams, for equality sources (phase -1: none)
struct EqCell {
    int phase = -1;
    uint64_t off = 0;
};
static void check_mat_diff_views(svdw_ctx* c, uint32_t phase, const DView& a, const DView& b,
                                 uint32_t rows, uint32_t cols, const BigU& tol,
                                 const Fr* diag_val = nullptr, EqCell pad_a = {},
                                 EqCell pad_b = {}, EqCell diag_b = {}) {
    PB pb(c->LB);
    pb.a.view[0] = a;
    pb.a.view[1] = b;
    uint8_t x = pb.load(0), y = pb.load(1);
    uint8_t dlt = pb.g_sub(x, y);
    pb.check_abs_less_than(dlt, tol);
    // pad / diag constants referenced by the views
    pb.a.view[0].pad_k = pb.kidx(fr_zero());
    pb.a.view[1].pad_k = pb.kidx(fr_zero());
    if (diag_val) pb.a.view[1].diag_k = pb.kidx(*diag_val);
    run_stage(c, phase, pb, rows * cols, cols, "check_mat_diff");
    // equality sources of the padded / diagonal entries: the zero padding
    // constant (check_svd_phase0), check_mat_id's zero and scalar_id cells
    RegionChecks& r = c->wit.layout_chk.back();
    if (pad_a.phase >= 0) { r.esrc[0].pad_phase = pad_a.phase; r.esrc[0].pad_off = pad_a.off; }
    if (b.mode != VIEW_STRIDED) {
        r.esrc[1] = RegionChecks::EqSrc();
        r.esrc[1].kind = EQS_MAT;                         // no strided part: pad or diagonal
    }
    if (pad_b.phase >= 0) { r.esrc[1].pad_phase = pad_b.phase; r.esrc[1].pad_off = pad_b.off; }
    if (diag_b.phase >= 0) { r.esrc[1].diag_phase = diag_b.phase; r.esrc[1].diag_off = diag_b.off; }
}
// sid_val: the scalar's value when the host knows it (svd_witness's q^2): the
// stage then takes it as a constant and does not read sid's cell, which may
// still be in flight on another stream.
static void check_mat_id(svdw_ctx* c, const svdw_mat& a, const svdw_vec& sid, const BigU& tol,
                         const Fr* sid_val = nullptr) {
    const svdw_vec zero = put_cell(c, a.phase, fr_zero(), true);   // ctx.load_constant(F::ZERO)
    DView b = ptr_view(c->dry || sid_val ? nullptr : cellp(c, sid.phase, sid.off), a.rows, a.cols, 0, 0);
    b.mode = sid_val ? VIEW_DIAGK : VIEW_DIAG;
    check_mat_diff_views(c, a.phase, view_of(c, a), b, a.rows, a.cols, tol, sid_val, EqCell{},
                         EqCell{(int)zero.phase, zero.off}, EqCell{(int)sid.phase, sid.off});
}
static svdw_mat mat_times_diag_mat(svdw_ctx* c, const svdw_mat& a, const svdw_vec& v) {
    REQUIRE(v.len <= a.cols, "mat_times_diag_mat: v longer than a's rows");
    PB pb(c->LB);
    pb.a.view[0] = view_of(c, a);
    pb.a.view[1] = view_of(c, svdw_mat{v.phase, a.rows, v.len, v.off, 0, v.stride});
    uint8_t x = pb.load(0), y = pb.load(1);
    pb.g_mul(x, y);
    uint64_t off = run_stage(c, a.phase, pb, a.rows * v.len, v.len, "mat_times_diag_mat");
    return svdw_mat{a.phase, a.rows, v.len, off + 3, (int64_t)4 * v.len, 4};
}

// signed_div_scale constants (svdw_div_scale; zero fields -> 3P, shift + 1)
struct DivScale {
    uint32_t s, nb;
};
static DivScale div_scale_of(const svdw_ctx* c, const svdw_div_scale* cfg) {
    DivScale d;
    d.s = cfg && cfg->shift_bits ? cfg->shift_bits : 3 * c->P;
    // the reference's cell counts (svdw.h); a shift alone >= 4P + 1 widens the div_mod
    d.nb = cfg && cfg->num_bits ? cfg->num_bits : std::max(4 * c->P + 1, d.s + 1);
    REQUIRE(d.s >= c->P && d.s < 254 && d.nb > d.s && d.nb <= 253 && d.nb - c->P <= 200,
            "signed_div_scale: need P <= shift_bits < num_bits <= 253, num_bits - P <= 200");
    return d;
}
// ZkMatrix::rescale_matrix (src/matrix/mod.rs:354-375): signed_div_scale of
// every entry of c_s, row-major; the result matrix is the final sub's cell 0.
static svdw_mat rescale_matrix(svdw_ctx* c, const svdw_mat& cs, DivScale d) {
    PB pb(c->LB);
    pb.a.view[0] = view_of(c, cs);
    pb.signed_div_scale(pb.load(0), c->P, d.s, d.nb);
    const uint32_t C = pb.a.C;
    uint64_t off = run_stage(c, cs.phase, pb, cs.rows * cs.cols, cs.cols, "rescale_matrix");
    return svdw_mat{cs.phase, cs.rows, cs.cols, off + C - 4, (int64_t)C * cs.cols, C};
}
static svdw_vec field_mat_vec_mul(svdw_ctx* c, uint32_t phase, const svdw_mat& a, const svdw_vec& v);
// ZkVector::inner_product (src/matrix/mod.rs:79-106): gate.inner_product(x, self)
// (the field_mat_vec_mul row layout with x as the row), then signed_div_scale.
static svdw_vec zkvector_inner_product(svdw_ctx* c, uint32_t phase, const svdw_vec& self,
                                       const svdw_vec& x, DivScale d) {
    REQUIRE(self.len == x.len && x.len >= 1, "ZkVector::inner_product: length mismatch");
    svdw_vec s = field_mat_vec_mul(c, phase, svdw_mat{x.phase, 1, x.len, x.off, 0, x.stride}, self);
    PB pb(c->LB);
    pb.a.view[0] = view_of(c, mat_of_vec(s));
    pb.signed_div_scale(pb.load(0), c->P, d.s, d.nb);
    const uint32_t C = pb.a.C;
    uint64_t off = run_stage(c, phase, pb, 1, 1, "signed_div_scale");
    return svdw_vec{phase, 1, off + C - 4, 1};
}
// ZkVector::_norm_square (src/matrix/mod.rs:112-119): self.inner_product(self).
static svdw_vec zkvector_norm_square(svdw_ctx* c, uint32_t phase, const svdw_vec& self, DivScale d) {
    return zkvector_inner_product(c, phase, self, self, d);
}
// ZkVector::_dist_square (src/matrix/mod.rs:135-148): diff_i = qsub(self_i, x_i)
// (FixedPointChip041::qsub = gate.sub [ext, inferred as for entries_in_desc_order]:
// cells [a - b, b, 1, a]), then diff._norm_square.
// qsqrt of a one-element vector (ZkVector::norm / dist's final step)
static svdw_vec qsqrt_vec(svdw_ctx* c, uint32_t phase, const svdw_vec& a, uint32_t nbits) {
    const uint32_t nb = nbits ? nbits : 2 * c->P;
    REQUIRE(nb >= 1 && nb + c->P <= 250, "qsqrt: need 1 <= sqrt_bits, sqrt_bits + P <= 250");
    PB pb(c->LB);
    pb.a.view[0] = view_of(c, mat_of_vec(a));
    pb.qsqrt(pb.load(0), c->P, nb);
    uint64_t off = run_stage(c, phase, pb, 1, 1, "qsqrt");
    return svdw_vec{phase, 1, off, 1};                   // y: the gadget's first cell
}
static svdw_vec zkvector_dist_square(svdw_ctx* c, uint32_t phase, const svdw_vec& self,
                                     const svdw_vec& x, DivScale d) {
    REQUIRE(self.len == x.len && x.len >= 1, "ZkVector::_dist_square: length mismatch");
    PB sb(c->LB);
    sb.a.view[0] = view_of(c, mat_of_vec(self));
    sb.a.view[1] = view_of(c, mat_of_vec(x));
    uint8_t a = sb.load(0), b = sb.load(1);
    sb.g_sub(a, b);
    const uint64_t soff = run_stage(c, phase, sb, self.len, 1, "qsub");
    const svdw_vec diff{phase, self.len, soff, 4};
    return zkvector_norm_square(c, phase, diff, d);
}
// ZkVector::mul (src/matrix/mod.rs:169-182): inner_product with each row of a
// (one row scan + one stage per row; config-1 plumbing, not the hot path).
static svdw_vec zkvector_mul(svdw_ctx* c, uint32_t phase, const svdw_vec& self, const svdw_mat& a,
                             DivScale d) {
    REQUIRE(a.cols == self.len, "ZkVector::mul: a.num_col != self.size()");
    svdw_vec first{}, prev{};
    for (uint32_t i = 0; i < a.rows; ++i) {
        svdw_vec row{a.phase, a.cols, a.off + (uint64_t)((int64_t)i * a.rs), a.cs};
        svdw_vec y = zkvector_inner_product(c, phase, self, row, d);
        if (i == 0) first = y;
        if (i == 1) first.stride = (int64_t)(y.off - prev.off);
        prev = y;
    }
    first.len = a.rows;
    return first;
}

// rows [r0, r1) of a matrix view
static svdw_mat row_block(const svdw_mat& a, uint64_t r0, uint64_t r1) {
    return svdw_mat{a.phase, (uint32_t)(r1 - r0), a.cols, a.off + r0 * a.rs, a.rs, a.cs};
}
// honest_prover_mat_mul (src/matrix/mod.rs:546-568). bits_a/bits_b: known bounds or ~0u.
// If the product was launched ahead on st2 (c->call.pre), only append and order st after it.
static svdw_mat honest_prover_mat_mul(svdw_ctx* c, uint32_t phase, const svdw_mat& a,
                                      const svdw_mat& b, uint32_t bits_a = ~0u,
                                      uint32_t bits_b = ~0u) {
    REQUIRE(a.cols == b.rows, "honest_prover_mat_mul: a.num_col != b.num_rows");
    const uint32_t N = a.rows, M = b.cols;
    uint64_t off;
    append(c, phase, (uint64_t)N * M, 0, &off, nullptr, "product", N);
    svdw_mat cs{phase, N, M, off, (int64_t)M, 1};
    if (c->gemm_log) c->gemm_log->push_back(off);
    uint64_t sr0 = 0, sr1 = N;                            // shard: rows of c_s computed here
    if (sharded(c)) {
        shard_rows(c, N, &sr0, &sr1);
        own(c, phase, false, off + sr0 * M, (sr1 - sr0) * M);
    }
    // |c_s| <= K * 2^bits_a * 2^bits_b, resolved when the operand bounds are known
    c->wit.prods.push_back({cs, a, b, clog2(a.cols)});
    if (bits_a == ~0u) bits_a = bits_of(c, a);
    if (bits_b == ~0u) bits_b = bits_of(c, b);
    if (c->dry) return cs;
    if (!c->call.pre.empty()) {
        if (c->call.pre.front().off != off) fail(SVDW_EDEVICE, "internal: pre-launched GEMM offset mismatch");
        // (launched on this very stream: already ordered; the three batched
        // products share one event: one wait per stream)
        if (c->call.pre.front().st != c->st && !(c->call.pre_wait_st == c->st && c->call.pre_wait_ev == c->call.pre.front().ev)) {
            dep_wait(c, c->st, c->call.pre.front().ev);
            c->call.pre_wait_st = c->st;
            c->call.pre_wait_ev = c->call.pre.front().ev;
        }
        c->call.pre.erase(c->call.pre.begin());
        return cs;
    }
    const bool sym = is_transpose_of(b, a);
    if (bits_a == ~0u || bits_b == ~0u) {
        std::vector<svdw_mat> ms{a};
        if (!sym) ms.push_back(b);
        auto bb = maxbits_many(c, ms);
        bits_a = bb[0];
        bits_b = sym ? bb[0] : bb[1];
        reg_bits(c, a, bits_a);
        reg_bits(c, b, bits_b);
    }
    if (sr1 > sr0)                                        // (unsharded: every row)
        gemm_exec(c, c->st, row_block(a, sr0, sr1), b, cellp(c, phase, off + sr0 * M), bits_a, bits_b);
    return cs;
}
// Words of the small operand for the row-scan products: |signed a| < 2^(32 na)
// when a's bound is known to the host, else 8 (full Montgomery).
static int scan_na(const svdw_ctx* c, const svdw_mat& a) {
    const uint32_t b = bits_of(c, a);
    if (b == ~0u || b > 192) return 8;
    return std::max(1, (int)((b + 31) / 32));
}
// The same bound as the device sees it: a quantized matrix's bit-length word, or
// a product of two of them (bits_a + bits_b + lk); wa = -1: unknown.
static NaSpec scan_spec(const svdw_ctx* c, const svdw_mat& a) {
    auto word = [&](const svdw_mat& m) -> int16_t {
        for (auto& r : c->wit.dwords)
            if (same_cells(r.m, m)) return r.word;
        return -1;
    };
    const int16_t w = word(a);
    if (w >= 0) return NaSpec{w, -1, 0, 0};
    for (auto& p : c->wit.prods)
        if (same_cells(p.cs, a)) {
            const int16_t wa = word(p.a), wb = word(p.b);
            if (wa >= 0 && wb >= 0) return NaSpec{wa, wb, (uint16_t)p.lk, 0};
        }
    return NaSpec{-1, -1, 0, 0};
}
// A scan job's bound for the device: host-known bits as a constant (wa = -2,
// bits in lk), else its device words (scan_spec).
static NaSpec job_spec(const svdw_ctx* c, const svdw_mat& a) {
    const uint32_t b = bits_of(c, a);
    if (b != ~0u) return NaSpec{-2, -1, (uint16_t)std::min(b, 65535u), 0};
    return scan_spec(c, a);
}
// na of a batch of scans: host-known (1..8), or 0 = decided on the device from
// the jobs' specs (job_spec), so the host needs no operand bounds
static int batch_na_host(const svdw_ctx* c, const svdw_mat* ms, int n) {
    int na = 1;
    bool host = true, dev = c->wit.dbitw != nullptr;
    for (int i = 0; i < n; ++i) {
        if (bits_of(c, ms[i]) != ~0u) na = std::max(na, scan_na(c, ms[i]));
        else host = false;
        if (job_spec(c, ms[i]).wa == -1) dev = false;
    }
    if (host) return na;
    return dev ? 0 : 8;
}
// A vector of len values as the scans take it: room for its canonical copy (bc)
// and its scaled table (bt).
static void ensure_pair(svdw_ctx* c, DBuf& bc, DBuf& bt, uint32_t len) {
    ensure_buf(c, bc, (size_t)len * sizeof(Fr));
    ensure_buf(c, bt, tab_len(len) * sizeof(Fr));
}
// mont_mul(w, f[s]) = slot s of w's scaled table: w * 2^(32 (s + 1)) for s < 6,
// w's Montgomery form for s = 6 (kernels.hpp kTabSlots)
static ScaleTab scale_tab() {
    ScaleTab t;
    for (int s = 0; s < kTabSlots - 1; ++s) {
        Fr x = fr_zero();
        x.w[s + 1] = 1;                                    // 2^(32 (s + 1)) < p
        t.f[s] = mont_mul(x, fr_r2());
    }
    t.f[kTabSlots - 1] = fr_r2();
    return t;
}
// field_mat_vec_mul with the vector given as canonical copy + scaled table.
// the equality sources of an inner-product row region: a's row i, the vector w
static void note_scan(svdw_ctx* c, const svdw_mat& a, const RegionChecks::EqSrc& w) {
    RegionChecks& r = c->wit.layout_chk.back();
    r.scan = true;
    r.unit = 3 * a.cols + 1;
    r.esrc[0] = eqsrc_mat(a);
    r.esrc[1] = w;
}
// An inner-product row region of a (a row: 3 a.cols + 1 cells, its total last;
// `total`: the first row's): this rank's rows, a row's cells, the region's first cell.
struct ScanRows { uint64_t r0, r1, rowc, base; };
static ScanRows scan_rows(const svdw_ctx* c, const svdw_mat& a, uint64_t total) {
    ScanRows s{0, a.rows, 3ull * a.cols + 1, total - 3ull * a.cols};
    if (sharded(c)) shard_rows(c, a.rows, &s.r0, &s.r1);
    return s;
}
static svdw_vec matvec_rows(svdw_ctx* c, uint32_t phase, const svdw_mat& a, const Fr* wc,
                            const Fr* tab, uint32_t tl, int na, const RegionChecks::EqSrc& wsrc) {
    const uint32_t R = a.rows, L = a.cols;
    uint64_t off;
    append(c, phase, (uint64_t)R * (3ull * L + 1), 0, &off, nullptr, "scan", R);
    note_scan(c, a, wsrc);
    const ScanRows s = scan_rows(c, a, off + 3ull * L);
    own(c, phase, false, off + s.r0 * s.rowc, (s.r1 - s.r0) * s.rowc);
    if (!c->dry) {
        ProfScope ps(c, c->st, a.cs == 1 ? "k_matvec_scan:rows" : "k_matvec_scan:cols", 32.0 * (double)R * (4.0 * L + 1) + 64.0 * L, (double)R * L);
        hipck(launch_matvec_scan(view_of(c, a), (uint32_t)s.r0, (uint32_t)s.r1, L, wc, tab, tl,
                                 cellp(c, phase, off + s.r0 * s.rowc), na, c->st), "k_matvec_scan");
    }
    return svdw_vec{phase, R, off + 3ull * L, (int64_t)(3ull * L + 1)};
}
// canonical copy into bc, scaled table into bt
static const Fr* vec_prep_view(svdw_ctx* c, const DView& w, uint32_t len, DBuf& bc, DBuf& bt) {
    ensure_pair(c, bc, bt, len);
    if (!c->dry) {
        ProfScope ps(c, c->st, "k_vec_prep", 32.0 * len * (2 + tab_len(1)), 0);
        hipck(launch_vec_prep(w, len, (Fr*)bc.p, (Fr*)bt.p, scale_tab(), c->st), "k_vec_prep");
    }
    return (const Fr*)bt.p;
}
static svdw_vec field_mat_vec_mul(svdw_ctx* c, uint32_t phase, const svdw_mat& a,
                                  const svdw_vec& v) {
    REQUIRE(a.cols == v.len, "field_mat_vec_mul: a[0].len() != v.len()");
    const int na = scan_na(c, a);
    const Fr* tab = vec_prep_view(c, view_of(c, svdw_mat{v.phase, 1, v.len, v.off, 0, v.stride}), v.len, c->w1c, c->w1t);
    return matvec_rows(c, phase, a, (const Fr*)c->w1c.p, tab, v.len, na, eqsrc_vec(v));
}
// ZkMatrix::verify_mul (src/matrix/mod.rs:251-282) for several (a, b, c_s) triples
// with one gamma: cells are appended exactly as consecutive verify_mul calls
// would append them, then the row scans run as three batched launches (all
// c_s.v scans, all b.v scans, all a.(b.v) scans) so the rows of every call
// share one wave of blocks.
// v = (1, g, g^2, ...): canonical (gpc) + scaled table (gtab), on stream s. The
// powers come from three host-side Montgomery tables (g^a, g^(16 b), g^(256 c)):
// three products per element on the device instead of a square-and-multiply chain.
void gamma_prep(svdw_ctx* c, uint32_t d, const Fr& gamma, hipStream_t s, const PowCells* pc) {
    if (c->dry) return;
    REQUIRE(!c->vmg.capturing, "internal: gamma inside a captured graph");
    const uint32_t len = std::max(d, 1u);
    REQUIRE((len + 255) / 256 <= (uint32_t)kGammaTab - 32, "verify_mul: vector too long");
    ensure_pair(c, c->gpc, c->gtab, len);
    GammaTab g;
    memset(&g, 0, sizeof g);
    const Fr one = fr_one_mont(), gm = fr_to_mont(gamma);
    g.t[0] = one;
    for (int i = 1; i < 16; ++i) g.t[i] = mont_mul(g.t[i - 1], gm);
    const Fr g16 = mont_mul(g.t[15], gm);
    g.t[16] = one;
    for (int i = 1; i < 16; ++i) g.t[16 + i] = mont_mul(g.t[15 + i], g16);
    const Fr g256 = mont_mul(g.t[31], g16);
    g.nhi = (len + 255) / 256;
    g.t[32] = one;
    for (uint32_t i = 1; i < g.nhi; ++i) g.t[32 + i] = mont_mul(g.t[31 + i], g256);
    {
        ProfScope ps(c, s, "k_gamma_prep", 32.0 * len * (1 + tab_len(1)), 0);
        hipck(launch_gamma_prep(g, len, (Fr*)c->gpc.p, (Fr*)c->gtab.p, scale_tab(), s, pc),
              "k_gamma_prep");
    }
    c->gp_gamma = gamma;
    c->gp_len = len;
}
// gamma vector for verify_mul on c->st: the one queued ahead when it matches,
// else prepared here
static void ensure_gamma_vec(svdw_ctx* c, uint32_t d, const Fr& gamma) {
    if (c->dry) return;
    if (c->gp_ev && c->gp_len >= d && fr_eq(c->gp_gamma, gamma)) {
        if (c->gp_st != c->st) dep_wait(c, c->st, c->gp_ev);
        return;
    }
    gamma_prep(c, d, gamma, c->st);
    c->gp_ev = nullptr;
}
void verify_mul_many(svdw_ctx* c, uint32_t phase, const VMul* vm, int n, const Fr& gamma) {
    REQUIRE(n >= 1 && n <= kMaxVerifyBatch, "internal: verify_mul batch size");
    c->ext_gamma = gamma;
    struct Plan {
        PB one, pows, eq;
        uint64_t one_off = 0, one_loff = 0, pows_off = 0, pows_loff = 0, eq_off = 0, eq_loff = 0;
        size_t eq_reg = 0;                // its layout region (views noted at launch)
        svdw_vec csv{}, bv{}, abv{};
        explicit Plan(uint32_t lb) : one(lb), pows(lb), eq(lb) {}
    };
    std::vector<Plan> pl;
    pl.reserve(n);
    uint32_t dmax = 0;
    auto scan_append = [&](const svdw_mat& a, const RegionChecks::EqSrc& w) {
        uint64_t off;
        append(c, phase, (uint64_t)a.rows * (3ull * a.cols + 1), 0, &off, nullptr, "scan", a.rows);
        note_scan(c, a, w);
        note_const(c, fr_zero());                             // inner_product's Constant(0)
        return svdw_vec{phase, a.rows, off + 3ull * a.cols, (int64_t)(3ull * a.cols + 1)};
    };
    // pass 1: the cell layout, in the reference's order
    for (int i = 0; i < n; ++i) {
        const svdw_mat &a = vm[i].a, &b = vm[i].b, &cs = vm[i].cs;
        REQUIRE(a.cols == b.rows, "verify_mul: a.num_col != b.num_rows");
        REQUIRE(cs.rows == a.rows, "verify_mul: c_s.len() != a.num_rows");
        REQUIRE(cs.cols == b.cols, "verify_mul: c_s[0].len() != b.num_col");
        const uint32_t d = cs.cols;
        dmax = std::max(dmax, d);
        pl.emplace_back(c->LB);
        Plan& p = pl.back();
        p.one.cell(p.one.K(fr_from_u64(1)));                  // load_witness(F::ONE)
        append(c, phase, p.one.a.C, 0, &p.one_off, &p.one_loff, "load_cell");
        note_gates(c, p.one);                                 // assert_is_const(one, 1)
        stage_own(c, phase, p.one, 1, 1, p.one_off, p.one_loff);
        if (d > 1) {                                          // v_i = mul(v_{i-1}, init_rand)
            uint8_t prev = p.pows.load(0), cur = p.pows.load(1);
            p.pows.gate(0);                               // mul(v_(i-1), init_rand)
            p.pows.kext = p.pows.kidx(gamma);             // gamma: a cell of the RLC context
            p.pows.vsrc[1] = false;                       // v_i: produced here
            note_const(c, fr_zero());
            p.pows.cell(p.pows.K(0)); p.pows.cell(prev); p.pows.cell(p.pows.K(gamma)); p.pows.cell(cur);
            append(c, phase, (uint64_t)(d - 1) * p.pows.a.C, 0, &p.pows_off, &p.pows_loff,
                   "verify_mul_gamma_pows");
            note_gates(c, p.pows);
            c->wit.gamma_slots.emplace_back(c->wit.layout_chk.size() - 1, p.pows.kext);
            // v_(i-1): the `one` cell, then the previous mul's output
            c->wit.layout_chk.back().esrc[0] = eqsrc_chain(phase, p.one_off, phase, p.pows_off + 3, 4);
            stage_own(c, phase, p.pows, d - 1, 1, p.pows_off, p.pows_loff);
        }
        const RegionChecks::EqSrc gsrc = eqsrc_chain(phase, p.one_off, phase, p.pows_off + 3, 4);
        p.csv = scan_append(cs, gsrc);
        p.bv = scan_append(b, gsrc);
        p.abv = scan_append(a, eqsrc_vec(p.bv));
        if (sharded(c)) {                                 // this rank's rows of the three scans
            for (const auto& sv : {std::make_pair(cs, p.csv), std::make_pair(b, p.bv),
                                   std::make_pair(a, p.abv)}) {
                const ScanRows s = scan_rows(c, sv.first, sv.second.off);
                own(c, phase, false, s.base + s.r0 * s.rowc, (s.r1 - s.r0) * s.rowc);
            }
        }
        uint8_t x = p.eq.load(0), y = p.eq.load(1);           // is_equal per row (result unused)
        p.eq.g_is_equal(x, y);
        append(c, phase, (uint64_t)a.rows * p.eq.a.C, (uint64_t)a.rows * p.eq.a.L, &p.eq_off,
               &p.eq_loff, "verify_mul_is_equal", a.rows);
        note_gates(c, p.eq);
        p.eq_reg = c->wit.layout_chk.size() - 1;
        c->wit.layout_chk.back().esrc[0] = eqsrc_mat(mat_of_vec(p.csv));
        c->wit.layout_chk.back().esrc[1] = eqsrc_mat(mat_of_vec(p.abv));
        stage_own(c, phase, p.eq, a.rows, 1, p.eq_off, p.eq_loff);
    }
    if (c->dry) return;
    host_mark(c, "verify_mul layout");
    // pass 2: launches
    ensure_gamma_vec(c, dmax, gamma);
    const Fr* gpc = (const Fr*)c->gpc.p;
    const Fr* gtab = (const Fr*)c->gtab.p;
    // verify_mul_witness: k_gamma_prep already wrote the one cell and the powers
    const bool pre = c->call.pows_pre.on && n == 1 && pl[0].one_off == c->call.pows_pre.one_off &&
                     pl[0].pows_off == c->call.pows_pre.pows_off && vm[0].cs.cols == c->call.pows_pre.d &&
                     pl[0].one_loff == 0;
    c->call.pows_pre.on = false;
    // the one cells and gamma powers: read by no kernel of the call (gpc, not
    // these cells, feeds the scans), so a pipelined svd_witness launches them
    // after the scans, off the head of phase 1's stream
    auto pows_launch = [&] {
        if (pre) return;
        // (a captured graph must not hold gamma: the powers' launch carries it)
        for (int i = 0; i < n; ++i) REQUIRE(!c->vmg.capturing || vm[i].cs.cols <= 1, "internal: gamma inside a captured graph");
        BatchScope bs(c);                                 // the one cells and gamma powers: one launch
        for (int i = 0; i < n; ++i) {
            Plan& p = pl[i];
            const uint32_t d = vm[i].cs.cols;
            stage_launch(c, phase, p.one, 1, 1, p.one_off, p.one_loff, "load_cell");
            if (d > 1) {
                p.pows.a.view[0] = ptr_view(gpc, d, 1, 1, 0);
                p.pows.a.view[1] = ptr_view(gpc + 1, d, 1, 1, 0);
                stage_launch(c, phase, p.pows, d - 1, 1, p.pows_off, p.pows_loff, "verify_mul_gamma_pows");
            }
        }
        bs.end();
    };
    const bool pows_late = c->call.in_pipe;
    if (!pows_late) pows_launch();
    // One scan launch over jobs (a_q against the vector wc_q / tab_q, cells at
    // v_q); operand widths host-known or read on the device (na 0).
    struct Scans {
        ScanBatch sb;
        svdw_mat ms[kMaxScanJobs];
        double bytes = 0, ops = 0;
        Scans() { memset(&sb, 0, sizeof sb); }
    };
    auto add_job = [&](Scans& S, const svdw_mat& a, const svdw_vec& v, const Fr* wc, const Fr* tab,
                       uint32_t tl) -> ScanJob& {
        REQUIRE(S.sb.njobs < (uint32_t)kMaxScanJobs, "internal: scan batch full");
        const ScanRows s = scan_rows(c, a, v.off);        // shard: this rank's rows
        S.ms[S.sb.njobs] = a;
        ScanJob& j = S.sb.job[S.sb.njobs++];
        j = ScanJob{f64_view(c, view_of(c, a)), wc, tab, tl, cellp(c, phase, s.base + s.r0 * s.rowc),
                    a.cols, (uint32_t)(s.r1 - s.r0), 0, (uint32_t)s.r0, job_spec(c, a)};
        S.bytes += 32.0 * (s.r1 - s.r0) * (4.0 * a.cols + 1) + 64.0 * a.cols;
        S.ops += (double)(s.r1 - s.r0) * a.cols;
        return j;
    };
    auto launch = [&](Scans& S, const char* name) {
        S.sb.bitw = c->wit.dbitw;
        S.sb.f = scale_tab();
        const int na = batch_na_host(c, S.ms, (int)S.sb.njobs);
        ProfScope ps(c, c->st, name, S.bytes, S.ops);
        hipck(launch_scan_batch(S.sb, na, c->st), "k_matvec_scan");
    };
    // b.g of job i: the b scan of the first job with the same b (m.v^T and
    // v.v^T share v^T) serves every later job with it
    int src[kMaxVerifyBatch];
    for (int i = 0; i < n; ++i) {
        src[i] = i;
        for (int k = 0; k < i; ++k)
            if (vm[k].b.phase == vm[i].b.phase && vm[k].b.off == vm[i].b.off &&
                vm[k].b.rows == vm[i].b.rows && vm[k].b.cols == vm[i].b.cols &&
                vm[k].b.rs == vm[i].b.rs && vm[k].b.cs == vm[i].b.cs) { src[i] = k; break; }
    }
    const Fr* wt[kMaxVerifyBatch];
    // b = X^T of an f64 input of svd_witness: X, else null
    auto f64_of = [&](const svdw_mat& b) -> const svdw_ctx::F64Src* {
        if (b.cols > kCrtMaxK) return nullptr;
        for (auto& s : c->call.f64src)
            if (is_transpose_of(b, s.m) && s.m.rs == (int64_t)s.m.cols && s.m.cs == 1) return &s;
        return nullptr;
    };
    bool all_f64 = true;
    for (int i = 0; i < n && all_f64; ++i) all_f64 = f64_of(vm[i].b) != nullptr;
    // launch order != append order: the b and a.(b.g) scans need only the
    // operands, the c_s scans wait for the products when those run elsewhere
    Scans bs_, as_;
    auto add_b = [&](Scans& S, int i) -> ScanJob& { return add_job(S, vm[i].b, pl[i].bv, gpc, gtab, c->gp_len); };
    auto add_a = [&](Scans& S, int i) {
        add_job(S, vm[i].a, pl[i].abv, (const Fr*)c->wbc[src[i]].p, wt[i], vm[i].b.rows);
    };
    if (all_f64) {
        // every entry of b.g from the f64 rows of X (quantized in registers),
        // column-parallel and coalesced: one launch for the distinct b's, then
        // the slices' sums folded into each vector's table (k_vec_prep_sum);
        // the b and a.(b.g) scans are then independent: one launch
        ColBatch cb;
        memset(&cb, 0, sizeof cb);
        cb.tab = gtab;
        cb.tl = c->gp_len;
        cb.bitw = c->wit.dbitw;
        int slot[kMaxVerifyBatch];
        size_t poff[kMaxVerifyBatch], ptot = 0;
        for (int i = 0; i < n; ++i) {
            if (src[i] != i) { slot[i] = slot[src[i]]; continue; }
            REQUIRE(cb.njobs < (uint32_t)kMaxColJobs, "internal: too many distinct b for k_colsum_f64");
            const svdw_ctx::F64Src* s = f64_of(vm[i].b);
            ColJob& j = cb.job[cb.njobs];
            j.x = s->x;
            j.R = s->m.rows;
            j.C = s->m.cols;
            j.ld = s->m.cols;
            j.spec = job_spec(c, vm[i].b);
            poff[cb.njobs] = ptot;
            ptot += (size_t)colsum_slices(j.R) * j.C;
            slot[i] = (int)cb.njobs++;
        }
        ensure_buf(c, c->colpart, ptot * sizeof(Fr));
        for (uint32_t q = 0; q < cb.njobs; ++q) cb.job[q].part = (Fr*)c->colpart.p + poff[q];
        {
            ProfScope ps(c, c->st, "k_colsum_f64", 0, 0);
            hipck(launch_colsum_f64(cb, (int)c->P, c->st), "k_colsum_f64");
        }
        // the distinct b's vectors in one launch
        VecPrepBatch vp;
        memset(&vp, 0, sizeof vp);
        double vbytes = 0;
        for (int i = 0; i < n; ++i) {
            if (src[i] != i) { wt[i] = wt[src[i]]; continue; }
            const uint32_t L = vm[i].b.rows;
            ensure_pair(c, c->wbc[i], c->wbt[i], L);
            REQUIRE(vp.njobs < (uint32_t)kMaxColJobs, "internal: too many distinct b for k_vec_prep_sum");
            vp.job[vp.njobs++] = VecPrepJob{cb.job[slot[i]].part, colsum_slices(cb.job[slot[i]].R), L,
                                            (Fr*)c->wbc[i].p, (Fr*)c->wbt[i].p, 0};
            vbytes += 32.0 * L * (2 + tab_len(1));
            wt[i] = (const Fr*)c->wbt[i].p;
        }
        {
            ProfScope ps(c, c->st, "k_vec_prep", vbytes, 0);
            hipck(launch_vec_prep_sum_multi(vp, scale_tab(), c->st), "k_vec_prep_sum_multi");
        }
        for (int i = 0; i < n; ++i) add_b(bs_, i);
        for (int i = 0; i < n; ++i) add_a(bs_, i);
        launch(bs_, "k_matvec_scan:ba");
    } else if (sharded(c)) {
        for (int i = 0; i < n; ++i) add_b(bs_, i);
        launch(bs_, "k_matvec_scan:b");
        // only this rank's rows of the b.g scans exist: every entry of b.g comes
        // from the values-only mat-vec instead (the distinct b's in one launch)
        ScanBatch vb;
        memset(&vb, 0, sizeof vb);
        svdw_mat vms[kMaxVerifyBatch];
        int nv = 0, slot[kMaxVerifyBatch];
        for (int i = 0; i < n; ++i) {
            if (src[i] != i) { slot[i] = slot[src[i]]; continue; }
            const svdw_mat b = vm[i].b;
            ensure_buf(c, c->bvfull[nv], (size_t)b.rows * sizeof(Fr));
            vb.job[nv] = ScanJob{f64_view(c, view_of(c, b)), nullptr, gtab, c->gp_len, (Fr*)c->bvfull[nv].p,
                                 b.cols, b.rows, 0, 0, job_spec(c, b)};
            vms[nv] = b;
            slot[i] = nv++;
        }
        vb.njobs = nv;
        vb.bitw = c->wit.dbitw;
        {
            ProfScope ps(c, c->st, "k_matvec_values", 0, 0);
            hipck(launch_matvec_values(vb, batch_na_host(c, vms, nv), c->st), "k_matvec_values");
        }
        for (int i = 0; i < n; ++i)
            wt[i] = src[i] != i ? wt[src[i]]
                                : vec_prep_view(c, ptr_view((const Fr*)c->bvfull[slot[i]].p, 1, vm[i].b.rows, 0, 1),
                                                vm[i].b.rows, c->wbc[i], c->wbt[i]);
        for (int i = 0; i < n; ++i) add_a(as_, i);
        launch(as_, "k_matvec_scan:a");
    } else {
        // every row of b scanned: the b scan of each distinct b also writes b.g
        // as the a scan's vector (canonical + table) from its row totals
        for (int i = 0; i < n; ++i) {
            ScanJob& j = add_b(bs_, i);
            if (src[i] != i) continue;
            const uint32_t L = vm[i].b.rows;
            ensure_pair(c, c->wbc[i], c->wbt[i], L);
            j.pc = (Fr*)c->wbc[i].p;
            j.ptab = (Fr*)c->wbt[i].p;
            j.plen = L;
        }
        for (int i = 0; i < n; ++i) wt[i] = (const Fr*)c->wbt[src[i]].p;
        launch(bs_, "k_matvec_scan:b");
        for (int i = 0; i < n; ++i) add_a(as_, i);
        launch(as_, "k_matvec_scan:a");
    }
    host_mark(c, "verify_mul b, a scans queued");
    for (hipEvent_t ev : c->call.wait_before_cs)
        dep_wait(c, c->st, ev);
    // the c_s scans; each row's is_equal(c_s.g, a.(b.g)) cells from its row
    // total and the a scan's last cell (k_matvec_scan_dpp's eq epilogue)
    Scans cs_;
    for (int i = 0; i < n; ++i) {
        Plan& p = pl[i];
        ScanJob& j = add_job(cs_, vm[i].cs, p.csv, gpc, gtab, c->gp_len);
        j.eq_out = cellp(c, phase, p.eq_off);
        j.eq_y = cellp(c, p.abv.phase, p.abv.off);
        j.eq_ys = (uint32_t)p.abv.stride;
        p.eq.a.view[0] = view_of(c, mat_of_vec(p.csv));
        p.eq.a.view[1] = view_of(c, mat_of_vec(p.abv));
        note_gates(c, p.eq, 1, p.eq_reg);
    }
    launch(cs_, "k_matvec_scan:cs");
    if (pows_late) pows_launch();
}

// err_calc (src/svd/mod.rs:155-163). Host f64, built with -ffp-contract=off.
void err_calc(uint32_t p, uint64_t size, double max_norm, double eps_svd, double eps_u, double* es, double* eu) {
    volatile double precision = pow(2.0, -1.0 * ((double)p + 1.0));
    double s = (double)size;
    *es = precision * s * (1.0 + max_norm + eps_svd + precision) + s * max_norm * precision +
          pow(1.0 + eps_u, 0.5) * (max_norm + eps_svd) * eps_u + pow(1.0 + eps_u, 0.5) * eps_svd;
    *eu = eps_u + precision * s * (2.0 * (1.0 + eps_u) + precision);
}
// `(err * (2u128.pow(2P) as f64)).round() as u128`
static BigU scale_err(double err, uint32_t p) {
    double x = round(err * ldexp(1.0, 2 * (int)p));
    if (!(x > 0)) return big_from_u128(0);
    if (x >= 340282366920938463463374607431768211456.0) return big_from_u128(~(unsigned __int128)0);
    return big_from_u128((unsigned __int128)x);
}

// The three products of check_svd_phase0 (A[g] * B[g], B = transposes) on pst
// from svd_witness's f64 inputs (gemm.cpp). log[g]: the products' stream
// offsets (dry replay); W: the device bit-length words of m, u, v.
static void prelaunch_products_f64(svdw_ctx* c, const svdw_mat (&A)[3], const svdw_mat (&B)[3],
                                   const std::vector<uint64_t>& log, uint32_t phase,
                                   const unsigned* W, hipStream_t pst) {
    svd_residues_f64(c, A, W, pst);
    // the stages beside the products wait for the residue planes, which then
    // run alone instead of beside the first (HBM-saturating) stages (same box:
    // 512^2 0.427 -> 0.422 ms, 1024^2 2.098 -> 2.072 ms, 8-way rank 0.36 -> 0.35)
    // ("res_wait" 0, pipelined with every load read from the f64 inputs: the
    // stages need nothing of this chain before the products, so st2 goes on
    // without waiting for the residue planes; -1: so on unsharded contexts,
    // tools/ab.py r6f: 512^2 0.378 -> 0.371 ms, 1024^2 2.035 -> 2.026 ms, while
    // the 8-way rank's chain is better served by the wait, 0.321 -> 0.327 ms)
    const bool rw = c->opt.res_wait >= 0 ? c->opt.res_wait != 0 : sharded(c);
    if (rw || !c->call.in_pipe || !c->opt.f64_views || c->call.f64reg.empty())
        stream_dep(c, pst, pst != c->st ? c->st : c->st2);
    c->call.gemm_batched = true;
    svd_products_f64(c, A, B, log, phase, W, pst);
    const hipEvent_t done = stream_dep(c, pst, nullptr);   // one completion point
    for (int g = 0; g < 3; ++g) {
        c->call.pre.push_back({log[g], done, pst});
        c->call.gemm_done.push_back(done);
    }
}

// check_svd_phase0
svdw_svd_payload check_svd_phase0(svdw_ctx* c, const svdw_mat& m, const svdw_mat& u, const svdw_mat& v,
                                  const svdw_vec& d, double err_svd, double err_u, uint32_t max_bits_d,
                                  const uint32_t* known_bits, const unsigned* dev_bits, bool dev_quantized) {
    REQUIRE(m.rows == u.rows, "check_svd_phase0: m.num_rows != u.num_rows");
    REQUIRE(m.cols == v.rows, "check_svd_phase0: m.num_col != v.num_rows");
    REQUIRE(u.rows == u.cols, "check_svd_phase0: u not square");
    REQUIRE(v.rows == v.cols, "check_svd_phase0: v not square");
    const uint32_t N = m.rows, M = m.cols, r = std::min(N, M);
    REQUIRE(d.len == r, "check_svd_phase0: d.len != min(N, M)");
    const uint32_t P = c->P;
    const uint32_t max_bits = max_bits_d + P;
    const svdw_mat ut = transposed(u), vt = transposed(v);
    uint64_t n0[2], nl0[2];                               // stream state at entry (for the replay)
    for (int p = 0; p < 2; ++p) { n0[p] = c->ph[p].n; nl0[p] = c->ph[p].nl; }
    auto prelaunch = [&] {
        if (c->dry || !c->opt.overlap || !known_bits || !c->call.pre.empty()) return;
        // The three products depend only on m, u, v: take their stream offsets
        // from a dry replay of this function and launch them now on st2, so the
        // integer GEMMs run under the HBM-bound check stages on st. Called after
        // the first check stage is queued, so the device is busy while the host
        // waits for the operand bit lengths.
        const bool on_device = dev_bits && c->opt.gemm_impl == SVDW_GEMM_MFMA;
        if (!on_device) fetch_bits(c);
        // residue planes straight from svd_witness's f64 inputs (one launch for m,
        // u and v) when they are on the device and the CRT path applies
        const bool from_f64 = on_device && dev_quantized && crt_product_f64(c, std::max(N, M)) &&
                              c->call.svd_f64[0] && c->call.svd_f64[1] && c->call.svd_f64[2];
        std::vector<uint64_t> key = {n0[0], n0[1], nl0[0], nl0[1], d.phase, d.len, d.off,
                                     (uint64_t)d.stride, f64_key(err_svd), f64_key(err_u), max_bits_d};
        for (const svdw_mat* x : {&m, &u, &v})
            key.insert(key.end(), {x->phase, x->rows, x->cols, x->off, (uint64_t)x->rs, (uint64_t)x->cs});
        std::vector<uint64_t> log;
        if (key == c->log_key) {
            log = c->log_val;
        } else {
            PlanCtx plan(c->P, c->LB, c);              // (nothing appended since entry: n0, nl0)
            plan.gemm_log = &log;
            check_svd_phase0(&plan, m, u, v, d, err_svd, err_u, max_bits_d, known_bits);
            REQUIRE(log.size() == 3, "internal: expected three products in check_svd_phase0");
            c->log_key = key;
            c->log_val = log;
        }
        // loads of m, u, v done: the quantization event when svd_witness recorded
        // one (the cell stream may already hold later stages), else st's position
        // products on the cell stream (prod_cell): already behind the loads there
        c->call.prod_on_cell = from_f64 && c->bits_pending && products_on_cell_stream(c);
        hipStream_t pst = c->call.prod_on_cell ? c->st : c->st2;
        if (c->call.prod_on_cell) {
        } else if (c->bits_pending) {
            dep_wait(c, c->st2, c->ev_bits);
        } else {
            stream_dep(c, c->st, c->st2);
        }
        const svdw_mat A[3] = {m, u, v}, B[3] = {vt, ut, vt};
        // per product: the operands' known bits, their device words (b's: v, u, v)
        const int ib[3] = {2, 1, 2};
        const unsigned* sl[3] = {dev_bits, dev_bits ? dev_bits + 1 : nullptr,
                                 dev_bits ? dev_bits + 2 : nullptr};
        if (from_f64) prelaunch_products_f64(c, A, B, log, m.phase, dev_bits, pst);   // (c->bits)
        bool vplanes = false;                            // v's planes built (digB) on this rank
        for (int g = 0; g < 3 && !from_f64; ++g) {
            // shard: rows [r0, r1) of the product only
            uint64_t r0 = 0, r1 = A[g].rows;
            if (sharded(c)) shard_rows(c, A[g].rows, &r0, &r1);
            const svdw_mat Ag = sharded(c) ? row_block(A[g], r0, r1) : A[g];
            Fr* outg = cellp(c, m.phase, log[g] + r0 * B[g].cols);
            // CRT: v's residue planes from m.v^T (covering v.v^T too) serve v.v^T:
            // as both operands unsharded (v.v^T symmetric), as the b operand when
            // the rows are sharded (u's planes go to digC so v's survive)
            const bool shd = sharded(c);
            if (r1 <= r0) {
                // nothing of this product on this rank
            } else if (on_device)
                gemm_exec(c, c->st2, Ag, B[g], outg, ~0u, ~0u, sl[g], sl[ib[g]], dev_quantized,
                          g == 0 ? sl[2] : nullptr, !shd && g == 2,
                          shd && g == 1 ? &c->digC : nullptr, shd && g == 2 && vplanes);
            else
                gemm_exec(c, c->st2, Ag, B[g], outg, known_bits[g], known_bits[ib[g]]);
            if (g == 0 && r1 > r0 && on_device) vplanes = true;
            c->call.pre.push_back({log[g], stream_dep(c, c->st2, nullptr), c->st2});
            c->call.gemm_done.push_back(c->call.pre.back().ev);
        }
        c->call.prelaunched = true;
        host_mark(c, "products queued");
    };
    prelaunch();
    // what goes aside on st2 (d checks, single constant cells) is read by no
    // later kernel: batched until the end of phase 0 (two launches)
    BatchScope aside(c, c->st2);
    if (!c->call.prelaunched) aside.close();
    {
        // The d checks (three latency-bound stages over r elements) depend on d
        // only: with the products queued ahead they go behind them on st2, off
        // the cell stream, which starts on the u / v bounds at once. Pipelined
        // (st2 then carries every stage of the call back to back, st3 phase 1),
        // on the cell stream behind the products, its least loaded stream.
        // (pipelined: where dchk_at puts them; st3 only when it exists)
        const int da = !c->call.in_pipe ? 1 : (c->opt.dchk_at == 2 && !c->st3 ? 1 : c->opt.dchk_at);
        const bool aside_d = c->opt.overlap && known_bits && !c->dry && c->bits_pending && da != 0;
        OnStream sw(c, aside_d ? (da == 2 ? &c->st3 : &c->st2) : nullptr);
        // d loaded -- unless every load these stages (and the bounds and u.d
        // queued behind them with the products on the cell stream) read comes
        // from the registered f64 inputs (f64_view): then st2 starts at once
        const bool from_f64 = c->opt.f64_views && !c->call.f64reg.empty() && c->call.prod_on_cell;
        if (sw.on() && !from_f64) dep_wait(c, c->st, c->ev_bits);
        BatchScope bs(c);                   // (desc_order_range reads desc_order_sub: two launches)
        entries_less_than(c, d, max_bits);
        entries_in_desc_order(c, d, max_bits);
        bs.end();
        host_mark(c, "d checks queued");
    }
    // svd_witness's phase 1 on the third stream, enqueued as soon as the products
    // are (their offsets from the dry replay give the payload): with only the
    // first phase-0 stages queued ahead of it, the third stream starts early
    // instead of after the host has queued all of phase 0.
    auto early_phase1 = [&](int at) {
        const int p1_at = c->opt.p1_at >= 0 ? c->opt.p1_at
                                         : (!sharded(c) ? 1 : (c->opt.shard_world >= 4 ? 0 : 3));
        if (!c->call.early_p1 || p1_at != at || !c->call.prelaunched || c->call.pre.size() != 3) return;
        const svdw_svd_payload pl{ut, vt, svdw_mat{m.phase, N, M, c->call.pre[0].off, (int64_t)M, 1},
                                  svdw_mat{m.phase, N, N, c->call.pre[1].off, (int64_t)N, 1},
                                  svdw_mat{m.phase, M, M, c->call.pre[2].off, (int64_t)M, 1}};
        // the products' bounds (|c_s| < 2^(bits_a + bits_b + lk)) before
        // honest_prover_mat_mul registers them: the c_s scans then size their
        // operand on the device (NaSpec) instead of falling back to full
        // Montgomery products (8-way shard rank: 81 -> 25 us)
        c->wit.prods.push_back({pl.m_times_vt, m, vt, clog2(M)});
        c->wit.prods.push_back({pl.u_times_ut, u, ut, clog2(N)});
        c->wit.prods.push_back({pl.v_times_vt, v, vt, clog2(M)});
        auto f = std::move(c->call.early_p1);
        c->call.early_p1 = nullptr;
        f(pl);
    };
    early_phase1(0);
    // The u, v bounds and u.d read only the loaded matrices: one launch when
    // batched (stage_batch), after which phase 1 is queued (p1_at 1 or 2).
    // With the products on the cell stream they go on st2 instead (behind the
    // d checks, in the same batch), and the cell stream waits for them before
    // the diff, by when they are done.
    const bool pc = c->call.prod_on_cell && c->call.prelaunched;
    OnStream on2(c, pc ? &c->st2 : nullptr);
    BatchScope bs(c);
    const bool batched = bs.mine || pc;
    BigU unit = big_from_u128(((unsigned __int128)1 << P) + 1);
    check_mat_entries_bounded(c, u, unit);
    host_mark(c, "bounds(u) queued");
    if (!batched) early_phase1(1);
    check_mat_entries_bounded(c, v, unit);
    host_mark(c, "bounds(v) queued");
    if (!batched) early_phase1(2);
    DView udv;
    EqCell udpad;
    // products on the cell stream: u.d (all the diff needs from st2) in a launch
    // ahead of the bounds, so the cell stream waits for it alone (pipelined, the
    // diff follows on st2 itself: u.d shares the bounds' launch)
    if (r == M) {
        c->call.stage_front = pc && !c->call.in_pipe;
        const svdw_mat ud = mat_times_diag_mat(c, u, d);
        c->call.stage_front = false;
        udv = view_of(c, ud);
    } else {
        const svdw_vec z = put_cell(c, 0 + u.phase, fr_zero(), true);   // zero padding constant
        udpad = EqCell{(int)z.phase, z.off};
        svdw_mat ud = mat_times_diag_mat(c, u, d);
        udv = view_of(c, ud);
        udv.cols = r;                                     // columns >= N read as 0
    }
    udv.rows = N;
    bs.end();
    on2.end();
    if (pc) {
        // the cell stream waits for u.d (and what precedes it on st2), not for
        // the d checks' dependent second group batched behind it; pipelined,
        // the diff is on st2 itself and st carries the next call: no wait
        flush_batch(c, c->st2, c->call.in_pipe ? nullptr : c->st);
    }
    if (batched) {
        host_mark(c, "bounds(u), bounds(v), u.d queued");
        early_phase1(1);
        early_phase1(2);
    }
    uint32_t bm = ~0u, bu = ~0u, bv = ~0u;
    if (known_bits && c->call.pre.empty()) {                  // products not launched ahead
        fetch_bits(c);
        bm = known_bits[0]; bu = known_bits[1]; bv = known_bits[2];
    }
    // products batched (one completion point): diff and the two ids in one launch;
    // pipelined (c->call.in_pipe), on st2 behind the bounds, so that st is free for
    // the next call's product chain (honest_prover_mat_mul's wait for the
    // products lands on st2)
    const bool dst2 = c->call.in_pipe && pc;
    OnStream on_diff(c, dst2 ? &c->st2 : nullptr);
    BatchScope bs2(c);
    if (!c->call.gemm_batched) bs2.close();
    svdw_mat mvt = honest_prover_mat_mul(c, m.phase, m, vt, bm, bv);
    BigU es = scale_err(err_svd, P), eu = scale_err(err_u, P);
    host_mark(c, "u.d queued");
    check_mat_diff_views(c, m.phase, udv, view_of(c, mvt), N, M, es, nullptr, udpad);
    host_mark(c, "diff queued");
    Fr q = pow2_fr(P);
    const Fr qq = fr_mul(q, q);
    svdw_vec q2 = put_cell(c, m.phase, qq, true);
    svdw_mat uut = honest_prover_mat_mul(c, m.phase, u, ut, bu, bu);
    check_mat_id(c, uut, q2, eu, &qq);
    svdw_mat vvt = honest_prover_mat_mul(c, m.phase, v, vt, bv, bv);
    check_mat_id(c, vvt, q2, eu, &qq);
    bs2.end();
    on_diff.end();
    aside.end();
    host_mark(c, "ids queued");
    return svdw_svd_payload{ut, vt, mvt, uut, vvt};
}
void check_svd_phase1(svdw_ctx* c, const svdw_mat& m, const svdw_mat& u, const svdw_mat& v, const svdw_svd_payload& pl,
                      const Fr& g) {
    const VMul vm[3] = {{m, pl.v_t, pl.m_times_vt}, {u, pl.u_t, pl.u_times_ut},
                        {v, pl.v_t, pl.v_times_vt}};
    verify_mul_many(c, 1, vm, 3, g);
}


// ================================================================== C ABI
extern "C" {

int svdw_reserve(svdw_ctx* c, uint32_t phase, uint64_t na, uint64_t nl) {
    return guarded([&] {
        REQUIRE(c && phase < 2, "bad argument");
        Stream& s = c->ph[phase];
        grow(c, s.adv, s.n, s.cap, na);
        grow(c, s.lk, s.nl, s.lcap, nl);
    });
}

int svdw_zkmatrix_new(svdw_ctx* c, uint32_t phase, const double* data, uint32_t rows,
                      uint32_t cols, int on_device, svdw_mat* out) {
    return guarded([&] {
        REQUIRE(c && out, "null argument");
        *out = zkmatrix_new(c, phase, data, rows, cols, on_device != 0);
    });
}
int svdw_zkvector_new(svdw_ctx* c, uint32_t phase, const double* data, uint32_t len, int on_device,
                      svdw_vec* out) {
    return guarded([&] {
        REQUIRE(c && out, "null argument");
        svdw_mat m = zkmatrix_new(c, phase, data, len, 1, on_device != 0);
        *out = svdw_vec{phase, len, m.off, 1};
    });
}
int svdw_transpose_matrix(const svdw_mat* a, svdw_mat* out) {
    return guarded([&] {
        REQUIRE(a && out, "null argument");
        *out = transposed(*a);
    });
}
int svdw_load_witness(svdw_ctx* c, uint32_t phase, const uint64_t value[4], svdw_vec* out) {
    return guarded([&] {
        REQUIRE(c && value && out, "null argument");
        *out = put_cell(c, phase, fr_from_words(value));
    });
}
int svdw_load_constant(svdw_ctx* c, uint32_t phase, const uint64_t value[4], svdw_vec* out) {
    return guarded([&] {
        REQUIRE(c && value && out, "null argument");
        *out = put_cell(c, phase, fr_from_words(value), true);
    });
}
int svdw_entries_less_than(svdw_ctx* c, const svdw_vec* d, uint32_t max_bits) {
    return guarded([&] {
        REQUIRE(c && d, "null argument");
        check_vec(c, *d);
        run_sized(c, [&](svdw_ctx* x) { entries_less_than(x, *d, max_bits); });
    });
}
int svdw_entries_in_desc_order(svdw_ctx* c, const svdw_vec* d, uint32_t max_bits) {
    return guarded([&] {
        REQUIRE(c && d, "null argument");
        check_vec(c, *d);
        run_sized(c, [&](svdw_ctx* x) { entries_in_desc_order(x, *d, max_bits); });
    });
}
int svdw_check_mat_entries_bounded(svdw_ctx* c, const svdw_mat* a, const uint64_t bnd[4]) {
    return guarded([&] {
        REQUIRE(c && a && bnd, "null argument");
        check_mat(c, *a);
        run_sized(c, [&](svdw_ctx* x) { check_mat_entries_bounded(x, *a, big_from_words(bnd)); });
    });
}
int svdw_check_mat_diff(svdw_ctx* c, const svdw_mat* a, const svdw_mat* b, const uint64_t tol[4]) {
    return guarded([&] {
        REQUIRE(c && a && b && tol, "null argument");
        check_mat(c, *a);
        check_mat(c, *b);
        REQUIRE(a->rows == b->rows && a->cols == b->cols, "check_mat_diff: shape mismatch");
        REQUIRE(a->phase == b->phase, "check_mat_diff: a and b in different phases");
        run_sized(c, [&](svdw_ctx* x) {
            check_mat_diff_views(x, a->phase, view_of(x, *a), view_of(x, *b), a->rows, a->cols,
                                 big_from_words(tol));
        });
    });
}
int svdw_check_mat_id(svdw_ctx* c, const svdw_mat* a, const svdw_vec* sid, const uint64_t tol[4]) {
    return guarded([&] {
        REQUIRE(c && a && sid && tol, "null argument");
        check_mat(c, *a);
        check_vec(c, *sid);
        run_sized(c, [&](svdw_ctx* x) { check_mat_id(x, *a, *sid, big_from_words(tol)); });
    });
}
int svdw_mat_times_diag_mat(svdw_ctx* c, const svdw_mat* a, const svdw_vec* v, svdw_mat* out) {
    return guarded([&] {
        REQUIRE(c && a && v && out, "null argument");
        check_mat(c, *a);
        check_vec(c, *v);
        *out = run_sized(c, [&](svdw_ctx* x) { return mat_times_diag_mat(x, *a, *v); });
    });
}
int svdw_rescale_matrix(svdw_ctx* c, const svdw_mat* cs, const svdw_div_scale* cfg, svdw_mat* out) {
    return guarded([&] {
        REQUIRE(c && cs && out, "null argument");
        check_mat(c, *cs);
        const DivScale d = div_scale_of(c, cfg);
        *out = run_sized(c, [&](svdw_ctx* x) { return rescale_matrix(x, *cs, d); });
    });
}
int svdw_zkvector_inner_product(svdw_ctx* c, uint32_t phase, const svdw_vec* self, const svdw_vec* x,
                                const svdw_div_scale* cfg, svdw_vec* out) {
    return guarded([&] {
        REQUIRE(c && self && x && out, "null argument");
        REQUIRE(phase < 2, "phase must be 0 or 1");
        check_vec(c, *self);
        check_vec(c, *x);
        const DivScale d = div_scale_of(c, cfg);
        *out = run_sized(c, [&](svdw_ctx* y) { return zkvector_inner_product(y, phase, *self, *x, d); });
    });
}
int svdw_zkvector_norm_square(svdw_ctx* c, uint32_t phase, const svdw_vec* self,
                              const svdw_div_scale* cfg, svdw_vec* out) {
    return guarded([&] {
        REQUIRE(c && self && out, "null argument");
        REQUIRE(phase < 2, "phase must be 0 or 1");
        check_vec(c, *self);
        const DivScale d = div_scale_of(c, cfg);
        *out = run_sized(c, [&](svdw_ctx* y) { return zkvector_norm_square(y, phase, *self, d); });
    });
}
int svdw_zkvector_norm(svdw_ctx* c, uint32_t phase, const svdw_vec* self, const svdw_div_scale* cfg,
                       uint32_t sqrt_bits, svdw_vec* out) {
    return guarded([&] {
        REQUIRE(c && self && out, "null argument");
        REQUIRE(phase < 2, "phase must be 0 or 1");
        check_vec(c, *self);
        const DivScale d = div_scale_of(c, cfg);
        *out = run_sized(c, [&](svdw_ctx* x) {
            return qsqrt_vec(x, phase, zkvector_norm_square(x, phase, *self, d), sqrt_bits);
        });
    });
}
int svdw_zkvector_dist(svdw_ctx* c, uint32_t phase, const svdw_vec* self, const svdw_vec* x,
                       const svdw_div_scale* cfg, uint32_t sqrt_bits, svdw_vec* out) {
    return guarded([&] {
        REQUIRE(c && self && x && out, "null argument");
        REQUIRE(phase < 2, "phase must be 0 or 1");
        check_vec(c, *self);
        check_vec(c, *x);
        const DivScale d = div_scale_of(c, cfg);
        *out = run_sized(c, [&](svdw_ctx* y) {
            return qsqrt_vec(y, phase, zkvector_dist_square(y, phase, *self, *x, d), sqrt_bits);
        });
    });
}
int svdw_zkvector_dist_square(svdw_ctx* c, uint32_t phase, const svdw_vec* self, const svdw_vec* x,
                              const svdw_div_scale* cfg, svdw_vec* out) {
    return guarded([&] {
        REQUIRE(c && self && x && out, "null argument");
        REQUIRE(phase < 2, "phase must be 0 or 1");
        check_vec(c, *self);
        check_vec(c, *x);
        const DivScale d = div_scale_of(c, cfg);
        *out = run_sized(c, [&](svdw_ctx* y) { return zkvector_dist_square(y, phase, *self, *x, d); });
    });
}
int svdw_zkvector_mul(svdw_ctx* c, uint32_t phase, const svdw_vec* self, const svdw_mat* a,
                      const svdw_div_scale* cfg, svdw_vec* out) {
    return guarded([&] {
        REQUIRE(c && self && a && out, "null argument");
        REQUIRE(phase < 2, "phase must be 0 or 1");
        check_vec(c, *self);
        check_mat(c, *a);
        const DivScale d = div_scale_of(c, cfg);
        *out = run_sized(c, [&](svdw_ctx* y) { return zkvector_mul(y, phase, *self, *a, d); });
    });
}
int svdw_honest_prover_mat_mul(svdw_ctx* c, uint32_t phase, const svdw_mat* a, const svdw_mat* b,
                               svdw_mat* out) {
    return guarded([&] {
        REQUIRE(c && a && b && out, "null argument");
        check_mat(c, *a);
        check_mat(c, *b);
        struct Solo {                        // a product queued on its own: the persistent GEMM
            svdw_ctx* c;
            ~Solo() { c->gemm_solo = false; }
        } solo{c};
        c->gemm_solo = true;
        *out = honest_prover_mat_mul(c, phase, *a, *b);
    });
}
int svdw_field_mat_vec_mul(svdw_ctx* c, uint32_t phase, const svdw_mat* a, const svdw_vec* v,
                           svdw_vec* out) {
    return guarded([&] {
        REQUIRE(c && a && v && out, "null argument");
        check_mat(c, *a);
        check_vec(c, *v);
        *out = run_sized(c, [&](svdw_ctx* x) { return field_mat_vec_mul(x, phase, *a, *v); });
    });
}
int svdw_verify_mul(svdw_ctx* c, uint32_t phase, const svdw_mat* a, const svdw_mat* b,
                    const svdw_mat* cs, const uint64_t gamma[4]) {
    return guarded([&] {
        REQUIRE(c && a && b && cs && gamma, "null argument");
        check_mat(c, *a);
        check_mat(c, *b);
        check_mat(c, *cs);
        const VMul v{*a, *b, *cs};
        run_sized(c, [&](svdw_ctx* x) { verify_mul_many(x, phase, &v, 1, fr_from_words(gamma)); });
    });
}
int svdw_err_calc(uint32_t p, uint64_t size, double max_norm, double eps_svd, double eps_u,
                  double* es, double* eu) {
    return guarded([&] {
        REQUIRE(es && eu, "null argument");
        err_calc(p, size, max_norm, eps_svd, eps_u, es, eu);
    });
}
int svdw_check_svd_phase0(svdw_ctx* c, const svdw_mat* m, const svdw_mat* u, const svdw_mat* v,
                          const svdw_vec* d, double err_svd, double err_u, uint32_t max_bits_d,
                          svdw_svd_payload* out) {
    return guarded([&] {
        REQUIRE(c && m && u && v && d && out, "null argument");
        check_mat(c, *m); check_mat(c, *u); check_mat(c, *v); check_vec(c, *d);
        REQUIRE(m->phase == 0 && u->phase == 0 && v->phase == 0 && d->phase == 0,
                "check_svd_phase0 inputs must live in phase 0");
        *out = run_sized(c, [&](svdw_ctx* x) {
            return check_svd_phase0(x, *m, *u, *v, *d, err_svd, err_u, max_bits_d);
        });
    });
}
int svdw_check_svd_phase1(svdw_ctx* c, const svdw_mat* m, const svdw_mat* u, const svdw_mat* v,
                          const svdw_svd_payload* pl, const uint64_t gamma[4]) {
    return guarded([&] {
        REQUIRE(c && m && u && v && pl && gamma, "null argument");
        run_sized(c, [&](svdw_ctx* x) { check_svd_phase1(x, *m, *u, *v, *pl, fr_from_words(gamma)); });
    });
}

}  // extern "C"
