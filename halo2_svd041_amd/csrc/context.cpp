// The context apart from the witness engine (engine.cpp, witness.cpp): its lifetime and
// device memory, the two lanes, options, the hand-off with a caller's stream,
// completion marks, the event profiler, and the C ABI entries of these.
#include <stdlib.h>

#include "engine_internal.hpp"
#include "gemm.hpp"                                         // set_debug_trace, for svdw_debug_trace
#include "commit.hpp"                                       // kCommitMaxBits, for the "commit_window_bits" option

void sync(svdw_ctx* c) {
    if (c->dry) return;
    REQUIRE(!c->vmg.capturing, "internal: synchronisation during graph capture");
    hipck(hipStreamSynchronize(c->st), "hipStreamSynchronize");
    hipck(hipStreamSynchronize(c->st2), "hipStreamSynchronize");
    if (c->st3) hipck(hipStreamSynchronize(c->st3), "hipStreamSynchronize");
    c->tail_pending = false;
    if (c->lane) sync(c->lane);
}
// After a pipelined svd_witness its tail (st2, st3) is not joined into st:
// anything else queued on the context waits for it first.
void settle(svdw_ctx* c) {
    if (c->dry || !c->tail_pending || c->call.in_pipe) return;
    for (int k = 0; k < 2; ++k)
        hipck(hipStreamWaitEvent(c->st, c->tail_ev[c->tail_last][k], 0), "hipStreamWaitEvent");
    c->tail_pending = false;
}
// Free the pipeline's other cell set (after the work that may read it).
void release_alt(svdw_ctx* c) {
    if (c->dry || set_bytes(c->alt) == 0) return;
    sync(c);
    for (auto& s : c->alt) {
        if (s.adv) hipck(hipFree(s.adv), "hipFree");
        if (s.lk) hipck(hipFree(s.lk), "hipFree");
        s = Stream{};
    }
    ++c->epoch;
}
void clear_streams(svdw_ctx* c) {
    c->wit.clear();
    c->owned.clear();
    c->phys.valid = false;
    c->bits_pending = false;
    for (auto& s : c->ph) { s.n = 0; s.nl = 0; }
}
void ensure_buf(svdw_ctx* c, DBuf& b, size_t bytes) {
    if (c->dry || b.cap >= bytes) return;
    REQUIRE(!c->vmg.capturing, "internal: allocation during graph capture");
    ++c->epoch;
    sync(c);
    if (b.p) hipck(hipFree(b.p), "hipFree");
    b.p = nullptr;
    size_t cap = std::max(bytes, b.cap + b.cap / 2);
    if (hipMalloc(&b.p, cap) != hipSuccess) {
        b.cap = 0;
        fail(SVDW_ENOMEM, "device allocation failed (scratch)");
    }
    b.cap = cap;
}
// Every scratch buffer of a state (release, footprint).
static std::vector<DBuf*> dbufs(svdw_ctx* c) {
    std::vector<DBuf*> v = {&c->f64in, &c->digA, &c->digB, &c->digC, &c->w1c, &c->w1t, &c->w2c, &c->w2t, &c->bits,
                            &c->gpc, &c->gtab, &c->gpc_alt, &c->gtab_alt, &c->crtR, &c->gbits, &c->colpart, &c->qfold,
                            &c->staging.buf};
    for (DBuf* d : c->circuit.dbufs()) v.push_back(d);
    for (DBuf* d : c->prover.dbufs()) v.push_back(d);
    for (DBuf* d : c->srs.dbufs()) v.push_back(d);
    for (DBuf* d : c->g1fft.dbufs()) v.push_back(d);
    for (DBuf* d : c->svd.dbufs()) v.push_back(d);
    for (DBuf* d : c->exp.dbufs()) v.push_back(d);
    for (DBuf* d : c->ingest.dbufs()) v.push_back(d);
    for (int i = 0; i < kMaxScanJobs; ++i) {
        v.push_back(&c->wbc[i]);
        v.push_back(&c->wbt[i]);
        v.push_back(&c->bvfull[i]);
    }
    return v;
}
// Device bytes a state holds (cell sets and scratch).
static double state_bytes(svdw_ctx* c) {
    double b = set_bytes(c->ph) + set_bytes(c->alt);
    for (DBuf* d : dbufs(c)) b += (double)d->cap;
    return b;
}
// Every device object is released on its own (a state whose creation failed
// part-way holds some of them only).
static void ctx_release(svdw_ctx* c) {
    if (!c) return;
    if (c->lane) ctx_release(c->lane);
    if (!c->dry) {
        for (hipStream_t t : {c->st_cell ? c->st_cell : c->st, c->st2, c->st3})
            if (t) (void)hipStreamSynchronize(t);
        vmg_drop(c);
        for (auto& s : c->ph) { (void)hipFree(s.adv); (void)hipFree(s.lk); }
        for (auto& s : c->alt) { (void)hipFree(s.adv); (void)hipFree(s.lk); }
        for (auto& t : c->tail_ev)
            for (auto e : t)
                if (e) (void)hipEventDestroy(e);
        for (DBuf* b : dbufs(c))
            if (b->p) (void)hipFree(b->p);
        if (c->hbits) (void)hipHostFree(c->hbits);
        if (c->svd.pinned) (void)hipHostFree(c->svd.pinned);
        if (c->ev_bits) (void)hipEventDestroy(c->ev_bits);
        for (auto e : c->xev)
            if (e) (void)hipEventDestroy(e);
        for (auto e : c->exp.ev)
            if (e) (void)hipEventDestroy(e);
        for (auto& m : c->mk.ev)
            for (auto e : m)
                if (e) (void)hipEventDestroy(e);
        for (auto& r : c->recs) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
        for (auto e : c->pool) (void)hipEventDestroy(e);
        for (auto e : c->deps) (void)hipEventDestroy(e);
        if (c->lin_ev) (void)hipEventDestroy(c->lin_ev);
        for (hipStream_t t : {c->st3, c->st2, c->st_cell ? c->st_cell : c->st})
            if (t) (void)hipStreamDestroy(t);
    }
    delete c;
}
// "lanes": may the next verify_mul_witness run on the other state? Yes when
// that state already holds as much device memory as this one (the calls have
// one shape), or when its growth to this one's footprint fits in free memory
// with 10 % of the device to spare; else the call stays on this state.
bool lane_fits(svdw_ctx* c) {
    const double need = state_bytes(c) - (c->lane ? state_bytes(c->lane) : 0.0);
    if (need <= 0) return true;
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) != hipSuccess) return false;
    return need + 0.1 * (double)tot <= (double)fr;
}
// Device state of a new context: its three streams, the pinned bit words, events.
static void ctx_init_device(svdw_ctx* c) {
    hipError_t e = hipSetDevice(c->device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->st, hipStreamNonBlocking);
    c->st_cell = c->st;
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->st2, hipStreamNonBlocking);
    // the third stream exists from the start: one created lazily inside a
    // call would not wait for what st already waits for (svdw_stream_wait)
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->st3, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipHostMalloc((void**)&c->hbits, 64 * sizeof(uint32_t), hipHostMallocDefault);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_bits, hipEventDisableTiming | hipEventReleaseToDevice);
    for (int k = 0; k < 4 && e == hipSuccess; ++k)
        e = hipEventCreateWithFlags(&c->tail_ev[k / 2][k % 2], hipEventDisableTiming | hipEventReleaseToDevice);
    c->stream_id[0] = c->st;
    c->stream_id[1] = c->st2;
    c->stream_id[2] = c->st3;
    size_t mfree = 0;
    if (e == hipSuccess) e = hipMemGetInfo(&mfree, &c->mem_total);
    if (e != hipSuccess) fail(SVDW_EDEVICE, std::string("HIP device init failed: ") + hipGetErrorString(e));
}
// The settings (options, shard, profiler) of `s` onto the lane `d`; a change
// bumps the lane's epoch (its captured graph no longer applies).
static void copy_settings(svdw_ctx* d, const svdw_ctx* s) {
    if (d->opt == s->opt) return;
    d->opt = s->opt;
    ++d->epoch;
}
// svdw_set_option's names: a value in [lo, hi] (else SVDW_EINVAL with `msg`)
// goes to `set` (a bool member takes value != 0).
struct OptionDef {
    const char* name;
    int64_t lo, hi;
    const char* msg;
    void (*set)(svdw_ctx*, int64_t);
};
template <auto Member>
static void set_opt(svdw_ctx* c, int64_t v) {
    c->opt.*Member = static_cast<std::remove_reference_t<decltype(c->opt.*Member)>>(v);
}
static void set_lanes(svdw_ctx* c, int64_t v) { c->lanes = (int)v; }   // (the handle's, not the state's)
static void set_pipeline(svdw_ctx* c, int64_t v) {
    c->opt.pipeline = (int)v;
    if (!v) {                                        // the other cell set is not needed any more
        release_alt(c);
        if (c->lane) release_alt(c->lane);
    }
}
static void set_stage_rot(svdw_ctx* c, int64_t v) {
    c->opt.stage_flags = v ? (c->opt.stage_flags | STAGE_ROT) : (c->opt.stage_flags & ~STAGE_ROT);
}
static const char kStageElemsMsg[] = "stage_elems: a multiple of 16 in [16, 256]";
static void set_stage_elems(svdw_ctx* c, int64_t v) {
    REQUIRE(v % 16 == 0, kStageElemsMsg);
    c->opt.stage_elems = (uint32_t)v;
}
static void set_commit_window_bits(svdw_ctx* c, int64_t v) {
    REQUIRE(v != 1, "commit_window_bits: 0 (the plan) or 2..16");
    c->opt.commit_window_bits = (uint32_t)v;
}
static void set_g1_window_bits(svdw_ctx* c, int64_t v) {
    REQUIRE(v != 1, "g1_window_bits: 0 (the plan) or 2..6");
    c->opt.g1_window_bits = (uint32_t)v;
}
using Opt = svdw_ctx::Options;
static const OptionDef kOptions[] = {
    {"lanes", 1, 2, "lanes: 1 or 2", set_lanes},   // verify_mul_witness on two alternating states
    {"pipeline", 0, 1, "pipeline: 0 or 1", set_pipeline},   // pipelined svd_witness (svd_witness)
    {"vm_linear", 0, 1, "vm_linear: 0 or 1", set_opt<&Opt::vm_linear>},   // captured verify_mul_witness on one stream
    {"graph", 0, 1, "graph: 0 or 1", set_opt<&Opt::graph_vm>},   // captured verify_mul_witness (vm_graph)
    {"gemm_impl", SVDW_GEMM_MFMA, SVDW_GEMM_VALU, "gemm_impl: 0 (mfma) or 1 (valu)", set_opt<&Opt::gemm_impl>},
    {"stage_elems", 16, 256, kStageElemsMsg, set_stage_elems},
    {"prod_cell", -1, 1, "prod_cell: -1, 0 or 1", set_opt<&Opt::prod_cell>},
    {"phase1_overlap", 0, 2, "phase1_overlap: 0, 1 or 2", set_opt<&Opt::phase1_overlap>},
    {"hold_us", 0, 100000, "hold_us: 0..100000", set_opt<&Opt::hold_us>},   // timing aid: GPU-only schedule of a witness
    {"rlc_prefix", INT64_MIN, INT64_MAX, "", set_opt<&Opt::rlc_prefix>},
    {"res_f64", INT64_MIN, INT64_MAX, "", set_opt<&Opt::res_f64>},
    {"gemm_crt", 0, 1, "gemm_crt: 0 or 1", set_opt<&Opt::gemm_crt>},
    {"res_wait", -1, 1, "res_wait: -1 (auto), 0 or 1", set_opt<&Opt::res_wait>},   // pipelined: st2 waits for the residue planes
    {"place_trials", 0, 8, "place_trials: 0..8", set_opt<&Opt::place_trials>},   // cell streams >= 256 MiB: best of this many placements
    {"stage_rot", 0, 1, "stage_rot: 0 or 1", set_stage_rot},   // phase B from a block-dependent window on
    {"gemm_kern", -1, 2, "gemm_kern: -1 (auto), 0, 1 or 2", set_opt<&Opt::gemm_kern>},   // CRT GEMM kernel variant (bit-identical)
    {"stage_batch", INT64_MIN, INT64_MAX, "", set_opt<&Opt::stage_batch>},   // small independent stages share k_stage_multi launches
    {"f64_views", INT64_MIN, INT64_MAX, "", set_opt<&Opt::f64_views>},
    {"p1_at", -1, 3, "p1_at: -1 (auto), 0, 1, 2 or 3", set_opt<&Opt::p1_at>},
    {"commit_window_bits", 0, kCommitMaxBits, "commit_window_bits: 0 (the plan) or 2..16", set_commit_window_bits},
    {"g1_window_bits", 0, 6, "g1_window_bits: 0 (the plan) or 2..6", set_g1_window_bits},
    {"commit_scratch_mib", 1, 65536, "commit_scratch_mib: 1..65536", set_opt<&Opt::commit_scratch_mib>},
    {"srs_chunk_rows", 0, 1 << 28, "srs_chunk_rows: 0 (what fits commit_scratch_mib) or 1..2^28", set_opt<&Opt::srs_chunk_rows>},
    {"dchk_at", 0, 2, "dchk_at: 0 (cell stream), 1 (st2) or 2 (st3)", set_opt<&Opt::dchk_at>},   // pipelined: the d checks' stream
    {"gamma_at", -1, 1, "gamma_at: -1 (auto), 0 (cell stream) or 1 (st3)", set_opt<&Opt::gamma_at>},   // pipelined: k_gamma_prep's stream
    {"overlap", INT64_MIN, INT64_MAX, "", set_opt<&Opt::overlap>},
};
// "lanes": exchange this state with the lane's (created on first use).
static_assert(std::is_nothrow_move_constructible<svdw_ctx>::value && std::is_nothrow_move_assignable<svdw_ctx>::value, "svdw_ctx moves");
void lane_switch(svdw_ctx* c) {
    if (!c->lane) {
        svdw_ctx* L = new svdw_ctx();
        L->P = c->P;
        L->LB = c->LB;
        L->device = c->device;
        L->dry = false;
        try {
            ctx_init_device(L);
        } catch (...) {
            ctx_release(L);
            throw;
        }
        c->lane = L;
    }
    svdw_ctx* L = c->lane;
    copy_settings(L, c);
    std::swap(*c, *L);
    std::swap(c->lane, L->lane);                  // (the handle keeps the lane and the option)
    std::swap(c->lanes, L->lanes);
    std::swap(c->mk, L->mk);
}
hipEvent_t xevent(svdw_ctx* c, int i) {
    if (!c->xev[i])
        hipck(hipEventCreateWithFlags(&c->xev[i], hipEventDisableTiming), "hipEventCreate");
    return c->xev[i];
}
// f(x, t, k) for every stream t of the handle's state and of its lane's: x the
// state, k the stream's place among that state's.
template <class F>
static void each_stream(svdw_ctx* c, F&& f) {
    for (svdw_ctx* x : {c, c->lane}) {
        if (!x) continue;
        int k = 0;
        for (hipStream_t t : {x->st, x->st2, x->st3})
            if (t) f(x, t, k++);
    }
}

extern "C" {

const char* svdw_last_error(void) { return g_err.c_str(); }

int svdw_ctx_create(const svdw_params* p, svdw_ctx** out) {
    return guarded([&] {
        REQUIRE(p && out, "null argument");
        if (p->precision_bits < 1 || p->precision_bits > 63)
            fail(SVDW_ERANGE, "precision_bits must be in [1, 63] (src/svd/mod.rs:74 uses u64)");
        if (p->lookup_bits < 8 || p->lookup_bits > 63)
            fail(SVDW_ERANGE, "lookup_bits must be in [8, 63]");
        svdw_ctx* c = new svdw_ctx();
        c->P = p->precision_bits;
        c->LB = p->lookup_bits;
        c->device = p->device;
        c->dry = p->device < 0;
        if (const char* h = getenv("SVDW_HOST_TRACE")) c->opt.host_trace = atoi(h) != 0;
        if (const char* g = getenv("SVDW_GEMM"))
            c->opt.gemm_impl = (!strcmp(g, "valu") || !strcmp(g, "dot4")) ? SVDW_GEMM_VALU : SVDW_GEMM_MFMA;
        if (!c->dry) {
            try {
                ctx_init_device(c);
            } catch (...) {
                ctx_release(c);
                throw;
            }
        }
        *out = c;
    });
}
int svdw_ctx_destroy(svdw_ctx* c) {
    return guarded([&] { ctx_release(c); });
}
int svdw_ctx_reset(svdw_ctx* c) {
    return guarded([&] {
        REQUIRE(c, "null ctx");
        sync(c);
        clear_streams(c);
        c->call.reset();
    });
}
// Stream-ordered hand-off with a caller's stream (e.g. torch's current stream):
// the context's streams wait for the work queued on `s` so far (inputs it is
// still writing, buffers it still reads), and `s` waits for the context's
// queued work (outputs it will read). No host wait either way.
// st waits at once; st2 / st3 inherit the wait from st where a call orders them
// after it, else wait themselves (xwait_side). With lanes, the lane's state too
// (the next verify_mul_witness runs there).
int svdw_stream_wait(svdw_ctx* c, void* stream) {
    return guarded([&] {
        REQUIRE(c, "null ctx");
        if (c->dry) return;
        const hipStream_t s = (hipStream_t)stream;
        const hipEvent_t e = xevent(c, 0);
        hipck(hipEventRecord(e, s), "hipEventRecord");
        for (svdw_ctx* x : {c, c->lane}) {
            if (!x) continue;
            hipck(hipStreamWaitEvent(x->st, e, 0), "hipStreamWaitEvent");
            x->xwait_side = e;
        }
    });
}
int svdw_stream_signal(svdw_ctx* c, void* stream) {
    return guarded([&] {
        REQUIRE(c, "null ctx");
        if (c->dry) return;
        const hipStream_t s = (hipStream_t)stream;
        each_stream(c, [&](svdw_ctx* x, hipStream_t t, int k) {
            flush_batch(x, t);
            const hipEvent_t e = xevent(x, 1 + k);
            hipck(hipEventRecord(e, t), "hipEventRecord");
            hipck(hipStreamWaitEvent(s, e, 0), "hipStreamWaitEvent");
        });
    });
}
int svdw_debug_trace(void* buf) {
    return guarded([&] { hipck(set_debug_trace(buf), "set_debug_trace"); });
}
int svdw_sync(svdw_ctx* c) {
    return guarded([&] { REQUIRE(c, "null ctx"); sync(c); });
}
// 1 when every launch queued on the context (both lanes) has completed, 0
// while some still runs; no host wait (hipStreamQuery).
int svdw_query(svdw_ctx* c) {
    int done = 1;
    const int rc = guarded([&] {
        REQUIRE(c, "null ctx");
        if (c->dry) return;
        each_stream(c, [&](svdw_ctx*, hipStream_t t, int) {
            if (!done) return;                      // (one busy stream answers the query)
            const hipError_t e = hipStreamQuery(t);
            if (e == hipErrorNotReady) {
                done = 0;
                return;
            }
            hipck(e, "hipStreamQuery");
        });
    });
    return rc ? rc : done;
}
// Completion marks (svdw_mark / svdw_mark_done / svdw_mark_wait): an event on
// each stream of both lanes, recorded behind what is queued there (pending
// batched stages launched first), so no stream waits for anything. A slot is
// reused 16 marks later; a ticket whose slot holds a later mark is answered
// by that mark (later done implies earlier done; not done reads as 0).
int svdw_mark(svdw_ctx* c, uint64_t* ticket) {
    return guarded([&] {
        REQUIRE(c && ticket, "null argument");
        const uint64_t t = ++c->mk.seq;
        *ticket = t;
        if (c->dry) return;
        const int k = (int)(t % svdw_ctx::kMarks);
        int i = 0;
        each_stream(c, [&](svdw_ctx* x, hipStream_t st, int) {
            flush_batch(x, st);
            hipEvent_t& e = c->mk.ev[k][i++];
            if (!e) hipck(hipEventCreateWithFlags(&e, hipEventDisableTiming), "hipEventCreate");
            hipck(hipEventRecord(e, st), "hipEventRecord");
        });
        c->mk.used[k] = (uint8_t)i;
        c->mk.t[k] = t;
    });
}
// the slot answering ticket t, or -1 (t not issued)
static int mark_slot(const svdw_ctx* c, uint64_t t) {
    if (!t || t > c->mk.seq) return -1;
    return (int)(t % svdw_ctx::kMarks);
}
int svdw_mark_done(svdw_ctx* c, uint64_t ticket) {
    int done = 1;
    const int rc = guarded([&] {
        REQUIRE(c, "null ctx");
        const int k = mark_slot(c, ticket);
        REQUIRE(k >= 0, "svdw_mark_done: ticket not issued");
        if (c->dry) return;
        for (int i = 0; i < c->mk.used[k]; ++i) {
            const hipError_t e = hipEventQuery(c->mk.ev[k][i]);
            if (e == hipErrorNotReady) {
                done = 0;
                return;
            }
            hipck(e, "hipEventQuery");
        }
    });
    return rc ? rc : done;
}
int svdw_mark_wait(svdw_ctx* c, uint64_t ticket) {
    return guarded([&] {
        REQUIRE(c, "null ctx");
        const int k = mark_slot(c, ticket);
        REQUIRE(k >= 0, "svdw_mark_wait: ticket not issued");
        if (c->dry) return;
        for (int i = 0; i < c->mk.used[k]; ++i) hipck(hipEventSynchronize(c->mk.ev[k][i]), "hipEventSynchronize");
    });
}
uint64_t svdw_advice_len(const svdw_ctx* c, uint32_t phase) { return c && phase < 2 ? c->ph[phase].n : 0; }
uint64_t svdw_lookup_len(const svdw_ctx* c, uint32_t phase) { return c && phase < 2 ? c->ph[phase].nl : 0; }
const void* svdw_advice_device_ptr(const svdw_ctx* c, uint32_t phase) { return c && phase < 2 ? c->ph[phase].adv : nullptr; }
const void* svdw_lookup_device_ptr(const svdw_ctx* c, uint32_t phase) { return c && phase < 2 ? c->ph[phase].lk : nullptr; }

int svdw_set_shard(svdw_ctx* c, uint32_t rank, uint32_t world) {
    return guarded([&] {
        REQUIRE(c, "null ctx");
        REQUIRE(world >= 1 && rank < world, "svdw_set_shard: need rank < world");
        ++c->epoch;
        c->opt.shard_rank = rank;
        c->opt.shard_world = world;
        c->owned.clear();
    });
}
int svdw_abi_version(void) { return SVDW_ABI_VERSION; }
int svdw_set_option(svdw_ctx* c, const char* name, int64_t value) {
    return guarded([&] {
        REQUIRE(c && name, "null argument");
        sync(c);
        ++c->epoch;                                  // a captured launch sequence may change
        for (const OptionDef& o : kOptions)
            if (!strcmp(o.name, name)) {
                REQUIRE(value >= o.lo && value <= o.hi, o.msg);
                return o.set(c, value);
            }
        fail(SVDW_EINVAL, std::string("unknown option ") + name);
    });
}
int svdw_graph_stats(svdw_ctx* c, uint64_t* captures, uint64_t* replays) {
    return guarded([&] {
        REQUIRE(c && captures && replays, "null argument");
        *captures = c->vmg.captures + (c->lane ? c->lane->vmg.captures : 0);
        *replays = c->vmg.replays + (c->lane ? c->lane->vmg.replays : 0);
    });
}
int svdw_set_gemm_impl(svdw_ctx* c, int impl) {
    return guarded([&] {
        REQUIRE(c, "null ctx");
        REQUIRE(impl == SVDW_GEMM_MFMA || impl == SVDW_GEMM_VALU, "unknown GEMM implementation");
        sync(c);
        ++c->epoch;
        c->opt.gemm_impl = impl;
    });
}
int svdw_profile_enable(svdw_ctx* c, int on) {
    return guarded([&] {
        REQUIRE(c, "null ctx");
        sync(c);
        for (auto& r : c->recs) { c->pool.push_back(r.e0); c->pool.push_back(r.e1); }
        c->recs.clear();
        c->opt.prof = on != 0;
    });
}
int svdw_profile_filter(svdw_ctx* c, const char* prefix) {
    return guarded([&] {
        REQUIRE(c, "null ctx");
        c->opt.prof_filter = prefix ? prefix : "";
    });
}
int svdw_profile_collect(svdw_ctx* c, svdw_kstat* out, uint32_t cap, uint32_t* n) {
    return guarded([&] {
        REQUIRE(c && n, "null argument");
        sync(c);
        std::vector<svdw_kstat> agg;
        for (auto& r : c->recs) {
            float ms = 0;
            hipck(hipEventElapsedTime(&ms, r.e0, r.e1), "hipEventElapsedTime");
            svdw_kstat* s = nullptr;
            for (auto& x : agg)
                if (r.name == x.name) s = &x;
            if (!s) {
                agg.emplace_back();
                s = &agg.back();
                memset(s, 0, sizeof(*s));
                snprintf(s->name, sizeof(s->name), "%s", r.name.c_str());
            }
            s->launches += 1;
            s->total_ms += ms;
            s->bytes += r.bytes;
            s->ops += r.ops;
            if (ms > s->max_ms) s->max_ms = ms;
            c->pool.push_back(r.e0);
            c->pool.push_back(r.e1);
        }
        c->recs.clear();
        *n = (uint32_t)agg.size();
        if (out)
            for (uint32_t i = 0; i < agg.size() && i < cap; ++i) out[i] = agg[i];
    });
}

}  // extern "C"
