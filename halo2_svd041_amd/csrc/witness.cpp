// The two witness calls, svd_witness and verify_mul_witness, on the engine
// (engine.cpp): what they share (the planned stream sizes, the opening and end
// of a call, the input loader), the calls, the captured graph of
// verify_mul_witness, and their C ABI entries with svdw_plan_svd.
#include "engine_internal.hpp"

// The bit-length words out[0 .. nred) folded inside the quantize launch
// (BitFold) when its first nred segments carry block maxima laid out back to
// back from qs.blockmax[0]; else k_bits_reduce over `seg`, a launch of its own.
static void bits_words(svdw_ctx* c, QuantSegs& qs, uint32_t nred, const BitSegs& seg, unsigned* out,
                       bool* folded) {
    *folded = false;
    if (c->dry || !qs.nseg || qs.nseg < nred || nred > 3) return;
    for (uint32_t s = 0; s < nred; ++s)
        if (qs.blockmax[s] != qs.blockmax[0] + qs.blk0[s] || qs.blk0[s] != seg.begin[s]) return;
    const uint32_t nblk = qs.blk0[nred];
    if (!c->qfold.p) {
        ensure_buf(c, c->qfold, 256);
        // the counters start at zero, before the quantize launch on st (a
        // null-stream hipMemset is not ordered against it)
        hipck(hipMemsetAsync(c->qfold.p, 0, c->qfold.cap, c->st), "hipMemsetAsync");
    }
    BitFold& f = qs.fold;
    f.bm = qs.blockmax[0];
    f.cnt = (unsigned*)c->qfold.p;
    f.wout = out;
    f.nblk = nblk;
    f.nred = nred;
    for (uint32_t s = 0; s <= nred; ++s) f.b[s] = qs.blk0[s];
    *folded = true;
}
// Exact cell stream sizes of a witness call from a dry replay of it (planner:
// the call on a fresh planning context), cached by key: no growth copies
// inside the step. grow_to_plan sizes the current cell set to them.
template <class F>
static void plan_sizes(svdw_ctx* c, const std::vector<uint64_t>& key, F&& planner) {
    if (key == c->plan_key) return;
    PlanCtx plan(c->P, c->LB);
    planner(&plan);
    c->plan_key = key;
    c->plan_val = {plan.ph[0].n, plan.ph[0].nl, plan.ph[1].n, plan.ph[1].nl};
}
static void grow_to_plan(svdw_ctx* c) {
    for (int p = 0; p < 2; ++p) {
        grow(c, c->ph[p].adv, 0, c->ph[p].cap, c->plan_val[2 * p]);
        grow(c, c->ph[p].lk, 0, c->ph[p].lcap, c->plan_val[2 * p + 1]);
    }
}
// The opening of a witness call: empty streams, and the call's state reset to
// what both witness functions start from (clear(), never a fresh vector: the
// 256^2 verify_mul_witness is host-bound, an allocation per call would show).
static void begin_call(svdw_ctx* c, const char* what) {
    c->ht0 = std::chrono::steady_clock::now();
    host_mark(c, what);
    clear_streams(c);
    c->dep_next = 0;
    c->call.reset();
}
// A witness call's side streams start after everything queued on st (the
// previous call's work joins st at its end): without this, the next call's
// gamma tables (st3) and first stages (st2, f64 views need no load) could
// overwrite buffers the previous call's kernels still read.
static void after_previous(svdw_ctx* c) {
    if (c->dry) return;
    const hipEvent_t e = stream_dep(c, c->st, c->st2);
    if (c->st3) dep_wait(c, c->st3, e);
    c->xwait_side = nullptr;                      // (st waited for the caller's stream)
}
// "hold_us": every stream of the step waits for st's hold (st2's first stages
// need no load with f64 views)
static void hold_step(svdw_ctx* c) {
    if (c->dry || !c->opt.hold_us) return;
    hipck(launch_hold(c->opt.hold_us, c->st), "k_hold");
    stream_dep(c, c->st, c->st3);
    stream_dep(c, c->st, c->st2);
}
static svdw_counts counts_of(const svdw_ctx* c) {
    return svdw_counts{c->ph[0].n, c->ph[1].n, c->ph[0].nl, c->ph[1].nl};
}
// One f64 input of a witness call: zkmatrix_new's arguments, and whether it
// gets a bit-length word.
struct WitInput { const double* data; uint32_t rows, cols; bool word, own_rows_only, own_rows_cols; };
// Loads the n <= 4 inputs of a witness call into phase 0 (out[i]: their
// matrices), device inputs quantized in one k_quantize_multi launch. The inputs
// with a word get the bit-length words at place(blocks) in their order: called
// once on a device context with the block count of them all, it returns where
// the words lie ([0, 64) the words, from 64 on the per-block maxima). Leaves the
// record's device words (wit.dbitw, wit.dwords) and the call's registered f64
// regions; returns how many inputs went into the one launch.
template <class Place>
static uint32_t load_inputs(svdw_ctx* c, const WitInput* in, int n, bool on_device, Place&& place, svdw_mat* out) {
    uint64_t count[4], total = 0;                         // values quantized: of m on a row-sharded rank, its rows'
    double bytes = 0;
    for (int i = 0; i < n; ++i) {
        uint64_t r0 = 0, r1 = in[i].rows;
        if (in[i].own_rows_only && sharded(c) && on_device) shard_rows(c, in[i].rows, &r0, &r1);
        total += count[i] = (r1 - r0) * in[i].cols;
        bytes += 40.0 * ((double)in[i].rows * in[i].cols);
    }
    // (host inputs go through launch_quantize, kQuantPerBlock values per block)
    QuantSegs qs;
    memset(&qs, 0, sizeof qs);
    qs.per_block = on_device ? quant_per_block(total) : kQuantPerBlock;
    BitSegs seg{};
    uint32_t nred = 0;
    for (int i = 0; i < n; ++i)
        if (in[i].word) {
            seg.begin[nred + 1] = seg.begin[nred] + (uint32_t)((count[i] + qs.per_block - 1) / qs.per_block);
            ++nred;
        }
    unsigned* dbits = c->dry ? nullptr : place((size_t)seg.begin[nred]);
    c->wit.dwords.clear();
    for (int i = 0, w = 0; i < n; ++i) {
        unsigned* blockmax = dbits && in[i].word ? dbits + 64 + seg.begin[w] : nullptr;
        out[i] = zkmatrix_new(c, 0, in[i].data, in[i].rows, in[i].cols, on_device, blockmax, &qs, in[i].own_rows_only,
                              in[i].own_rows_cols);
        if (dbits && in[i].word) c->wit.dwords.push_back({out[i], (int16_t)w});
        if (on_device && !c->dry)
            c->call.f64reg.push_back({out[i].phase, out[i].off, (uint64_t)in[i].rows * in[i].cols, in[i].data});
        w += in[i].word;
    }
    bool folded = false;
    bits_words(c, qs, nred, seg, dbits, &folded);
    if (qs.nseg) {
        ProfScope ps(c, c->st, "k_quantize", bytes, 0);
        hipck(launch_quantize_multi(qs, (int)c->P, c->st), "k_quantize_multi");
    }
    // the words: the GEMMs' digit counts (read lazily, fetch_bits) and the
    // device-side choices (row-scan operand widths)
    if (dbits && !folded) hipck(launch_bits_reduce(dbits + 64, seg, nred, dbits, c->st), "k_bits_reduce");
    c->wit.dbitw = dbits;
    return qs.nseg;
}
// A pipelined svd_witness takes the other cell set and gamma tables (call
// j - 1's scans still read these), or gives them back.
static void swap_cell_sets(svdw_ctx* c) {
    for (int p = 0; p < 2; ++p) std::swap(c->ph[p], c->alt[p]);
    std::swap(c->gpc, c->gpc_alt);
    std::swap(c->gtab, c->gtab_alt);
}
// svd_witness on the one cell set: behind everything queued, at the planned size.
static void run_unpipelined(svdw_ctx* c) {
    settle(c);
    after_previous(c);
    grow_to_plan(c);
}
// The end of a pipelined svd_witness: no join into st, its stages (st2) and row
// scans (st3) end at this parity's tail events, the next call takes the other
// parity. checked: a HIP error fails the call (the return), else it is ignored
// (unwinding: the tail is whatever reached st2 / st3).
static void record_tail(svdw_ctx* c, bool checked) {
    const int par = c->pipe_par;
    for (int k = 0; k < 2; ++k) {
        const hipError_t e = hipEventRecord(c->tail_ev[par][k], k ? c->st3 : c->st2);
        if (checked) hipck(e, "hipEventRecord");
    }
    c->tail_valid[par] = true;
    c->tail_pending = true;
    c->tail_last = par;
    c->pipe_par ^= 1;
    c->call.in_pipe = false;
}
// The end of a witness call, by return or by unwinding. An exception inside a
// pipelined call: its tail is whatever reached st2 / st3 -- join it. Then
// nothing of the call's state outlives it, so the modular calls that follow
// queue as on a fresh context (put_cell and check_svd_phase0 read prelaunched
// and prod_on_cell).
struct CallEnd {
    svdw_ctx* c;
    ~CallEnd() {
        if (c->call.in_pipe) record_tail(c, false);
        c->call.reset();
    }
};
static svdw_counts svd_witness(svdw_ctx* c, const double* m, const double* u, const double* v,
                               const double* d, uint32_t N, uint32_t M, bool on_device,
                               const svdw_svd_config& cfg, const Fr& gamma) {
    REQUIRE(N >= 1 && M >= 1, "empty matrix");
    const uint32_t r = std::min(N, M);
    begin_call(c, "svd_witness start");
    CallEnd call_end{c};
    if (!c->dry) {
        // exact sizes from the dry planner: no growth copies inside the step
        plan_sizes(c, {N, M, cfg.max_bits_d, f64_key(cfg.max_norm), f64_key(cfg.eps_svd), f64_key(cfg.eps_u),
                       c->opt.rlc_prefix},
                   [&](svdw_ctx* plan) {
                       plan->opt.rlc_prefix = c->opt.rlc_prefix;
                       svd_witness(plan, nullptr, nullptr, nullptr, nullptr, N, M, false, cfg, gamma);
                   });
        // Pipelined (svd_witness_pipe): device inputs on the f64 product path
        // with the products on the cell stream, and two cell sets that fit in
        // at most 60 % of the device memory (1024^2 P=63: 2 x 9.3 GB; 4096^2
        // P=63, 2 x 148 GB, runs unpipelined)
        const double wbytes = 32.0 * (double)(c->plan_val[0] + c->plan_val[1] + c->plan_val[2] + c->plan_val[3]);
        const bool qualifies = c->opt.pipeline && on_device && c->opt.overlap && crt_product_f64(c, std::max(N, M)) &&
                               products_on_cell_stream(c);
        // The other cell set must already hold this witness, or its growth must
        // fit in the device's free memory now (other contexts, the lane's state
        // and torch's allocations count) with 10 % of the device to spare for
        // scratch; else the call runs unpipelined and the set is released.
        bool fits = qualifies;
        if (qualifies) {
            const double need = wbytes - set_bytes(c->alt);
            if (need > 0) {
                size_t fr = 0, tot = 0;
                hipck(hipMemGetInfo(&fr, &tot), "hipMemGetInfo");
                fits = need + 0.1 * (double)tot <= (double)fr;
            }
        }
        if (qualifies && !fits) release_alt(c);
        c->call.in_pipe = fits;
        if (c->call.in_pipe) {
            // the other cell set (last written by call j - 2): every stream waits
            // for that call's tail, the last reader of these cells and bit words
            // (st2's first stages write cells that call's st3 scans read)
            swap_cell_sets(c);
            clear_streams(c);
            // (tail_ev[.][0] was recorded on st2, [.][1] on st3: a stream does not
            // wait for its own earlier work)
            if (c->tail_valid[c->pipe_par])
                for (hipStream_t t : {c->st, c->st2, c->st3})
                    for (int k = 0; k < 2; ++k)
                        if (t != (k ? c->st3 : c->st2))
                            hipck(hipStreamWaitEvent(t, c->tail_ev[c->pipe_par][k], 0), "hipStreamWaitEvent");
            if (c->xwait_side) {                  // the caller's stream (svdw_stream_wait)
                for (hipStream_t t : {c->st2, c->st3})
                    hipck(hipStreamWaitEvent(t, c->xwait_side, 0), "hipStreamWaitEvent");
                c->xwait_side = nullptr;
            }
            try {
                grow_to_plan(c);
            } catch (const SvdwError& e) {
                if (e.code != SVDW_ENOMEM) throw;
                // the other set could not be allocated after all: back to this
                // set, unpipelined (the waits already queued are harmless)
                swap_cell_sets(c);
                c->call.in_pipe = false;
                release_alt(c);
                clear_streams(c);
                run_unpipelined(c);
            }
        } else {
            run_unpipelined(c);
        }
    }
    // examples/svd_example.rs:183-184 run rlc.load_rlc_cache((ctx_gate, ctx_rlc), gate, 1)
    // on the phase-1 pair before check_svd_phase1. As recalled from axiom-eth's
    // RlcChip (un-vendored; parity unpinned), an empty cache loads gamma as
    // compute_rlc_fixed_len(ctx_rlc, [one, zero]) with one = ctx_gate.load_constant(1),
    // zero = ctx_gate.load_zero(): two constant cells at the head of ctx_gate (the
    // stream here); [E(one), E(zero), W(gamma)] go to ctx_rlc, whose cell 2 is init_rand.
    c->wit.ext_off = 0;
    c->rlc.n = 0;
    if (c->opt.rlc_prefix) {
        const svdw_vec one = put_cell(c, 1, fr_from_u64(1), true);
        const svdw_vec zero = put_cell(c, 1, fr_zero(), true);
        c->wit.ext_off = 2;
        c->rlc.n = 3;
        c->rlc.cells[0] = fr_from_u64(1);
        c->rlc.cells[1] = fr_zero();
        c->rlc.cells[2] = gamma;
        c->rlc.src[0] = (uint64_t)one.phase << 62 | one.off;
        c->rlc.src[1] = (uint64_t)zero.phase << 62 | zero.off;
    }
    c->gp_ev = nullptr;
    hold_step(c);
    if (!c->dry) {
        // gamma^j depends on gamma only: queue it first, on its own stream, so it
        // runs beside quantization instead of on the phase-1 chain (pipelined: on
        // the cell stream, the least loaded one, into this parity's tables)
        const bool g3 = c->opt.gamma_at == 1 || (c->opt.gamma_at < 0 && sharded(c));
        hipStream_t gs = c->call.in_pipe && !(g3 && c->st3) ? c->st_cell : c->st3;
        gamma_prep(c, std::max(N, M), gamma, gs);
        c->gp_ev = stream_dep(c, gs, nullptr);
        c->gp_st = gs;
        host_mark(c, "gamma_prep queued");
    }
    // m: only this rank's rows are quantized on a row-sharded rank (zkmatrix_new)
    // (u, v: the rank's rows and column block only, when b.g comes from the f64
    // inputs and so do the products' residue planes: no kernel reads the rest)
    const bool part = sharded(c) && on_device && c->opt.overlap && crt_product_f64(c, std::max(N, M));
    const WitInput in[4] = {{m, N, M, true, true, false}, {u, N, N, true, false, part}, {v, M, M, true, false, part},
                            {d, r, 1, false, false, false}};
    svdw_mat z[4];
    // (Round 4 measured the quantization beside the product chain instead: the
    // bit-length words from a read-only k_bits_f64 on st, the cells on st2; it
    // was 0.7-4 % slower at 1024^2, 512^2 and on 8-way ranks -- the words'
    // cross-block reduction costs what the cells' stores did -- and was removed.)
    load_inputs(c, in, 4, on_device, [&](size_t blocks) {
        // [0, 3): bit-length maxima of m, u, v; from word 64: per-block maxima
        // (pipelined: a half per parity, call j - 1's row scans still read theirs)
        const size_t words = (64 + blocks + 63) / 64 * 64;
        ensure_buf(c, c->bits, 2 * words * sizeof(unsigned));
        return (unsigned*)c->bits.p + (c->call.in_pipe ? c->pipe_par * words : 0);
    }, z);
    const svdw_mat &zm = z[0], &zu = z[1], &zv = z[2], &zdm = z[3];
    const unsigned* dbits = c->wit.dbitw;
    svdw_vec zd{0, r, zdm.off, 1};
    double es, eu;
    err_calc(c->P, std::max(N, M), cfg.max_norm, cfg.eps_svd, cfg.eps_u, &es, &eu);
    if (!c->dry) {   // operand bit lengths (GEMM digit counts): read lazily, see fetch_bits
        flush_batch(c, c->st);
        hipck(hipEventRecord(c->ev_bits, c->st), "hipEventRecord");
        c->bits_pending = true;
        c->qmat[0] = zm; c->qmat[1] = zu; c->qmat[2] = zv;
        host_mark(c, "quantize + bits queued");
    }
    // Phase 1 needs only the products (queued on st2 by check_svd_phase0), the
    // quantized operands and gamma: run it on st2 behind the GEMMs, concurrently
    // with the HBM-bound phase-0 checks still on st (its row scans are
    // VALU-bound), and join the streams afterwards.
    // Mode 2: on a third stream that starts after quantization; the b.g and
    // a.(b.g) scans run at once, the c_s.g scans wait for the products; queued
    // from inside check_svd_phase0 right after its first stage (p1_at).
    // Mode 1 on a row-sharded rank becomes mode 2: there the products are only a
    // row block, the st2 chain (products + phase 1) is the critical path and the
    // operand-only scans fit beside the products (tools/shard_sim.py, 8 ranks:
    // 0.62 -> 0.54 ms). So does a small witness (max(N, M) < 1024), where the
    // st2 chain is also the critical path (tools/ab.py: 512^2 P=32 0.559 ->
    // 0.454 ms, 768^2 P=63 1.328 -> 1.272 ms); from 1024 on it is neutral to
    // 1 % slower.
    const bool p1_small = std::max(N, M) < 1024;
    // (pipelined: st2 carries the diff and ids after the bounds, phase 1 goes to st3)
    const int p1mode = c->opt.phase1_overlap == 1 && (sharded(c) || p1_small || c->call.in_pipe) ? 2 : c->opt.phase1_overlap;
    bool p1_queued = false;
    auto queue_phase1 = [&](const svdw_svd_payload& pl, bool overlap) {
        const bool p1_overlap = p1mode && overlap;
        hipStream_t p1s = p1mode == 2 ? c->st3 : c->st2;
        // phase 1 beside the products (st3, or st2 while the products run on the
        // cell stream): it waits for the loads, and its c_s scans for the products
        if (p1_overlap && (p1s == c->st3 || c->call.prod_on_cell)) {
            dep_wait(c, p1s, c->ev_bits);
            c->call.wait_before_cs = c->call.gemm_done;
        }
        {
            OnStream on(c, p1_overlap ? (p1s == c->st3 ? &c->st3 : &c->st2) : nullptr);
            check_svd_phase1(c, zm, zu, zv, pl, gamma);
        }
        c->call.wait_before_cs.clear();
        p1_queued = true;
        host_mark(c, "phase 1 (early) queued");
    };
    if (p1mode == 2 && !c->dry) c->call.early_p1 = [&](const svdw_svd_payload& pl) { queue_phase1(pl, true); };
    if (on_device && !c->dry) {
        c->call.svd_f64[0] = m; c->call.svd_f64[1] = u; c->call.svd_f64[2] = v;
        c->call.f64src = {{zu, u}, {zv, v}};
    }
    svdw_svd_payload pl =
        check_svd_phase0(c, zm, zu, zv, zd, es, eu, cfg.max_bits_d, c->qbits, dbits, true);
    c->call.early_p1 = nullptr;
    const bool p1_overlap = p1mode && c->call.prelaunched && !c->dry;
    hipStream_t p1s = p1mode == 2 ? c->st3 : c->st2;
    host_mark(c, "phase 0 queued");
    if (!p1_queued) queue_phase1(pl, p1_overlap);
    host_mark(c, "phase 1 queued");
    if (c->call.in_pipe) {
        // no join into st: the next call's product chain starts on st while this
        // call's stages (st2) and row scans (st3) finish; they end at tail_ev
        flush_batch(c, c->st2);
        flush_batch(c, c->st3);
        record_tail(c, true);
        host_mark(c, "svd_witness end (pipelined)");
        return counts_of(c);
    }
    if (p1_overlap) stream_dep(c, p1s, c->st);
    // st2 also carries the d checks and single cells queued aside (and, with
    // phase 1 on st3, nothing else joins it): join it too
    if (c->call.prelaunched && !c->dry && !(p1_overlap && p1s == c->st2)) stream_dep(c, c->st2, c->st);
    host_mark(c, "svd_witness end");
    return counts_of(c);
}

// README.md:32-46 as one call: ZkMatrix::new(a), ZkMatrix::new(b), c_s =
// honest_prover_mat_mul(a, b) into phase 0, verify_mul(a, b, c_s, gamma) into
// phase 1 -- the modular calls' cells, enqueued without host waits: a and b
// quantized in one launch, the GEMM's modulus count and the row scans' operand
// widths decided on the device from the bit-length words, gamma^j prepared
// first on the side stream.
// verify_mul_witness's phase 1 opens with verify_mul's one cell and its d - 1
// gamma-power elements (verify_mul_many's first appends at phase-1 offsets 0
// and 1): k_gamma_prep writes them when the phase-1 stream holds them
static bool vm_pow_cells(svdw_ctx* c, uint32_t M, const Fr& gamma, PowCells* pc) {
    memset(pc, 0, sizeof *pc);
    if (M <= 1 || c->ph[1].cap < 1 + 4ull * (M - 1)) return false;
    pc->one = cellp(c, 1, 0);
    pc->pows = cellp(c, 1, 1);
    pc->d = M;
    pc->gamma = gamma;
    return true;
}
static svdw_counts verify_mul_witness(svdw_ctx* c, const double* a, const double* b, uint32_t N,
                                      uint32_t K, uint32_t M, bool on_device, const Fr& gamma) {
    REQUIRE(N >= 1 && K >= 1 && M >= 1, "empty matrix");
    REQUIRE(!sharded(c), "verify_mul_witness: not for row-sharded contexts");
    begin_call(c, "verify_mul_witness start");
    CallEnd call_end{c};
    settle(c);
    after_previous(c);
    if (!c->dry) {
        plan_sizes(c, {0x766d77ull, N, K, M}, [&](svdw_ctx* plan) {
            verify_mul_witness(plan, nullptr, nullptr, N, K, M, false, gamma);
        });
        grow_to_plan(c);
    }
    c->wit.ext_off = 0;
    c->gp_ev = nullptr;
    hold_step(c);
    host_mark(c, "plan + gamma_prep queued");
    if (!c->dry) {
        PowCells pc;                                      // (vm_pow_cells)
        // (queued ahead: only if that launch wrote them where they are now)
        if (c->ph[1].n == 0 && vm_pow_cells(c, M, gamma, &pc) && (!c->vmg.gp_external || c->vmg.gp_ext_one == pc.one))
            c->call.pows_pre = {true, 0, 1, M};
        if (c->vmg.gp_external) {                         // queued on st ahead of the captured graph
            c->gp_gamma = gamma;
            c->gp_len = std::max(M, 1u);
        } else {
            gamma_prep(c, M, gamma, c->st3, pc.one ? &pc : nullptr);
        }
        c->gp_ev = stream_dep(c, c->st3, nullptr);
        c->gp_st = c->st3;
    }
    // (quantization stays on the chain here: beside it on st2, config 2 measured
    // 0.091-0.096 -> 0.106 ms, host-bound, round 4)
    const WitInput in[2] = {{a, N, K, true, false, false}, {b, K, M, true, false, false}};
    svdw_mat z[2];
    const uint32_t nseg = load_inputs(c, in, 2, on_device, [&](size_t blocks) {
        ensure_buf(c, c->bits, (64 + blocks) * sizeof(unsigned));
        return (unsigned*)c->bits.p;
    }, z);
    const svdw_mat &za = z[0], &zb = z[1];
    const unsigned* dbits = c->wit.dbitw;
    host_mark(c, "quantize queued");
    // c_s = a * b (honest_prover_mat_mul's cells), the CRT GEMM sized on the device
    uint64_t off;
    append(c, 0, (uint64_t)N * M, 0, &off, nullptr, "product", N);
    const svdw_mat cs{0, N, M, off, (int64_t)M, 1};
    const uint32_t lk = clog2(K);
    c->wit.prods.push_back({cs, za, zb, lk});
    // device inputs: residue planes of a and b^T straight from the f64 inputs
    // (one launch), the GEMM and combine on st, and verify_mul on the third
    // stream from the loads on: its one / gamma-power cells and the b and a
    // scans run beside the product, only the c_s scans wait for it
    const bool f64 = on_device && !c->dry && crt_product_f64(c, K) && nseg == 2;
    hipEvent_t loaded = nullptr;
    if (f64) {
        loaded = stream_dep(c, c->st, nullptr);
        product_f64(c, c->st, a, b, N, K, M, cellp(c, 0, off), dbits);
    } else if (!c->dry) {
        gemm_exec(c, c->st, za, zb, cellp(c, 0, off), ~0u, ~0u, dbits, dbits + 1, true);
    }
    host_mark(c, "product queued");
    const VMul vm{za, zb, cs};
    if (f64) {
        c->call.wait_before_cs = {stream_dep(c, c->st, nullptr)};
        dep_wait(c, c->st3, loaded);
        {
            OnStream on(c, &c->st3);
            verify_mul_many(c, 1, &vm, 1, gamma);
        }
        c->call.wait_before_cs.clear();
        stream_dep(c, c->st3, c->st);                     // join
    } else {
        verify_mul_many(c, 1, &vm, 1, gamma);
    }
    host_mark(c, "verify_mul_witness end");
    return counts_of(c);
}

// ---------------------------------------- captured verify_mul_witness (graph)
// A device-input verify_mul_witness enqueues ~20 HIP calls for a GPU step of
// ~70 us at 256^2 (BASELINE config 2), so the host bounds it. Every call of
// one key (shape, input pointers, buffer epoch) enqueues the same launches:
// nothing in it waits for the device, and gamma reaches the device only as
// k_gamma_prep's tables. So k_gamma_prep goes out eagerly on st (by value),
// the rest is captured once (on the second call of a key, when every buffer
// is sized) and replayed with one hipGraphLaunch; the host state the call
// leaves (layout, checks, counts) is restored from the capture, with gamma
// patched into the constants that hold it.
static svdw_counts vmg_restore(svdw_ctx* c, const Fr& gamma) {
    const auto& g = c->vmg;
    clear_streams(c);
    c->wit = g.rec;
    c->wit.patch_gamma(gamma);
    c->ext_gamma = gamma;
    c->ph[0].n = g.counts.advice0;
    c->ph[1].n = g.counts.advice1;
    c->ph[0].nl = g.counts.lookup0;
    c->ph[1].nl = g.counts.lookup1;
    return g.counts;
}
// caller: the caller's stream (svdw_verify_mul_witness_on), waited for by the
// state that runs the call (after the lane switch)
static svdw_counts verify_mul_witness_api(svdw_ctx* c, const double* a, const double* b, uint32_t N,
                                          uint32_t K, uint32_t M, bool on_device, const Fr& gamma,
                                          hipStream_t caller = nullptr, bool has_caller = false) {
    const bool plain = on_device && !c->dry && !c->opt.prof && !c->opt.hold_us && !sharded(c) && N >= 1 && K >= 1 &&
                       M >= 1;
    if (plain && c->lanes > 1 && lane_fits(c)) lane_switch(c);
    if (has_caller && !c->dry) {
        const hipEvent_t e = xevent(c, 0);
        hipck(hipEventRecord(e, caller), "hipEventRecord");
        hipck(hipStreamWaitEvent(c->st, e, 0), "hipStreamWaitEvent");
        c->xwait_side = e;                        // (st2 / st3: through st, see after_previous)
    }
    const bool usable = c->opt.graph_vm && plain;
    if (!usable) {
        vmg_drop(c);
        c->vmg.seen.clear();
        return verify_mul_witness(c, a, b, N, K, M, on_device, gamma);
    }
    c->ht0 = std::chrono::steady_clock::now();
    settle(c);                     // (before any linear scope: it waits on tail events)
    struct Linear {                // vm_linear: every launch of the call on st
        svdw_ctx* c;
        hipStream_t s2 = nullptr, s3 = nullptr;
        bool on = false;
        explicit Linear(svdw_ctx* cc) : c(cc) {
            if (!c->opt.vm_linear) return;
            if (!c->lin_ev) hipck(hipEventCreateWithFlags(&c->lin_ev, hipEventDisableTiming), "hipEventCreate");
            s2 = c->st2;
            s3 = c->st3;
            c->st2 = c->st3 = c->st;
            c->vmg.linear = on = true;
        }
        ~Linear() {
            if (!on) return;
            c->st2 = s2;
            c->st3 = s3;
            c->vmg.linear = false;
        }
    } lin{c};
    struct Flags {                 // set here, ahead of verify_mul_witness, and kept over its eager
        svdw_ctx* c;               // rerun below: this function's end clears them, no witness call does
        void external(const Fr* one) {
            c->vmg.gp_external = true;
            c->vmg.gp_ext_one = one;
        }
        void capturing(bool on) { c->vmg.capturing = on; }
        ~Flags() {
            c->vmg.gp_external = false;
            c->vmg.gp_ext_one = nullptr;
            c->vmg.capturing = false;
            c->gp_ev = nullptr;
        }
    } flags{c};
    // gamma's tables (and the one / gamma-power cells when phase 1 holds them)
    // on st, ahead of everything the call queues. (Round 4 tried them on st3
    // beside the graph, the graph's scans waiting through an external event
    // node (hipEventWaitExternal): the runtime aborted in the capture/replay.)
    settle(c);
    PowCells pc;
    const bool pw = vm_pow_cells(c, M, gamma, &pc);
    gamma_prep(c, M, gamma, c->st, pw ? &pc : nullptr);
    host_mark(c, "vm: gamma_prep queued");
    flags.external(pw ? pc.one : nullptr);
    // (the cell set and gamma tables too: a pipelined svd_witness alternates between two)
    auto key_now = [&] {
        return std::vector<uint64_t>{N, K, M, (uint64_t)(uintptr_t)a, (uint64_t)(uintptr_t)b, c->epoch,
                                     (uint64_t)(uintptr_t)c->ph[0].adv, (uint64_t)(uintptr_t)c->ph[1].adv,
                                     (uint64_t)(uintptr_t)c->ph[0].lk, (uint64_t)(uintptr_t)c->ph[1].lk,
                                     (uint64_t)(uintptr_t)c->gpc.p, (uint64_t)(uintptr_t)c->gtab.p};
    };
    const std::vector<uint64_t> key = key_now();
    if (c->vmg.exec && key == c->vmg.key) {
        const svdw_counts k = vmg_restore(c, gamma);
        host_mark(c, "vm: host state restored");
        hipck(hipGraphLaunch(c->vmg.exec, c->st), "hipGraphLaunch");
        c->xwait_side = nullptr;                      // (its side streams fork from st)
        host_mark(c, "vm: graph launched");
        ++c->vmg.replays;
        return k;
    }
    if (key == c->vmg.seen) {
        vmg_drop(c);
        hipGraph_t graph = nullptr;
        hipck(hipStreamBeginCapture(c->st, hipStreamCaptureModeRelaxed), "hipStreamBeginCapture");
        flags.capturing(true);
        svdw_counts k{};
        try {
            k = verify_mul_witness(c, a, b, N, K, M, on_device, gamma);
            stream_dep(c, c->st2, c->st);                  // every forked stream joins st
            if (c->st3) stream_dep(c, c->st3, c->st);
        } catch (...) {
            // nothing captured ran: end the capture and run the call eagerly
            flags.capturing(false);
            graph = nullptr;
            if (hipStreamEndCapture(c->st, &graph) == hipSuccess && graph) (void)hipGraphDestroy(graph);
            (void)hipGetLastError();
            c->vmg.seen.clear();
            return verify_mul_witness(c, a, b, N, K, M, on_device, gamma);
        }
        flags.capturing(false);
        hipck(hipStreamEndCapture(c->st, &graph), "hipStreamEndCapture");
        hipGraphExec_t exec = nullptr;
        const hipError_t e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        hipck(e, "hipGraphInstantiate");
        c->vmg.exec = exec;
        c->vmg.key = key;
        c->vmg.rec = c->wit;                              // the snapshot vmg_restore puts back
        c->vmg.counts = k;
        hipck(hipGraphLaunch(exec, c->st), "hipGraphLaunch");
        ++c->vmg.captures;
        return k;
    }
    vmg_drop(c);
    const svdw_counts k = verify_mul_witness(c, a, b, N, K, M, on_device, gamma);
    c->vmg.seen = key_now();
    return k;
}

// ================================================================== C ABI
extern "C" {

int svdw_svd_witness(svdw_ctx* c, const double* m, const double* u, const double* v,
                     const double* d, uint32_t N, uint32_t M, int on_device,
                     const svdw_svd_config* cfg, const uint64_t gamma[4], svdw_counts* counts) {
    return guarded([&] {
        REQUIRE(c && cfg && gamma, "null argument");
        REQUIRE(c->dry || (m && u && v && d), "null input matrix");
        svdw_counts k = svd_witness(c, m, u, v, d, N, M, on_device != 0, *cfg, fr_from_words(gamma));
        if (counts) *counts = k;
    });
}
int svdw_verify_mul_witness(svdw_ctx* c, const double* a, const double* b, uint32_t N, uint32_t K,
                            uint32_t M, int on_device, const uint64_t gamma[4], svdw_counts* counts) {
    return guarded([&] {
        REQUIRE(c && gamma, "null argument");
        REQUIRE(c->dry || (a && b), "null input matrix");
        svdw_counts k = verify_mul_witness_api(c, a, b, N, K, M, on_device != 0, fr_from_words(gamma));
        if (counts) *counts = k;
    });
}
int svdw_verify_mul_witness_on(svdw_ctx* c, void* stream, const double* a, const double* b, uint32_t N,
                               uint32_t K, uint32_t M, const uint64_t gamma[4], svdw_counts* counts) {
    return guarded([&] {
        REQUIRE(c && gamma, "null argument");
        REQUIRE(c->dry || (a && b), "null input matrix");
        svdw_counts k = verify_mul_witness_api(c, a, b, N, K, M, true, fr_from_words(gamma), (hipStream_t)stream,
                                               true);
        if (counts) *counts = k;
    });
}
int svdw_plan_svd(uint32_t N, uint32_t M, uint32_t p, uint32_t lb, const svdw_svd_config* cfg,
                  svdw_counts* counts) {
    return guarded([&] {
        REQUIRE(cfg && counts, "null argument");
        if (p < 1 || p > 63) fail(SVDW_ERANGE, "precision_bits must be in [1, 63]");
        if (lb < 8 || lb > 63) fail(SVDW_ERANGE, "lookup_bits must be in [8, 63]");
        PlanCtx plan(p, lb);
        *counts = svd_witness(&plan, nullptr, nullptr, nullptr, nullptr, N, M, false, *cfg, fr_zero());
    });
}

}  // extern "C"
