// What the host files share: engine.cpp (the witness engine), witness.cpp (the
// two witness calls on it), context.cpp (the
// context's lifetime, lanes, options, stream hand-off, marks, profiling),
// export.cpp (read-out), ingest.cpp (text ingest), gemm.cpp (the exact field
// product), circuit.cpp (the assigned-witness calls), prover.cpp (the prover
// calls), srs.cpp (the SRS calls), g1_fft.cpp (the G1 transform calls) and svd.cpp (the
// decomposition). In order: the C ABI's error plumbing, device buffers, the entries'
// host Fr helpers, each family's state, the host record of a witness, the
// context (svdw_ctx), the functions that cross a file boundary, the staged call.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <functional>
#include <new>
#include <set>
#include <stdexcept>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/svdw.h"
#include "kernels.hpp"
#include "pow_table.hpp"

using namespace svdw;                                      // (the files are the engine's own)

// ------------------------------------------------------------------ errors
inline thread_local std::string g_err;
struct SvdwError {
    int code;
    std::string msg;
};
[[noreturn]] inline void fail(int code, const std::string& msg) { throw SvdwError{code, msg}; }
inline void hipck(hipError_t e, const char* what) {
    if (e != hipSuccess) fail(SVDW_EDEVICE, std::string(what) + ": " + hipGetErrorString(e));
}
template <class F>
int guarded(F&& f) {
    try {
        f();
        return SVDW_OK;
    } catch (const SvdwError& e) {
        g_err = e.msg;
        return e.code;
    } catch (const std::bad_alloc&) {
        g_err = "out of host memory";
        return SVDW_ENOMEM;
    } catch (const std::exception& e) {
        g_err = e.what();
        return SVDW_EINVAL;
    }
}
#define REQUIRE(cond, msg) \
    do {                   \
        if (!(cond)) fail(SVDW_EINVAL, msg); \
    } while (0)

// A device allocation that only grows (ensure_buf).
struct DBuf {
    void* p = nullptr;
    size_t cap = 0;
};

// ------------------------------------------- host Fr helpers of the entries
inline void check_form(int form) {
    REQUIRE(form == SVDW_FORM_CANONICAL || form == SVDW_FORM_MONTGOMERY,
            "unknown form (SVDW_FORM_CANONICAL or SVDW_FORM_MONTGOMERY)");
}
// The four 64-bit words as they are (not reduced: fr_reduced).
inline Fr fr_raw_words(const uint64_t w[4]) {
    Fr x;
    for (int i = 0; i < 8; ++i) x.w[i] = (uint32_t)(w[i / 2] >> (32 * (i & 1)));
    return x;
}
inline void fr_store_words(const Fr& x, uint64_t w[4]) {
    for (int i = 0; i < 4; ++i) w[i] = (uint64_t)x.w[2 * i] | ((uint64_t)x.w[2 * i + 1] << 32);
}
inline bool fr_reduced(const Fr& x) {
    Fr t;
    return sub_p(t, x) != 0;                               // x - p borrows: x < p
}

// The checks several entries repeat, each under the entry's name f (scratch_cap, which reads the context: below).
inline void need_columns(const std::string& f, uint32_t n, const char* where = "") {
    if (n > 65535) fail(SVDW_ERANGE, f + ": more than 65535 columns" + where);
}
inline void need_k(const std::string& f, uint32_t k) {
    if (k < 1 || k > 28) fail(SVDW_ERANGE, f + ": k must be in [1, 28]");
}
inline void need_pointer(const std::string& f, const void* p) { REQUIRE(p, f + ": null column pointer"); }
// [o0, o1) (the output `out`) and [i0, i1) (`in`) do not meet.
inline void need_apart(const std::string& f, const char* out, uintptr_t o0, uintptr_t o1, const char* in, uintptr_t i0,
                       uintptr_t i1) {
    REQUIRE(i1 <= o0 || o1 <= i0, f + ": " + out + " overlaps " + in);
}
// A nested call of the interface: its error becomes this call's.
inline void nested(int rc) {
    if (rc != SVDW_OK) fail(rc, g_err);
}
// ------------------------------------------------- the families' state
// The device scratch of every staged call of either family (stage, below), in the
// staged-call layout, and the host vector it is uploaded from.
struct StagedScratch {
    DBuf buf;
    std::vector<char> upload;
};
// What the assigned-witness calls (circuit.cpp) keep on a context.
struct CircuitState {
    DBuf eq_cp, eq_ks;                      // the equality records of one phase (eq_gen_device): live within a call
    DBuf eq_in;                             // the generator's input: err word, regions, eq words, constants
    DBuf gateq[2];                          // svdw_assign_columns: the gate-start bits of a phase's virtual stream
    std::vector<DBuf*> dbufs() { return {&eq_cp, &eq_ks, &eq_in, &gateq[0], &gateq[1]}; }
};
// What the prover calls (prover.cpp) keep on a context between calls.
struct ProverState {
    struct DomainSlot {                     // the domain's omega_k table (pow_table.hpp) on the host and on the device
        std::vector<Fr> cells;
        DBuf buf;
        PowTable host{}, dev{};             // the views of cells and of buf
    } domain[29];                           // by k = 1..28: filled on first use (domain_table, prover.cpp), then kept
    DBuf ntt_tw, ntt_tmp;                   // transforms (ntt.hpp): the 1024 stage twiddles; the buffer between passes
    DBuf commit_ws;                         // commitments (commit.hpp): the window sums and one batch of tasks
    DBuf cycles_ws;                         // sigma's cycles (permutation_cycles.hpp): the sort's arrays and tables
    // quotient (quotient.hpp): the extended columns of l_0, l_last, l_active (R form) of the key below, and the
    // scratch they are built in
    DBuf basis, basis_tmp;
    uint32_t basis_k = 0, basis_ek = 0, basis_unusable = 0;
    Fr basis_shift{};
    std::vector<DBuf*> dbufs() {
        std::vector<DBuf*> v = {&ntt_tw, &ntt_tmp, &basis, &basis_tmp, &commit_ws, &cycles_ws};
        for (DomainSlot& s : domain) v.push_back(&s.buf);
        return v;
    }
};
// What the SRS calls (srs.cpp) keep on a context between calls.
struct SrsState {
    // the fixed-base tables (srs.hpp) by (base, window bits): built on first use, replaced in turn
    struct Table {
        DBuf buf;
        uint32_t base[16] = {};             // the base's 64 bytes as given
        int base_form = 0;
        uint32_t c = 0;                     // 0: empty
    } table[4];
    uint32_t next = 0;                      // the slot the next new table takes
    DBuf ws;                                // a call's scratch: a scalar column, accumulators, prefix products
    std::vector<DBuf*> dbufs() {
        std::vector<DBuf*> v = {&ws};
        for (Table& t : table) v.push_back(&t.buf);
        return v;
    }
};
// What the G1 transform calls (g1_fft.cpp) keep on a context between calls.
struct G1FftState {
    DBuf work;                              // svdw_g1_fft: the working array, 2^k XYZZ points
    DBuf ws;                                // a piece's accumulators and tables; svdw_check_lagrange's two columns
    std::vector<DBuf*> dbufs() { return {&work, &ws}; }
};
// What the decomposition (svd.cpp) keeps on a context between calls.
struct SvdState {
    DBuf ws;                                // the working array, the partial Gram matrices, norms, order, words
    DBuf io;                                // host inputs and outputs staged on the device: m, u, d, v
    unsigned long long* pinned = nullptr;   // the host's view of a sweep's counter and of the load's words
    std::vector<DBuf*> dbufs() { return {&ws, &io}; }
};
#pragma GCC visibility push(hidden)
// Read-out (export.cpp: svdw_copy_cells, the host variants of svdw_export_* /
// svdw_dequantize_*): two staging halves of at most kExportChunk bytes each, and
// the events that order them ([0..1] half converted, [2..3] half copied out,
// [4..5] the join of st2 / st3 into st ahead of every read-out).
struct ExportState {
    DBuf half[2];
    hipEvent_t ev[6] = {};
    std::vector<DBuf*> dbufs() { return {&half[0], &half[1]}; }
};
// The scratch of the device ingest (ingest.cpp, svdw_parse_svd_input_device).
struct IngestState {
    DBuf xfer, entry, counts;               // per chunk of text: its transfer, entry state and counts (passes 1, 2)
    DBuf pow10;                             // serde's table of 10^k, written once
    DBuf values, num_pos, num_depth;        // per number: its f64 value, byte position and bracket depth (pass 3)
    DBuf row_pos, key_pos;                  // the byte positions of the row opens and of the depth-1 strings
    DBuf errors;                            // the structural-error list ([0] count, [1..255]) and the validation word
    DBuf queries;                           // the members' positions and the number / row ranges found for them
    std::vector<DBuf*> dbufs() {
        return {&xfer, &entry, &counts, &pow10, &values, &num_pos, &num_depth, &row_pos, &key_pos, &errors, &queries};
    }
};

// ------------------------------------------- the host record of a witness
// What a witness call leaves on the host about the cells it appended: the calls
// on a finished witness (circuit.cpp) and the row scans read it, and a replay of
// the captured verify_mul_witness puts it back as a whole (VmGraph::rec). The
// members are listed here and in clear() only.
struct WitnessRecord {
    std::vector<svdw_region> layout;        // every appended region of the current witness
    // per region: gate offsets within one element's cells and cells per element
    // (program regions; empty otherwise; svdw_check_gates)
    std::vector<RegionChecks> layout_chk;
    // distinct constant cell values (halo2-base Constant / load_constant):
    // the fixed-column count of svdw_physical_layout
    std::set<std::array<uint32_t, 8>> consts;
    // (layout_chk index, eqk slot) of the constants that hold gamma (the
    // verify_mul gamma powers' init_rand), patched on replay
    std::vector<std::pair<size_t, int>> gamma_slots;
    // Known magnitude bounds of matrices written in this witness: cell (i, j) of
    // `m` satisfies |signed value| < 2^bits.
    struct MatBits { svdw_mat m; uint32_t bits; };
    std::vector<MatBits> mbits;
    // products c_s = a * b (K = 2^lk-bounded inner dimension): |c_s| < 2^(bits_a + bits_b + lk)
    struct Prod { svdw_mat cs, a, b; uint32_t lk; };
    std::vector<Prod> prods;
    // Device bit-length words of matrices written in this witness (svd_witness:
    // quantized m, u, v at dbitw[0..2]): the row scans decide their operand
    // width on the device from these (NaSpec), so the host never waits for them.
    struct DevBits { svdw_mat m; int16_t word; };
    std::vector<DevBits> dwords;
    const unsigned* dbitw = nullptr;
    uint64_t ext_off = 0;                   // the cell of the last verify_mul's init_rand in the RLC context
    // Empties the members in place, as copy-assignment refills them in place: a
    // witness call allocates nothing here once the containers have grown (begin_call).
    void clear() {
        layout.clear();
        layout_chk.clear();
        consts.clear();
        gamma_slots.clear();
        mbits.clear();
        prods.clear();
        dwords.clear();
        dbitw = nullptr;
        ext_off = 0;
    }
    // The constants that hold gamma take the gamma of a replayed call.
    void patch_gamma(const Fr& gamma) {
        for (const auto& s : gamma_slots) layout_chk.at(s.first).eqk.at((size_t)s.second) = gamma;
    }
};
#pragma GCC visibility pop

// -------------------------------------------------------------- context
struct Stream {
    Fr* adv = nullptr;
    uint64_t n = 0, cap = 0;
    Fr* lk = nullptr;
    uint64_t nl = 0, lcap = 0;
};
struct svdw_ctx {
    // ---- options: svdw_set_option (kOptions), svdw_set_gemm_impl, svdw_set_shard,
    // the profiler switches; a lane takes them over as a whole (copy_settings)
    struct Options {
        int gemm_impl = SVDW_GEMM_MFMA;         // svdw_set_gemm_impl
        // STAGE_* (4 KiB-aligned block store windows; "stage_rot" 1: phase B from a
        // block-dependent window on, tools/r6/place_ab.py over 8 placements of the
        // 1024^2 cell streams: 1.739-1.891 -> 1.728-1.825 ms, mean 1.815 -> 1.751)
        uint32_t stage_flags = STAGE_ALIGN | STAGE_ROT;
        uint32_t stage_elems = kStageElems;     // "stage_elems": elements per stage block (16..256)
        int gemm_crt = 1;                       // "gemm_crt": multi-modular GEMM (else digits)
        // "gemm_kern": CRT GEMM kernel (CrtBatch::kern); -1: wide tiles or the
        // persistent grid for a product queued on its own (svdw_honest_prover_mat_mul,
        // gemm_solo; CrtBatch::kern 3), one block per unit inside the witness calls,
        // beside their stage kernels
        int gemm_kern = -1;
        int res_wait = -1;                      // "res_wait": stages wait for the residue planes
        int place_trials = 6;                   // "place_trials": candidate placements of a new cell stream
        bool res_f64 = true;                    // "res_f64": CRT residue planes of m, u, v from the
                                                // f64 inputs, one launch (else from the cells)
        int phase1_overlap = 1;                 // "phase1_overlap": 0 off, 1 on st2 behind the
                                                // GEMMs, 2 on st3 from quantization on
        int prod_cell = 1;                      // "prod_cell": svd_witness's products (residues, GEMM,
                                                // combine) on the cell stream and the u / v bounds and
                                                // u.d beside them on st2 (1), not (0); -1: on row-sharded
                                                // ranks only. On by default: the product chain is the
                                                // critical path sharded, and unsharded it measured
                                                // 2.5 % faster at 1024^2 and 2048^2, neutral at 512^2
        uint32_t hold_us = 0;                   // "hold_us": timing aid, st spins this long first
        uint32_t commit_window_bits = 0;        // "commit_window_bits": svdw_commit's window, 0: svdw_commit_plan's
                                                // (a tuning aid, tools/commit_bench.py; the result reports it)
        uint32_t g1_window_bits = 0;            // "g1_window_bits": svdw_g1_fft's window, 0: g1_plan's (a tuning aid,
                                                // tools/g1_fft_bench.py; the result reports it)
        uint32_t commit_scratch_mib = 1024;     // "commit_scratch_mib": svdw_commit's workspace cap per batch of tasks
        uint32_t srs_chunk_rows = 0;            // "srs_chunk_rows": rows per chunk of svdw_srs_setup, 0: what fits
                                                // commit_scratch_mib (a testing aid; the result reports it)
        bool rlc_prefix = false;                // "rlc_prefix": svd_witness's phase 1 starts with the
                                                // ctx_gate cells of load_rlc_cache(.., 1)
        int p1_at = -1;                         // "p1_at": phase 1 on st3 (mode 2) enqueued after
                                                // phase-0 stage 0 / 1 / 2 (the u, v bounds), 3: at the
                                                // end; -1: auto (tools/shard_sim.py --opt p1_at=):
                                                // 0 on a rank of >= 4, 3 of 2-3, else 1
        // pipelined svd_witness: "dchk_at" the d checks on the cell stream behind
        // the products (0), on st2 with the bounds and u.d (1) or on st3 ahead of
        // phase 1 (2); "gamma_at" k_gamma_prep at the head of the cell stream (0) or
        // of st3 (1); -1: st3 on a row-sharded rank, whose cell stream (quantize ->
        // residues -> GEMM -> combine, then the diff on st2) is the step's chain
        // (8-way rank 0.331 -> 0.316-0.321 ms; 1024^2 / 512^2 +0.5 %, r5p / r5q)
        int dchk_at = 0, gamma_at = -1;
        bool f64_views = true;                  // "f64_views": launches read registered f64 inputs (f64_view)
        bool overlap = true;                    // "overlap": products queued ahead of the check stages
        bool stage_batch = true;                // "stage_batch": stage launches share k_stage_multi (BatchScope)
        int graph_vm = 1;                       // "graph": 0 off, 1 verify_mul_witness captured (vm_graph)
        // "vm_linear": the captured verify_mul_witness runs on the context stream
        // alone (st2 = st3 = st while it is queued: a linear graph, no fork / join
        // events); concurrency comes from the two lanes instead.
        int vm_linear = 1;
        int pipeline = 1;                       // "pipeline": 1 on, 0 off (svd_witness_pipe, below)
        // Row-block sharding of one witness: this context computes the
        // rows [R rank / world, R (rank + 1) / world) of every row-parallel stage
        // (R = that stage's row count) into the globally laid-out streams; shared
        // inputs (quantized operands, single constants, the Freivalds b.g values)
        // are computed in full. `owned` lists the cell ranges this rank is the
        // source of, for reassembly.
        uint32_t shard_rank = 0, shard_world = 1;
        // built-in event profiler (svdw_profile_*): one start/stop event pair per launch
        bool prof = false;
        std::string prof_filter;                // record only kernels whose name starts with this
        // SVDW_HOST_TRACE=1: host-side timestamps of svd_witness's enqueue points on
        // stderr (µs since the call started), to find host waits inside a call
        bool host_trace = false;
        auto tied() const {
            return std::tie(gemm_impl, stage_flags, stage_elems, gemm_crt, gemm_kern, res_wait, place_trials,
                            res_f64, phase1_overlap, prod_cell, hold_us, rlc_prefix, p1_at, dchk_at, gamma_at,
                            f64_views, overlap, stage_batch, graph_vm, vm_linear, pipeline, shard_rank,
                            shard_world, prof, prof_filter, host_trace);
        }
        bool operator==(const Options& o) const { return tied() == o.tied(); }
    } opt;
    // ---- one witness call (svd_witness, verify_mul_witness): meaningful while the
    // call is being enqueued. Call::reset returns all of it to its initial value:
    // at the call's opening (begin_call), at its end by return or by unwinding
    // (CallEnd) and in svdw_ctx_reset, so the modular calls find a fresh context's.
    struct PreGemm {
        uint64_t off;
        hipEvent_t ev;
        hipStream_t st;                     // the stream it was launched on
    };
    // svd_witness's quantized matrices and their device f64 inputs (u, v): a
    // row-sharded rank takes b.g of b = u^T, v^T from the f64 rows directly
    // (k_colsum_f64), not from cells. Cleared at the end of the witness.
    struct F64Src { svdw_mat m; const double* x; };
    // loaded regions whose f64 source is on the device for the current call:
    // launches read them through VIEW_F64 (quantized in registers) instead of
    // waiting for the quantized cells (f64_view)
    struct F64Region { uint32_t phase; uint64_t off, n; const double* x; };
    struct Call {
        bool in_pipe = false;                   // inside a pipelined svd_witness
        bool prelaunched = false;               // this witness's products were queued on st2
        bool prod_on_cell = false;              // this witness's products went on the cell stream
        bool gemm_batched = false;              // this witness's products went out as one batch
        std::vector<PreGemm> pre;               // GEMMs launched ahead on st2, in append order
        hipStream_t pre_wait_st = nullptr;      // the last (stream, event) waited on for them
        hipEvent_t pre_wait_ev = nullptr;
        std::vector<hipEvent_t> gemm_done;      // their completion events (this witness)
        std::vector<hipEvent_t> wait_before_cs; // verify_mul_many: wait before the c_s scans
        const double* svd_f64[3] = {nullptr, nullptr, nullptr};   // device f64 m, u, v of svd_witness
        std::vector<F64Region> f64reg;
        std::vector<F64Src> f64src;
        std::function<void(const svdw_svd_payload&)> early_p1;   // phase 1's enqueue at p1_at (svd_witness)
        bool stage_front = false;               // stage_launch: the stage goes ahead of the batch's groups
        // verify_mul_witness: the one cell and gamma powers written by k_gamma_prep
        // (phase-1 offsets one_off / pows_off for d), so verify_mul does not launch them
        struct PowsPre {
            bool on = false;
            uint64_t one_off = 0, pows_off = 0;
            uint32_t d = 0;
        } pows_pre;
        // The only list of the members: the vectors are emptied in place (a witness
        // call allocates nothing here once they have grown, begin_call).
        void reset() {
            in_pipe = prelaunched = prod_on_cell = gemm_batched = stage_front = false;
            pre.clear();
            pre_wait_st = nullptr;
            pre_wait_ev = nullptr;
            gemm_done.clear();
            wait_before_cs.clear();
            svd_f64[0] = svd_f64[1] = svd_f64[2] = nullptr;
            f64reg.clear();
            f64src.clear();
            early_p1 = nullptr;
            pows_pre = PowsPre{};
        }
    } call;
    // ---- the handle: parameters, streams, cells, caches, scratch
    std::chrono::steady_clock::time_point ht0;   // host_trace: when the call started
    int device = -1;
    bool dry = true;
    hipStream_t st = nullptr;
    uint32_t P = 32, LB = 19;
    Stream ph[2];
    // Pipelined svd_witness ("pipeline", svd_witness_pipe): consecutive
    // witnesses alternate between two sets of cell streams (ph and alt), so call
    // j's product chain (st) runs beside call j - 1's HBM-bound stages (st2) and
    // row scans (st3) instead of after them. Call j's st first waits for call
    // j - 2's tail (tail_ev[parity]: its last work on st2 / st3), the last user
    // of this cell set and of this half of the bit-length words. Anything else
    // that touches the streams after a pipelined call settles first (settle).
    Stream alt[2];
    int pipe_par = 0;                       // this call's parity (cell set, bit words)
    hipEvent_t tail_ev[2][2] = {};          // [parity][st2, st3]
    bool tail_valid[2] = {false, false};
    bool tail_pending = false;              // the last pipelined call's tail not yet joined into st
    int tail_last = 0;
    size_t mem_total = 0;                   // device memory (hipMemGetInfo at create)
    // "lanes" 2: svdw_verify_mul_witness on its captured-graph path alternates
    // between two complete context states, this one and `lane` (own streams,
    // cells, scratch, graph). The states are exchanged (std::swap) at the start
    // of a call, so call j + 1 runs on the other state's streams beside call j
    // and the handle always holds the latest call's cells. sync, stream_wait,
    // stream_signal, graph_stats and destroy cover both; lane / lanes stay with
    // the handle.
    int lanes = 2;                          // (config 2, same box: 0.081 -> 0.058 ms per call)
    svdw_ctx* lane = nullptr;
    // svdw_stream_wait's event (the caller's stream), not yet waited on by
    // st2 / st3: st waits at once; the side streams inherit it through
    // after_previous or the captured graph's fork from st, and the pipelined
    // svd_witness (whose side streams do not wait for st) waits explicitly
    hipEvent_t xwait_side = nullptr;
    DBuf f64in, digA, digB, digC, w1c, w1t, w2c, w2t, bits, gpc, gtab, crtR, gbits;
    DBuf gpc_alt, gtab_alt;                 // pipelined svd_witness: gamma tables of the other parity
    DBuf wbc[kMaxScanJobs], wbt[kMaxScanJobs];   // b.v per batched verify_mul (canonical, table)
    // gamma^j (canonical gpc, scaled table gtab, kernels.hpp kTabSlots) of the
    // current verify_mul calls: recomputed for every witness (a fresh challenge
    // each time). svd_witness queues it first thing on a side stream (gp_ev).
    Fr gp_gamma{};
    uint32_t gp_len = 0;
    hipEvent_t gp_ev = nullptr;
    hipStream_t gp_st = nullptr;            // the stream gp_ev was recorded on
    WitnessRecord wit;                      // the host record of the current witness: cleared with the streams
    // svd_witness: bit lengths of quantized m, u, v travel to pinned host memory
    // behind ev_bits; the host waits for them only where the GEMM launches need
    // them (fetch_bits), with check stages already queued on the device.
    uint32_t* hbits = nullptr;
    hipEvent_t ev_bits = nullptr;
    bool bits_pending = false;
    uint32_t qbits[3] = {0, 0, 0};
    svdw_mat qmat[3] = {};
    // the event profiler's records (opt.prof): one start/stop event pair per launch
    struct Rec {
        std::string name;
        double bytes, ops;
        hipEvent_t e0, e1;
    };
    std::vector<Rec> recs;
    std::vector<hipEvent_t> pool;
    hipStream_t stream_id[3] = {};          // st, st2, st3 as created (st / st2 / st3 are swapped at times)
    bool gemm_solo = false;                 // svdw_honest_prover_mat_mul: a product queued on its own (gemm_kern)
    Fr ext_gamma{};                          // init_rand of the last verify_mul (equality source 2; its cell: wit.ext_off)
    // ctx_rlc of the last svd_witness with rlc_prefix: [E(one), E(zero), W(gamma)]
    // and the phase-1 offsets of the two ctx_gate constants its first cells copy
    struct RlcTrace {
        uint32_t n = 0;
        Fr cells[3];
        uint64_t src[2];
    } rlc;
    // Host-side replays cached for repeated calls of the same shape: the dry
    // plan of svd_witness's stream sizes (key: N, M, config) and prelaunch's
    // product offsets (key: stream state at entry, operand views, bounds).
    std::vector<uint64_t> plan_key, plan_val, log_key, log_val;
    struct Seg { uint32_t phase, lookup; uint64_t off, n; };
    std::vector<Seg> owned;                 // row-sharded: the cell ranges this rank is the source of
    DBuf bvfull[kMaxScanJobs];              // shard mode: full b.g values per verify_mul
    DBuf colpart;
    DBuf qfold;                             // k_quantize_multi's fold counters + group maxima
    // second stream: GEMMs overlap the HBM-bound stages; third: phase 1
    hipStream_t st2 = nullptr;
    hipStream_t st3 = nullptr;
    hipStream_t st_cell = nullptr;          // the cell stream proper (st is swapped at times)
    hipEvent_t xev[4] = {};                 // svdw_stream_wait / _signal (caller's stream)
    // svdw_mark ring: slot k holds ticket t[k]'s events (one per stream of
    // both lanes), recorded on the context's own streams (no waits); it stays
    // with the handle when lanes exchange states (lane_switch)
    static constexpr int kMarks = 16;
    struct Marks {
        hipEvent_t ev[kMarks][6] = {};
        uint64_t t[kMarks] = {};
        uint8_t used[kMarks] = {};
        uint64_t seq = 0;
    } mk;
    // svdw_physical_layout's plan: per phase, the virtual index of each advice
    // column's row 0 and each full column's break point
    struct Phys {
        bool valid = false;
        uint32_t k = 0, min_rows = 0;
        uint64_t R = 0;
        std::vector<uint64_t> start[2], bp[2];
        // svdw_permutation_edges: the distinct constants in the order of their placement in the fixed columns
        bool fixed_ready = false;
        std::vector<Fr> fixed;
    } phys;
    std::vector<uint64_t>* gemm_log = nullptr;   // dry run: offsets of honest_prover_mat_mul
    std::vector<hipEvent_t> deps;           // dependency events (no timing)
    size_t dep_next = 0;
    // Stage batches (BatchScope, "stage_batch"): stage launches on a stream with
    // an open batch are collected and issued as k_stage_multi launches when the
    // scope closes, when a stage reads cells a pending stage writes, or before
    // anything else is recorded or launched on that stream.
    struct Pending {
        StageArgs a;
        std::string name;
        double bytes;
    };
    // A batch holds groups issued in order, one k_stage_multi launch each: a
    // stage joins the group after the last one holding a stage whose cells it
    // reads, so a dependent stage (entries_in_desc_order's range checks of its
    // subtractions) defers only itself, not the independent stages after it.
    struct Batch {
        hipStream_t st;
        std::vector<std::vector<Pending>> groups;
        size_t last = 0;                   // group of the latest stage
    };
    std::vector<Batch> batches;
    StagedScratch staging;                  // every staged call's scratch (circuit.cpp, prover.cpp)
    CircuitState circuit;                   // the assigned-witness calls (circuit.cpp)
    ProverState prover;                     // the prover calls (prover.cpp)
    SrsState srs;                           // the SRS calls (srs.cpp)
    G1FftState g1fft;                       // the G1 transform calls (g1_fft.cpp)
    SvdState svd;                           // the decomposition (svd.cpp)
    ExportState exp;                        // read-out (export.cpp)
    IngestState ingest;                     // the device ingest (ingest.cpp)
    // ---- captured verify_mul_witness ("graph", vm_graph): the launch sequence of
    // a device-input call is captured once into a HIP graph (the second call of
    // a shape, when every buffer is sized) and replayed by later calls of the
    // same key; gamma enters only through k_gamma_prep, launched eagerly on st
    // ahead of the graph (gp_external), so the graph itself is gamma-free.
    hipEvent_t lin_ev = nullptr;            // "vm_linear": stream_dep's placeholder (vmg.linear)
    uint64_t epoch = 0;                     // bumped by every allocation / option change
    struct VmGraph {
        std::vector<uint64_t> key, seen;    // replay key; the last eager call's key
        hipGraphExec_t exec = nullptr;
        // Set by svdw_verify_mul_witness's wrapper ahead of the witness call it makes
        // and kept over it (its Linear and Flags scopes write them, nothing else):
        // `linear` while a vm_linear call is queued (stream_dep returns lin_ev,
        // never recorded, and dep_wait skips it)
        bool linear = false;
        bool capturing = false;             // st is capturing: no allocation, no sync
        bool gp_external = false;           // k_gamma_prep already queued ahead of the graph
        const Fr* gp_ext_one = nullptr;     // the one cell it wrote (null: none)
        WitnessRecord rec;                  // the record the captured call left behind (restored on replay)
        svdw_counts counts{};
        uint64_t replays = 0, captures = 0;
    } vmg;
};

// The functions that cross a file boundary (the library exports only the C ABI).
#pragma GCC visibility push(hidden)
// ---- context.cpp
void sync(svdw_ctx* c);                                    // every stream of the context has run dry
void settle(svdw_ctx* c);                                  // st waits for the tail of a pipelined svd_witness
void ensure_buf(svdw_ctx* c, DBuf& b, size_t bytes);
void release_alt(svdw_ctx* c);                             // frees the pipeline's other cell set
void clear_streams(svdw_ctx* c);                           // empty streams, an empty witness record
bool lane_fits(svdw_ctx* c);                               // "lanes": the next call may run on the other state
void lane_switch(svdw_ctx* c);                             // "lanes": exchanges this state with the lane's
hipEvent_t xevent(svdw_ctx* c, int i);                     // the i-th hand-off event of a state, made on first use
// ---- engine.cpp
void flush_batch(svdw_ctx* c, hipStream_t s, hipStream_t waiter = nullptr, hipEvent_t then_wait = nullptr);
DView view_of(svdw_ctx* c, const svdw_mat& m);             // the cells of m as a kernel's operand
// ---- engine.cpp, for the witness calls (witness.cpp): each is described where it is defined
Fr fr_from_words(const uint64_t w[4]);                     // an entry's four words as a value mod p
hipEvent_t stream_dep(svdw_ctx* c, hipStream_t from, hipStream_t to);
void dep_wait(svdw_ctx* c, hipStream_t s, hipEvent_t e);
void host_mark(svdw_ctx* c, const char* what);
void grow(svdw_ctx* c, Fr*& ptr, uint64_t used, uint64_t& cap, uint64_t need);
void append(svdw_ctx* c, uint32_t phase, uint64_t n, uint64_t nl, uint64_t* off, uint64_t* loff, const char* tag,
            uint64_t rows = 1);
svdw_vec put_cell(svdw_ctx* c, uint32_t phase, const Fr& v, bool constant = false);
svdw_mat zkmatrix_new(svdw_ctx* c, uint32_t phase, const double* data, uint32_t rows, uint32_t cols, bool on_device,
                      unsigned* blockmax = nullptr, QuantSegs* qs = nullptr, bool own_rows_only = false,
                      bool own_rows_cols = false);
void gamma_prep(svdw_ctx* c, uint32_t d, const Fr& gamma, hipStream_t s, const PowCells* pc = nullptr);
struct VMul {                                              // one verify_mul: c_s = a * b
    svdw_mat a, b, cs;
};
void verify_mul_many(svdw_ctx* c, uint32_t phase, const VMul* vm, int n, const Fr& gamma);
void err_calc(uint32_t p, uint64_t size, double max_norm, double eps_svd, double eps_u, double* es, double* eu);
svdw_svd_payload check_svd_phase0(svdw_ctx* c, const svdw_mat& m, const svdw_mat& u, const svdw_mat& v,
                                  const svdw_vec& d, double err_svd, double err_u, uint32_t max_bits_d,
                                  const uint32_t* known_bits = nullptr, const unsigned* dev_bits = nullptr,
                                  bool dev_quantized = false);
void check_svd_phase1(svdw_ctx* c, const svdw_mat& m, const svdw_mat& u, const svdw_mat& v, const svdw_svd_payload& pl,
                      const Fr& g);
// ---- gemm.cpp: the exact field product c_s = a * b
extern const uint32_t kCrtMaxK;                            // largest inner dimension of the integer GEMMs
// The rules of a witness call's products: the CRT path applies (inner dimension
// K); the residue planes also come straight from the f64 inputs, dims = the
// largest inner dimension of the call's products ("res_f64", matrix cores);
// "prod_cell"'s value with -1 resolved.
bool crt_product(const svdw_ctx* c, uint32_t K);
bool crt_product_f64(const svdw_ctx* c, uint32_t dims);
bool products_on_cell_stream(const svdw_ctx* c);
bool is_transpose_of(const svdw_mat& b, const svdw_mat& a);
// max over each matrix of bit-length(|signed(x)|), read back (the host waits)
std::vector<uint32_t> maxbits_many(svdw_ctx* c, const std::vector<svdw_mat>& ms);
void gemm_exec(svdw_ctx* c, hipStream_t s, const svdw_mat& a, const svdw_mat& b, Fr* out, uint32_t bits_a,
               uint32_t bits_b, const unsigned* sa = nullptr, const unsigned* sb = nullptr, bool quantized = false,
               const unsigned* b_cover = nullptr, bool a_from_b = false, DBuf* bbuf = nullptr, bool b_ready = false);
// check_svd_phase0's three products from the f64 inputs in two steps, so the
// caller orders other streams between the residue planes and the GEMMs
void svd_residues_f64(svdw_ctx* c, const svdw_mat (&A)[3], const unsigned* W, hipStream_t pst);
void svd_products_f64(svdw_ctx* c, const svdw_mat (&A)[3], const svdw_mat (&B)[3], const std::vector<uint64_t>& log,
                      uint32_t phase, const unsigned* W, hipStream_t pst);
// verify_mul_witness's product from its f64 inputs
void product_f64(svdw_ctx* c, hipStream_t s, const double* a, const double* b, uint32_t N, uint32_t K, uint32_t M,
                 Fr* out, const unsigned* dbits);
// ---- prover.cpp: the context's table of omega_k's powers, uploaded on first use (ProverState::DomainSlot)
const ProverState::DomainSlot& domain_table(svdw_ctx* c, uint32_t k);
// ---- small helpers that more than one file needs
// Device bytes held by a set of cell streams (both phases, advice + lookups).
inline double set_bytes(const Stream (&s)[2]) {
    return 32.0 * (double)(s[0].cap + s[0].lcap + s[1].cap + s[1].lcap);
}
// The captured verify_mul_witness (engine.cpp) no longer applies.
inline void vmg_drop(svdw_ctx* c) {
    if (c->vmg.exec) (void)hipGraphExecDestroy(c->vmg.exec);
    c->vmg.exec = nullptr;
    c->vmg.key.clear();
}
inline svdw_mat mat_of_vec(const svdw_vec& v) {   // len x 1 column
    return svdw_mat{v.phase, v.len, 1, v.off, v.stride, 0};
}
inline void check_mat(const svdw_ctx* c, const svdw_mat& m) {
    REQUIRE(m.phase < 2, "matrix phase must be 0 or 1");
    REQUIRE(m.rows >= 1 && m.cols >= 1, "empty matrix");
    // every referenced cell must already exist
    int64_t lo = (int64_t)m.off, hi = (int64_t)m.off;
    int64_t er = (int64_t)(m.rows - 1) * m.rs, ec = (int64_t)(m.cols - 1) * m.cs;
    lo += std::min<int64_t>(er, 0) + std::min<int64_t>(ec, 0);
    hi += std::max<int64_t>(er, 0) + std::max<int64_t>(ec, 0);
    REQUIRE(lo >= 0 && (uint64_t)hi < c->ph[m.phase].n, "matrix view outside its phase stream");
}
inline void check_vec(const svdw_ctx* c, const svdw_vec& v) { check_mat(c, mat_of_vec(v)); }
// A dry context of precision p and lookup bits lb, for a replay that plans:
// empty, or starting at the stream counts of `at`.
struct PlanCtx : svdw_ctx {
    PlanCtx(uint32_t p, uint32_t lb, const svdw_ctx* at = nullptr) {
        P = p;
        LB = lb;
        for (int i = 0; at && i < 2; ++i) { ph[i].n = at->ph[i].n; ph[i].nl = at->ph[i].nl; }
    }
};
// Launches go out on c->st: this scope sends those queued inside it to a side
// stream instead, by exchanging st with that stream's slot (&c->st2, &c->st3;
// null: no redirection) until it ends, by end() or by unwinding. (st_cell and
// stream_id still name the streams as created.)
struct OnStream {
    svdw_ctx* c;
    hipStream_t* slot;
    OnStream(svdw_ctx* cc, hipStream_t* s) : c(cc), slot(s) {
        if (slot) std::swap(c->st, *slot);
    }
    OnStream(const OnStream&) = delete;
    OnStream& operator=(const OnStream&) = delete;
    ~OnStream() { end(); }
    void end() {
        if (slot) std::swap(c->st, *slot);
        slot = nullptr;
    }
    bool on() const { return slot != nullptr; }
};
inline uint64_t f64_key(double x) {                        // a double in a replay's cache key
    uint64_t k;
    memcpy(&k, &x, sizeof k);
    return k;
}
#pragma GCC visibility pop
inline bool sharded(const svdw_ctx* c) { return c->opt.shard_world > 1; }
// rows of a row-parallel stage (R rows) that this rank computes / owns
inline void shard_rows(const svdw_ctx* c, uint64_t R, uint64_t* r0, uint64_t* r1) {
    *r0 = R * c->opt.shard_rank / c->opt.shard_world;
    *r1 = R * (c->opt.shard_rank + 1) / c->opt.shard_world;
}
inline Fr* cellp(svdw_ctx* c, uint32_t phase, uint64_t off) { return c->ph[phase].adv + off; }
inline svdw_mat transposed(const svdw_mat& m) {
    return svdw_mat{m.phase, m.cols, m.rows, m.off, m.cs, m.rs};
}
inline uint32_t clog2(uint32_t k) {                        // least l with 2^l >= k
    uint32_t l = 0;
    while ((1ull << l) < k) ++l;
    return l;
}
inline uint32_t ceil_to(uint32_t x, uint32_t a) { return (x + a - 1) / a * a; }
// The check every device entry makes, under the entry's name f.
inline void need_device(const svdw_ctx* c, const std::string& f) { REQUIRE(!c->dry, f + " needs a device context"); }
// The scratch cap of a G1 call in bytes (the option "commit_scratch_mib").
inline uint64_t scratch_cap(const svdw_ctx* c) { return (uint64_t)c->opt.commit_scratch_mib << 20; }
// RAII: brackets one kernel launch with HIP events on the context stream.
struct ProfScope {
    svdw_ctx* c;
    long idx = -1;
    static hipEvent_t ev(svdw_ctx* c) {
        if (!c->pool.empty()) {
            hipEvent_t e = c->pool.back();
            c->pool.pop_back();
            return e;
        }
        // timing-only events: skip the system-scope fence (cache writeback and
        // invalidate) a default event performs, which would perturb what it measures
        hipEvent_t e;
        hipck(hipEventCreateWithFlags(&e, hipEventDisableSystemFence), "hipEventCreate");
        return e;
    }
    hipStream_t s = nullptr;
    bool ext = false;                       // stage launches: events recorded by their dispatch
    // stage: the scope holds stage launches only (launch_stage*), which record
    // the events themselves (set_launch_events): no event records between the
    // launches, which cost a few us of stream time each
    ProfScope(svdw_ctx* cc, hipStream_t ss, const std::string& name, double bytes, double ops,
              bool batch = false, bool stage = false)
        : c(cc), s(ss) {
        if (!batch) flush_batch(c, s);      // earlier batched stages go first
        if (!c->opt.prof || c->dry) return;
        if (!c->opt.prof_filter.empty() && name.compare(0, c->opt.prof_filter.size(), c->opt.prof_filter) != 0)
            return;
        // every launch is tagged with its stream (@cell, @s2, @s3 as created), so a
        // bench can report the busiest stream's stage rate beside the all-stream one
        const char* tag = s == c->stream_id[0] ? "@cell" : s == c->stream_id[1] ? "@s2"
                          : s == c->stream_id[2] ? "@s3" : "";
        svdw_ctx::Rec r{name + tag, bytes, ops, ev(c), ev(c)};
        ext = stage;
        if (ext)
            set_launch_events(r.e0, r.e1);
        else
            hipck(hipEventRecord(r.e0, s), "hipEventRecord");
        c->recs.push_back(r);
        idx = (long)c->recs.size() - 1;
    }
    ~ProfScope() {
        if (idx < 0) return;
        if (ext && launch_events_used()) return;
        if (ext) (void)hipEventRecord(c->recs[idx].e0, s);       // nothing launched: an empty interval
        (void)hipEventRecord(c->recs[idx].e1, s);
    }
};
// ------------------------------------------------------- the staged call
// What a call staged in the context's scratch ("Host code of the calls
// on a witness and the staged-call layout"): 128 bytes of counters, the pointers
// padded to 32 bytes, the Fr cells, then the call's own arrays from `free` on.
struct Staged {
    unsigned long long* cnt = nullptr;
    const Fr* const* ptrs = nullptr;
    const Fr* cells = nullptr;
    char* free = nullptr;
};
// Size the scratch for the na pointers of a then the nb of b, ncells Fr cells
// (written by fill) and scratch_bytes after them; zero the counters on the
// stream, and with them the first `zeroed` bytes of free where nothing is
// uploaded in between; upload pointers and cells in one copy.
template <class Fill>
Staged stage(svdw_ctx* c, const void* const* a, uint32_t na, const void* const* b, uint32_t nb, size_t ncells,
             size_t scratch_bytes, Fill&& fill, size_t zeroed = 0) {
    StagedScratch& ss = c->staging;
    const size_t pbytes = ((size_t)(na + nb) * sizeof(void*) + 31) / 32 * 32, up = pbytes + ncells * sizeof(Fr);
    REQUIRE(!zeroed || !up, "internal: zeroed scratch behind an upload");
    ss.upload.assign(up, 0);
    if (na) memcpy(ss.upload.data(), a, na * sizeof(void*));
    if (nb) memcpy(ss.upload.data() + na * sizeof(void*), b, nb * sizeof(void*));
    fill((Fr*)(ss.upload.data() + pbytes));
    ensure_buf(c, ss.buf, 128 + up + scratch_bytes);
    char* base = (char*)ss.buf.p;
    hipck(hipMemsetAsync(base, 0, 128 + zeroed, c->st), "hipMemsetAsync");
    if (up) hipck(hipMemcpyAsync(base + 128, ss.upload.data(), up, hipMemcpyHostToDevice, c->st), "H2D");
    return Staged{(unsigned long long*)base, (const Fr* const*)(base + 128), (const Fr*)(base + 128 + pbytes),
                  base + 128 + up};
}
// The cells as `bytes` bytes of anything (a call's words, bit tables, indices),
// copied from src: the kernels read them from Staged::cells on.
inline Staged stage_bytes(svdw_ctx* c, const void* src, size_t bytes, size_t scratch_bytes = 0) {
    const auto fill = [&](Fr* t) { if (bytes) memcpy(t, src, bytes); };
    return stage(c, nullptr, 0, nullptr, 0, (bytes + sizeof(Fr) - 1) / sizeof(Fr), scratch_bytes, fill);
}
// The counters alone, and scratch_bytes whose first `zeroed` are zeroed with them.
inline Staged stage_counters(svdw_ctx* c, size_t scratch_bytes = 0, size_t zeroed = 0) {
    return stage(c, nullptr, 0, nullptr, 0, 0, scratch_bytes, [](Fr*) {}, zeroed);
}
// h[0..n) = the counters, once the stream has run dry.
inline void read_counters(svdw_ctx* c, const unsigned long long* cnt, unsigned long long* h, size_t n) {
    hipck(hipMemcpyAsync(h, cnt, n * sizeof *h, hipMemcpyDeviceToHost, c->st), "D2H");
    hipck(hipStreamSynchronize(c->st), "hipStreamSynchronize");
}
// One launch on the context's stream under its profile label.
template <class Launch>
void profiled(svdw_ctx* c, const char* label, double bytes, Launch&& launch) {
    ProfScope ps(c, c->st, label, bytes, 0);
    hipck(launch(), label);
}
