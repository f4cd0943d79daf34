// KZG commitments of columns on the device (commit.hip): for each column of
// n = 2^k Fr cells the multi-scalar multiplication sum_i s_i P_i over n shared
// BN254 G1 bases (g1.hpp), and a bit-serial checker that shares nothing with it.
//
// Pippenger with signed c-bit digits. A cell, as a canonical integer below
// r < 2^254, is cut into W = ceil(255 / c) digits d_w in (-2^(c-1), 2^(c-1)]
// with carry (g1_signed_digits, g1_mul.hpp: the one recoder of this family, the
// SRS's and the G1 transforms'); a negative digit adds the base with
// y -> q - y. A task is one (column, window); task
// g = column W + window. Tasks run in batches of T under the workspace cap
// (commit_task_bytes; the option "commit_scratch_mib"); per batch:
//
//  k_commit_digits<false>  cursor[t][|d| - 1] += 1 for every non-zero digit of a
//                          non-identity base (zero digits and identity bases are
//                          dropped here, and counted once per call)
//  k_commit_scan           start = exclusive scan of cursor over the B = 2^(c-1)
//                          buckets, start[B] = m the task's entries; cursor = start
//  k_commit_digits<true>   sorted[t][cursor[b]++] = row | sign << 31
//  k_commit_runs           the sorted list cut into runs of kCommitRun entries,
//                          whatever the bucket boundaries; thread u adds run u with
//                          the mixed add and emits at every boundary it crosses. A
//                          bucket that lies inside the run goes to buckets[t][b];
//                          the first segment of a bucket that began before the run
//                          goes to slot 2u, the last segment of a bucket that goes
//                          on after it to slot 2u + 1 (a run inside one bucket: slot
//                          2u); unused slots are the identity
//  k_commit_tree           level j node i = the sum of nodes 16 i .. 16 i + 15 of
//                          level j - 1 over the slots, while a level has more than
//                          kCommitFan nodes
//  k_commit_fold           the thread in whose run a spanning bucket begins sums its
//                          slots, a contiguous range, from at most 2 (kCommitFan - 1)
//                          nodes per level (nodes inside the range hold nothing else)
//  k_commit_chunks         a thread per kCommitChunk buckets [j0, j0 + ..): the two
//                          running sums S = sum B_j and A = sum (j - j0 + 1) B_j from
//                          the top down, then A + j0 S by double-and-add (bucket j
//                          holds |d| = j + 1)
//  k_commit_window         a block per task tree-sums the chunks in LDS
//
// and after the last batch k_commit_horner, a thread per column: Horner over the
// windows (c doublings each), one Fq inversion to affine, 64 B out. The work of a
// thread is bounded whatever the scalars: kCommitRun mixed adds and as many
// bucket searches (each at most 2 log2 B probes) in k_commit_runs, kCommitFan - 1
// adds in k_commit_tree, 2 (kCommitFan - 1) adds per level, at most 7 levels, in
// k_commit_fold. A column of equal cells (one bucket of n entries) costs what a
// random column costs in k_commit_runs.
//
// The checker: for each bit b < 254, T_b = the sum of the bases whose scalar has
// bit b set (strided mixed adds per thread, an LDS tree per block, partials per
// block), then a block per column folds the partials and runs Horner over the
// bits, one doubling each, and compares with the given affine commitment
// cross-multiplied. k_commit_check_bases counts bases off the curve.
//
// As grand_product.hpp and ntt.hpp ask: loops over points stay rolled (#pragma
// unroll 1 around the inlined laws), no register arrays under a runtime index
// (the digits shift the scalar down instead of indexing its words), 64-bit row
// indices. Points are read and written in bases_form through g1.hpp's
// g1_affine_to_mont and g1_affine_to_form alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fr.hpp"
#include "g1.hpp"
#include "g1_mul.hpp"

namespace svdw {

static constexpr uint32_t kCommitRun = 16;                 // sorted entries per thread of k_commit_runs
static constexpr uint32_t kCommitFan = 16;                 // children per node over the slots
static constexpr uint32_t kCommitChunk = 32;               // buckets per thread of k_commit_chunks
static constexpr uint32_t kCommitMaxBits = 16;             // window bits at the most
static constexpr unsigned kCommitThreads = 256;
static constexpr unsigned kCommitTreeThreads = 128;        // blocks that tree-sum in LDS (16 KiB)
static constexpr uint32_t kCommitScalarBits = 254;         // r < 2^254
static constexpr uint32_t kCommitCheckBlocks = 64;         // row blocks per (column, bit) of the checker at the most

// Window bits c and windows W = ceil(255 / c) of a size-2^k commitment: the c in
// [2, kCommitMaxBits] with the fewest adds, n W sorted (mixed) adds and
// 2 * 2^(c-1) W reduction (full) adds per column, a full add weighed 1.4 mixed
// ones (14 products against 10); made non-decreasing in k.
inline void commit_plan(uint32_t k, uint32_t* window_bits, uint32_t* windows) {
    uint32_t best = 2;
    for (uint32_t kk = 1; kk <= k; ++kk) {
        double cost = 0;
        uint32_t arg = best;
        for (uint32_t c = best; c <= kCommitMaxBits; ++c) {
            const double W = (255 + c - 1) / c;
            const double v = W * ((double)(1ull << kk) + 1.4 * 2.0 * (double)(1ull << (c - 1)));
            if (c == best || v < cost) {
                cost = v;
                arg = c;
            }
        }
        best = arg;
    }
    *window_bits = best;
    *windows = (255 + best - 1) / best;
}

// The slots of one task: 2 per run, and the nodes of every level above them.
__host__ __device__ inline uint64_t commit_slots0(uint64_t n) { return 2 * ((n + kCommitRun - 1) / kCommitRun); }
inline uint64_t commit_slots_all(uint64_t n) {
    uint64_t ns = commit_slots0(n), all = ns;
    while (ns > kCommitFan) {
        ns = (ns + kCommitFan - 1) / kCommitFan;
        all += ns;
    }
    return all;
}
__host__ __device__ inline uint64_t commit_chunks(uint64_t B) { return (B + kCommitChunk - 1) / kCommitChunk; }
// Workspace bytes of one task in a batch.
inline uint64_t commit_task_bytes(uint64_t n, uint64_t B) {
    return 4 * B + 4 * (B + 1 + 3) + 4 * n + sizeof(G1Xyzz) * (commit_slots_all(n) + B + commit_chunks(B));
}

// One batch of T tasks g0 .. g0 + T - 1 of a call. The arrays are the batch's,
// [T][..] each; windows is the call's, [ncols W].
struct CommitBatch {
    const Fr* const* cols;                                 // the call's ncols column pointers (device table)
    const G1Affine* bases;
    uint32_t* cursor;                                      // [T][B]
    uint32_t* start;                                       // [T][B + 1]
    uint32_t* sorted;                                      // [T][n]
    G1Xyzz* slots;                                         // level j at slots + T * (nodes of the levels below), [T][ns_j]
    G1Xyzz* buckets;                                       // [T][B]
    G1Xyzz* chunks;                                        // [T][commit_chunks(B)]
    G1Xyzz* windows;
    unsigned long long* cnt;                               // [0] zero scalars, [1] identity bases, [2] identity outputs
    uint32_t k, c, W, ncols, g0, T;
    int form, bases_form;
};
// Everything of a batch up to its window sums, queued on st.
hipError_t launch_commit_batch(const CommitBatch& a, hipStream_t st);
// out[col] = the affine sum over the windows, in bases_form.
hipError_t launch_commit_horner(const G1Xyzz* windows, uint32_t ncols, uint32_t c, uint32_t W, int bases_form,
                                G1Affine* out, unsigned long long* cnt, hipStream_t st);

inline uint32_t commit_check_blocks(uint64_t n) {
    const uint64_t nb = (n + kCommitTreeThreads - 1) / kCommitTreeThreads;
    return (uint32_t)(nb < kCommitCheckBlocks ? nb : kCommitCheckBlocks);
}
// Columns col0 .. col0 + nc - 1 of cols against commitments; part: nc x 254 x
// commit_check_blocks(n) points. cnt[0] += columns checked, cnt[1] += failures.
hipError_t launch_commit_check(const Fr* const* cols, const G1Affine* bases, const G1Affine* commitments,
                               uint32_t k, uint32_t col0, uint32_t nc, int form, int bases_form, G1Xyzz* part,
                               unsigned long long* cnt, hipStream_t st);
// cnt[2] += bases, cnt[3] += bases that are neither (0, 0) nor on the curve.
hipError_t launch_commit_check_bases(const G1Affine* bases, uint64_t n, int bases_form, unsigned long long* cnt,
                                     hipStream_t st);
// dst[i] = sum of reps copies of (src[i % nsrc] taken as Montgomery affine), by
// repeated mixed adds in registers; a probe of the add rate (tools/commit_bench.py).
hipError_t launch_commit_add_probe(const G1Affine* src, uint32_t nsrc, uint64_t nthreads, uint32_t reps,
                                   G1Xyzz* dst, hipStream_t st);

}  // namespace svdw
