// Kernels of commit.hpp: Pippenger over signed digits with a counting sort per
// (column, window), bucket sums as a segmented reduction over fixed runs, and
// the bit-serial checker.
#include "commit.hpp"

namespace svdw {
namespace {

__device__ __forceinline__ Fr load_scalar(const Fr* col, uint64_t row, int form) {
    const Fr s = col[row];
    return form == 0 ? s : fr_from_mont(s);
}

// SCATTER false: the histogram and the call's counters; true: the scatter.
template <bool SCATTER>
__global__ __launch_bounds__(kCommitThreads) void k_commit_digits(CommitBatch a, uint32_t col_lo) {
    const uint64_t n = 1ull << a.k, row = (uint64_t)blockIdx.x * kCommitThreads + threadIdx.x;
    if (row >= n) return;
    const uint32_t col = col_lo + blockIdx.y, B = 1u << (a.c - 1);
    const uint64_t gcol = (uint64_t)col * a.W;             // the column's first task
    const bool first = gcol >= a.g0 && gcol < (uint64_t)a.g0 + a.T;   // window 0 is in this batch
    const G1Affine p = a.bases[row];
    const bool idb = g1_affine_is_identity(p);
    const Fr s = load_scalar(a.cols[col], row, a.form);
    if (!SCATTER && first) {
        if (fr_is_zero(s)) atomicAdd(&a.cnt[0], 1ull);
        if (idb && col == 0) atomicAdd(&a.cnt[1], 1ull);
    }
    if (idb) return;
    g1_signed_digits(s, a.c, a.W, [&](uint32_t w, uint32_t mag, uint32_t neg) {
        const uint64_t g = gcol + w;
        if (!mag || g < a.g0 || g >= (uint64_t)a.g0 + a.T) return;   // a zero digit adds nothing
        const uint64_t t = g - a.g0;
        const uint32_t b = mag - 1;                        // bucket b holds |d| = b + 1
        if (SCATTER) {
            const uint32_t pos = atomicAdd(&a.cursor[t * B + b], 1u);
            a.sorted[(t << a.k) + pos] = (uint32_t)row | (neg << 31);
        } else {
            atomicAdd(&a.cursor[t * B + b], 1u);
        }
    });
}

// start[t] = the exclusive scan of cursor[t], start[t][B] the total; cursor = start.
__global__ __launch_bounds__(kCommitThreads) void k_commit_scan(CommitBatch a) {
    __shared__ uint32_t sh[kCommitThreads];
    const uint32_t B = 1u << (a.c - 1), t = blockIdx.x, tid = threadIdx.x;
    uint32_t* cur = a.cursor + (uint64_t)t * B;
    uint32_t* st = a.start + (uint64_t)t * (B + 1);
    const uint32_t per = (B + kCommitThreads - 1) / kCommitThreads;
    const uint32_t lo = min(tid * per, B), hi = min(lo + per, B);
    uint32_t sum = 0;
    for (uint32_t i = lo; i < hi; ++i) sum += cur[i];
    sh[tid] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < kCommitThreads; d <<= 1) {    // inclusive scan of the threads' sums
        const uint32_t v = tid >= d ? sh[tid - d] : 0;
        __syncthreads();
        sh[tid] += v;
        __syncthreads();
    }
    uint32_t base = sh[tid] - sum;
    for (uint32_t i = lo; i < hi; ++i) {
        const uint32_t v = cur[i];
        st[i] = base;
        cur[i] = base;
        base += v;
    }
    if (tid == kCommitThreads - 1) st[B] = sh[tid];
}

// The largest b in [lo, B) with st[b] <= pos, given st[lo] <= pos: a gallop from
// lo, then a bisection; at most 2 log2 B probes.
__device__ __forceinline__ uint32_t bucket_of(const uint32_t* st, uint32_t B, uint32_t pos, uint32_t lo) {
    uint32_t step = 1;
    while (lo + step < B && st[lo + step] <= pos) {
        lo += step;
        step <<= 1;
    }
    uint32_t hi = min(lo + step, B);
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (st[mid] <= pos) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kCommitThreads) void k_commit_runs(CommitBatch a) {
    const uint64_t n = 1ull << a.k, nruns = (n + kCommitRun - 1) / kCommitRun;
    const uint64_t u = (uint64_t)blockIdx.x * kCommitThreads + threadIdx.x;
    if (u >= nruns) return;
    const uint32_t B = 1u << (a.c - 1), t = blockIdx.y;
    const uint32_t* st = a.start + (uint64_t)t * (B + 1);
    const uint32_t* sorted = a.sorted + ((uint64_t)t << a.k);
    G1Xyzz* slot = a.slots + (uint64_t)t * (2 * nruns) + 2 * u;
    G1Xyzz* bucket = a.buckets + (uint64_t)t * B;
    slot[0] = g1_identity();
    slot[1] = g1_identity();
    const uint32_t m = st[B];
    const uint64_t begin64 = u * kCommitRun;
    if (begin64 >= m) return;
    const uint32_t begin = (uint32_t)begin64, end = min(begin + kCommitRun, m);
    uint32_t b = bucket_of(st, B, begin, 0), bend = st[b + 1];
    G1Xyzz acc = g1_identity();
#pragma unroll 1
    for (uint32_t pos = begin; pos < end; ++pos) {
        if (pos == bend) {                                 // a boundary: the segment of bucket b ends here
            if (st[b] >= begin) bucket[b] = acc;
            else slot[0] = acc;
            acc = g1_identity();
            b = bucket_of(st, B, pos, b + 1);
            bend = st[b + 1];
        }
        const uint32_t e = sorted[pos];
        G1Affine p = g1_affine_to_mont(a.bases[e & 0x7fffffffu], a.bases_form);
        if (e >> 31) p.y = fq_neg(p.y);
        acc = g1_add_mixed(acc, p);
    }
    if (st[b] < begin) slot[0] = acc;                      // began before the run (and may go on after it)
    else if (bend > end) slot[1] = acc;                    // begins here, goes on
    else bucket[b] = acc;
}

// Level `lev` (>= 1) of the slots from the level below.
__global__ __launch_bounds__(kCommitThreads) void k_commit_tree(CommitBatch a, uint64_t off_below, uint64_t n_below,
                                                                uint64_t n_here) {
    const uint64_t i = (uint64_t)blockIdx.x * kCommitThreads + threadIdx.x;
    if (i >= n_here) return;
    const uint32_t t = blockIdx.y;
    const G1Xyzz* src = a.slots + off_below * a.T + (uint64_t)t * n_below;
    G1Xyzz* dst = a.slots + (off_below + n_below) * a.T + (uint64_t)t * n_here;
    const uint64_t lo = i * kCommitFan, hi = min(lo + kCommitFan, n_below);
    G1Xyzz acc = src[lo];
#pragma unroll 1
    for (uint64_t j = lo + 1; j < hi; ++j) acc = g1_add(acc, src[j]);
    dst[i] = acc;
}

// The sum of slots [lo, hi) of task t: whole nodes where the range holds them.
__device__ __forceinline__ G1Xyzz slots_sum(const CommitBatch& a, uint32_t t, uint64_t lo, uint64_t hi) {
    const uint64_t n = 1ull << a.k;
    uint64_t ns = commit_slots0(n), off = 0;
    G1Xyzz acc = g1_identity();
#pragma unroll 1
    while (lo < hi) {
        const G1Xyzz* lev = a.slots + off * a.T + (uint64_t)t * ns;
        const bool top = ns <= kCommitFan;
        const uint64_t lo_up = top ? hi : min((lo + kCommitFan - 1) / kCommitFan * kCommitFan, hi);
        const uint64_t hi_dn = top ? hi : max(hi / kCommitFan * kCommitFan, lo_up);
        uint64_t i = lo == lo_up ? hi_dn : lo;             // [lo, lo_up) then [hi_dn, hi)
#pragma unroll 1
        while (i < hi) {
            acc = g1_add(acc, lev[i]);
            if (++i == lo_up) i = hi_dn;
        }
        if (top) break;
        lo = lo_up / kCommitFan;
        hi = hi_dn / kCommitFan;
        off += ns;
        ns = (ns + kCommitFan - 1) / kCommitFan;
    }
    return acc;
}

__global__ __launch_bounds__(kCommitThreads) void k_commit_fold(CommitBatch a) {
    const uint64_t n = 1ull << a.k, nruns = (n + kCommitRun - 1) / kCommitRun;
    const uint64_t u = (uint64_t)blockIdx.x * kCommitThreads + threadIdx.x;
    if (u >= nruns) return;
    const uint32_t B = 1u << (a.c - 1), t = blockIdx.y;
    const uint32_t* st = a.start + (uint64_t)t * (B + 1);
    const uint32_t m = st[B];
    const uint64_t begin = u * kCommitRun;
    if (begin >= m) return;
    const uint32_t end = (uint32_t)min(begin + kCommitRun, (uint64_t)m);
    const uint32_t b = bucket_of(st, B, end - 1, 0);
    if (st[b] < begin || st[b + 1] <= end) return;         // no spanning bucket begins in this run
    const uint64_t u1 = (st[b + 1] - 1) / kCommitRun;      // the run it ends in
    a.buckets[(uint64_t)t * B + b] = slots_sum(a, t, 2 * u + 1, 2 * u1 + 1);
}

__global__ __launch_bounds__(kCommitThreads) void k_commit_chunks(CommitBatch a) {
    const uint32_t B = 1u << (a.c - 1), t = blockIdx.y;
    const uint32_t nch = (uint32_t)commit_chunks(B), ch = blockIdx.x * kCommitThreads + threadIdx.x;
    if (ch >= nch) return;
    const G1Xyzz* bucket = a.buckets + (uint64_t)t * B;
    const uint32_t j0 = ch * kCommitChunk, hi = min(j0 + kCommitChunk, B);
    G1Xyzz run = g1_identity(), acc = g1_identity();
#pragma unroll 1
    for (uint32_t j = hi; j-- > j0;) {
        run = g1_add(run, bucket[j]);
        acc = g1_add(acc, run);
    }
    G1Xyzz sc = g1_identity();                             // j0 run
#pragma unroll 1
    for (int bit = (int)kCommitMaxBits - 1; bit >= 0; --bit) {
        sc = g1_double(sc);
        if ((j0 >> bit) & 1) sc = g1_add(sc, run);
    }
    a.chunks[(uint64_t)t * nch + ch] = g1_add(acc, sc);
}

// The block's sum of acc over its kCommitTreeThreads threads, in thread 0.
__device__ __forceinline__ G1Xyzz block_sum(G1Xyzz acc, G1Xyzz* sh) {
    const uint32_t tid = threadIdx.x;
    sh[tid] = acc;
    __syncthreads();
#pragma unroll 1
    for (uint32_t s = kCommitTreeThreads / 2; s > 0; s >>= 1) {
        if (tid < s) sh[tid] = g1_add(sh[tid], sh[tid + s]);
        __syncthreads();
    }
    return sh[0];
}

__global__ __launch_bounds__(kCommitTreeThreads) void k_commit_window(CommitBatch a) {
    __shared__ G1Xyzz sh[kCommitTreeThreads];
    const uint32_t B = 1u << (a.c - 1), t = blockIdx.x, nch = (uint32_t)commit_chunks(B);
    const G1Xyzz* chunk = a.chunks + (uint64_t)t * nch;
    G1Xyzz acc = g1_identity();
#pragma unroll 1
    for (uint32_t i = threadIdx.x; i < nch; i += kCommitTreeThreads) acc = g1_add(acc, chunk[i]);
    acc = block_sum(acc, sh);
    if (threadIdx.x == 0) a.windows[(uint64_t)a.g0 + t] = acc;
}

__global__ __launch_bounds__(64) void k_commit_horner(const G1Xyzz* windows, uint32_t ncols, uint32_t c, uint32_t W,
                                                      int bases_form, G1Affine* out, unsigned long long* cnt) {
    const uint32_t col = blockIdx.x * 64 + threadIdx.x;
    if (col >= ncols) return;
    const G1Xyzz* win = windows + (uint64_t)col * W;
    G1Xyzz acc = g1_identity();
#pragma unroll 1
    for (uint32_t w = W; w-- > 0;) {
#pragma unroll 1
        for (uint32_t i = 0; i < c; ++i) acc = g1_double(acc);
        acc = g1_add(acc, win[w]);
    }
    if (g1_is_identity(acc)) atomicAdd(&cnt[2], 1ull);
    out[col] = g1_affine_to_form(g1_to_affine(acc), bases_form);
}

// ---- the checker
__global__ __launch_bounds__(kCommitTreeThreads) void k_commit_check_bits(const Fr* const* cols, const G1Affine* bases,
                                                                          uint32_t k, uint32_t col0, int form,
                                                                          int bases_form, G1Xyzz* part) {
    __shared__ G1Xyzz sh[kCommitTreeThreads];
    const uint64_t n = 1ull << k;
    const uint32_t bit = blockIdx.y, lc = blockIdx.z, wi = bit >> 5, sh_bit = bit & 31;
    const Fr* col = cols[col0 + lc];
    G1Xyzz acc = g1_identity();
#pragma unroll 1
    for (uint64_t row = (uint64_t)blockIdx.x * kCommitTreeThreads + threadIdx.x; row < n;
         row += (uint64_t)gridDim.x * kCommitTreeThreads) {
        const Fr s = load_scalar(col, row, form);
        uint32_t word = s.w[0];                            // select chain: no run-time index into s
#pragma unroll
        for (int j = 1; j < 8; ++j) word = (wi == (uint32_t)j) ? s.w[j] : word;
        if ((word >> sh_bit) & 1) acc = g1_add_mixed(acc, g1_affine_to_mont(bases[row], bases_form));
    }
    acc = block_sum(acc, sh);
    if (threadIdx.x == 0) part[((uint64_t)lc * kCommitScalarBits + bit) * gridDim.x + blockIdx.x] = acc;
}

__global__ __launch_bounds__(kCommitThreads) void k_commit_check_fold(const G1Xyzz* part, uint32_t nb,
                                                                      const G1Affine* commitments, uint32_t col0,
                                                                      int bases_form, unsigned long long* cnt) {
    __shared__ G1Xyzz sh[kCommitThreads];
    const uint32_t lc = blockIdx.x, bit = threadIdx.x;
    G1Xyzz acc = g1_identity();
    if (bit < kCommitScalarBits) {
        const G1Xyzz* p = part + ((uint64_t)lc * kCommitScalarBits + bit) * nb;
#pragma unroll 1
        for (uint32_t i = 0; i < nb; ++i) acc = g1_add(acc, p[i]);
    }
    sh[bit] = acc;
    __syncthreads();
    if (bit != 0) return;
    acc = g1_identity();
#pragma unroll 1
    for (uint32_t b = kCommitScalarBits; b-- > 0;) {
        acc = g1_double(acc);
        acc = g1_add(acc, sh[b]);
    }
    const G1Affine given = commitments[col0 + lc];
    const bool reduced = fq_reduced(given.x) && fq_reduced(given.y);
    atomicAdd(&cnt[0], 1ull);
    if (!reduced || !g1_eq_affine(acc, g1_affine_to_mont(given, bases_form))) atomicAdd(&cnt[1], 1ull);
}

__global__ __launch_bounds__(kCommitThreads) void k_commit_check_bases(const G1Affine* bases, uint64_t n, int bases_form,
                                                                       unsigned long long* cnt) {
    const uint64_t row = (uint64_t)blockIdx.x * kCommitThreads + threadIdx.x;
    if (row >= n) return;
    const G1Affine raw = bases[row];
    const bool reduced = fq_reduced(raw.x) && fq_reduced(raw.y);
    const G1Affine p = g1_affine_to_mont(raw, bases_form);
    atomicAdd(&cnt[2], 1ull);
    if (!g1_affine_is_identity(raw) && !(reduced && g1_on_curve(p))) atomicAdd(&cnt[3], 1ull);
}

__global__ __launch_bounds__(kCommitThreads) void k_commit_add_probe(const G1Affine* src, uint32_t nsrc,
                                                                     uint64_t nthreads, uint32_t reps, G1Xyzz* dst) {
    const uint64_t i = (uint64_t)blockIdx.x * kCommitThreads + threadIdx.x;
    if (i >= nthreads) return;
    const G1Affine p = src[i % nsrc];
    G1Xyzz acc = g1_from_affine(src[(i + 1) % nsrc]);
#pragma unroll 1
    for (uint32_t r = 0; r < reps; ++r) acc = g1_add_mixed(acc, p);
    dst[i] = acc;
}

}  // namespace

hipError_t launch_commit_batch(const CommitBatch& a, hipStream_t st) {
    const uint64_t n = 1ull << a.k, B = 1ull << (a.c - 1), nruns = (n + kCommitRun - 1) / kCommitRun;
    hipError_t e = hipMemsetAsync(a.cursor, 0, (size_t)a.T * B * sizeof(uint32_t), st);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(a.buckets, 0, (size_t)a.T * B * sizeof(G1Xyzz), st);   // all-zero words: the identity
    if (e != hipSuccess) return e;
    // the columns this batch's tasks belong to
    const uint32_t col_lo = a.g0 / a.W, col_hi = (uint32_t)(((uint64_t)a.g0 + a.T - 1) / a.W);
    const dim3 gd(blocks_of(n, kCommitThreads), col_hi - col_lo + 1);
    hipLaunchKernelGGL(k_commit_digits<false>, gd, dim3(kCommitThreads), 0, st, a, col_lo);
    hipLaunchKernelGGL(k_commit_scan, dim3(a.T), dim3(kCommitThreads), 0, st, a);
    hipLaunchKernelGGL(k_commit_digits<true>, gd, dim3(kCommitThreads), 0, st, a, col_lo);
    const dim3 gr(blocks_of(nruns, kCommitThreads), a.T);
    hipLaunchKernelGGL(k_commit_runs, gr, dim3(kCommitThreads), 0, st, a);
    uint64_t off = 0, ns = commit_slots0(n);
    while (ns > kCommitFan) {
        const uint64_t up = (ns + kCommitFan - 1) / kCommitFan;
        hipLaunchKernelGGL(k_commit_tree, dim3(blocks_of(up, kCommitThreads), a.T), dim3(kCommitThreads), 0, st, a,
                           off, ns, up);
        off += ns;
        ns = up;
    }
    hipLaunchKernelGGL(k_commit_fold, gr, dim3(kCommitThreads), 0, st, a);
    hipLaunchKernelGGL(k_commit_chunks, dim3(blocks_of(commit_chunks(B), kCommitThreads), a.T),
                       dim3(kCommitThreads), 0, st, a);
    hipLaunchKernelGGL(k_commit_window, dim3(a.T), dim3(kCommitTreeThreads), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_commit_horner(const G1Xyzz* windows, uint32_t ncols, uint32_t c, uint32_t W, int bases_form,
                                G1Affine* out, unsigned long long* cnt, hipStream_t st) {
    hipLaunchKernelGGL(k_commit_horner, dim3(blocks_of(ncols, 64)), dim3(64), 0, st, windows, ncols, c, W, bases_form,
                       out, cnt);
    return hipGetLastError();
}

hipError_t launch_commit_check(const Fr* const* cols, const G1Affine* bases, const G1Affine* commitments,
                               uint32_t k, uint32_t col0, uint32_t nc, int form, int bases_form, G1Xyzz* part,
                               unsigned long long* cnt, hipStream_t st) {
    const uint32_t nb = commit_check_blocks(1ull << k);
    hipLaunchKernelGGL(k_commit_check_bits, dim3(nb, kCommitScalarBits, nc), dim3(kCommitTreeThreads), 0, st, cols,
                       bases, k, col0, form, bases_form, part);
    hipLaunchKernelGGL(k_commit_check_fold, dim3(nc), dim3(kCommitThreads), 0, st, part, nb, commitments, col0,
                       bases_form, cnt);
    return hipGetLastError();
}

hipError_t launch_commit_check_bases(const G1Affine* bases, uint64_t n, int bases_form, unsigned long long* cnt,
                                     hipStream_t st) {
    hipLaunchKernelGGL(k_commit_check_bases, dim3(blocks_of(n, kCommitThreads)), dim3(kCommitThreads), 0, st, bases,
                       n, bases_form, cnt);
    return hipGetLastError();
}

hipError_t launch_commit_add_probe(const G1Affine* src, uint32_t nsrc, uint64_t nthreads, uint32_t reps,
                                   G1Xyzz* dst, hipStream_t st) {
    hipLaunchKernelGGL(k_commit_add_probe, dim3(blocks_of(nthreads, kCommitThreads)), dim3(kCommitThreads), 0, st,
                       src, nsrc, nthreads, reps, dst);
    return hipGetLastError();
}

}  // namespace svdw
