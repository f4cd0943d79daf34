// gfx950 kernels that build sigma from the copy constraints and check a mapping
// (permutation_cycles.hpp). Integer work only: per cell the builder reads and
// writes some 30 bytes outside the sort and 16 bytes per member and sort pass;
// the union's cost is the depth of the trees it meets, which path halving keeps
// short. Cell ids are uint32_t, every index that counts cells is uint64_t
// (cells may be 2^32).
#include <hip/hip_runtime.h>

#include "permutation_cycles.hpp"

namespace svdw {

// ------------------------------------------------------------------ helpers
__device__ __forceinline__ uint32_t pc_ld(const uint32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void pc_st(uint32_t* p, uint32_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint64_t pc_entry(const PcShape& s, uint64_t id) {
    return (id >> s.k) << 32 | (id & (s.rows - 1));
}
// The id of entry e = col << 32 | row if it is a cell of the first `rows` rows.
__device__ __forceinline__ bool pc_cell(const PcShape& s, uint64_t e, uint64_t rows, uint32_t& id) {
    const uint64_t col = e >> 32, row = e & 0xffffffffull;
    if (col >= s.total_cols || row >= rows) return false;
    id = (uint32_t)(col << s.k | row);
    return true;
}
// g += the wave's sum of v (every lane of the wave calls it).
__device__ __forceinline__ void pc_count(unsigned long long* g, uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(g, (unsigned long long)v);
}
// The exclusive prefix of v over the block's threads and the block's total.
__device__ __forceinline__ uint64_t pc_block_scan(uint64_t v, uint64_t& total) {
    __shared__ uint64_t sh[kPcThreads];
    const uint32_t t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
#pragma unroll 1
    for (uint32_t d = 1; d < kPcThreads; d <<= 1) {
        const uint64_t x = t >= d ? sh[t - d] : 0;
        __syncthreads();
        sh[t] += x;
        __syncthreads();
    }
    const uint64_t incl = sh[t];
    total = sh[kPcThreads - 1];
    __syncthreads();
    return incl - v;
}
static unsigned pc_grid(uint64_t n) {
    const uint64_t nb = (n + kPcThreads - 1) / kPcThreads;
    return (unsigned)(nb < 8192 ? (nb ? nb : 1) : 8192);
}
static bool pc_bad(const PcShape& s) {
    return s.k < 1 || s.k > 28 || !s.total_cols || s.rows != (1ull << s.k) || s.usable > s.rows ||
           s.cells != ((uint64_t)s.total_cols << s.k) || s.cells > (1ull << 32);
}

// -------------------------------------------------------------------- union
__global__ __launch_bounds__(kPcThreads) void k_pc_init(uint64_t n, uint32_t* __restrict__ parent) {
    const uint64_t step = (uint64_t)gridDim.x * kPcThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kPcThreads + threadIdx.x; i < n; i += step) parent[i] = (uint32_t)i;
}
// The root of x as far as this thread can see, with path halving. x only falls.
__device__ __forceinline__ uint32_t pc_find(uint32_t* parent, uint32_t x) {
    for (;;) {
        const uint32_t p = pc_ld(parent + x);
        if (p >= x) return x;                              // p == x: a root
        const uint32_t g = pc_ld(parent + p);
        if (g < p) pc_st(parent + x, g);                   // an ancestor still, whatever else was stored since
        x = g < p ? g : p;
    }
}
__global__ __launch_bounds__(kPcThreads) void k_pc_union(const PcShape s, const uint64_t* __restrict__ edges,
                                                         uint64_t n_edges, uint32_t* parent,
                                                         unsigned long long* cnt) {
    const uint64_t step = (uint64_t)gridDim.x * kPcThreads;
    uint32_t oor = 0, self = 0;
#pragma unroll 1
    for (uint64_t e = (uint64_t)blockIdx.x * kPcThreads + threadIdx.x; e < n_edges; e += step) {
        uint32_t a, b;
        if (!pc_cell(s, edges[2 * e], s.usable, a) || !pc_cell(s, edges[2 * e + 1], s.usable, b)) {
            ++oor;
            continue;
        }
        if (a == b) {
            ++self;
            continue;
        }
#pragma unroll 1
        for (;;) {
            a = pc_find(parent, a);
            b = pc_find(parent, b);
            if (a == b) break;
            const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
            const uint32_t old = atomicCAS(parent + hi, hi, lo);
            if (old == hi) break;
            a = old < hi ? old : lo;                       // hi has a parent by now: old < hi
            b = lo;
        }
    }
    pc_count(cnt, oor);
    pc_count(cnt + 1, self);
}
__global__ __launch_bounds__(kPcThreads) void k_pc_flatten(uint64_t n, uint32_t* parent) {
    const uint64_t step = (uint64_t)gridDim.x * kPcThreads;
#pragma unroll 1
    for (uint64_t i = (uint64_t)blockIdx.x * kPcThreads + threadIdx.x; i < n; i += step) {
        uint32_t p = pc_ld(parent + i);
        if (p >= i) continue;
#pragma unroll 1
        for (;;) {
            const uint32_t q = pc_ld(parent + p);
            if (q >= p) break;
            p = q;
        }
        pc_st(parent + i, p);
    }
}
__global__ __launch_bounds__(kPcThreads) void k_pc_flag(uint64_t n, const uint32_t* __restrict__ parent,
                                                        uint8_t* __restrict__ flag) {
    const uint64_t step = (uint64_t)gridDim.x * kPcThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kPcThreads + threadIdx.x; i < n; i += step) {
        const uint32_t p = parent[i];
        if (p < i) flag[p] = 1;
    }
}

// --------------------------------------------------------------------- scan
// Src: uint32_t operator()(uint64_t i) for i < n. Sink: operator()(i, value,
// the sum of the values before i).
struct PcMember {
    const uint32_t* parent;
    const uint8_t* flag;
    __device__ __forceinline__ uint32_t operator()(uint64_t i) const { return parent[i] != (uint32_t)i || flag[i]; }
};
struct PcCompact {
    const uint32_t* parent;
    uint32_t *key, *val;
    uint64_t m;
    __device__ __forceinline__ void operator()(uint64_t i, uint32_t v, uint64_t at) const {
        if (v && at < m) {
            key[at] = parent[i];
            val[at] = (uint32_t)i;
        }
    }
};
struct PcWords {
    uint32_t* w;
    __device__ __forceinline__ uint32_t operator()(uint64_t i) const { return w[i]; }
    __device__ __forceinline__ void operator()(uint64_t i, uint32_t, uint64_t at) const { w[i] = (uint32_t)at; }
};
template <class Src>
__global__ __launch_bounds__(kPcThreads) void k_pc_sum(const Src src, uint64_t n, uint64_t* __restrict__ bsum) {
    const uint64_t base = (uint64_t)blockIdx.x * kPcTile + (uint64_t)threadIdx.x * kPcItems;
    uint64_t sum = 0, total;
#pragma unroll
    for (uint32_t q = 0; q < kPcItems; ++q)
        if (base + q < n) sum += src(base + q);
    pc_block_scan(sum, total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}
// One block: bsum becomes its exclusive prefix, *total the sum.
__global__ __launch_bounds__(kPcThreads) void k_pc_carry(uint64_t* __restrict__ bsum, uint64_t nb,
                                                         unsigned long long* total) {
    const uint64_t run = (nb + kPcThreads - 1) / kPcThreads;
    const uint64_t lo = threadIdx.x * run < nb ? threadIdx.x * run : nb, hi = lo + run < nb ? lo + run : nb;
    uint64_t sum = 0, all;
#pragma unroll 1
    for (uint64_t j = lo; j < hi; ++j) sum += bsum[j];
    uint64_t acc = pc_block_scan(sum, all);
#pragma unroll 1
    for (uint64_t j = lo; j < hi; ++j) {
        const uint64_t v = bsum[j];
        bsum[j] = acc;
        acc += v;
    }
    if (threadIdx.x == 0 && total) *total = all;
}
template <class Src, class Sink>
__global__ __launch_bounds__(kPcThreads) void k_pc_apply(const Src src, const Sink sink, uint64_t n,
                                                         const uint64_t* __restrict__ bsum) {
    const uint64_t base = (uint64_t)blockIdx.x * kPcTile + (uint64_t)threadIdx.x * kPcItems;
    uint32_t v[kPcItems];
    uint64_t sum = 0, total;
#pragma unroll
    for (uint32_t q = 0; q < kPcItems; ++q) {
        v[q] = base + q < n ? src(base + q) : 0u;
        sum += v[q];
    }
    uint64_t acc = pc_block_scan(sum, total) + bsum[blockIdx.x];
#pragma unroll
    for (uint32_t q = 0; q < kPcItems; ++q) {
        if (base + q < n) sink(base + q, v[q], acc);
        acc += v[q];
    }
}

// --------------------------------------------------------------------- sort
// hist[d * nblk + b] = the keys of block b's tile with digit d.
__global__ __launch_bounds__(kPcThreads) void k_pc_hist(const uint32_t* __restrict__ key, uint64_t m, uint32_t shift,
                                                        uint64_t nblk, uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * kPcSortTile;
#pragma unroll 1
    for (uint32_t j = 0; j < kPcSortIters; ++j) {
        const uint64_t i = base + (uint64_t)j * kPcThreads + threadIdx.x;
        if (i < m) atomicAdd(&h[(key[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[(uint64_t)threadIdx.x * nblk + blockIdx.x] = h[threadIdx.x];
}
// hist scanned over (digit, block). Wave w takes the tile's w-th quarter in order,
// 64 keys a step; a key's place is its digit's start for the block, plus the
// earlier waves' keys of that digit, plus the wave's earlier ones, plus the lanes
// below it in its step: the order of equal digits is kept.
__global__ __launch_bounds__(kPcThreads) void k_pc_scatter(const uint32_t* __restrict__ key,
                                                           const uint32_t* __restrict__ val, uint64_t m,
                                                           uint32_t shift, uint64_t nblk,
                                                           const uint32_t* __restrict__ hist,
                                                           uint32_t* __restrict__ key2, uint32_t* __restrict__ val2) {
    constexpr uint32_t kWaves = kPcThreads / 64;
    __shared__ uint32_t wb[kWaves][256];
    const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (uint32_t q = 0; q < kWaves; ++q) wb[q][threadIdx.x] = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * kPcSortTile + (uint64_t)w * (64 * kPcSortIters) + lane;
#pragma unroll 1
    for (uint32_t j = 0; j < kPcSortIters; ++j) {
        const uint64_t i = base + (uint64_t)j * 64;
        if (i < m) atomicAdd(&wb[w][(key[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    {
        uint32_t at = hist[(uint64_t)threadIdx.x * nblk + blockIdx.x];
        for (uint32_t q = 0; q < kWaves; ++q) {
            const uint32_t c = wb[q][threadIdx.x];
            wb[q][threadIdx.x] = at;
            at += c;
        }
    }
    __syncthreads();
#pragma unroll 1
    for (uint32_t j = 0; j < kPcSortIters; ++j) {          // the same count for every thread: block barriers inside
        const uint64_t i = base + (uint64_t)j * 64;
        const bool ok = i < m;
        const uint32_t kk = ok ? key[i] : 0u, vv = ok ? val[i] : 0u, d = (kk >> shift) & 255u;
        unsigned long long peers = __ballot(ok);
#pragma unroll
        for (uint32_t bit = 0; bit < 8; ++bit) {
            const unsigned long long bb = __ballot(ok && ((d >> bit) & 1u));
            peers &= ((d >> bit) & 1u) ? bb : ~bb;
        }
        const uint32_t rank = __popcll(peers & ((1ull << lane) - 1)), n = __popcll(peers);
        const uint32_t at = ok ? wb[w][d] : 0u;
        __syncthreads();
        if (ok && rank + 1 == n) wb[w][d] = at + n;
        __syncthreads();
        if (ok && (uint64_t)at + rank < m) {
            key2[at + rank] = kk;
            val2[at + rank] = vv;
        }
    }
}

// --------------------------------------------------------------------- link
__global__ __launch_bounds__(kPcThreads) void k_pc_link(const PcShape s, const uint32_t* __restrict__ key,
                                                        const uint32_t* __restrict__ val, uint64_t m,
                                                        uint64_t* __restrict__ mapping, unsigned long long* cnt) {
    __shared__ unsigned long long big;
    if (threadIdx.x == 0) big = 0;
    __syncthreads();
    const uint64_t step = (uint64_t)gridDim.x * kPcThreads;
    uint32_t ends = 0;
    unsigned long long mine = 0;
#pragma unroll 1
    for (uint64_t j = (uint64_t)blockIdx.x * kPcThreads + threadIdx.x; j < m; j += step) {
        const uint32_t r = key[j], c = val[j];
        const bool end = j + 1 == m || key[j + 1] != r;
        const uint32_t next = end ? r : val[j + 1];
        if (c < s.cells) mapping[c] = pc_entry(s, next);
        if (end) {                                         // the segment's head: the first key that is not below r
            uint64_t lo = 0, hi = j;
            while (lo < hi) {
                const uint64_t mid = lo + (hi - lo) / 2;
                if (key[mid] < r) lo = mid + 1;
                else hi = mid;
            }
            ++ends;
            if (j - lo + 1 > mine) mine = j - lo + 1;
        }
    }
    if (mine) atomicMax(&big, mine);
    pc_count(cnt, ends);
    __syncthreads();
    if (threadIdx.x == 0 && big) atomicMax(cnt + 1, big);
}
__global__ __launch_bounds__(kPcThreads) void k_pc_identity(const PcShape s, const uint32_t* __restrict__ parent,
                                                            const uint8_t* __restrict__ flag,
                                                            uint64_t* __restrict__ mapping) {
    const uint64_t step = (uint64_t)gridDim.x * kPcThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kPcThreads + threadIdx.x; i < s.cells; i += step)
        if (parent[i] == (uint32_t)i && !flag[i]) mapping[i] = pc_entry(s, i);
}

// ------------------------------------------------------------------ checker
__global__ __launch_bounds__(kPcThreads) void k_pm_hits(const PcShape s, const uint64_t* __restrict__ mapping,
                                                        uint32_t* hit, uint2* __restrict__ nm,
                                                        unsigned long long* cnt) {
    const uint64_t step = (uint64_t)gridDim.x * kPcThreads;
    uint32_t bad = 0, pad = 0;
#pragma unroll 1
    for (uint64_t i = (uint64_t)blockIdx.x * kPcThreads + threadIdx.x; i < s.cells; i += step) {
        const uint64_t e = mapping[i];
        uint32_t to = (uint32_t)i;
        if (pc_cell(s, e, s.rows, to)) atomicAdd(hit + to, 1u);
        else { ++bad; to = (uint32_t)i; }
        if ((i & (s.rows - 1)) >= s.usable && e != pc_entry(s, i)) ++pad;
        nm[i] = make_uint2(to, (uint32_t)i);
    }
    pc_count(cnt, bad);
    pc_count(cnt + 1, pad);
}
__global__ __launch_bounds__(kPcThreads) void k_pm_double(uint64_t n, const uint2* __restrict__ in,
                                                          uint2* __restrict__ out) {
    const uint64_t step = (uint64_t)gridDim.x * kPcThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kPcThreads + threadIdx.x; i < n; i += step) {
        const uint2 a = in[i];
        const uint2 b = a.x < n ? in[a.x] : a;
        out[i] = make_uint2(b.x, a.y < b.y ? a.y : b.y);
    }
}
__global__ __launch_bounds__(kPcThreads) void k_pm_descents(const PcShape s, const uint64_t* __restrict__ mapping,
                                                            const uint32_t* __restrict__ hit,
                                                            const uint2* __restrict__ nm, uint32_t* desc,
                                                            unsigned long long* cnt) {
    const uint64_t step = (uint64_t)gridDim.x * kPcThreads;
    uint32_t bad = 0;
#pragma unroll 1
    for (uint64_t i = (uint64_t)blockIdx.x * kPcThreads + threadIdx.x; i < s.cells; i += step) {
        if (hit[i] != 1) ++bad;
        uint32_t to;
        if (pc_cell(s, mapping[i], s.rows, to) && to < i) {
            const uint32_t mn = nm[i].y;
            if (mn < s.cells) atomicAdd(desc + mn, 1u);
        }
    }
    pc_count(cnt, bad);
}
__global__ __launch_bounds__(kPcThreads) void k_pm_cycles(const PcShape s, const uint64_t* __restrict__ mapping,
                                                          const uint2* __restrict__ nm,
                                                          const uint32_t* __restrict__ desc, unsigned long long* cnt) {
    const uint64_t step = (uint64_t)gridDim.x * kPcThreads;
    uint32_t cyc = 0, bad = 0;
#pragma unroll 1
    for (uint64_t i = (uint64_t)blockIdx.x * kPcThreads + threadIdx.x; i < s.cells; i += step) {
        uint32_t to;
        if (nm[i].y != (uint32_t)i || !pc_cell(s, mapping[i], s.rows, to) || to == (uint32_t)i) continue;
        ++cyc;
        if (desc[i] != 1) ++bad;
    }
    pc_count(cnt, cyc);
    pc_count(cnt + 1, bad);
}
__global__ __launch_bounds__(kPcThreads) void k_pm_edges(const PcShape s, const uint64_t* __restrict__ edges,
                                                         uint64_t n_edges, const uint2* __restrict__ nm,
                                                         unsigned long long* cnt) {
    const uint64_t step = (uint64_t)gridDim.x * kPcThreads;
    uint32_t seen = 0, bad = 0;
#pragma unroll 1
    for (uint64_t e = (uint64_t)blockIdx.x * kPcThreads + threadIdx.x; e < n_edges; e += step) {
        uint32_t a, b;
        if (!pc_cell(s, edges[2 * e], s.usable, a) || !pc_cell(s, edges[2 * e + 1], s.usable, b)) continue;
        ++seen;
        if (nm[a].y != nm[b].y) ++bad;
    }
    pc_count(cnt, seen);
    pc_count(cnt + 1, bad);
}

// ------------------------------------------------------- the witness's edges
__device__ __forceinline__ uint64_t pcw_entry(const PcColumns& w, uint32_t phase, uint64_t p) {
    return (uint64_t)(w.base[phase & 1] + (uint32_t)(p >> w.k)) << 32 | (p & ((1ull << w.k) - 1));
}
struct PcIsExt {
    const uint64_t* recs;
    __device__ __forceinline__ uint32_t operator()(uint64_t i) const { return (recs[2 * i] >> 62) == 2; }
};
// Record i of the phase, `at` external ones before it: to its group's list, in order.
struct PcSplit {
    const uint64_t* recs;
    PcColumns w;
    uint32_t phase;
    uint64_t *copy, *ext;
    uint64_t ncopy, next;                                  // the lists' lengths, as the host counted them
    unsigned* err;
    __device__ __forceinline__ void operator()(uint64_t i, uint32_t v, uint64_t at) const {
        const uint64_t src = recs[2 * i], off = src & ((1ull << 62) - 1), dst = pcw_entry(w, phase, recs[2 * i + 1]);
        if (v ? at >= next : i - at >= ncopy) {
            atomicOr(err, 2u);
            return;
        }
        uint64_t* o = v ? ext + 2 * at : copy + 2 * (i - at);
        o[0] = v ? (uint64_t)w.ext_col << 32 | (off & 0xffffffffull) : pcw_entry(w, (uint32_t)(src >> 62), off);
        o[1] = dst;
    }
};
// table: ntab values of 4 words, ascending as 256-bit numbers. Record i = (cell,
// 4 words): out[2 i] = its cell's entry, out[2 i + 1] = its value's place in the
// table; first[place] = min(first[place], g0 + i). A value that is not in the
// table sets *err.
__global__ __launch_bounds__(kPcThreads) void k_pcw_consts(const uint64_t* __restrict__ recs, uint64_t nk,
                                                           const uint64_t* __restrict__ table, uint32_t ntab,
                                                           uint64_t g0, const PcColumns w, uint32_t phase,
                                                           unsigned long long* first, uint64_t* __restrict__ out,
                                                           unsigned* err) {
    const uint64_t step = (uint64_t)gridDim.x * kPcThreads;
#pragma unroll 1
    for (uint64_t i = (uint64_t)blockIdx.x * kPcThreads + threadIdx.x; i < nk; i += step) {
        const uint64_t* r = recs + 5 * i;
        uint32_t lo = 0, hi = ntab;
        while (lo < hi) {                                   // the first table value that is not below the record's
            const uint32_t mid = lo + (hi - lo) / 2;
            const uint64_t* t = table + 4 * (uint64_t)mid;
            int less = 0;
            for (int q = 3; q >= 0; --q)
                if (t[q] != r[1 + q]) {
                    less = t[q] < r[1 + q];
                    break;
                }
            if (less) lo = mid + 1;
            else hi = mid;
        }
        bool found = lo < ntab;
        for (int q = 0; found && q < 4; ++q) found = table[4 * (uint64_t)lo + q] == r[1 + q];
        // few values, many records: almost every record finds an earlier one already there
        if (!found) atomicOr(err, 1u);
        else if (__hip_atomic_load(first + lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > g0 + i)
            atomicMin(first + lo, (unsigned long long)(g0 + i));
        out[2 * i] = pcw_entry(w, phase, r[0]);
        out[2 * i + 1] = found ? lo : 0;
    }
}
// out[2 i + 1]: a place in the table becomes the fixed cell of the constant's rank.
__global__ __launch_bounds__(kPcThreads) void k_pcw_place(uint64_t* __restrict__ out, uint64_t n,
                                                          const uint32_t* __restrict__ rank, uint32_t ntab,
                                                          uint32_t fixed_col, uint32_t nfixed) {
    const uint64_t step = (uint64_t)gridDim.x * kPcThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kPcThreads + threadIdx.x; i < n; i += step) {
        const uint64_t at = out[2 * i + 1];
        const uint32_t r = at < ntab ? rank[at] : 0u;
        out[2 * i + 1] = (uint64_t)(fixed_col + r % nfixed) << 32 | r / nfixed;
    }
}

// ----------------------------------------------------------------- launches
// The kernels of one scan over n values: the tile sums and their carry (sums),
// then the tiles again into the sink (if any).
template <class Src, class Sink>
static hipError_t pc_scan(const Src& src, const Sink* sink, uint64_t n, uint64_t* bsum, unsigned long long* total,
                          bool sums, hipStream_t st) {
    const uint64_t nb = pc_tiles(n);
    if (!nb || nb > 0x7fffffffull) return hipErrorInvalidValue;
    if (sums) {
        hipLaunchKernelGGL(k_pc_sum<Src>, dim3((unsigned)nb), dim3(kPcThreads), 0, st, src, n, bsum);
        hipLaunchKernelGGL(k_pc_carry, dim3(1), dim3(kPcThreads), 0, st, bsum, nb, total);
    }
    if (sink)
        hipLaunchKernelGGL((k_pc_apply<Src, Sink>), dim3((unsigned)nb), dim3(kPcThreads), 0, st, src, *sink, n, bsum);
    return hipGetLastError();
}
hipError_t launch_pc_init(const PcShape& s, uint32_t* parent, hipStream_t st) {
    if (pc_bad(s) || !parent) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pc_init, dim3(pc_grid(s.cells)), dim3(kPcThreads), 0, st, s.cells, parent);
    return hipGetLastError();
}
hipError_t launch_pc_union(const PcShape& s, const uint64_t* edges, uint64_t n_edges, uint32_t* parent,
                           unsigned long long* cnt, hipStream_t st) {
    if (!n_edges) return hipSuccess;
    if (pc_bad(s) || !edges || !parent || !cnt) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pc_union, dim3(pc_grid(n_edges)), dim3(kPcThreads), 0, st, s, edges, n_edges, parent, cnt);
    return hipGetLastError();
}
hipError_t launch_pc_flatten(const PcShape& s, uint32_t* parent, hipStream_t st) {
    if (pc_bad(s) || !parent) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pc_flatten, dim3(pc_grid(s.cells)), dim3(kPcThreads), 0, st, s.cells, parent);
    return hipGetLastError();
}
hipError_t launch_pc_flag(const PcShape& s, const uint32_t* parent, uint8_t* flag, hipStream_t st) {
    if (pc_bad(s) || !parent || !flag) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pc_flag, dim3(pc_grid(s.cells)), dim3(kPcThreads), 0, st, s.cells, parent, flag);
    return hipGetLastError();
}
hipError_t launch_pc_member_scan(const PcShape& s, const uint32_t* parent, const uint8_t* flag, uint64_t* bsum,
                                 unsigned long long* total, hipStream_t st) {
    if (pc_bad(s) || !parent || !flag || !bsum || !total) return hipErrorInvalidValue;
    return pc_scan<PcMember, PcCompact>(PcMember{parent, flag}, nullptr, s.cells, bsum, total, true, st);
}
hipError_t launch_pc_compact(const PcShape& s, const uint32_t* parent, const uint8_t* flag, const uint64_t* bsum,
                             uint64_t m, uint32_t* key, uint32_t* val, hipStream_t st) {
    if (!m) return hipSuccess;
    if (pc_bad(s) || !parent || !flag || !bsum || !key || !val || m > s.cells) return hipErrorInvalidValue;
    const PcCompact sink{parent, key, val, m};
    return pc_scan(PcMember{parent, flag}, &sink, s.cells, const_cast<uint64_t*>(bsum), nullptr, false, st);
}
hipError_t launch_pc_sort_pass(const uint32_t* key, const uint32_t* val, uint64_t m, uint32_t shift, uint32_t* hist,
                               uint64_t* bsum, uint32_t* key2, uint32_t* val2, hipStream_t st) {
    if (!m) return hipSuccess;
    if (!key || !val || !hist || !bsum || !key2 || !val2 || shift > 24 || m > (1ull << 32))
        return hipErrorInvalidValue;
    const uint64_t nblk = pc_sort_blocks(m);
    hipLaunchKernelGGL(k_pc_hist, dim3((unsigned)nblk), dim3(kPcThreads), 0, st, key, m, shift, nblk, hist);
    const PcWords words{hist};
    const hipError_t e = pc_scan(words, &words, 256 * nblk, bsum, nullptr, true, st);   // the table, in place
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_pc_scatter, dim3((unsigned)nblk), dim3(kPcThreads), 0, st, key, val, m, shift, nblk, hist,
                       key2, val2);
    return hipGetLastError();
}
hipError_t launch_pc_link(const PcShape& s, const uint32_t* key, const uint32_t* val, uint64_t m, uint64_t* mapping,
                          unsigned long long* cnt, hipStream_t st) {
    if (!m) return hipSuccess;
    if (pc_bad(s) || !key || !val || !mapping || !cnt || m > s.cells) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pc_link, dim3(pc_grid(m)), dim3(kPcThreads), 0, st, s, key, val, m, mapping, cnt);
    return hipGetLastError();
}
hipError_t launch_pc_identity(const PcShape& s, const uint32_t* parent, const uint8_t* flag, uint64_t* mapping,
                              hipStream_t st) {
    if (pc_bad(s) || !parent || !flag || !mapping) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pc_identity, dim3(pc_grid(s.cells)), dim3(kPcThreads), 0, st, s, parent, flag, mapping);
    return hipGetLastError();
}
hipError_t launch_pm_hits(const PcShape& s, const uint64_t* mapping, uint32_t* hit, uint2* nm, unsigned long long* cnt,
                          hipStream_t st) {
    if (pc_bad(s) || !mapping || !hit || !nm || !cnt) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pm_hits, dim3(pc_grid(s.cells)), dim3(kPcThreads), 0, st, s, mapping, hit, nm, cnt);
    return hipGetLastError();
}
hipError_t launch_pm_double(const PcShape& s, const uint2* in, uint2* out, hipStream_t st) {
    if (pc_bad(s) || !in || !out || in == out) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pm_double, dim3(pc_grid(s.cells)), dim3(kPcThreads), 0, st, s.cells, in, out);
    return hipGetLastError();
}
hipError_t launch_pm_descents(const PcShape& s, const uint64_t* mapping, const uint32_t* hit, const uint2* nm,
                              uint32_t* desc, unsigned long long* cnt, hipStream_t st) {
    if (pc_bad(s) || !mapping || !hit || !nm || !desc || !cnt) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pm_descents, dim3(pc_grid(s.cells)), dim3(kPcThreads), 0, st, s, mapping, hit, nm, desc, cnt);
    return hipGetLastError();
}
hipError_t launch_pm_cycles(const PcShape& s, const uint64_t* mapping, const uint2* nm, const uint32_t* desc,
                            unsigned long long* cnt, hipStream_t st) {
    if (pc_bad(s) || !mapping || !nm || !desc || !cnt) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pm_cycles, dim3(pc_grid(s.cells)), dim3(kPcThreads), 0, st, s, mapping, nm, desc, cnt);
    return hipGetLastError();
}
hipError_t launch_pm_edges(const PcShape& s, const uint64_t* edges, uint64_t n_edges, const uint2* nm,
                           unsigned long long* cnt, hipStream_t st) {
    if (!n_edges) return hipSuccess;
    if (pc_bad(s) || !edges || !nm || !cnt) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pm_edges, dim3(pc_grid(n_edges)), dim3(kPcThreads), 0, st, s, edges, n_edges, nm, cnt);
    return hipGetLastError();
}

hipError_t launch_pcw_split(const uint64_t* recs, uint64_t nc, const PcColumns& w, uint32_t phase, uint64_t* bsum,
                            uint64_t* copy, uint64_t ncopy, uint64_t* ext, uint64_t next, unsigned* err,
                            hipStream_t st) {
    if (!nc) return hipSuccess;
    if (!recs || !bsum || !copy || !ext || !err || phase > 1 || w.k < 1 || w.k > 31 || ncopy + next != nc)
        return hipErrorInvalidValue;
    const PcSplit sink{recs, w, phase, copy, ext, ncopy, next, err};
    return pc_scan(PcIsExt{recs}, &sink, nc, bsum, nullptr, true, st);
}
hipError_t launch_pcw_consts(const uint64_t* recs, uint64_t nk, const uint64_t* table, uint32_t ntab, uint64_t g0,
                             const PcColumns& w, uint32_t phase, unsigned long long* first, uint64_t* out,
                             unsigned* err, hipStream_t st) {
    if (!nk) return hipSuccess;
    if (!recs || !table || !ntab || !first || !out || !err || phase > 1 || w.k < 1 || w.k > 31)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pcw_consts, dim3(pc_grid(nk)), dim3(kPcThreads), 0, st, recs, nk, table, ntab, g0, w, phase,
                       first, out, err);
    return hipGetLastError();
}
hipError_t launch_pcw_place(uint64_t* out, uint64_t n, const uint32_t* rank, uint32_t ntab, uint32_t fixed_col,
                            uint32_t nfixed, hipStream_t st) {
    if (!n) return hipSuccess;
    if (!out || !rank || !ntab || !nfixed) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pcw_place, dim3(pc_grid(n)), dim3(kPcThreads), 0, st, out, n, rank, ntab, fixed_col, nfixed);
    return hipGetLastError();
}

}  // namespace svdw
