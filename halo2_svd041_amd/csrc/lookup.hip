// gfx950 kernels of the lookup argument's permuted columns (lookup.hpp). All of
// them are HBM- or L2-bound: one cell per lane as in export.hip (two 16 B loads
// or stores), grid-stride over a capped grid, one column per blockIdx.y, 64-bit
// cell indices (ncols * 2^k exceeds 2^32 at k = 31).
#include <hip/hip_runtime.h>

#include "export.hpp"
#include "lookup.hpp"

namespace svdw {

static constexpr unsigned kLkThreads = 256;
static constexpr unsigned kLkMaxBlocks = 4096;   // per column

// 2^288 mod p: mont_mul_rounds<1>(v, 2^288) = v 2^256 mod p, the Montgomery
// form of a value below 2^32 in one CIOS round instead of fr_to_mont's eight.
#define SVDW_2_288_WORDS 0x15b8b9dau, 0x93e78865u, 0xb05ea154u, 0x16df2426u, \
                         0x302ab839u, 0x1271b743u, 0xec6c226eu, 0x06bc037eu
__device__ __forceinline__ Fr fr_2_288() {
    Fr r;
    constexpr uint32_t K[8] = {SVDW_2_288_WORDS};
#pragma unroll
    for (int i = 0; i < 8; ++i) r.w[i] = K[i];
    return r;
}
template <int FORM>
__device__ __forceinline__ Fr lk_cell(uint32_t v) {
    Fr x = fr_zero();
    x.w[0] = v;
    if (FORM == kFormMontgomery) x = mont_mul_rounds<1>(x, fr_2_288());
    return x;
}
// The table index of a cell in FORM, false when it is >= 2^lb (lb < 32): any of
// its 256 bits above lb set, k_check_lookups' test.
template <int FORM>
__device__ __forceinline__ bool lk_value(Fr x, uint32_t lb, uint32_t& v) {
    if (FORM == kFormMontgomery) x = fr_from_mont(x);
    uint32_t hi = x.w[0] >> lb;
#pragma unroll
    for (int w = 1; w < 8; ++w) hi |= x.w[w];
    v = x.w[0];
    return hi == 0;
}

// ---------------------------------------------------------------- histogram
// A column of a range-checked witness is near uniform over the 2^lb values but
// for a few hot ones (measured at 1024^2, P = 63: one value holds 2-9 % of a
// column; padding rows are zeros), and a million atomics on one address
// serialise. So each block aggregates in LDS first: kLkSlots counters, slot =
// the value's low bits, owned by the first value of the block that claims it
// (its high bits are the slot's tag). A hot value claims its slot within the
// block's first rows and is flushed as one global atomic per block; a value
// whose slot is taken goes to memory directly, one no-return atomic on a
// near-uniform address. Below kLkSlots values the slots are the histogram.
// Zeros (the padding rows are not even read) and 2^lb - 1 stay in registers.
static constexpr unsigned kLkSlotBits = 11, kLkSlots = 1u << kLkSlotBits;
static constexpr uint32_t kLkFree = 0xffffffffu;
template <int FORM>
__global__ __launch_bounds__(kLkThreads) void k_lk_hist(const LkSrc s, uint64_t usable, uint32_t lb,
                                                        uint32_t* __restrict__ cnt, unsigned long long* oot) {
    __shared__ uint32_t tag[kLkSlots], num[kLkSlots], sh[3];
    for (unsigned i = threadIdx.x; i < kLkSlots; i += kLkThreads) {
        tag[i] = kLkFree;
        num[i] = 0;
    }
    if (threadIdx.x < 3) sh[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t c = blockIdx.y, top = (1u << lb) - 1u;
    uint32_t* h = cnt + ((uint64_t)c << lb);
    uint32_t n0 = 0, n1 = 0, nb = 0;
    const uint64_t step = (uint64_t)gridDim.x * kLkThreads;
    for (uint64_t r = (uint64_t)blockIdx.x * kLkThreads + threadIdx.x; r < usable; r += step) {
        const uint64_t i = (uint64_t)c * s.stride + r;
        if (r >= s.span || i >= s.total) {               // a row past the assigned ones
            ++n0;
            continue;
        }
        uint32_t v;
        if (!lk_value<FORM>(ld_fr(s.p + i), lb, v)) {
            ++nb;
            continue;
        }
        if (v == 0) {
            ++n0;
        } else if (v == top) {
            ++n1;
        } else {
            const uint32_t sl = v & (kLkSlots - 1u), tg = v >> kLkSlotBits;
            uint32_t own = *(volatile uint32_t*)&tag[sl];
            if (own == kLkFree) {
                own = atomicCAS(&tag[sl], kLkFree, tg);
                if (own == kLkFree) own = tg;
            }
            if (own == tg) atomicAdd(&num[sl], 1u);
            else atomicAdd(h + v, 1u);
        }
    }
    if (n0) atomicAdd(&sh[0], n0);
    if (n1) atomicAdd(&sh[1], n1);
    if (nb) atomicAdd(&sh[2], nb);
    __syncthreads();
    for (unsigned i = threadIdx.x; i < kLkSlots; i += kLkThreads)
        if (num[i]) atomicAdd(h + ((tag[i] << kLkSlotBits) | i), num[i]);
    if (threadIdx.x == 0 && sh[0]) atomicAdd(h, sh[0]);
    if (threadIdx.x == 1 && sh[1]) atomicAdd(h + top, sh[1]);
    if (threadIdx.x == 2 && sh[2]) atomicAdd(oot, (unsigned long long)sh[2]);
}

hipError_t launch_lk_hist(const LkSrc& src, int form, uint32_t ncols, uint64_t usable, uint32_t lb,
                          uint32_t* cnt, unsigned long long* oot, hipStream_t st) {
    if (!ncols || !usable) return hipSuccess;
    if (!cnt || !oot || lb < 1 || lb > 31 || ncols > 65535 || (src.total && !src.p) ||
        (form != kFormCanonical && form != kFormMontgomery))
        return hipErrorInvalidValue;
    const uint64_t nb = (usable + kLkThreads - 1) / kLkThreads;
    const dim3 g((unsigned)(nb < kLkMaxBlocks ? nb : kLkMaxBlocks), ncols), b(kLkThreads);
    if (form == kFormMontgomery) hipLaunchKernelGGL((k_lk_hist<kFormMontgomery>), g, b, 0, st, src, usable, lb, cnt, oot);
    else hipLaunchKernelGGL((k_lk_hist<kFormCanonical>), g, b, 0, st, src, usable, lb, cnt, oot);
    return hipGetLastError();
}

// -------------------------------------------------------------------- scans
// Exclusive prefix (ea, eb) of the pair (a, b) over the block's 256 threads and
// the block totals (ta, tb).
__device__ __forceinline__ void lk_block_scan2(uint32_t a, uint32_t b, uint32_t& ea, uint32_t& eb,
                                               uint32_t& ta, uint32_t& tb) {
    __shared__ uint32_t wa[kLkThreads / 64], wb[kLkThreads / 64];
    const unsigned lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint32_t ia = a, ib = b;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t xa = __shfl_up(ia, d), xb = __shfl_up(ib, d);
        if (lane >= (unsigned)d) {
            ia += xa;
            ib += xb;
        }
    }
    if (lane == 63) {
        wa[w] = ia;
        wb[w] = ib;
    }
    __syncthreads();
    uint32_t oa = 0, ob = 0;
    ta = tb = 0;
#pragma unroll
    for (unsigned k = 0; k < kLkThreads / 64; ++k) {
        if (k < w) {
            oa += wa[k];
            ob += wb[k];
        }
        ta += wa[k];
        tb += wb[k];
    }
    ea = oa + ia - a;
    eb = ob + ib - b;
    __syncthreads();                                       // wa / wb are reused by the next call
}
// A thread's four bins of column c's tile blockIdx.x (zero past B).
__device__ __forceinline__ uint4 lk_load_bins(const uint32_t* h, uint32_t v0, uint32_t B) {
    return v0 < B ? *reinterpret_cast<const uint4*>(h + v0) : make_uint4(0, 0, 0, 0);
}
// 1: the sums of cnt and of present over each tile of kLkScanTile bins
__global__ __launch_bounds__(kLkThreads) void k_lk_scan_sums(const LkScratch s, uint32_t lb, uint32_t nblk) {
    const uint32_t c = blockIdx.y, B = 1u << lb, v0 = blockIdx.x * kLkScanTile + threadIdx.x * 4;
    const uint4 q = lk_load_bins(s.cnt + ((uint64_t)c << lb), v0, B);
    uint32_t ea, eb, ta, tb;
    lk_block_scan2(q.x + q.y + q.z + q.w, (q.x != 0) + (q.y != 0) + (q.z != 0) + (q.w != 0), ea, eb, ta, tb);
    if (threadIdx.x == 0) {
        uint32_t* o = s.bsum + ((uint64_t)c * nblk + blockIdx.x) * 2;
        o[0] = ta;
        o[1] = tb;
    }
}
// 2: one block per column turns the tile sums into their exclusive scans, in place
__global__ __launch_bounds__(kLkThreads) void k_lk_scan_blocks(const LkScratch s, uint32_t nblk) {
    const uint32_t c = blockIdx.x;
    uint32_t* bs = s.bsum + (uint64_t)c * nblk * 2;
    uint32_t ca = 0, cb = 0;
    for (uint32_t base = 0; base < nblk; base += kLkThreads) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t a = i < nblk ? bs[2 * (uint64_t)i] : 0u, b = i < nblk ? bs[2 * (uint64_t)i + 1] : 0u;
        uint32_t ea, eb, ta, tb;
        lk_block_scan2(a, b, ea, eb, ta, tb);
        if (i < nblk) {
            bs[2 * (uint64_t)i] = ca + ea;
            bs[2 * (uint64_t)i + 1] = cb + eb;
        }
        ca += ta;
        cb += tb;
    }
    if (threadIdx.x == 0) s.tot[c] = cb;
}
// 3: start, pincl and the compaction of the absent values: v >= 1 with
// cnt[v] == 0 has (v - 1) - (present values in [1, v)) absent values below it.
__global__ __launch_bounds__(kLkThreads) void k_lk_scan_write(const LkScratch s, uint32_t lb, uint32_t nblk) {
    const uint32_t c = blockIdx.y, B = 1u << lb, v0 = blockIdx.x * kLkScanTile + threadIdx.x * 4;
    const uint64_t col = (uint64_t)c << lb;
    const uint32_t* h = s.cnt + col;
    const uint4 q = lk_load_bins(h, v0, B);
    uint32_t ea, eb, ta, tb;
    lk_block_scan2(q.x + q.y + q.z + q.w, (q.x != 0) + (q.y != 0) + (q.z != 0) + (q.w != 0), ea, eb, ta, tb);
    if (v0 >= B) return;
    const uint32_t* bs = s.bsum + ((uint64_t)c * nblk + blockIdx.x) * 2;
    const uint32_t p0 = h[0] != 0;
    const uint32_t cj[4] = {q.x, q.y, q.z, q.w};
    uint32_t run = bs[0] + ea, pe = bs[1] + eb, st[4], pi[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t v = v0 + j, below = pe;             // present values in [0, v)
        st[j] = run;
        run += cj[j];
        pe += cj[j] != 0;
        pi[j] = pe;
        if (!cj[j] && v) s.absent[col + (v - 1u) - (below - p0)] = v;
    }
    *reinterpret_cast<uint4*>(s.start + col + v0) = make_uint4(st[0], st[1], st[2], st[3]);
    *reinterpret_cast<uint4*>(s.pincl + col + v0) = make_uint4(pi[0], pi[1], pi[2], pi[3]);
}

hipError_t launch_lk_scans(const LkScratch& s, uint32_t ncols, uint32_t lb, hipStream_t st) {
    if (!ncols) return hipSuccess;
    if (lb < 2 || lb > 31 || ncols > 65535 || !s.cnt || !s.start || !s.pincl || !s.absent || !s.bsum || !s.tot)
        return hipErrorInvalidValue;
    const uint32_t nblk = (uint32_t)lk_scan_blocks(1ull << lb);
    hipLaunchKernelGGL(k_lk_scan_sums, dim3(nblk, ncols), dim3(kLkThreads), 0, st, s, lb, nblk);
    hipLaunchKernelGGL(k_lk_scan_blocks, dim3(ncols), dim3(kLkThreads), 0, st, s, nblk);
    hipLaunchKernelGGL(k_lk_scan_write, dim3(nblk, ncols), dim3(kLkThreads), 0, st, s, lb, nblk);
    return hipGetLastError();
}

// --------------------------------------------------------------------- fill
// The largest v in [lo, hi] with start[v] <= r (start[lo] <= r): the value whose
// run holds row r, as empty bins share the start of the next present value.
__device__ __forceinline__ uint32_t lk_find(const uint32_t* __restrict__ start, uint32_t lo, uint32_t hi, uint32_t r) {
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo + 1u) >> 1);
        if (start[mid] <= r) lo = mid;
        else hi = mid - 1u;
    }
    return lo;
}
// A tile of 256 consecutive rows: two lanes search all B bins for the values of
// the tile's first and last row, every lane then searches between those two
// (a handful of bins in the near-uniform part, none inside a long run).
template <int FORM>
__global__ __launch_bounds__(kLkThreads) void k_lk_fill(const LkScratch s, uint64_t rows, uint64_t usable,
                                                        uint32_t lb, Fr* __restrict__ pin, Fr* __restrict__ ptab) {
    __shared__ uint32_t ends[2];
    const uint32_t c = blockIdx.y, B = 1u << lb;
    const uint64_t col = (uint64_t)c << lb;
    const uint32_t* start = s.start + col;
    const uint32_t* pincl = s.pincl + col;
    const uint32_t* absent = s.absent + col;
    const uint32_t D = s.tot[c], p0 = s.cnt[col] != 0;
    const uint64_t nL = usable - D, z0 = 1 + usable - B - p0;
    const uint64_t ntiles = (rows + kLkThreads - 1) / kLkThreads;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t r0 = t * kLkThreads, r = r0 + threadIdx.x;
        if (r0 < usable) {
            const uint64_t rl = (r0 + kLkThreads < usable ? r0 + kLkThreads : usable) - 1;
            if (threadIdx.x == 0) ends[0] = lk_find(start, 0, B - 1u, (uint32_t)r0);
            if (threadIdx.x == 64) ends[1] = lk_find(start, 0, B - 1u, (uint32_t)rl);
        }
        __syncthreads();
        Fr a = fr_zero(), b = fr_zero();
        if (r < usable) {
            const uint32_t v = lk_find(start, ends[0], ends[1], (uint32_t)r);
            uint32_t sv = v;
            if ((uint32_t)r != start[v]) {                 // a repeated row takes a leftover table entry
                const uint64_t i = nL - 1 - (r - pincl[v]);
                sv = i < z0 || i - z0 >= B ? 0u : absent[i - z0];
            }
            a = lk_cell<FORM>(v);
            b = lk_cell<FORM>(sv);
        }
        if (r < rows) {
            st_fr(pin + (uint64_t)c * rows + r, a);
            st_fr(ptab + (uint64_t)c * rows + r, b);
        }
        __syncthreads();                                   // ends is rewritten by the next tile
    }
}

hipError_t launch_lk_fill(const LkScratch& s, uint32_t ncols, uint64_t rows, uint64_t usable, uint32_t lb,
                          int form, Fr* pin, Fr* ptab, hipStream_t st) {
    if (!ncols || !rows) return hipSuccess;
    if (!pin || !ptab || lb < 2 || lb > 31 || ncols > 65535 || usable > rows || usable >= (1ull << 32) ||
        (1ull << lb) > usable || (form != kFormCanonical && form != kFormMontgomery))
        return hipErrorInvalidValue;
    const uint64_t nt = (rows + kLkThreads - 1) / kLkThreads;
    const dim3 g((unsigned)(nt < kLkMaxBlocks ? nt : kLkMaxBlocks), ncols), b(kLkThreads);
    if (form == kFormMontgomery) hipLaunchKernelGGL((k_lk_fill<kFormMontgomery>), g, b, 0, st, s, rows, usable, lb, pin, ptab);
    else hipLaunchKernelGGL((k_lk_fill<kFormCanonical>), g, b, 0, st, s, rows, usable, lb, pin, ptab);
    return hipGetLastError();
}

// -------------------------------------------------------------------- check
// k_check_cells' counting pattern: per-thread counts, an LDS sum per block, one
// global atomic per counter and block.
__device__ __forceinline__ void lk_block_flush(const uint32_t (&v)[4], unsigned long long* cnt) {
    __shared__ unsigned long long s[4];
    if (threadIdx.x < 4) s[threadIdx.x] = 0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (v[k]) atomicAdd(&s[k], (unsigned long long)v[k]);
    __syncthreads();
    if (threadIdx.x < 4 && s[threadIdx.x]) atomicAdd(cnt + threadIdx.x, s[threadIdx.x]);
}
// Adjacency A'[0] == S'[0], A'[r] == S'[r] or A'[r] == A'[r - 1] on the usable
// rows (equality of cells is equality in either form), zero cells below them.
__global__ __launch_bounds__(kLkThreads) void k_lk_adjacent(const Fr* __restrict__ pin, const Fr* __restrict__ ptab,
                                                            uint64_t rows, uint64_t usable, unsigned long long* cnt) {
    uint32_t v[4] = {0, 0, 0, 0};
    const Fr* A = pin + (uint64_t)blockIdx.y * rows;
    const Fr* S = ptab + (uint64_t)blockIdx.y * rows;
    const uint64_t step = (uint64_t)gridDim.x * kLkThreads;
    for (uint64_t r = (uint64_t)blockIdx.x * kLkThreads + threadIdx.x; r < rows; r += step) {
        const Fr a = ld_fr(A + r), t = ld_fr(S + r);
        if (r < usable) {
            ++v[0];
            v[1] += !(fr_eq(a, t) || (r && fr_eq(a, ld_fr(A + r - 1))));
        } else {
            v[2] += 2;
            v[3] += !fr_is_zero(a) + !fr_is_zero(t);
        }
    }
    lk_block_flush(v, cnt);
}
hipError_t launch_lk_adjacent(const Fr* pin, const Fr* ptab, uint32_t ncols, uint64_t rows, uint64_t usable,
                              unsigned long long* cnt, hipStream_t st) {
    if (!ncols || !rows) return hipSuccess;
    if (!pin || !ptab || !cnt || ncols > 65535 || usable > rows) return hipErrorInvalidValue;
    const uint64_t nb = (rows + kLkThreads - 1) / kLkThreads;
    hipLaunchKernelGGL(k_lk_adjacent, dim3((unsigned)(nb < kLkMaxBlocks ? nb : kLkMaxBlocks), ncols),
                       dim3(kLkThreads), 0, st, pin, ptab, rows, usable, cnt);
    return hipGetLastError();
}
// The multisets, bin by bin: A' against the input column, S' against the table
// T[:usable] = one of each value and 1 + usable - B zeros.
__global__ __launch_bounds__(kLkThreads) void k_lk_compare(const uint32_t* __restrict__ ha,
                                                           const uint32_t* __restrict__ hpin,
                                                           const uint32_t* __restrict__ htab, uint64_t nbins,
                                                           uint64_t usable, uint32_t lb, unsigned long long* cnt) {
    uint32_t v[4] = {0, 0, 0, 0};
    const uint32_t B = 1u << lb, zeros = (uint32_t)(1 + usable - B);
    const uint64_t step = (uint64_t)gridDim.x * kLkThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kLkThreads + threadIdx.x; i < nbins; i += step) {
        const uint32_t val = (uint32_t)i & (B - 1u);
        v[0] += 2;
        v[1] += (ha[i] != hpin[i]) + (htab[i] != (val ? 1u : zeros));
    }
    lk_block_flush(v, cnt);
}
hipError_t launch_lk_compare(const uint32_t* ha, const uint32_t* hpin, const uint32_t* htab, uint32_t ncols,
                             uint64_t usable, uint32_t lb, unsigned long long* cnt, hipStream_t st) {
    if (!ncols) return hipSuccess;
    if (!ha || !hpin || !htab || !cnt || lb < 1 || lb > 31 || (1ull << lb) > usable) return hipErrorInvalidValue;
    const uint64_t nbins = (uint64_t)ncols << lb, nb = (nbins + kLkThreads - 1) / kLkThreads;
    hipLaunchKernelGGL(k_lk_compare, dim3((unsigned)(nb < kLkMaxBlocks ? nb : kLkMaxBlocks)), dim3(kLkThreads), 0, st,
                       ha, hpin, htab, nbins, usable, lb, cnt);
    return hipGetLastError();
}

}  // namespace svdw
