// The passes of a grand-product argument on the device, written once for the
// lookup argument (lookup_product.hip) and the permutation argument
// (permutation_product.hip). Per item (a column there, a set of columns here;
// one per blockIdx.y) and usable row r, a leaf gives two factors N[r], D[r], and
//
//   Z[i] = K * prod_{r < i} N[r] * prod_{r >= i} D[r],   K = start * (prod_r D[r])^-1,
//
// rows (usable, rows) zero: a prefix product, a suffix product, one inversion.
//
//  k_gp_tiles   the products of N and of D over each tile of kGpTile rows
//  carry stage  per item the exclusive prefix (N) and suffix (D) of the tile
//               products and K; the argument's own kernels (the permutation
//               chains its sets' starts there), built from gp_run,
//               gp_run_products, lp_block_scan and gp_fold
//  k_gp_write   the tile again: local prefix / suffix products, a block scan
//               seeded with the tile's carries, Z written
//  k_gp_check   the division-free recurrence, the boundary rows and the padding
//               (shares no scan and no inversion with those above)
//
// They are VALU-bound: a mont_mul is about 480 instructions, a row's cells a few
// 32 B loads or stores. So every loop over rows, scan steps and a set's columns
// stays rolled (#pragma unroll 1: one inlined mont_mul per use, not per
// iteration), the rows a thread keeps between two loops live in registers
// behind a select chain (a runtime index would move them to scratch) or in LDS,
// and what counts is the multiplications per row. 64-bit row indices.
//
// Powers of R = 2^256: a leaf hands its factors over in whatever power its form
// gives them, the same for N and D; products are mont_mul trees whose neutral
// element is one() = R, so every Z[i] and the item's product of D carry one and
// the same power, which the inverse in K cancels. inv0: a zero D[r] enters the
// products as one() and zeroes N[r] (gp_leaves, the one place).
//
// A leaf is a plain struct of values and pointers, passed to the kernel by value:
//
//   uint64_t rows(), usable();  Fr one();
//   struct Cursor;              per-thread state that follows the row
//   Cursor cursor(r);           at row r < rows
//   void factors(item, r, cursor, n, d);   the raw N[r], D[r], r < usable
//
// and for k_gp_check
//
//   void advance(cursor);       by the grid's stride, once per iteration
//   Fr zone();                  1 in the form of Z
//   Fr first(item, Z);          what Z[0] must equal
//   bool closes(item);          whether Z[usable] must be in {0, 1}
//
// The constants and the two inline functions below are the host's too; the rest
// is device code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fr.hpp"

namespace svdw {

static constexpr uint32_t kGpTile = 1024;                      // rows per tile
static constexpr unsigned kGpThreads = 256, kGpWaves = kGpThreads / 64;   // of the passes and the carry stages
static constexpr unsigned kGpItems = kGpTile / kGpThreads;     // consecutive rows per thread of k_gp_write
static constexpr unsigned kGpCheckBlocks = 4096;               // per item at the most, k_gp_check
inline uint64_t gp_tiles(uint64_t rows) { return (rows + kGpTile - 1) / kGpTile; }
inline unsigned gp_check_blocks(uint64_t rows) {
    const uint64_t nb = (rows + kGpThreads - 1) / kGpThreads;
    return (unsigned)(nb < kGpCheckBlocks ? nb : kGpCheckBlocks);
}

// ------------------------------------------------- Fr in shuffles and selects
__device__ __forceinline__ Fr lp_shfl_up(const Fr& x, unsigned d) {
    Fr r;
#pragma unroll
    for (int w = 0; w < 8; ++w) r.w[w] = __shfl_up(x.w[w], d);
    return r;
}
__device__ __forceinline__ Fr lp_shfl_down(const Fr& x, unsigned d) {
    Fr r;
#pragma unroll
    for (int w = 0; w < 8; ++w) r.w[w] = __shfl_down(x.w[w], d);
    return r;
}
__device__ __forceinline__ Fr lp_shfl_xor(const Fr& x, unsigned m) {
    Fr r;
#pragma unroll
    for (int w = 0; w < 8; ++w) r.w[w] = __shfl_xor(x.w[w], (int)m);
    return r;
}
__device__ __forceinline__ Fr lp_select(bool take, const Fr& a, const Fr& b) {
    Fr r;
#pragma unroll
    for (int w = 0; w < 8; ++w) r.w[w] = take ? a.w[w] : b.w[w];
    return r;
}
// a[j] with a runtime j: a select chain, as a runtime index would move a to scratch.
__device__ __forceinline__ void lp_put(Fr (&a)[kGpItems], unsigned j, const Fr& v) {
#pragma unroll
    for (unsigned k = 0; k < kGpItems; ++k) a[k] = lp_select(j == k, v, a[k]);
}
__device__ __forceinline__ Fr lp_get(const Fr (&a)[kGpItems], unsigned j) {
    Fr r = a[0];
#pragma unroll
    for (unsigned k = 1; k < kGpItems; ++k) r = lp_select(j == k, a[k], r);
    return r;
}

// --------------------------------------------------------------- block scan
// Over the block's threads: xn = cn * the pn of the threads below, xd = cd * the
// pd of the threads above (cn, cd the same for the whole block); with TOTALS
// tn, td = the products of all pn, all pd. One call per kernel (wn, wd).
template <bool TOTALS>
__device__ __forceinline__ void lp_block_scan(const Fr& one, Fr pn, Fr pd, const Fr& cn, const Fr& cd, Fr& xn, Fr& xd,
                                              Fr& tn, Fr& td) {
    __shared__ Fr wn[kGpWaves], wd[kGpWaves];
    const unsigned lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
#pragma unroll 1
    for (unsigned d = 1; d < 64; d <<= 1) {
        const Fr a = lp_shfl_up(pn, d), b = lp_shfl_down(pd, d);
        pn = mont_mul(pn, lp_select(lane >= d, a, one));
        pd = mont_mul(pd, lp_select(lane + d < 64u, b, one));
    }
    if (lane == 63) wn[w] = pn;                            // inclusive prefix: the wave's product of pn
    if (lane == 0) wd[w] = pd;                             // inclusive suffix
    const Fr en = lp_select(lane > 0, lp_shfl_up(pn, 1), one), ed = lp_select(lane < 63, lp_shfl_down(pd, 1), one);
    __syncthreads();
    Fr on = cn, od = cd;
#pragma unroll 1
    for (unsigned k = 0; k < kGpWaves; ++k) {              // k against w: the same for all lanes of a wave
        if (k < w) on = mont_mul(on, wn[k]);
        if (k > w) od = mont_mul(od, wd[k]);
    }
    xn = mont_mul(on, en);
    xd = mont_mul(od, ed);
    if (TOTALS) {
        tn = td = one;
#pragma unroll 1
        for (unsigned k = 0; k < kGpWaves; ++k) {
            tn = mont_mul(tn, wn[k]);
            td = mont_mul(td, wd[k]);
        }
    }
}

// The leaf's factors of row r < usable with inv0: a zero denominator enters the
// products of D as the neutral element and zeroes the row's numerator. True for
// such a row.
template <class Leaf>
__device__ __forceinline__ bool gp_leaves(const Leaf& leaf, uint32_t item, uint64_t r, Fr& n, Fr& d) {
    leaf.factors(item, r, leaf.cursor(r), n, d);
    const bool z = fr_is_zero(d);
    n = lp_select(z, fr_zero(), n);
    d = lp_select(z, leaf.one(), d);
    return z;
}

// -------------------------------------------------------------------- tiles
// One wave per tile, 16 rows per lane at a stride of 64 (a product has no
// order, so the loads are coalesced), then a butterfly over the lanes.
// tp[(item * nt + t) * 2 + {0, 1}] = the products of N, of D over tile t;
// cnt[0] += rows with a zero denominator.
template <class Leaf>
__global__ __launch_bounds__(kGpThreads) void k_gp_tiles(const Leaf leaf, uint64_t nt, Fr* __restrict__ tp,
                                                         unsigned long long* cnt) {
    __shared__ uint32_t zs;
    if (threadIdx.x == 0) zs = 0;
    __syncthreads();
    const unsigned lane = threadIdx.x & 63u;
    const uint32_t c = blockIdx.y;
    const uint64_t t = (uint64_t)blockIdx.x * kGpWaves + (threadIdx.x >> 6), usable = leaf.usable();
    const Fr one = leaf.one();
    uint32_t nz = 0;
    if (t < nt) {                                          // the same for all lanes of a wave
        Fr pn = one, pd = one;
#pragma unroll 1
        for (uint64_t r0 = t * kGpTile; r0 < (t + 1) * kGpTile && r0 < usable; r0 += 64) {
            const uint64_t r = r0 + lane;
            Fr n = one, d = one;
            if (r < usable) nz += gp_leaves(leaf, c, r, n, d);
            pn = mont_mul(pn, n);
            pd = mont_mul(pd, d);
        }
#pragma unroll 1
        for (unsigned m = 1; m < 64; m <<= 1) {
            pn = mont_mul(pn, lp_shfl_xor(pn, m));
            pd = mont_mul(pd, lp_shfl_xor(pd, m));
            nz += __shfl_xor(nz, (int)m);
        }
        if (lane == 0) {
            Fr* o = tp + ((uint64_t)c * nt + t) * 2;
            st_fr(o, pn);
            st_fr(o + 1, pd);
            if (nz) atomicAdd(&zs, nz);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && zs) atomicAdd(cnt, (unsigned long long)zs);
}

// -------------------------------------------------------------------- carry
// One block of kGpThreads per item over its nt tile products (col), a run
// [lo, hi) of consecutive tiles per thread.
__device__ __forceinline__ void gp_run(uint64_t nt, uint64_t& lo, uint64_t& hi) {
    const uint64_t per = (nt + kGpThreads - 1) / kGpThreads;
    lo = threadIdx.x * per < nt ? threadIdx.x * per : nt;
    hi = lo + per < nt ? lo + per : nt;
}
// pn, pd = the products of N, of D over the run.
__device__ __forceinline__ void gp_run_products(const Fr* __restrict__ col, uint64_t lo, uint64_t hi, const Fr& one,
                                                Fr& pn, Fr& pd) {
    pn = pd = one;
#pragma unroll 1
    for (uint64_t i = lo; i < hi; ++i) {
        pn = mont_mul(pn, ld_fr(col + 2 * i));
        pd = mont_mul(pd, ld_fr(col + 2 * i + 1));
    }
}
// In place, the carries k_gp_write multiplies in: tile i's slots become xn *
// (the N of the run's tiles below i) and xd * (the D of those above), with xn =
// K * the N of the runs below, xd = the D of the runs above.
__device__ __forceinline__ void gp_fold(Fr* __restrict__ col, uint64_t lo, uint64_t hi, Fr xn, Fr xd) {
#pragma unroll 1
    for (uint64_t i = lo; i < hi; ++i) {
        const Fr v = ld_fr(col + 2 * i);
        st_fr(col + 2 * i, xn);
        xn = mont_mul(xn, v);
    }
#pragma unroll 1
    for (uint64_t i = hi; i-- > lo;) {
        const Fr v = ld_fr(col + 2 * i + 1);
        st_fr(col + 2 * i + 1, xd);
        xd = mont_mul(xd, v);
    }
}

// -------------------------------------------------------------------- write
// A tile per block, kGpItems consecutive rows per thread. Row i of the tile
// gets (the N of the thread's rows below i) * (the D of its rows from i on)
// * (the N of the threads and tiles below, K) * (the D of those above).
// z (items x rows cells): rows [0, usable] the product, rows above zero.
template <class Leaf>
__global__ __launch_bounds__(kGpThreads) void k_gp_write(const Leaf leaf, const Fr* __restrict__ tp,
                                                         Fr* __restrict__ z) {
    __shared__ Fr sd[kGpItems][kGpThreads];                // a thread's own slots only
    const uint32_t c = blockIdx.y;
    const uint64_t t = blockIdx.x, nt = gridDim.x, rows = leaf.rows(), usable = leaf.usable();
    const uint64_t rb = t * kGpTile + (uint64_t)threadIdx.x * kGpItems;
    const Fr one = leaf.one();
    Fr* zc = z + (uint64_t)c * rows;
    if (t * kGpTile > usable) {                            // a tile of blinding rows
#pragma unroll 1
        for (unsigned j = 0; j < kGpItems; ++j)
            if (rb + j < rows) st_fr(zc + rb + j, fr_zero());
        return;
    }
    Fr pl[kGpItems];
#pragma unroll
    for (unsigned k = 0; k < kGpItems; ++k) pl[k] = one;
    Fr tn = one, td = one;
#pragma unroll 1
    for (unsigned j = 0; j < kGpItems; ++j) {
        Fr n = one, d = one;
        if (rb + j < usable) (void)gp_leaves(leaf, c, rb + j, n, d);
        lp_put(pl, j, tn);
        tn = mont_mul(tn, n);
        sd[j][threadIdx.x] = d;
    }
#pragma unroll 1
    for (unsigned j = kGpItems; j-- > 0;) {
        td = mont_mul(td, sd[j][threadIdx.x]);
        sd[j][threadIdx.x] = td;
    }
    const Fr* cr = tp + ((uint64_t)c * nt + t) * 2;
    Fr xn, xd, un0, un1;
    lp_block_scan<false>(one, tn, td, ld_fr(cr), ld_fr(cr + 1), xn, xd, un0, un1);
    const Fr cc = mont_mul(xn, xd);
#pragma unroll 1
    for (unsigned j = 0; j < kGpItems; ++j) {
        const uint64_t r = rb + j;
        if (r >= rows) break;
        Fr v = fr_zero();
        if (r <= usable) v = mont_mul(mont_mul(lp_get(pl, j), sd[j][threadIdx.x]), cc);
        st_fr(zc + r, v);
    }
}

// -------------------------------------------------------------------- check
// Z[r + 1] D[r] == Z[r] N[r] on the usable rows with the raw N and D (both
// sides carry the same power of R, so the words are compared), Z[0] == first,
// Z[usable] in {0, 1} where the item closes, zero cells above. cnt[0..1] +=
// recurrence rows checked / failed, cnt[2..3] += boundary rows, cnt[4..5] +=
// padding cells: k_check_cells' counting (per-thread counts, an LDS sum per
// block, one global atomic per counter and block). The cursor is taken for the
// thread's first row and advanced once per iteration, usable row or not.
template <class Leaf>
__global__ __launch_bounds__(kGpThreads) void k_gp_check(const Leaf leaf, const Fr* __restrict__ z,
                                                         unsigned long long* cnt) {
    __shared__ unsigned long long sh[6];
    if (threadIdx.x < 6) sh[threadIdx.x] = 0;
    __syncthreads();
    uint32_t v[6] = {0, 0, 0, 0, 0, 0};
    const uint32_t c = blockIdx.y;
    const uint64_t rows = leaf.rows(), usable = leaf.usable();
    const Fr* Z = z + (uint64_t)c * rows;
    const Fr zone = leaf.zone();
    const uint64_t step = (uint64_t)gridDim.x * kGpThreads;
    uint64_t r = (uint64_t)blockIdx.x * kGpThreads + threadIdx.x;
    typename Leaf::Cursor cur{};
    if (r < rows) cur = leaf.cursor(r);
#pragma unroll 1
    for (; r < rows; r += step) {
        const Fr zr = ld_fr(Z + r);
        if (r < usable) {                                  // usable < rows: Z[r + 1] is a row of the item
            Fr n, d;
            leaf.factors(c, r, cur, n, d);
            ++v[0];
            v[1] += !fr_eq(mont_mul(ld_fr(Z + r + 1), d), mont_mul(zr, n));
        }
        if (r == 0) {
            ++v[2];
            v[3] += !fr_eq(zr, leaf.first(c, Z));
        }
        if (r == usable && leaf.closes(c)) {
            ++v[2];
            v[3] += !(fr_is_zero(zr) || fr_eq(zr, zone));
        }
        if (r > usable) {
            ++v[4];
            v[5] += !fr_is_zero(zr);
        }
        leaf.advance(cur);
    }
#pragma unroll
    for (int k = 0; k < 6; ++k)
        if (v[k]) atomicAdd(&sh[k], (unsigned long long)v[k]);
    __syncthreads();
    if (threadIdx.x < 6 && sh[threadIdx.x]) atomicAdd(cnt + threadIdx.x, sh[threadIdx.x]);
}

}  // namespace svdw
