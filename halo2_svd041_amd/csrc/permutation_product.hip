// gfx950 kernels of the permutation argument's grand products
// (permutation_product.hpp). VALU-bound like lookup_product.hip, whose pass
// structure and scan (fr_scan.hpp) they keep: a mont_mul is about 480
// instructions, so the loops over a set's columns, over a thread's rows and over
// the steps of a scan stay rolled (one inlined mont_mul per use), the column
// base pointers and beta delta^j come from device tables at a uniform index,
// and what counts is the multiplications. With m the columns of a set, per row
// of the set (per cell: divide by m):
//
//   leaf (pp_factors)   4 m + 1     per column beta sigma, beta delta^j omega^r,
//                                   the two running products; omega^r once
//   k_pp_tiles          4 m + 3.75  the leaf, into the lane's two products, 12 / 16
//                                   for the butterfly
//   k_pp_write          4 m + 9.5   the leaf, the thread's prefix and suffix, two
//                                   for the row's Z, 18 / kLpItems for the block
//                                   scan
//   k_pp_check          4 m + 4     the leaf, both sides, the omega step
//   k_pp_values         2 per cell
//
// One set per blockIdx.y, 64-bit row indices.
#include <hip/hip_runtime.h>

#include "export.hpp"
#include "fr_scan.hpp"
#include "permutation_product.hpp"

namespace svdw {

static_assert(kPpCarryThreads == kLpThreads, "the carry kernels scan with lp_block_scan");
static constexpr unsigned kPpMaxBlocks = 4096;               // per set, k_pp_check

__device__ __forceinline__ Fr pp_omega(const Fr* __restrict__ wlo, const Fr* __restrict__ whi, uint32_t h, uint64_t r) {
    return mont_mul(ld_fr(whi + (r >> h)), ld_fr(wlo + (r & ((1ull << h) - 1))));
}
// The factors of row r < usable of the set of columns [j0, j1), w = omega^r R.
// j counts over all columns: the identity term of column j is delta^j omega^r.
__device__ __forceinline__ void pp_factors(const PpArgs& a, uint32_t j0, uint32_t j1, uint64_t r, const Fr& w, Fr& n,
                                           Fr& d) {
    n = d = a.one;
#pragma unroll 1
    for (uint32_t j = j0; j < j1; ++j) {
        const Fr v = fr_add(ld_fr(a.cols[j] + r), a.g);
        const Fr sg = mont_mul(ld_fr(a.sig[j] + r), a.bR);
        const Fr id = mont_mul(w, ld_fr(a.bd + j));
        n = mont_mul(n, fr_add(v, id));
        d = mont_mul(d, fr_add(v, sg));
    }
}
// The same with inv0: a zero denominator enters the products of D as the
// neutral element and zeroes the row's numerator. True for such a row.
__device__ __forceinline__ bool pp_leaves(const PpArgs& a, uint32_t j0, uint32_t j1, uint64_t r, Fr& n, Fr& d) {
    pp_factors(a, j0, j1, r, pp_omega(a.wlo, a.whi, a.h, r), n, d);
    const bool z = fr_is_zero(d);
    n = lp_select(z, fr_zero(), n);
    d = lp_select(z, a.one, d);
    return z;
}
__device__ __forceinline__ uint32_t pp_set_end(const PpArgs& a, uint32_t j0) {
    return a.ncols - j0 < a.chunk ? a.ncols : j0 + a.chunk;
}

// -------------------------------------------------------------------- tiles
// One wave per tile, 16 rows per lane at a stride of 64, then a butterfly over
// the lanes (k_lp_tiles with the set's leaves).
__global__ __launch_bounds__(kLpThreads) void k_pp_tiles(const PpArgs a, uint64_t nt, Fr* __restrict__ tp,
                                                         unsigned long long* cnt) {
    __shared__ uint32_t zs;
    if (threadIdx.x == 0) zs = 0;
    __syncthreads();
    const unsigned lane = threadIdx.x & 63u;
    const uint32_t s = blockIdx.y, j0 = s * a.chunk, j1 = pp_set_end(a, j0);
    const uint64_t t = (uint64_t)blockIdx.x * kLpWaves + (threadIdx.x >> 6);
    uint32_t nz = 0;
    if (t < nt) {                                          // the same for all lanes of a wave
        Fr pn = a.one, pd = a.one;
#pragma unroll 1
        for (uint64_t r0 = t * kLpTile; r0 < (t + 1) * kLpTile && r0 < a.usable; r0 += 64) {
            const uint64_t r = r0 + lane;
            Fr n = a.one, d = a.one;
            if (r < a.usable) nz += pp_leaves(a, j0, j1, r, n, d);
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
            Fr* o = tp + ((uint64_t)s * nt + t) * 2;
            st_fr(o, pn);
            st_fr(o + 1, pd);
            if (nz) atomicAdd(&zs, nz);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && zs) atomicAdd(cnt, (unsigned long long)zs);
}

// -------------------------------------------------------------------- carry
// The thread's run of consecutive tiles, the same in k_pp_totals and k_pp_fold.
__device__ __forceinline__ void pp_run(uint64_t nt, uint64_t& lo, uint64_t& hi) {
    const uint64_t per = (nt + kLpThreads - 1) / kLpThreads;
    lo = threadIdx.x * per < nt ? threadIdx.x * per : nt;
    hi = lo + per < nt ? lo + per : nt;
}
// One block per set over its nt tile products: the runs' products and the
// block scan give xs[(s * threads + thread) * 2 + {0, 1}] = the products of N
// of the runs below, of D of the runs above. sv[2 s] = (the set's product of N)
// / (its product of D) * R, the factor from start_s to start_{s+1}; sv[2 s + 1]
// = the inverse of the product of D, times R (canonical Z) or R^2 (Montgomery
// Z): the power that the product itself carries cancels, whatever it is.
__global__ __launch_bounds__(kLpThreads) void k_pp_totals(const Fr* __restrict__ tp, const Fr one, int mont,
                                                          uint64_t nt, Fr* __restrict__ xs, Fr* __restrict__ sv) {
    const uint32_t s = blockIdx.x;
    const Fr* col = tp + (uint64_t)s * nt * 2;
    uint64_t lo, hi;
    pp_run(nt, lo, hi);
    Fr pn = one, pd = one;
#pragma unroll 1
    for (uint64_t i = lo; i < hi; ++i) {
        pn = mont_mul(pn, ld_fr(col + 2 * i));
        pd = mont_mul(pd, ld_fr(col + 2 * i + 1));
    }
    Fr xn, xd, tn, td;
    lp_block_scan<true>(one, pn, pd, one, one, xn, xd, tn, td);
    Fr* x = xs + ((uint64_t)s * kLpThreads + threadIdx.x) * 2;
    st_fr(x, xn);
    st_fr(x + 1, xd);
    if (threadIdx.x == 0) {
        const Fr k = fr_to_mont(fr_inv(td));               // td != 0: no factor of it is zero
        const Fr k2 = fr_to_mont(k);
        st_fr(sv + 2 * (uint64_t)s, mont_mul(tn, k2));
        st_fr(sv + 2 * (uint64_t)s + 1, mont ? k2 : k);
    }
}
// The chain, nsets multiplications by one thread: sv[2 s] becomes start_s R,
// sv[2 s + 1] the set's inverse times start_s. After the last set the start is
// that set's Z[usable].
__global__ void k_pp_chain(Fr* __restrict__ sv, const Fr one, uint32_t nsets, unsigned long long* cnt) {
    if (blockIdx.x || threadIdx.x) return;
    Fr start = one;
#pragma unroll 1
    for (uint32_t s = 0; s < nsets; ++s) {
        const Fr f = ld_fr(sv + 2 * (uint64_t)s), k = ld_fr(sv + 2 * (uint64_t)s + 1);
        st_fr(sv + 2 * (uint64_t)s, start);
        st_fr(sv + 2 * (uint64_t)s + 1, mont_mul(k, start));
        start = mont_mul(start, f);
    }
    if (!fr_eq(start, one)) atomicAdd(cnt + 1, 1ull);
}
// One block per set: tile t's slots become (the set's inverse and start) * (the
// products of N below t) and (the products of D above t).
__global__ __launch_bounds__(kLpThreads) void k_pp_fold(Fr* __restrict__ tp, const Fr* __restrict__ xs,
                                                        const Fr* __restrict__ sv, uint64_t nt) {
    const uint32_t s = blockIdx.x;
    Fr* col = tp + (uint64_t)s * nt * 2;
    uint64_t lo, hi;
    pp_run(nt, lo, hi);
    const Fr* x = xs + ((uint64_t)s * kLpThreads + threadIdx.x) * 2;
    Fr xn = mont_mul(ld_fr(x), ld_fr(sv + 2 * (uint64_t)s + 1)), xd = ld_fr(x + 1);
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
// A tile per block, kLpItems consecutive rows per thread (k_lp_write with the
// set's leaves).
__global__ __launch_bounds__(kLpThreads) void k_pp_write(const PpArgs a, const Fr* __restrict__ tp,
                                                         Fr* __restrict__ z) {
    __shared__ Fr sd[kLpItems][kLpThreads];                // a thread's own slots only
    const uint32_t s = blockIdx.y, j0 = s * a.chunk, j1 = pp_set_end(a, j0);
    const uint64_t t = blockIdx.x, nt = gridDim.x;
    const uint64_t rb = t * kLpTile + (uint64_t)threadIdx.x * kLpItems;
    Fr* zc = z + (uint64_t)s * a.rows;
    if (t * kLpTile > a.usable) {                          // a tile of blinding rows
#pragma unroll 1
        for (unsigned j = 0; j < kLpItems; ++j)
            if (rb + j < a.rows) st_fr(zc + rb + j, fr_zero());
        return;
    }
    Fr pl[kLpItems];
#pragma unroll
    for (unsigned k = 0; k < kLpItems; ++k) pl[k] = a.one;
    Fr tn = a.one, td = a.one;
#pragma unroll 1
    for (unsigned j = 0; j < kLpItems; ++j) {
        Fr n = a.one, d = a.one;
        if (rb + j < a.usable) (void)pp_leaves(a, j0, j1, rb + j, n, d);
        lp_put(pl, j, tn);
        tn = mont_mul(tn, n);
        sd[j][threadIdx.x] = d;
    }
#pragma unroll 1
    for (unsigned j = kLpItems; j-- > 0;) {
        td = mont_mul(td, sd[j][threadIdx.x]);
        sd[j][threadIdx.x] = td;
    }
    const Fr* cr = tp + ((uint64_t)s * nt + t) * 2;
    Fr xn, xd, un0, un1;
    lp_block_scan<false>(a.one, tn, td, ld_fr(cr), ld_fr(cr + 1), xn, xd, un0, un1);
    const Fr cc = mont_mul(xn, xd);
#pragma unroll 1
    for (unsigned j = 0; j < kLpItems; ++j) {
        const uint64_t r = rb + j;
        if (r >= a.rows) break;
        Fr v = fr_zero();
        if (r <= a.usable) v = mont_mul(mont_mul(lp_get(pl, j), sd[j][threadIdx.x]), cc);
        st_fr(zc + r, v);
    }
}

// -------------------------------------------------------------------- check
// Z_s[r + 1] D_s[r] == Z_s[r] N_s[r] on the usable rows with the raw N and D
// (both sides carry the same power of R, so the words are compared), Z_0[0] == 1,
// Z_s[0] == Z_{s-1}[usable], the last Z[usable] in {0, 1}, zero cells above.
// omega^r: the table for the thread's first row, then steps of wstep =
// omega^(gridDim.x * kLpThreads) R; only the table itself is shared with the
// passes above. k_lp_check's counting.
__global__ __launch_bounds__(kLpThreads) void k_pp_check(const PpArgs a, const Fr* __restrict__ z, const Fr zone,
                                                         const Fr wstep, unsigned long long* cnt) {
    __shared__ unsigned long long sh[6];
    if (threadIdx.x < 6) sh[threadIdx.x] = 0;
    __syncthreads();
    uint32_t v[6] = {0, 0, 0, 0, 0, 0};
    const uint32_t s = blockIdx.y, j0 = s * a.chunk, j1 = pp_set_end(a, j0);
    const Fr* Z = z + (uint64_t)s * a.rows;
    const uint64_t step = (uint64_t)gridDim.x * kLpThreads;
    uint64_t r = (uint64_t)blockIdx.x * kLpThreads + threadIdx.x;
    Fr w = a.one;
    if (r < a.rows) w = pp_omega(a.wlo, a.whi, a.h, r);
#pragma unroll 1
    for (; r < a.rows; r += step) {
        const Fr zr = ld_fr(Z + r);
        if (r < a.usable) {                                // usable < rows: Z[r + 1] is a row of the column
            Fr n, d;
            pp_factors(a, j0, j1, r, w, n, d);
            ++v[0];
            v[1] += !fr_eq(mont_mul(ld_fr(Z + r + 1), d), mont_mul(zr, n));
        }
        if (r == 0) {
            ++v[2];
            v[3] += !fr_eq(zr, s ? ld_fr(Z - a.rows + a.usable) : zone);
        }
        if (r == a.usable && s + 1 == a.nsets) {
            ++v[2];
            v[3] += !(fr_is_zero(zr) || fr_eq(zr, zone));
        }
        if (r > a.usable) {
            ++v[4];
            v[5] += !fr_is_zero(zr);
        }
        w = mont_mul(w, wstep);
    }
#pragma unroll
    for (int k = 0; k < 6; ++k)
        if (v[k]) atomicAdd(&sh[k], (unsigned long long)v[k]);
    __syncthreads();
    if (threadIdx.x < 6 && sh[threadIdx.x]) atomicAdd(cnt + threadIdx.x, sh[threadIdx.x]);
}

// ------------------------------------------------------------------- values
__global__ __launch_bounds__(kLpThreads) void k_pp_values(const uint64_t* __restrict__ mapping,
                                                          const Fr* __restrict__ dl, const Fr* __restrict__ wlo,
                                                          const Fr* __restrict__ whi, uint32_t h, uint32_t first_col,
                                                          uint32_t total_cols, uint64_t rows, uint64_t cells,
                                                          Fr* __restrict__ out, unsigned long long* cnt) {
    __shared__ uint32_t bad;
    if (threadIdx.x == 0) bad = 0;
    __syncthreads();
    const uint64_t step = (uint64_t)gridDim.x * kLpThreads;
    uint32_t nb = 0;
#pragma unroll 1
    for (uint64_t i = (uint64_t)blockIdx.x * kLpThreads + threadIdx.x; i < cells; i += step) {
        uint64_t col, row;
        if (mapping) {
            const uint64_t e = mapping[i];
            col = e >> 32;
            row = e & 0xffffffffull;
        } else {
            col = first_col + i / rows;
            row = i % rows;
        }
        Fr v = fr_zero();
        if (col < total_cols && row < rows) v = mont_mul(pp_omega(wlo, whi, h, row), ld_fr(dl + col));
        else ++nb;
        st_fr(out + i, v);
    }
    if (nb) atomicAdd(&bad, nb);
    __syncthreads();
    if (threadIdx.x == 0 && bad) atomicAdd(cnt, (unsigned long long)bad);
}

// ----------------------------------------------------------------- launches
static bool pp_bad(const PpArgs& a, int form) {
    return !a.cols || !a.sig || !a.bd || !a.wlo || !a.whi || !a.ncols || !a.chunk || a.ncols > 65535 ||
           a.nsets != pp_sets(a.ncols, a.chunk) || a.usable >= a.rows || a.rows > (1ull << 31) ||
           (a.rows & (a.rows - 1)) || a.h > 31 || (1ull << a.h) > a.rows ||
           (form != kFormCanonical && form != kFormMontgomery);
}
static Fr pp_zone(const PpArgs& a, int form) { return form == kFormMontgomery ? a.one : fr_from_u64(1); }

hipError_t launch_pp_tiles(const PpArgs& a, int form, Fr* tp, unsigned long long* cnt, hipStream_t st) {
    if (pp_bad(a, form) || !tp || !cnt) return hipErrorInvalidValue;
    const uint64_t nt = lp_tiles(a.rows);
    const dim3 g((unsigned)((nt + kLpWaves - 1) / kLpWaves), a.nsets), b(kLpThreads);
    hipLaunchKernelGGL(k_pp_tiles, g, b, 0, st, a, nt, tp, cnt);
    return hipGetLastError();
}
hipError_t launch_pp_totals(const PpArgs& a, int form, const Fr* tp, Fr* xs, Fr* sv, hipStream_t st) {
    if (pp_bad(a, form) || !tp || !xs || !sv) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pp_totals, dim3(a.nsets), dim3(kLpThreads), 0, st, tp, a.one,
                       (int)(form == kFormMontgomery), lp_tiles(a.rows), xs, sv);
    return hipGetLastError();
}
hipError_t launch_pp_chain(const PpArgs& a, Fr* sv, unsigned long long* cnt, hipStream_t st) {
    if (!a.nsets || !sv || !cnt) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pp_chain, dim3(1), dim3(64), 0, st, sv, a.one, a.nsets, cnt);
    return hipGetLastError();
}
hipError_t launch_pp_fold(const PpArgs& a, int form, Fr* tp, const Fr* xs, const Fr* sv, hipStream_t st) {
    if (pp_bad(a, form) || !tp || !xs || !sv) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pp_fold, dim3(a.nsets), dim3(kLpThreads), 0, st, tp, xs, sv, lp_tiles(a.rows));
    return hipGetLastError();
}
hipError_t launch_pp_write(const PpArgs& a, int form, const Fr* tp, Fr* z, hipStream_t st) {
    if (pp_bad(a, form) || !tp || !z) return hipErrorInvalidValue;
    const dim3 g((unsigned)lp_tiles(a.rows), a.nsets), b(kLpThreads);
    hipLaunchKernelGGL(k_pp_write, g, b, 0, st, a, tp, z);
    return hipGetLastError();
}
static unsigned pp_check_blocks(uint64_t rows) {
    const uint64_t nb = (rows + kLpThreads - 1) / kLpThreads;
    return (unsigned)(nb < kPpMaxBlocks ? nb : kPpMaxBlocks);
}
uint64_t pp_check_stride(uint64_t rows) { return (uint64_t)pp_check_blocks(rows) * kLpThreads; }
hipError_t launch_pp_check(const PpArgs& a, int form, const Fr* z, const Fr& wstep, unsigned long long* cnt,
                           hipStream_t st) {
    if (pp_bad(a, form) || !z || !cnt) return hipErrorInvalidValue;
    const dim3 g(pp_check_blocks(a.rows), a.nsets), b(kLpThreads);
    hipLaunchKernelGGL(k_pp_check, g, b, 0, st, a, z, pp_zone(a, form), wstep, cnt);
    return hipGetLastError();
}
hipError_t launch_pp_values(const uint64_t* mapping, const Fr* dl, const Fr* wlo, const Fr* whi, uint32_t h,
                            uint32_t first_col, uint32_t ncols, uint32_t total_cols, uint64_t rows, Fr* out,
                            unsigned long long* cnt, hipStream_t st) {
    if (!ncols) return hipSuccess;
    if (!dl || !wlo || !whi || !out || !cnt || !rows || (rows & (rows - 1)) || rows > (1ull << 31) ||
        (1ull << h) > rows || ncols > 65535 || total_cols > 65535)
        return hipErrorInvalidValue;
    const uint64_t cells = (uint64_t)ncols * rows, nb = (cells + kLpThreads - 1) / kLpThreads;
    hipLaunchKernelGGL(k_pp_values, dim3((unsigned)(nb < 65536 ? nb : 65536)), dim3(kLpThreads), 0, st, mapping, dl,
                       wlo, whi, h, first_col, total_cols, rows, cells, out, cnt);
    return hipGetLastError();
}

}  // namespace svdw
