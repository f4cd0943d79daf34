// gfx950 kernels of the lookup argument's grand product (lookup_product.hpp).
// They are VALU-bound: a mont_mul is about 480 instructions, a row's cells four
// 32 B loads or stores. So the loops over a thread's rows and over the steps of
// a scan stay rolled (one inlined mont_mul per use, not per iteration), the
// rows a thread keeps between two loops live in registers behind a select chain
// or in LDS, and what counts is the multiplications per row. One column per
// blockIdx.y, 64-bit row indices.
#include <hip/hip_runtime.h>

#include "export.hpp"
#include "fr_scan.hpp"
#include "lookup_product.hpp"

namespace svdw {

static constexpr unsigned kLpMaxBlocks = 4096;               // per column, k_lp_check

// The factors of row r < usable of column c (A1, S1: the column's A', S'):
// n = (A + beta)(T + gamma), d = (A' + beta)(S' + gamma), each one mont_mul of
// the sums as the form hands them over. Canonical cells: both come out times
// 2^-256. Montgomery cells: d comes out in Montgomery form, and n too, as the
// canonical A + beta meets (T + gamma) 2^512 (T 2^512 is one CIOS round of the
// row index).
template <int FORM>
__device__ __forceinline__ void lp_factors(const LkSrc& s, const Fr* __restrict__ A1, const Fr* __restrict__ S1,
                                           const LpChal& ch, uint32_t c, uint64_t r, uint32_t lb, Fr& n, Fr& d) {
    const uint64_t i = (uint64_t)c * s.stride + r;
    const Fr a = (r >= s.span || i >= s.total) ? fr_zero() : ld_fr(s.p + i);   // a row past the assigned ones
    Fr t = fr_zero();
    t.w[0] = (r >> lb) ? 0u : (uint32_t)r;
    if (FORM == kFormMontgomery) t = fr_add(mont_mul_rounds<1>(t, ch.t2), ch.g2);
    else t = fr_add(t, ch.g0);
    n = mont_mul(fr_add(a, ch.b0), t);
    d = mont_mul(fr_add(ld_fr(A1 + r), ch.bx), fr_add(ld_fr(S1 + r), ch.gx));
}
// The same with inv0: a zero denominator enters the products of D as the
// neutral element and zeroes the row's numerator. True for such a row.
template <int FORM>
__device__ __forceinline__ bool lp_leaves(const LkSrc& s, const Fr* __restrict__ A1, const Fr* __restrict__ S1,
                                          const LpChal& ch, uint32_t c, uint64_t r, uint32_t lb, Fr& n, Fr& d) {
    lp_factors<FORM>(s, A1, S1, ch, c, r, lb, n, d);
    const bool z = fr_is_zero(d);
    n = lp_select(z, fr_zero(), n);
    d = lp_select(z, ch.one, d);
    return z;
}
template <int FORM>
__device__ __forceinline__ Fr lp_one(const LpChal& ch) {
    return FORM == kFormMontgomery ? ch.one : fr_from_u64(1);
}

// -------------------------------------------------------------------- tiles
// One wave per tile, 16 rows per lane at a stride of 64 (a product has no
// order, so the loads are coalesced), then a butterfly over the lanes.
template <int FORM>
__global__ __launch_bounds__(kLpThreads) void k_lp_tiles(const LkSrc s, const Fr* __restrict__ pin,
                                                         const Fr* __restrict__ ptab, const LpChal ch, uint64_t rows,
                                                         uint64_t usable, uint32_t lb, uint64_t nt,
                                                         Fr* __restrict__ tp, unsigned long long* cnt) {
    __shared__ uint32_t zs;
    if (threadIdx.x == 0) zs = 0;
    __syncthreads();
    const unsigned lane = threadIdx.x & 63u;
    const uint32_t c = blockIdx.y;
    const uint64_t t = (uint64_t)blockIdx.x * kLpWaves + (threadIdx.x >> 6);
    uint32_t nz = 0;
    if (t < nt) {                                          // the same for all lanes of a wave
        const Fr* A1 = pin + (uint64_t)c * rows;
        const Fr* S1 = ptab + (uint64_t)c * rows;
        Fr pn = ch.one, pd = ch.one;
#pragma unroll 1
        for (uint64_t r0 = t * kLpTile; r0 < (t + 1) * kLpTile && r0 < usable; r0 += 64) {
            const uint64_t r = r0 + lane;
            Fr n = ch.one, d = ch.one;
            if (r < usable) nz += lp_leaves<FORM>(s, A1, S1, ch, c, r, lb, n, d);
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
// One block per column over its nt tile products, a run of consecutive tiles
// per thread: the run's products, the block scan, then tile t's slots become
// K * (the products of N below t) and (the products of D above t). K = the
// inverse of the column's product of D, times 2^256 (canonical Z) or 2^512
// (Montgomery Z): the power that the product itself carries cancels, whatever
// it is. Z[usable] = K * the product of all N.
template <int FORM>
__global__ __launch_bounds__(kLpThreads) void k_lp_carry(Fr* __restrict__ tp, const LpChal ch, uint64_t nt,
                                                         unsigned long long* cnt) {
    __shared__ Fr kc;
    Fr* col = tp + (uint64_t)blockIdx.x * nt * 2;
    const uint64_t per = (nt + kLpThreads - 1) / kLpThreads;
    const uint64_t lo = threadIdx.x * per < nt ? threadIdx.x * per : nt, hi = lo + per < nt ? lo + per : nt;
    Fr pn = ch.one, pd = ch.one;
#pragma unroll 1
    for (uint64_t i = lo; i < hi; ++i) {
        pn = mont_mul(pn, ld_fr(col + 2 * i));
        pd = mont_mul(pd, ld_fr(col + 2 * i + 1));
    }
    Fr xn, xd, tn, td;
    lp_block_scan<true>(ch.one, pn, pd, ch.one, ch.one, xn, xd, tn, td);
    if (threadIdx.x == 0) {
        Fr k = fr_to_mont(fr_inv(td));                     // td != 0: no factor of it is zero
        if (FORM == kFormMontgomery) k = fr_to_mont(k);
        kc = k;
        if (!fr_eq(mont_mul(tn, k), lp_one<FORM>(ch))) atomicAdd(cnt + 1, 1ull);
    }
    __syncthreads();
    xn = mont_mul(xn, kc);
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
// A tile per block, kLpItems consecutive rows per thread. Row i of the tile
// gets (the N of the thread's rows below i) * (the D of its rows from i on)
// * (the N of the threads and tiles below, K) * (the D of those above).
template <int FORM>
__global__ __launch_bounds__(kLpThreads) void k_lp_write(const LkSrc s, const Fr* __restrict__ pin,
                                                         const Fr* __restrict__ ptab, const LpChal ch, uint64_t rows,
                                                         uint64_t usable, uint32_t lb, const Fr* __restrict__ tp,
                                                         Fr* __restrict__ z) {
    __shared__ Fr sd[kLpItems][kLpThreads];                // a thread's own slots only
    const uint32_t c = blockIdx.y;
    const uint64_t t = blockIdx.x, nt = gridDim.x;
    const uint64_t rb = t * kLpTile + (uint64_t)threadIdx.x * kLpItems;
    Fr* zc = z + (uint64_t)c * rows;
    if (t * kLpTile > usable) {                            // a tile of blinding rows
#pragma unroll 1
        for (unsigned j = 0; j < kLpItems; ++j)
            if (rb + j < rows) st_fr(zc + rb + j, fr_zero());
        return;
    }
    const Fr* A1 = pin + (uint64_t)c * rows;
    const Fr* S1 = ptab + (uint64_t)c * rows;
    Fr pl[kLpItems];
#pragma unroll
    for (unsigned k = 0; k < kLpItems; ++k) pl[k] = ch.one;
    Fr tn = ch.one, td = ch.one;
#pragma unroll 1
    for (unsigned j = 0; j < kLpItems; ++j) {
        Fr n = ch.one, d = ch.one;
        if (rb + j < usable) (void)lp_leaves<FORM>(s, A1, S1, ch, c, rb + j, lb, n, d);
        lp_put(pl, j, tn);
        tn = mont_mul(tn, n);
        sd[j][threadIdx.x] = d;
    }
#pragma unroll 1
    for (unsigned j = kLpItems; j-- > 0;) {
        td = mont_mul(td, sd[j][threadIdx.x]);
        sd[j][threadIdx.x] = td;
    }
    const Fr* cr = tp + ((uint64_t)c * nt + t) * 2;
    Fr xn, xd, un0, un1;
    lp_block_scan<false>(ch.one, tn, td, ld_fr(cr), ld_fr(cr + 1), xn, xd, un0, un1);
    const Fr cc = mont_mul(xn, xd);
#pragma unroll 1
    for (unsigned j = 0; j < kLpItems; ++j) {
        const uint64_t r = rb + j;
        if (r >= rows) break;
        Fr v = fr_zero();
        if (r <= usable) v = mont_mul(mont_mul(lp_get(pl, j), sd[j][threadIdx.x]), cc);
        st_fr(zc + r, v);
    }
}

// -------------------------------------------------------------------- check
// Z[r + 1] (A'[r] + beta)(S'[r] + gamma) == Z[r] (A[r] + beta)(T[r] + gamma) on
// the usable rows (both sides carry the same power of 2^256, so the words are
// compared), Z[0] == 1, Z[usable] in {0, 1}, zero cells above. k_check_cells'
// counting: per-thread counts, an LDS sum per block, one global atomic per
// counter and block.
template <int FORM>
__global__ __launch_bounds__(kLpThreads) void k_lp_check(const LkSrc s, const Fr* __restrict__ pin,
                                                         const Fr* __restrict__ ptab, const Fr* __restrict__ z,
                                                         const LpChal ch, uint64_t rows, uint64_t usable, uint32_t lb,
                                                         unsigned long long* cnt) {
    __shared__ unsigned long long sh[6];
    if (threadIdx.x < 6) sh[threadIdx.x] = 0;
    __syncthreads();
    uint32_t v[6] = {0, 0, 0, 0, 0, 0};
    const uint32_t c = blockIdx.y;
    const Fr* A1 = pin + (uint64_t)c * rows;
    const Fr* S1 = ptab + (uint64_t)c * rows;
    const Fr* Z = z + (uint64_t)c * rows;
    const Fr one = lp_one<FORM>(ch);
    const uint64_t step = (uint64_t)gridDim.x * kLpThreads;
#pragma unroll 1
    for (uint64_t r = (uint64_t)blockIdx.x * kLpThreads + threadIdx.x; r < rows; r += step) {
        const Fr zr = ld_fr(Z + r);
        if (r < usable) {                                  // usable < rows: Z[r + 1] is a row of the column
            Fr n, d;
            lp_factors<FORM>(s, A1, S1, ch, c, r, lb, n, d);
            ++v[0];
            v[1] += !fr_eq(mont_mul(ld_fr(Z + r + 1), d), mont_mul(zr, n));
        }
        if (r == 0) {
            ++v[2];
            v[3] += !fr_eq(zr, one);
        }
        if (r == usable) {
            ++v[2];
            v[3] += !(fr_is_zero(zr) || fr_eq(zr, one));
        }
        if (r > usable) {
            ++v[4];
            v[5] += !fr_is_zero(zr);
        }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k)
        if (v[k]) atomicAdd(&sh[k], (unsigned long long)v[k]);
    __syncthreads();
    if (threadIdx.x < 6 && sh[threadIdx.x]) atomicAdd(cnt + threadIdx.x, sh[threadIdx.x]);
}

// ----------------------------------------------------------------- launches
static bool lp_bad(const LkSrc& src, const void* pin, const void* ptab, int form, uint32_t ncols, uint64_t rows,
                   uint64_t usable, uint32_t lb) {
    return !pin || !ptab || (src.total && !src.p) || lb < 1 || lb > 31 || ncols > 65535 || usable >= rows ||
           rows > (1ull << 31) || (form != kFormCanonical && form != kFormMontgomery);
}
hipError_t launch_lp_tiles(const LkSrc& src, const Fr* pin, const Fr* ptab, const LpChal& ch, int form,
                           uint32_t ncols, uint64_t rows, uint64_t usable, uint32_t lb, Fr* tp,
                           unsigned long long* cnt, hipStream_t st) {
    if (!ncols) return hipSuccess;
    if (lp_bad(src, pin, ptab, form, ncols, rows, usable, lb) || !tp || !cnt) return hipErrorInvalidValue;
    const uint64_t nt = lp_tiles(rows);
    const dim3 g((unsigned)((nt + kLpWaves - 1) / kLpWaves), ncols), b(kLpThreads);
    if (form == kFormMontgomery)
        hipLaunchKernelGGL((k_lp_tiles<kFormMontgomery>), g, b, 0, st, src, pin, ptab, ch, rows, usable, lb, nt, tp, cnt);
    else
        hipLaunchKernelGGL((k_lp_tiles<kFormCanonical>), g, b, 0, st, src, pin, ptab, ch, rows, usable, lb, nt, tp, cnt);
    return hipGetLastError();
}
hipError_t launch_lp_carry(Fr* tp, const LpChal& ch, int form, uint32_t ncols, uint64_t rows, unsigned long long* cnt,
                           hipStream_t st) {
    if (!ncols) return hipSuccess;
    if (!tp || !cnt || !rows || (form != kFormCanonical && form != kFormMontgomery)) return hipErrorInvalidValue;
    const uint64_t nt = lp_tiles(rows);
    if (form == kFormMontgomery)
        hipLaunchKernelGGL((k_lp_carry<kFormMontgomery>), dim3(ncols), dim3(kLpThreads), 0, st, tp, ch, nt, cnt);
    else
        hipLaunchKernelGGL((k_lp_carry<kFormCanonical>), dim3(ncols), dim3(kLpThreads), 0, st, tp, ch, nt, cnt);
    return hipGetLastError();
}
hipError_t launch_lp_write(const LkSrc& src, const Fr* pin, const Fr* ptab, const LpChal& ch, int form,
                           uint32_t ncols, uint64_t rows, uint64_t usable, uint32_t lb, const Fr* tp, Fr* z,
                           hipStream_t st) {
    if (!ncols) return hipSuccess;
    if (lp_bad(src, pin, ptab, form, ncols, rows, usable, lb) || !tp || !z) return hipErrorInvalidValue;
    const dim3 g((unsigned)lp_tiles(rows), ncols), b(kLpThreads);
    if (form == kFormMontgomery)
        hipLaunchKernelGGL((k_lp_write<kFormMontgomery>), g, b, 0, st, src, pin, ptab, ch, rows, usable, lb, tp, z);
    else
        hipLaunchKernelGGL((k_lp_write<kFormCanonical>), g, b, 0, st, src, pin, ptab, ch, rows, usable, lb, tp, z);
    return hipGetLastError();
}
hipError_t launch_lp_check(const LkSrc& src, const Fr* pin, const Fr* ptab, const Fr* z, const LpChal& ch, int form,
                           uint32_t ncols, uint64_t rows, uint64_t usable, uint32_t lb, unsigned long long* cnt,
                           hipStream_t st) {
    if (!ncols) return hipSuccess;
    if (lp_bad(src, pin, ptab, form, ncols, rows, usable, lb) || !z || !cnt) return hipErrorInvalidValue;
    const uint64_t nb = (rows + kLpThreads - 1) / kLpThreads;
    const dim3 g((unsigned)(nb < kLpMaxBlocks ? nb : kLpMaxBlocks), ncols), b(kLpThreads);
    if (form == kFormMontgomery)
        hipLaunchKernelGGL((k_lp_check<kFormMontgomery>), g, b, 0, st, src, pin, ptab, z, ch, rows, usable, lb, cnt);
    else
        hipLaunchKernelGGL((k_lp_check<kFormCanonical>), g, b, 0, st, src, pin, ptab, z, ch, rows, usable, lb, cnt);
    return hipGetLastError();
}

}  // namespace svdw
