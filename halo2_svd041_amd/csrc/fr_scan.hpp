// Device pieces the two grand products share (lookup_product.hip,
// permutation_product.hip): Fr through the wave shuffles, a select chain in
// place of a runtime-indexed register array, and the block scan of a prefix
// product of N with a suffix product of D. Device code only.
#pragma once
#include <hip/hip_runtime.h>

#include "fr.hpp"
#include "lookup_product.hpp"

namespace svdw {

static constexpr unsigned kLpThreads = 256, kLpWaves = kLpThreads / 64;
static constexpr unsigned kLpItems = kLpTile / kLpThreads;   // consecutive rows per thread of a write pass

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
__device__ __forceinline__ void lp_put(Fr (&a)[kLpItems], unsigned j, const Fr& v) {
#pragma unroll
    for (unsigned k = 0; k < kLpItems; ++k) a[k] = lp_select(j == k, v, a[k]);
}
__device__ __forceinline__ Fr lp_get(const Fr (&a)[kLpItems], unsigned j) {
    Fr r = a[0];
#pragma unroll
    for (unsigned k = 1; k < kLpItems; ++k) r = lp_select(j == k, a[k], r);
    return r;
}

// --------------------------------------------------------------- block scan
// Over the block's threads: xn = cn * the pn of the threads below, xd = cd * the
// pd of the threads above (cn, cd the same for the whole block); with TOTALS
// tn, td = the products of all pn, all pd. One call per kernel (wn, wd).
template <bool TOTALS>
__device__ __forceinline__ void lp_block_scan(const Fr& one, Fr pn, Fr pd, const Fr& cn, const Fr& cd, Fr& xn, Fr& xd,
                                              Fr& tn, Fr& td) {
    __shared__ Fr wn[kLpWaves], wd[kLpWaves];
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
    for (unsigned k = 0; k < kLpWaves; ++k) {              // k against w: the same for all lanes of a wave
        if (k < w) on = mont_mul(on, wn[k]);
        if (k > w) od = mont_mul(od, wd[k]);
    }
    xn = mont_mul(on, en);
    xd = mont_mul(od, ed);
    if (TOTALS) {
        tn = td = one;
#pragma unroll 1
        for (unsigned k = 0; k < kLpWaves; ++k) {
            tn = mont_mul(tn, wn[k]);
            td = mont_mul(td, wd[k]);
        }
    }
}

}  // namespace svdw
