// gfx950 kernels of the SHPLONK opening (open.hpp): the linear combination of
// columns and the division by (X - s) as tiles, carry and write.
#include <hip/hip_runtime.h>

#include "export.hpp"
#include "grand_product.hpp"                                // the Fr shuffles and selects
#include "open.hpp"

namespace svdw {

__device__ __forceinline__ Fr open_pow(const PowTable& p, uint64_t e) {
    return pow_at(p, e & ((1ull << p.bits) - 1));           // beyond the table only where the power meets a zero
}

// --------------------------------------------------------------------- fold
__global__ __launch_bounds__(kOpenFoldThreads) void k_open_fold(const Fr* const* __restrict__ cols,
                                                                const Fr* __restrict__ sc, uint32_t ncols,
                                                                const Fr* __restrict__ acc, const Fr cacc, uint64_t n,
                                                                Fr* __restrict__ out) {
    const uint64_t step = (uint64_t)gridDim.x * kOpenFoldThreads;
#pragma unroll 1
    for (uint64_t r = (uint64_t)blockIdx.x * kOpenFoldThreads + threadIdx.x; r < n; r += step) {
        Fr s = fr_zero();
        if (acc) s = mont_mul(ld_fr(acc + r), cacc);
#pragma unroll 1
        for (uint32_t j = 0; j < ncols; ++j) s = fr_add(s, mont_mul(ld_fr(cols[j] + r), ld_fr(sc + j)));
        st_fr(out + r, s);
    }
}

// -------------------------------------------------------------------- tiles
__global__ __launch_bounds__(kOpenThreads) void k_open_tiles(const Fr* __restrict__ a, uint64_t n, const PowTable pw,
                                                             uint64_t nt, Fr* __restrict__ tot) {
    const unsigned lane = threadIdx.x & 63u;
    const uint64_t t = (uint64_t)blockIdx.x * kOpenWaves + (threadIdx.x >> 6);
    if (t >= nt) return;                                    // the same for all lanes of a wave
    const Fr s64 = open_pow(pw, 64);
    Fr v = fr_zero();
#pragma unroll 1
    for (unsigned m = kOpenTile / 64; m-- > 0;) {
        const uint64_t r = t * kOpenTile + m * 64 + lane;
        v = mont_mul(v, s64);
        if (r < n) v = fr_add(v, ld_fr(a + r));
    }
    v = mont_mul(v, open_pow(pw, lane));
#pragma unroll 1
    for (unsigned m = 1; m < 64; m <<= 1) v = fr_add(v, lp_shfl_xor(v, m));
    if (lane == 0) st_fr(tot + t, v);
}

// --------------------------------------------------------------- block scan
// Thread i holds v, the value of its run of `len` coefficients at the run's
// first one, and m = s^len R. Returns what enters the thread from above, at its
// run's end: sum_{j > i} v_j s^(len (j - i - 1)) + s^(len (kOpenThreads - 1 - i)) seed.
// One call per kernel (wt).
__device__ __forceinline__ Fr open_block_scan(Fr v, Fr m, const Fr& seed, const PowTable& pw, uint32_t len) {
    __shared__ Fr wt[kOpenWaves];
    const unsigned lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
#pragma unroll 1
    for (unsigned d = 1; d < 64; d <<= 1) {
        const Fr b = lp_shfl_down(v, d);
        v = fr_add(v, mont_mul(lp_select(lane + d < 64u, b, fr_zero()), m));
        m = mont_mul(m, m);
    }
    if (lane == 0) wt[w] = v;                               // the wave's value at its first coefficient
    const Fr ex = lp_select(lane < 63, lp_shfl_down(v, 1), fr_zero());
    __syncthreads();
    Fr o = seed;                                            // m = s^(64 len) R
#pragma unroll 1
    for (unsigned k = kOpenWaves; k-- > w + 1;) o = fr_add(mont_mul(o, m), wt[k]);
    return fr_add(ex, mont_mul(o, open_pow(pw, (uint64_t)len * (63u - lane))));
}

// -------------------------------------------------------------------- carry
// One block. Round j takes the totals [j kOpenCarryCap, (j + 1) kOpenCarryCap),
// one per thread; a thread's totals of all rounds are consecutive, its run (the
// last runs may be short or empty: totals past nt are zero): a Horner in S down
// the run, the block scan over the runs, then down the run again handing each
// tile what enters it from above.
__global__ __launch_bounds__(kOpenThreads) void k_open_carry(Fr* __restrict__ tot, uint64_t nt, const PowTable pw) {
    const uint64_t rounds = (nt + kOpenCarryCap - 1) / kOpenCarryCap;
    const uint64_t lo = threadIdx.x * rounds < nt ? threadIdx.x * rounds : nt, hi = lo + rounds < nt ? lo + rounds : nt;
    const Fr S = open_pow(pw, kOpenTile);
    Fr v = fr_zero();
#pragma unroll 1
    for (uint64_t i = hi; i-- > lo;) v = fr_add(mont_mul(v, S), ld_fr(tot + i));
    // a short run has nothing above it: what enters it is zero wherever its end is taken to be
    Fr e = open_block_scan(v, open_pow(pw, kOpenTile * rounds), fr_zero(), pw, (uint32_t)(kOpenTile * rounds));
#pragma unroll 1
    for (uint64_t i = hi; i-- > lo;) {
        const Fr t = ld_fr(tot + i);
        st_fr(tot + i, e);
        e = fr_add(mont_mul(e, S), t);
    }
}

// -------------------------------------------------------------------- write
template <bool ACC>
__global__ __launch_bounds__(kOpenThreads) void k_open_write(const Fr* a, uint64_t n, const PowTable pw,
                                                             const Fr* __restrict__ carry, const Fr vR, Fr* out,
                                                             Fr* __restrict__ rem) {
    static_assert(kOpenItems == 4, "four named coefficients per thread");
    const uint64_t t = blockIdx.x, rb = t * kOpenTile + (uint64_t)threadIdx.x * kOpenItems;
    const Fr s = open_pow(pw, 1);
    const Fr a0 = rb < n ? ld_fr(a + rb) : fr_zero(), a1 = rb + 1 < n ? ld_fr(a + rb + 1) : fr_zero(),
             a2 = rb + 2 < n ? ld_fr(a + rb + 2) : fr_zero(), a3 = rb + 3 < n ? ld_fr(a + rb + 3) : fr_zero();
    const Fr val = fr_add(a0, mont_mul(fr_add(a1, mont_mul(fr_add(a2, mont_mul(a3, s)), s)), s));
    const Fr q3 = open_block_scan(val, open_pow(pw, kOpenItems), carry ? ld_fr(carry + t) : fr_zero(), pw, kOpenItems);
    const Fr q2 = fr_add(a3, mont_mul(q3, s)), q1 = fr_add(a2, mont_mul(q2, s)), q0 = fr_add(a1, mont_mul(q1, s));
    if (rem && rb == 0) st_fr(rem, fr_add(a0, mont_mul(q0, s)));
#pragma unroll 1
    for (unsigned j = 0; j < kOpenItems; ++j) {
        const uint64_t r = rb + j;
        if (r >= n) break;
        Fr q = lp_select(j == 0, q0, lp_select(j == 1, q1, lp_select(j == 2, q2, q3)));
        if (ACC) q = fr_add(q, mont_mul(ld_fr(out + r), vR));
        st_fr(out + r, q);
    }
}

// ----------------------------------------------------------------- launches
static bool open_bad(uint64_t n, const PowTable& pw) {
    return !n || n > (1ull << 28) || pw.bits < kOpenLogTile || pw.bits > 28 || pow_table_bad(pw, pw.bits) ||
           (1ull << pw.bits) < n;
}
hipError_t launch_open_fold(const Fr* const* cols, const Fr* sc, uint32_t ncols, const Fr* acc, const Fr& cacc,
                            uint64_t n, Fr* out, hipStream_t st) {
    if (!n) return hipSuccess;
    if ((ncols && (!cols || !sc)) || !out || n > (1ull << 28)) return hipErrorInvalidValue;
    const uint64_t nb = (n + kOpenFoldThreads - 1) / kOpenFoldThreads;
    hipLaunchKernelGGL(k_open_fold, dim3((unsigned)(nb < kOpenFoldBlocks ? nb : kOpenFoldBlocks)),
                       dim3(kOpenFoldThreads), 0, st, cols, sc, ncols, acc, cacc, n, out);
    return hipGetLastError();
}
hipError_t launch_open_tiles(const Fr* a, uint64_t n, const PowTable& pw, Fr* tot, hipStream_t st) {
    if (open_bad(n, pw) || !a || !tot) return hipErrorInvalidValue;
    const uint64_t nt = open_tiles(n);
    hipLaunchKernelGGL(k_open_tiles, dim3((unsigned)((nt + kOpenWaves - 1) / kOpenWaves)), dim3(kOpenThreads), 0, st,
                       a, n, pw, nt, tot);
    return hipGetLastError();
}
hipError_t launch_open_carry(Fr* tot, uint64_t nt, const PowTable& pw, hipStream_t st) {
    if (!nt || !tot || pw.bits > 28 || pow_table_bad(pw, pw.bits) || nt > open_tiles(1ull << pw.bits))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_open_carry, dim3(1), dim3(kOpenThreads), 0, st, tot, nt, pw);
    return hipGetLastError();
}
hipError_t launch_open_write(const Fr* a, uint64_t n, const PowTable& pw, const Fr* carry, const Fr* v, Fr* out,
                             Fr* rem, hipStream_t st) {
    if (open_bad(n, pw) || !a || !out || (!carry && open_tiles(n) > 1)) return hipErrorInvalidValue;
    const dim3 g((unsigned)open_tiles(n)), b(kOpenThreads);
    if (v) hipLaunchKernelGGL(k_open_write<true>, g, b, 0, st, a, n, pw, carry, *v, out, rem);
    else hipLaunchKernelGGL(k_open_write<false>, g, b, 0, st, a, n, pw, carry, fr_zero(), out, rem);
    return hipGetLastError();
}

}  // namespace svdw
