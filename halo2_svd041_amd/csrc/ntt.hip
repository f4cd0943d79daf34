// gfx950 kernels of the Fr transforms (ntt.hpp). Multiplications (mont_mul) per
// element, with b the radix bits of the pass:
//
//   k_ntt_pass   (b - 1) / 2    the radix-2 stages in LDS but the last, one per
//                               butterfly of two cells; the last stage has none
//                + 2            the factor omega_N^(s p i) to the next pass, formed
//                               from the two-level table and applied (not on the
//                               last pass)
//                + 2            shift^i on the first pass's load (forward with a
//                               shift), or shift^i 2^-k on the last pass's store
//                               (inverse with a shift); + 1 for the inverse's
//                               2^-k alone; + 0 forward without a shift
//   so a forward transform without a shift costs (k - P) / 2 + 2 (P - 1) per
//   element over its P passes, 14.5 at k = 24, and an inverse one more.
//   k_ntt_eval   1 + (8 + 2 bits(n) + 1) / run per coefficient and point:
//                Horner in x^256 over the thread's run, the 8 squarings for
//                x^256, x^(first index) by square and multiply, one to apply
//                it; run = 256 from n = 2^16 on
//   k_ntt_eval_sum, k_ntt_compare   none
#include <hip/hip_runtime.h>

#include "export.hpp"
#include "grand_product.hpp"
#include "ntt.hpp"

namespace svdw {

static constexpr uint32_t kNttTile = 1u << kNttLogTile;

// ------------------------------------------------------------ the LDS tile
__device__ __forceinline__ uint32_t ntt_slot(uint32_t pos) { return pos ^ ((pos >> 5) & 31u); }
__device__ __forceinline__ Fr ntt_get(const uint32_t (*sh)[kNttTile], uint32_t pos) {
    const uint32_t s = ntt_slot(pos);
    Fr r;
#pragma unroll
    for (int w = 0; w < 8; ++w) r.w[w] = sh[w][s];
    return r;
}
__device__ __forceinline__ void ntt_put(uint32_t (*sh)[kNttTile], uint32_t pos, const Fr& v) {
    const uint32_t s = ntt_slot(pos);
#pragma unroll
    for (int w = 0; w < 8; ++w) sh[w][s] = v.w[w];
}

// ------------------------------------------------------------------- a pass
__global__ __launch_bounds__(kNttThreads) void k_ntt_pass(const NttPass a) {
    __shared__ uint32_t sh[8][kNttTile];
    const uint32_t col = blockIdx.y, tid = threadIdx.x;
    const uint32_t lc = (a.k < kNttLogTile ? a.k : kNttLogTile) - a.b;
    const uint32_t r = 1u << a.b, c = 1u << lc, T = r << lc;
    const uint64_t N = 1ull << a.k, stride = N >> a.b, rows_in = 1ull << a.kin;
    const uint64_t t0 = (uint64_t)blockIdx.x << lc;
    const Fr* __restrict__ in = a.cols ? a.cols[col] : a.src + (uint64_t)col * N;
    Fr* __restrict__ out = a.dst + (uint64_t)col * N;

    // gather: cell e of the tile is row j = e / c of butterfly t0 + e % c
#pragma unroll 1
    for (uint32_t e = tid; e < T; e += kNttThreads) {
        const uint64_t idx = t0 + (e & (c - 1)) + (uint64_t)(e >> lc) * stride;
        Fr v = fr_zero();
        if (idx < rows_in) {
            v = ld_fr(in + idx);
            if (a.pre) v = mont_mul(v, pow_at(a.f, idx));
        }
        ntt_put(sh, e, v);
    }
    __syncthreads();

    // the stages hh = r / 2 .. 2 over j, for every butterfly of the tile at once
#pragma unroll 1
    for (uint32_t hh = r >> 1; hh >= 2; hh >>= 1) {
        const uint32_t tstep = (kNttTile / 2) / hh;
#pragma unroll 1
        for (uint32_t bf = tid; bf < T / 2; bf += kNttThreads) {
            const uint32_t tt = bf & (c - 1), jj = bf >> lc, u = jj & (hh - 1);
            const uint32_t pa = ((((jj - u) << 1) + u) << lc) + tt, pb = pa + (hh << lc);
            const Fr x = ntt_get(sh, pa), y = ntt_get(sh, pb);
            ntt_put(sh, pa, fr_add(x, y));
            ntt_put(sh, pb, mont_mul(fr_sub(x, y), ld_fr(a.tw + u * tstep)));
        }
        __syncthreads();
    }

    // scatter: output i of butterfly t sits at row brev(i), its last stage
    // folded in. The first pass writes one run (i fastest), the others runs of c.
    const uint64_t smask = (1ull << a.ls) - 1;
#pragma unroll 1
    for (uint32_t e = tid; e < T; e += kNttThreads) {
        const uint32_t i = a.ls ? e >> lc : e & (r - 1), tt = a.ls ? e & (c - 1) : e >> a.b;
        const uint32_t j = __brev(i) >> (32 - a.b), pos = (j << lc) + tt;
        const Fr x = ntt_get(sh, pos & ~c), y = ntt_get(sh, pos | c);
        Fr v = (j & 1) ? fr_sub(x, y) : fr_add(x, y);
        const uint64_t t = t0 + tt, p = t >> a.ls;
        const uint64_t o = (t & smask) + ((((p << a.b) + i)) << a.ls);
        Fr f = a.fc;
        bool mul = a.post == 1;
        if (!a.last) {
            uint64_t ex = (p * i) << a.ls;                 // < N
            if (a.inverse) ex = (N - ex) & (N - 1);
            f = pow_at(a.w, ex);
            mul = true;
        } else if (a.post == 2) {
            f = pow_at(a.f, o);
            mul = true;
        }
        if (mul) v = mont_mul(v, f);
        st_fr(out + o, v);
    }
}

hipError_t launch_ntt_pass(const NttPass& a, hipStream_t st) {
    if (!a.ncols) return hipSuccess;
    const uint32_t lt = a.k < kNttLogTile ? a.k : kNttLogTile;
    if ((!a.cols && !a.src) || !a.dst || !a.tw || a.k < 1 || a.k > 28 || a.kin < 1 || a.kin > a.k || a.b < 1 ||
        a.b > lt || a.ls + a.b > a.k || a.ncols > 65535 || (!a.last && pow_table_bad(a.w, a.k)) ||
        ((a.pre || a.post == 2) && pow_table_bad(a.f, a.kin)) || a.post > 2 || (a.last && a.ls + a.b != a.k))
        return hipErrorInvalidValue;
    const dim3 g((unsigned)(1u << (a.k - lt)), a.ncols), b(kNttThreads);
    hipLaunchKernelGGL(k_ntt_pass, g, b, 0, st, a);
    return hipGetLastError();
}

// --------------------------------------------------------------- evaluation
// Thread `tid` of block bx takes the coefficients base + 256 i, base = bx 256
// run + tid, i < run (coalesced over the block): x^base times Horner in x^256.
__global__ __launch_bounds__(kNttThreads) void k_ntt_eval(const Fr* const* __restrict__ cols,
                                                          const Fr* __restrict__ src, uint64_t n, uint32_t run,
                                                          uint32_t nbits, const Fr* __restrict__ pts, const Fr one,
                                                          Fr* __restrict__ part) {
    __shared__ Fr ws[kGpWaves];
    const uint32_t col = blockIdx.z, q = blockIdx.y;
    const Fr* __restrict__ cf = cols ? cols[col] : src + (uint64_t)col * n;
    const Fr x = ld_fr(pts + q);
    Fr xs = x;
#pragma unroll 1
    for (int i = 0; i < 8; ++i) xs = mont_mul(xs, xs);     // x^256 R
    const uint64_t base = (uint64_t)blockIdx.x * kNttThreads * run + threadIdx.x;
    Fr acc = fr_zero();
#pragma unroll 1
    for (uint32_t i = run; i-- > 0;) {
        const uint64_t idx = base + (uint64_t)kNttThreads * i;
        acc = mont_mul(acc, xs);
        if (idx < n) acc = fr_add(acc, ld_fr(cf + idx));
    }
    Fr pw = one;                                           // x^base R
#pragma unroll 1
    for (uint32_t bit = nbits; bit-- > 0;) {
        pw = mont_mul(pw, pw);
        if ((base >> bit) & 1) pw = mont_mul(pw, x);
    }
    acc = mont_mul(acc, pw);
#pragma unroll 1
    for (unsigned m = 1; m < 64; m <<= 1) acc = fr_add(acc, lp_shfl_xor(acc, m));
    if ((threadIdx.x & 63u) == 0) ws[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        Fr s = ws[0];
#pragma unroll 1
        for (unsigned w = 1; w < kGpWaves; ++w) s = fr_add(s, ws[w]);
        st_fr(part + ((uint64_t)col * gridDim.y + q) * gridDim.x + blockIdx.x, s);
    }
}
__global__ __launch_bounds__(kNttThreads) void k_ntt_eval_sum(const Fr* __restrict__ part, uint32_t nblocks,
                                                              uint32_t npoints, uint64_t cells, uint64_t out_stride,
                                                              Fr* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * kNttThreads + threadIdx.x;
    if (i >= cells) return;
    const Fr* p = part + i * nblocks;
    Fr s = ld_fr(p);
#pragma unroll 1
    for (uint32_t b = 1; b < nblocks; ++b) s = fr_add(s, ld_fr(p + b));
    st_fr(out + (i / npoints) * out_stride + i % npoints, s);
}
__global__ __launch_bounds__(kNttThreads) void k_ntt_compare(const Fr* const* __restrict__ cols,
                                                             const Fr* __restrict__ src, uint32_t k,
                                                             uint32_t log_samples, uint64_t seed, uint64_t s0,
                                                             uint32_t nsamp, uint64_t cells,
                                                             const Fr* __restrict__ vals, unsigned long long* cnt) {
    __shared__ uint32_t bad;
    if (threadIdx.x == 0) bad = 0;
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * kNttThreads + threadIdx.x;
    if (i < cells) {
        const uint32_t col = (uint32_t)(i / nsamp);
        const uint64_t row = ntt_sample_row(k, log_samples, seed, s0 + i % nsamp);
        const Fr* cf = cols ? cols[col] : src + ((uint64_t)col << k);
        if (!fr_eq(ld_fr(cf + row), ld_fr(vals + i))) atomicAdd(&bad, 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint64_t first = (uint64_t)blockIdx.x * kNttThreads;
        const uint64_t here = cells - first < kNttThreads ? cells - first : kNttThreads;
        atomicAdd(cnt, (unsigned long long)here);
        if (bad) atomicAdd(cnt + 1, (unsigned long long)bad);
    }
}

static uint32_t ntt_bits(uint64_t n) {                     // bits of n - 1
    uint32_t b = 0;
    while (b < 63 && (1ull << b) < n) ++b;
    return b;
}
hipError_t launch_ntt_eval(const Fr* const* cols, const Fr* src, uint64_t n, uint32_t ncols, const Fr* pts,
                           uint32_t npoints, Fr* part, hipStream_t st) {
    if (!ncols || !npoints) return hipSuccess;
    if ((!cols && !src) || !n || n > (1ull << 28) || ncols > 65535 || npoints > 65535 || !pts || !part)
        return hipErrorInvalidValue;
    const dim3 g(ntt_eval_blocks(n), npoints, ncols), b(kNttThreads);
    hipLaunchKernelGGL(k_ntt_eval, g, b, 0, st, cols, src, n, ntt_eval_run(n), ntt_bits(n), pts,
                       fr_one_mont(), part);
    return hipGetLastError();
}
hipError_t launch_ntt_eval_sum(const Fr* part, uint32_t nblocks, uint32_t ncols, uint32_t npoints, uint64_t out_stride,
                               Fr* out, hipStream_t st) {
    if (!ncols || !npoints) return hipSuccess;
    if (!part || !nblocks || !out || out_stride < npoints) return hipErrorInvalidValue;
    const uint64_t cells = (uint64_t)ncols * npoints;
    hipLaunchKernelGGL(k_ntt_eval_sum, dim3((unsigned)((cells + kNttThreads - 1) / kNttThreads)), dim3(kNttThreads), 0,
                       st, part, nblocks, npoints, cells, out_stride, out);
    return hipGetLastError();
}
hipError_t launch_ntt_compare(const Fr* const* cols, const Fr* src, uint32_t k, uint32_t log_samples, uint64_t seed,
                              uint64_t s0, uint32_t nsamp, uint32_t ncols, const Fr* vals, unsigned long long* cnt,
                              hipStream_t st) {
    if (!ncols || !nsamp) return hipSuccess;
    if ((!cols && !src) || k < 1 || k > 28 || log_samples > k || s0 + nsamp > (1ull << log_samples) || !vals || !cnt)
        return hipErrorInvalidValue;
    const uint64_t cells = (uint64_t)ncols * nsamp;
    hipLaunchKernelGGL(k_ntt_compare, dim3((unsigned)((cells + kNttThreads - 1) / kNttThreads)), dim3(kNttThreads), 0,
                       st, cols, src, k, log_samples, seed, s0, nsamp, cells, vals, cnt);
    return hipGetLastError();
}

}  // namespace svdw
