// gfx950 kernels of the permutation argument's grand products
// (permutation_product.hpp): the leaf, the three kernels of the carry stage and
// k_pp_values; the passes are grand_product.hpp's. One set per blockIdx.y. The
// column base pointers and beta delta^j come from device tables at a uniform
// index. With m the columns of a set, multiplications per row of the set (per
// cell: divide by m):
//
//   leaf (PpLeaf)       4 m + 1     per column beta sigma, beta delta^j omega^r,
//                                   the two running products; omega^r once
//   k_pp_tiles          4 m + 3.75  the leaf, into the lane's two products, 12 / 16
//                                   for the butterfly
//   k_pp_write          4 m + 9.5   the leaf, the thread's prefix and suffix, two
//                                   for the row's Z, 18 / kGpItems for the block
//                                   scan
//   k_pp_check          4 m + 4     the leaf, both sides, the omega step
//   k_pp_values         2 per cell
#include <hip/hip_runtime.h>

#include "export.hpp"
#include "grand_product.hpp"
#include "permutation_product.hpp"

namespace svdw {

// The leaf. The cursor is w = omega^r R, from the table.
struct PpLeaf {
    PpArgs a;
    struct Cursor {
        Fr w;
    };

    __device__ __forceinline__ uint64_t rows() const { return a.rows; }
    __device__ __forceinline__ uint64_t usable() const { return a.usable; }
    __device__ __forceinline__ Fr one() const { return a.one; }
    __device__ __forceinline__ Cursor cursor(uint64_t r) const { return {pow_at(a.w, r)}; }
    // The factors of row r < usable of set s, the columns [j0, j1). j counts over
    // all columns: the identity term of column j is delta^j omega^r.
    __device__ __forceinline__ void factors(uint32_t s, uint64_t r, const Cursor& c, Fr& n, Fr& d) const {
        const uint32_t j0 = s * a.chunk, j1 = a.ncols - j0 < a.chunk ? a.ncols : j0 + a.chunk;
        n = d = a.one;
#pragma unroll 1
        for (uint32_t j = j0; j < j1; ++j) {
            const Fr v = fr_add(ld_fr(a.cols[j] + r), a.g);
            const Fr sg = mont_mul(ld_fr(a.sig[j] + r), a.bR);
            const Fr id = mont_mul(c.w, ld_fr(a.bd + j));
            n = mont_mul(n, fr_add(v, id));
            d = mont_mul(d, fr_add(v, sg));
        }
    }
};
// What k_gp_check asks for besides: Z_0[0] == 1, Z_s[0] == Z_{s-1}[usable], the
// last Z[usable] in {0, 1}. The cursor comes from the table for the thread's
// first row, then steps by wstep = omega^(the grid's stride) R; only the table
// itself is shared with the passes above.
struct PpCheckLeaf : PpLeaf {
    Fr z1, wstep;                                          // z1: 1 in the form of Z

    __device__ __forceinline__ void advance(Cursor& c) const { c.w = mont_mul(c.w, wstep); }
    __device__ __forceinline__ Fr zone() const { return z1; }
    __device__ __forceinline__ Fr first(uint32_t s, const Fr* Z) const {
        return s ? ld_fr(Z - a.rows + a.usable) : z1;
    }
    __device__ __forceinline__ bool closes(uint32_t s) const { return s + 1 == a.nsets; }
};

// -------------------------------------------------------------------- carry
// One block per set over its nt tile products: the runs' products and the
// block scan give xs[(s * threads + thread) * 2 + {0, 1}] = the products of N
// of the runs below, of D of the runs above. sv[2 s] = (the set's product of N)
// / (its product of D) * R, the factor from start_s to start_{s+1}; sv[2 s + 1]
// = the inverse of the product of D, times R (canonical Z) or R^2 (Montgomery
// Z): the power that the product itself carries cancels, whatever it is.
__global__ __launch_bounds__(kGpThreads) void k_pp_totals(const Fr* __restrict__ tp, const Fr one, int mont,
                                                          uint64_t nt, Fr* __restrict__ xs, Fr* __restrict__ sv) {
    const uint32_t s = blockIdx.x;
    uint64_t lo, hi;
    gp_run(nt, lo, hi);
    Fr pn, pd, xn, xd, tn, td;
    gp_run_products(tp + (uint64_t)s * nt * 2, lo, hi, one, pn, pd);
    lp_block_scan<true>(one, pn, pd, one, one, xn, xd, tn, td);
    Fr* x = xs + ((uint64_t)s * kGpThreads + threadIdx.x) * 2;
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
// One block per set: the fold with K = the set's inverse times its start.
__global__ __launch_bounds__(kGpThreads) void k_pp_fold(Fr* __restrict__ tp, const Fr* __restrict__ xs,
                                                        const Fr* __restrict__ sv, uint64_t nt) {
    const uint32_t s = blockIdx.x;
    uint64_t lo, hi;
    gp_run(nt, lo, hi);
    const Fr* x = xs + ((uint64_t)s * kGpThreads + threadIdx.x) * 2;
    gp_fold(tp + (uint64_t)s * nt * 2, lo, hi, mont_mul(ld_fr(x), ld_fr(sv + 2 * (uint64_t)s + 1)), ld_fr(x + 1));
}

// ------------------------------------------------------------------- values
__global__ __launch_bounds__(kGpThreads) void k_pp_values(const uint64_t* __restrict__ mapping,
                                                          const Fr* __restrict__ dl, const PowTable w,
                                                          uint32_t first_col, uint32_t total_cols, uint64_t rows,
                                                          uint64_t cells, Fr* __restrict__ out,
                                                          unsigned long long* cnt) {
    __shared__ uint32_t bad;
    if (threadIdx.x == 0) bad = 0;
    __syncthreads();
    const uint64_t step = (uint64_t)gridDim.x * kGpThreads;
    uint32_t nb = 0;
#pragma unroll 1
    for (uint64_t i = (uint64_t)blockIdx.x * kGpThreads + threadIdx.x; i < cells; i += step) {
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
        if (col < total_cols && row < rows) v = mont_mul(pow_at(w, row), ld_fr(dl + col));
        else ++nb;
        st_fr(out + i, v);
    }
    if (nb) atomicAdd(&bad, nb);
    __syncthreads();
    if (threadIdx.x == 0 && bad) atomicAdd(cnt, (unsigned long long)bad);
}

// ----------------------------------------------------------------- launches
static bool pp_bad(const PpArgs& a, int form) {
    return !a.cols || !a.sig || !a.bd || !a.ncols || !a.chunk || a.ncols > 65535 ||
           a.nsets != pp_sets(a.ncols, a.chunk) || a.usable >= a.rows || a.rows > (1ull << 31) ||
           (a.rows & (a.rows - 1)) || pow_table_bad(a.w, (uint32_t)__builtin_ctzll(a.rows)) ||
           (form != kFormCanonical && form != kFormMontgomery);
}

hipError_t launch_pp_tiles(const PpArgs& a, int form, Fr* tp, unsigned long long* cnt, hipStream_t st) {
    if (pp_bad(a, form) || !tp || !cnt) return hipErrorInvalidValue;
    const uint64_t nt = gp_tiles(a.rows);
    const dim3 g((unsigned)((nt + kGpWaves - 1) / kGpWaves), a.nsets), b(kGpThreads);
    hipLaunchKernelGGL(k_gp_tiles<PpLeaf>, g, b, 0, st, PpLeaf{a}, nt, tp, cnt);
    return hipGetLastError();
}
hipError_t launch_pp_totals(const PpArgs& a, int form, const Fr* tp, Fr* xs, Fr* sv, hipStream_t st) {
    if (pp_bad(a, form) || !tp || !xs || !sv) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pp_totals, dim3(a.nsets), dim3(kGpThreads), 0, st, tp, a.one,
                       (int)(form == kFormMontgomery), gp_tiles(a.rows), xs, sv);
    return hipGetLastError();
}
hipError_t launch_pp_chain(const PpArgs& a, Fr* sv, unsigned long long* cnt, hipStream_t st) {
    if (!a.nsets || !sv || !cnt) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pp_chain, dim3(1), dim3(64), 0, st, sv, a.one, a.nsets, cnt);
    return hipGetLastError();
}
hipError_t launch_pp_fold(const PpArgs& a, int form, Fr* tp, const Fr* xs, const Fr* sv, hipStream_t st) {
    if (pp_bad(a, form) || !tp || !xs || !sv) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pp_fold, dim3(a.nsets), dim3(kGpThreads), 0, st, tp, xs, sv, gp_tiles(a.rows));
    return hipGetLastError();
}
hipError_t launch_pp_write(const PpArgs& a, int form, const Fr* tp, Fr* z, hipStream_t st) {
    if (pp_bad(a, form) || !tp || !z) return hipErrorInvalidValue;
    const dim3 g((unsigned)gp_tiles(a.rows), a.nsets), b(kGpThreads);
    hipLaunchKernelGGL(k_gp_write<PpLeaf>, g, b, 0, st, PpLeaf{a}, tp, z);
    return hipGetLastError();
}
uint64_t pp_check_stride(uint64_t rows) { return (uint64_t)gp_check_blocks(rows) * kGpThreads; }
hipError_t launch_pp_check(const PpArgs& a, int form, const Fr* z, const Fr& wstep, unsigned long long* cnt,
                           hipStream_t st) {
    if (pp_bad(a, form) || !z || !cnt) return hipErrorInvalidValue;
    const dim3 g(gp_check_blocks(a.rows), a.nsets), b(kGpThreads);
    const PpCheckLeaf leaf{{a}, form == kFormMontgomery ? a.one : fr_from_u64(1), wstep};
    hipLaunchKernelGGL(k_gp_check<PpCheckLeaf>, g, b, 0, st, leaf, z, cnt);
    return hipGetLastError();
}
hipError_t launch_pp_values(const uint64_t* mapping, const Fr* dl, const PowTable& w, uint32_t first_col,
                            uint32_t ncols, uint32_t total_cols, uint64_t rows, Fr* out, unsigned long long* cnt,
                            hipStream_t st) {
    if (!ncols) return hipSuccess;
    if (!dl || !out || !cnt || !rows || (rows & (rows - 1)) || rows > (1ull << 31) ||
        pow_table_bad(w, (uint32_t)__builtin_ctzll(rows)) || ncols > 65535 || total_cols > 65535)
        return hipErrorInvalidValue;
    const uint64_t cells = (uint64_t)ncols * rows, nb = (cells + kGpThreads - 1) / kGpThreads;
    hipLaunchKernelGGL(k_pp_values, dim3((unsigned)(nb < 65536 ? nb : 65536)), dim3(kGpThreads), 0, st, mapping, dl,
                       w, first_col, total_cols, rows, cells, out, cnt);
    return hipGetLastError();
}

}  // namespace svdw
