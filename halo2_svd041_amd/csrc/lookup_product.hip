// gfx950 kernels of the lookup argument's grand product (lookup_product.hpp):
// the leaf and the carry kernel; the passes are grand_product.hpp's. One column
// per blockIdx.y.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "export.hpp"
#include "grand_product.hpp"
#include "lookup_product.hpp"

namespace svdw {

template <int FORM>
__device__ __forceinline__ Fr lp_one(const LpChal& ch) {       // 1 in the form of Z
    return FORM == kFormMontgomery ? ch.one : fr_from_u64(1);
}
// The leaf. The factors of row r < usable of column c (A1, S1: the column's A',
// S'): n = (A + beta)(T + gamma), d = (A' + beta)(S' + gamma), each one mont_mul
// of the sums as the form hands them over. Canonical cells: both come out times
// 2^-256. Montgomery cells: d comes out in Montgomery form, and n too, as the
// canonical A + beta meets (T + gamma) 2^512 (T 2^512 is one CIOS round of the
// row index). No cursor: nothing follows the row.
template <int FORM>
struct LpLeaf {
    LpArgs a;
    struct Cursor {};

    __device__ __forceinline__ uint64_t rows() const { return a.rows; }
    __device__ __forceinline__ uint64_t usable() const { return a.usable; }
    __device__ __forceinline__ Fr one() const { return a.ch.one; }
    __device__ __forceinline__ Cursor cursor(uint64_t) const { return {}; }
    __device__ __forceinline__ void advance(Cursor&) const {}
    __device__ __forceinline__ void factors(uint32_t c, uint64_t r, const Cursor&, Fr& n, Fr& d) const {
        const LkSrc& s = a.src;
        const LpChal& ch = a.ch;
        const Fr* A1 = a.pin + (uint64_t)c * a.rows;
        const Fr* S1 = a.ptab + (uint64_t)c * a.rows;
        const uint64_t i = (uint64_t)c * s.stride + r;
        const Fr v = (r >= s.span || i >= s.total) ? fr_zero() : ld_fr(s.p + i);   // a row past the assigned ones
        Fr t = fr_zero();
        t.w[0] = (r >> a.lb) ? 0u : (uint32_t)r;
        if (FORM == kFormMontgomery) t = fr_add(mont_mul_rounds<1>(t, ch.t2), ch.g2);
        else t = fr_add(t, ch.g0);
        n = mont_mul(fr_add(v, ch.b0), t);
        d = mont_mul(fr_add(ld_fr(A1 + r), ch.bx), fr_add(ld_fr(S1 + r), ch.gx));
    }
    __device__ __forceinline__ Fr zone() const { return lp_one<FORM>(a.ch); }
    __device__ __forceinline__ Fr first(uint32_t, const Fr*) const { return zone(); }
    __device__ __forceinline__ bool closes(uint32_t) const { return true; }
};

// -------------------------------------------------------------------- carry
// One block per column: the runs' products, the block scan, then the fold with
// K = the inverse of the column's product of D, times 2^256 (canonical Z) or
// 2^512 (Montgomery Z): the power that the product itself carries cancels,
// whatever it is. Z[usable] = K * the product of all N.
template <int FORM>
__global__ __launch_bounds__(kGpThreads) void k_lp_carry(Fr* __restrict__ tp, const LpChal ch, uint64_t nt,
                                                         unsigned long long* cnt) {
    __shared__ Fr kc;
    Fr* col = tp + (uint64_t)blockIdx.x * nt * 2;
    uint64_t lo, hi;
    gp_run(nt, lo, hi);
    Fr pn, pd, xn, xd, tn, td;
    gp_run_products(col, lo, hi, ch.one, pn, pd);
    lp_block_scan<true>(ch.one, pn, pd, ch.one, ch.one, xn, xd, tn, td);
    if (threadIdx.x == 0) {
        Fr k = fr_to_mont(fr_inv(td));                     // td != 0: no factor of it is zero
        if (FORM == kFormMontgomery) k = fr_to_mont(k);
        kc = k;
        if (!fr_eq(mont_mul(tn, k), lp_one<FORM>(ch))) atomicAdd(cnt + 1, 1ull);
    }
    __syncthreads();
    gp_fold(col, lo, hi, mont_mul(xn, kc), xd);
}


// ----------------------------------------------------------------- launches
static bool lp_bad(const LpArgs& a, int form) {
    return !a.pin || !a.ptab || (a.src.total && !a.src.p) || a.lb < 1 || a.lb > 31 || a.ncols > 65535 ||
           a.usable >= a.rows || a.rows > (1ull << 31) || (form != kFormCanonical && form != kFormMontgomery);
}
// launch(f), f an integral constant of the (valid) form: the kernels' FORM.
template <class F>
static hipError_t lp_in_form(int form, F&& launch) {
    if (form == kFormMontgomery) launch(std::integral_constant<int, kFormMontgomery>{});
    else launch(std::integral_constant<int, kFormCanonical>{});
    return hipGetLastError();
}
hipError_t launch_lp_tiles(const LpArgs& a, int form, Fr* tp, unsigned long long* cnt, hipStream_t st) {
    if (!a.ncols) return hipSuccess;
    if (lp_bad(a, form) || !tp || !cnt) return hipErrorInvalidValue;
    const uint64_t nt = gp_tiles(a.rows);
    const dim3 g((unsigned)((nt + kGpWaves - 1) / kGpWaves), a.ncols), b(kGpThreads);
    return lp_in_form(form, [&](auto f) {
        using Leaf = LpLeaf<decltype(f)::value>;
        hipLaunchKernelGGL(k_gp_tiles<Leaf>, g, b, 0, st, Leaf{a}, nt, tp, cnt);
    });
}
hipError_t launch_lp_carry(const LpArgs& a, int form, Fr* tp, unsigned long long* cnt, hipStream_t st) {
    if (!a.ncols) return hipSuccess;
    if (lp_bad(a, form) || !tp || !cnt) return hipErrorInvalidValue;
    return lp_in_form(form, [&](auto f) {
        hipLaunchKernelGGL(k_lp_carry<decltype(f)::value>, dim3(a.ncols), dim3(kGpThreads), 0, st, tp, a.ch,
                           gp_tiles(a.rows), cnt);
    });
}
hipError_t launch_lp_write(const LpArgs& a, int form, const Fr* tp, Fr* z, hipStream_t st) {
    if (!a.ncols) return hipSuccess;
    if (lp_bad(a, form) || !tp || !z) return hipErrorInvalidValue;
    const dim3 g((unsigned)gp_tiles(a.rows), a.ncols), b(kGpThreads);
    return lp_in_form(form, [&](auto f) {
        using Leaf = LpLeaf<decltype(f)::value>;
        hipLaunchKernelGGL(k_gp_write<Leaf>, g, b, 0, st, Leaf{a}, tp, z);
    });
}
hipError_t launch_lp_check(const LpArgs& a, int form, const Fr* z, unsigned long long* cnt, hipStream_t st) {
    if (!a.ncols) return hipSuccess;
    if (lp_bad(a, form) || !z || !cnt) return hipErrorInvalidValue;
    const dim3 g(gp_check_blocks(a.rows), a.ncols), b(kGpThreads);
    return lp_in_form(form, [&](auto f) {
        using Leaf = LpLeaf<decltype(f)::value>;
        hipLaunchKernelGGL(k_gp_check<Leaf>, g, b, 0, st, Leaf{a}, z, cnt);
    });
}

}  // namespace svdw
