// gfx950 kernels of the quotient polynomial (quotient.hpp): k_quotient, one
// extended row per thread, and the two small kernels around it (the Lagrange
// columns of l_0, l_last, l_active; the count of h's tail coefficients).
#include <hip/hip_runtime.h>

#include "export.hpp"
#include "quotient.hpp"

namespace svdw {

// A cell-derived value as a multiplier: x phi -> x R.
template <bool MONT>
__device__ __forceinline__ Fr q_up(const Fr& v) {
    if (MONT) return v;
    return mont_mul(v, fr_r2());
}
__device__ __forceinline__ Fr q_fold(const Fr& h, const Fr& y, const Fr& e) { return fr_add(mont_mul(h, y), e); }

template <bool MONT>
__global__ __launch_bounds__(kQuotientThreads) void k_quotient(const QuotientArgs a) {
    const uint64_t N = 1ull << a.ek, mask = N - 1;
    const uint64_t j = (uint64_t)blockIdx.x * kQuotientThreads + threadIdx.x;
    if (j >= N) return;
    const uint64_t r1 = (j + (1ull << a.le)) & mask;       // omega X
    Fr h = fr_zero();

    // 1. gates: q (a(X) + a(omega X) a(omega^2 X) - a(omega^3 X))
    {
        const uint64_t r2 = (j + (2ull << a.le)) & mask, r3 = (j + (3ull << a.le)) & mask;
#pragma unroll 1
        for (uint32_t i = 0; i < a.ng; ++i) {
            const Fr* __restrict__ c = a.ptrs[i];
            const Fr t = mont_mul(q_up<MONT>(ld_fr(c + r1)), ld_fr(c + r2));
            const Fr s = fr_sub(fr_add(ld_fr(c + j), t), ld_fr(c + r3));
            h = q_fold(h, a.y, mont_mul(q_up<MONT>(ld_fr(a.ptrs[a.ng + i] + j)), s));
        }
    }
    if (a.np | a.nl) {
        const Fr l0 = ld_fr(a.l0 + j), ll = ld_fr(a.llast + j), la = ld_fr(a.lact + j);

        // 2. permutation
        if (a.np) {
            const Fr* const* __restrict__ v = a.ptrs + 2 * (size_t)a.ng;
            const Fr* const* __restrict__ sig = v + a.np;
            const Fr* const* __restrict__ pz = sig + a.np;
            const uint64_t ru = (j + (a.usable << a.le)) & mask;   // omega^usable X
            // X_j R = omega_e^j shift R
            const Fr xs = mont_mul(pow_at(a.w, j), a.shift);
            h = q_fold(h, a.y, mont_mul(l0, fr_sub(a.one, ld_fr(pz[0] + j))));
            {
                const Fr z = ld_fr(pz[a.nsets - 1] + j);
                h = q_fold(h, a.y, mont_mul(ll, mont_mul(q_up<MONT>(z), fr_sub(z, a.one))));
            }
#pragma unroll 1
            for (uint32_t s = 1; s < a.nsets; ++s)
                h = q_fold(h, a.y, mont_mul(l0, fr_sub(ld_fr(pz[s] + j), ld_fr(pz[s - 1] + ru))));
#pragma unroll 1
            for (uint32_t s = 0; s < a.nsets; ++s) {
                const uint32_t c0 = s * a.chunk, c1 = a.np - c0 < a.chunk ? a.np : c0 + a.chunk;
                Fr left = ld_fr(pz[s] + r1), right = ld_fr(pz[s] + j);
#pragma unroll 1
                for (uint32_t c = c0; c < c1; ++c) {
                    const Fr vg = fr_add(ld_fr(v[c] + j), a.gamma);
                    const Fr sg = mont_mul(ld_fr(sig[c] + j), a.beta);
                    const Fr id = mont_mul(xs, ld_fr(a.bd + c));
                    left = mont_mul(q_up<MONT>(fr_add(vg, sg)), left);
                    right = mont_mul(q_up<MONT>(fr_add(vg, id)), right);
                }
                h = q_fold(h, a.y, mont_mul(la, fr_sub(left, right)));
            }
        }

        // 3. lookups
        {
            const Fr* const* __restrict__ lk = a.ptrs + 2 * (size_t)a.ng + 2 * (size_t)a.np + a.nsets;
            const uint64_t rm = (j + N - (1ull << a.le)) & mask;   // omega^-1 X
#pragma unroll 1
            for (uint32_t i = 0; i < a.nl; ++i) {
                const Fr z = ld_fr(lk[4 * (size_t)a.nl + i] + j);
                const Fr ap = ld_fr(lk[2 * (size_t)a.nl + i] + j), sp = ld_fr(lk[3 * (size_t)a.nl + i] + j);
                h = q_fold(h, a.y, mont_mul(l0, fr_sub(a.one, z)));
                h = q_fold(h, a.y, mont_mul(ll, mont_mul(q_up<MONT>(z), fr_sub(z, a.one))));
                {
                    Fr left = mont_mul(q_up<MONT>(fr_add(ap, a.betaf)), fr_add(sp, a.gamma));
                    left = mont_mul(q_up<MONT>(ld_fr(lk[4 * (size_t)a.nl + i] + r1)), left);
                    Fr right = mont_mul(q_up<MONT>(fr_add(ld_fr(lk[i] + j), a.betaf)),
                                        fr_add(ld_fr(lk[(size_t)a.nl + i] + j), a.gamma));
                    right = mont_mul(q_up<MONT>(z), right);
                    h = q_fold(h, a.y, mont_mul(la, fr_sub(left, right)));
                }
                const Fr d = fr_sub(ap, sp);
                h = q_fold(h, a.y, mont_mul(l0, d));
                const Fr dd = mont_mul(q_up<MONT>(d), fr_sub(ap, ld_fr(lk[2 * (size_t)a.nl + i] + rm)));
                h = q_fold(h, a.y, mont_mul(la, dd));
            }
        }
    }
    st_fr(a.out + j, mont_mul(h, ld_fr(a.inv + (j & ((1ull << a.le) - 1)))));
}

hipError_t launch_quotient(const QuotientArgs& a, int form, hipStream_t st) {
    if (!a.ng && !a.np && !a.nl) return hipSuccess;
    if (!a.ptrs || !a.inv || !a.out || a.ek < 1 || a.ek > 28 || a.le > a.ek || a.ng > 65535 || a.np > 65535 ||
        a.nl > 65535 || (a.np && (!a.chunk || !a.bd || pow_table_bad(a.w, a.ek) ||
                                  a.nsets != (a.np + a.chunk - 1) / a.chunk)) ||
        (!a.np && a.nsets) || ((a.np | a.nl) && (!a.l0 || !a.llast || !a.lact)) ||
        a.usable >= (1ull << (a.ek - a.le)) || (form != kFormCanonical && form != kFormMontgomery))
        return hipErrorInvalidValue;
    const dim3 g((unsigned)(((1ull << a.ek) + kQuotientThreads - 1) / kQuotientThreads)), b(kQuotientThreads);
    if (form == kFormMontgomery)
        hipLaunchKernelGGL(k_quotient<true>, g, b, 0, st, a);
    else
        hipLaunchKernelGGL(k_quotient<false>, g, b, 0, st, a);
    return hipGetLastError();
}

__global__ __launch_bounds__(kQuotientThreads) void k_quotient_basis(Fr* __restrict__ out, uint64_t n, uint64_t usable,
                                                                     const Fr one) {
    const uint64_t i = (uint64_t)blockIdx.x * kQuotientThreads + threadIdx.x;
    if (i >= 3 * n) return;
    const uint64_t col = i / n, r = i % n;
    const bool on = col == 0 ? r == 0 : col == 1 ? r == usable : r < usable;
    st_fr(out + i, on ? one : fr_zero());
}
hipError_t launch_quotient_basis(Fr* out, uint64_t n, uint64_t usable, const Fr& one, hipStream_t st) {
    if (!out || !n || n > (1ull << 28) || usable >= n) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_quotient_basis, dim3((unsigned)((3 * n + kQuotientThreads - 1) / kQuotientThreads)),
                       dim3(kQuotientThreads), 0, st, out, n, usable, one);
    return hipGetLastError();
}

__global__ __launch_bounds__(kQuotientThreads) void k_quotient_tail(const Fr* __restrict__ h, uint64_t from, uint64_t N,
                                                                    unsigned long long* cnt) {
    __shared__ uint32_t bad;
    if (threadIdx.x == 0) bad = 0;
    __syncthreads();
    const uint64_t step = (uint64_t)gridDim.x * kQuotientThreads;
    uint32_t nb = 0;
#pragma unroll 1
    for (uint64_t i = from + (uint64_t)blockIdx.x * kQuotientThreads + threadIdx.x; i < N; i += step)
        nb += !fr_is_zero(ld_fr(h + i));
    if (nb) atomicAdd(&bad, nb);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (blockIdx.x == 0) atomicAdd(cnt, (unsigned long long)(N - from));
        if (bad) atomicAdd(cnt + 1, (unsigned long long)bad);
    }
}
hipError_t launch_quotient_tail(const Fr* h, uint64_t from, uint64_t N, unsigned long long* cnt, hipStream_t st) {
    if (!h || !cnt || from > N || N > (1ull << 28)) return hipErrorInvalidValue;
    if (from == N) return hipSuccess;
    const uint64_t nb = (N - from + kQuotientThreads - 1) / kQuotientThreads;
    hipLaunchKernelGGL(k_quotient_tail, dim3((unsigned)(nb < 4096 ? nb : 4096)), dim3(kQuotientThreads), 0, st, h, from,
                       N, cnt);
    return hipGetLastError();
}

}  // namespace svdw
