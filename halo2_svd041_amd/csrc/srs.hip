// Kernels of srs.hpp: the table of a fixed base, the fixed-base multiplication
// with one inversion per thread and group of outputs, and the setup's two
// scalar columns.
#include "srs.hpp"

namespace svdw {
namespace {

// Thread w: P_w = [2^(c w)] base by c w doublings, into table[w B].
__global__ __launch_bounds__(128) void k_fb_windows(G1Affine base, int base_form, uint32_t c, uint32_t W,
                                                    G1Affine* table) {
    const uint32_t w = threadIdx.x;
    if (w >= W) return;
    G1Xyzz acc = g1_from_affine(g1_affine_to_mont(base, base_form));
    const uint32_t nd = c * w;
#pragma unroll 1
    for (uint32_t i = 0; i < nd; ++i) acc = g1_double(acc);
    table[(uint64_t)w << (c - 1)] = g1_to_affine(acc);
}

// Thread (w, d), 2 <= d <= B: table[w B + d - 1] = [d] table[w B].
__global__ __launch_bounds__(kCommitThreads) void k_fb_table(uint32_t c, uint32_t W, G1Affine* table) {
    const uint64_t e = (uint64_t)blockIdx.x * kCommitThreads + threadIdx.x;
    if (e >= ((uint64_t)W << (c - 1))) return;
    const uint32_t d = (uint32_t)(e & ((1ull << (c - 1)) - 1)) + 1;
    if (d == 1) return;                                    // k_fb_windows wrote it, and every other thread reads it
    const G1Affine p = table[e - (d - 1)];
    G1Xyzz acc = g1_identity();
#pragma unroll 1
    for (int bit = (int)c - 1; bit >= 0; --bit) {
        acc = g1_double(acc);
        if ((d >> bit) & 1) acc = g1_add_mixed(acc, p);
    }
    table[e] = g1_to_affine(acc);
}

__global__ __launch_bounds__(kFbThreads) void k_fb_mul(FbMul a) {
    const uint64_t first = (uint64_t)blockIdx.x * (kFbThreads * kFbGroup) + threadIdx.x;
    Fq run = fq_one();
#pragma unroll 1
    for (uint32_t g = 0; g < kFbGroup; ++g) {
        const uint64_t i = first + (uint64_t)g * kFbThreads;
        if (i >= a.n) break;
        Fr s = a.scalars[i];
        if (a.form != 0) s = fr_from_mont(s);
        if (fr_is_zero(s)) atomicAdd(&a.cnt[i >= a.split ? 2 : 0], 1ull);
        G1Xyzz acc = g1_identity();
        g1_signed_digits(s, a.c, a.W, [&](uint32_t w, uint32_t mag, uint32_t neg) {
            if (!mag) return;                              // a zero digit adds nothing
            G1Affine p = a.table[((uint64_t)w << (a.c - 1)) + (mag - 1)];
            if (neg) p.y = fq_neg(p.y);
            acc = g1_add_mixed(acc, p);
        });
        a.acc[i] = acc;
        a.pre[i] = run;
        if (!g1_is_identity(acc)) run = fq_mul(run, acc.zzz);
    }
    Fq inv = fq_inv(run);                                  // run != 0: a product of non-zero ZZZ
#pragma unroll 1
    for (uint32_t g = kFbGroup; g-- > 0;) {
        const uint64_t i = first + (uint64_t)g * kFbThreads;
        if (i >= a.n) continue;
        const G1Xyzz acc = a.acc[i];
        const bool second = i >= a.split;                  // the call's second array
        G1Affine r;
        if (g1_is_identity(acc)) {
            atomicAdd(&a.cnt[second ? 3 : 1], 1ull);
            r.x = r.y = fq_zero();
        } else {
            r = g1_affine_shared_inv(acc, a.pre[i], inv, a.base_form);
        }
        if (second) a.out2[i - a.split] = r;
        else a.out[i] = r;
    }
}

__global__ __launch_bounds__(kCommitThreads) void k_srs_powers(PowTable pw, uint64_t i0, uint64_t m, Fr* out) {
    const uint64_t j = (uint64_t)blockIdx.x * kCommitThreads + threadIdx.x;
    if (j >= m) return;
    st_fr(out + j, pow_at(pw, i0 + j));
}

__global__ __launch_bounds__(kSrsThreads) void k_srs_lagrange(PowTable dom, Fr sR, Fr coef, int in_domain, uint64_t i0,
                                                              uint64_t m, Fr* out) {
    const uint64_t first = (uint64_t)blockIdx.x * (kSrsThreads * kSrsInvGroup) + threadIdx.x;
    if (in_domain) {                                       // l_i(omega^j) = [i == j]
#pragma unroll 1
        for (uint32_t g = 0; g < kSrsInvGroup; ++g) {
            const uint64_t j = first + (uint64_t)g * kSrsThreads;
            if (j >= m) break;
            st_fr(out + j, fr_eq(pow_at(dom, i0 + j), sR) ? fr_one_mont() : fr_zero());
        }
        return;
    }
    Fr run = fr_one_mont();
#pragma unroll 1
    for (uint32_t g = 0; g < kSrsInvGroup; ++g) {
        const uint64_t j = first + (uint64_t)g * kSrsThreads;
        if (j >= m) break;
        st_fr(out + j, run);                               // the prefix waits in the output cell
        run = mont_mul(run, fr_sub(sR, pow_at(dom, i0 + j)));
    }
    Fr inv = fr_to_mont(fr_inv(fr_from_mont(run)));        // no s - omega^i is zero here
#pragma unroll 1
    for (uint32_t g = kSrsInvGroup; g-- > 0;) {
        const uint64_t j = first + (uint64_t)g * kSrsThreads;
        if (j >= m) continue;
        const Fr w = pow_at(dom, i0 + j), den = fr_sub(sR, w);
        const Fr dinv = mont_mul(inv, ld_fr(out + j));
        inv = mont_mul(inv, den);
        st_fr(out + j, mont_mul(mont_mul(coef, w), dinv));
    }
}

}  // namespace

hipError_t launch_fb_table(G1Affine base, int base_form, uint32_t c, G1Affine* table, hipStream_t st) {
    const uint32_t W = fb_windows(c);
    hipLaunchKernelGGL(k_fb_windows, dim3(1), dim3(128), 0, st, base, base_form, c, W, table);
    hipLaunchKernelGGL(k_fb_table, dim3(blocks_of(fb_table_points(c), kCommitThreads)), dim3(kCommitThreads), 0, st, c,
                       W, table);
    return hipGetLastError();
}

hipError_t launch_fb_mul(const FbMul& a, hipStream_t st) {
    if (!a.n) return hipSuccess;
    hipLaunchKernelGGL(k_fb_mul, dim3(blocks_of(a.n, (uint64_t)kFbThreads * kFbGroup)), dim3(kFbThreads), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_srs_powers(PowTable pw, uint64_t i0, uint64_t m, Fr* out, hipStream_t st) {
    if (!m) return hipSuccess;
    hipLaunchKernelGGL(k_srs_powers, dim3(blocks_of(m, kCommitThreads)), dim3(kCommitThreads), 0, st, pw, i0, m, out);
    return hipGetLastError();
}

hipError_t launch_srs_lagrange(PowTable dom, Fr sR, Fr coef, bool in_domain, uint64_t i0, uint64_t m, Fr* out,
                               hipStream_t st) {
    if (!m) return hipSuccess;
    hipLaunchKernelGGL(k_srs_lagrange, dim3(blocks_of(m, (uint64_t)kSrsThreads * kSrsInvGroup)), dim3(kSrsThreads), 0,
                       st, dom, sR, coef, in_domain ? 1 : 0, i0, m, out);
    return hipGetLastError();
}

}  // namespace svdw
