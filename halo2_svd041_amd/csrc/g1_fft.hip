// Kernels of g1_fft.hpp: the table of a point's small multiples, the
// variable-base multiplication, a stage's butterflies, the affine output, and
// the first stage of the transform.
#include "g1_fft.hpp"

namespace svdw {
namespace {

// The point of item t: element idx of the affine input or of the working array.
__device__ __forceinline__ uint64_t g1_item_index(const G1Mul& a, uint64_t t) {
    return ((t >> a.shift) << (a.shift + 1)) + (t & ((1ull << a.shift) - 1)) + a.offset;
}
__device__ __forceinline__ G1Xyzz g1_item_point(const G1Mul& a, uint64_t idx) {
    if (!a.points) return a.work[idx];
    return g1_from_affine(g1_affine_to_mont(a.points[idx], a.bases_form));
}
// The exponent of item t's twiddle, before the inverse's sign.
__device__ __forceinline__ uint64_t g1_item_exponent(const G1Mul& a, uint64_t t) { return (t & a.tw_mask) << a.tw_shift; }
__device__ __forceinline__ bool g1_item_skipped(const G1Mul& a, uint64_t t) {
    return a.twiddle && a.skip_one && g1_item_exponent(a, t) == 0;
}
// The scalar of item t as a canonical integer.
__device__ __forceinline__ Fr g1_item_scalar(const G1Mul& a, uint64_t t) {
    if (!a.twiddle) {
        const Fr s = a.scalars[t];
        return a.form != 0 ? fr_from_mont(s) : s;
    }
    uint64_t e = g1_item_exponent(a, t);
    if (a.inverse && e) e = a.n - e;
    Fr w = pow_at(a.dom, e);
    if (a.has_factor) w = mont_mul(w, a.factor);
    return fr_from_mont(w);
}

__global__ __launch_bounds__(kG1Threads) void k_g1_table(G1Mul a) {
    const uint64_t i = (uint64_t)blockIdx.x * kG1Threads + threadIdx.x;
    if (i >= a.m) return;
    const uint64_t t = a.t0 + i;
    if (g1_item_skipped(a, t)) return;
    const G1Xyzz p = g1_item_point(a, g1_item_index(a, t));
    G1Xyzz* T = a.table + i;
    G1Xyzz cur = p;
    *T = p;
    const uint32_t B = 1u << (a.c - 1);
#pragma unroll 1
    for (uint32_t d = 1; d < B; ++d) {                     // the first add is the doubling
        cur = g1_add(cur, p);
        T += a.m;
        *T = cur;
    }
}

// [s] P for the point whose table column starts at T (stride m): the signed
// digits go to the lane's column of dig, every window written (|d| in the low
// bits, 0x80 the sign), then top window first, c doublings and one complete add
// per window.
__device__ __forceinline__ G1Xyzz g1_mul_walk(const G1Xyzz* T, uint64_t m, Fr s, uint32_t c, uint32_t W,
                                              uint8_t (*dig)[kG1Threads], uint32_t lane) {
    g1_signed_digits(s, c, W,
                     [&](uint32_t w, uint32_t mag, uint32_t neg) { dig[w][lane] = (uint8_t)(mag | neg << 7); });
    G1Xyzz acc = g1_identity();
#pragma unroll 1
    for (uint32_t w = W; w-- > 0;) {
#pragma unroll 1
        for (uint32_t j = 0; j < c; ++j) acc = g1_double(acc);
        const uint32_t d = dig[w][lane], mag = d & 0x7fu;
        if (mag) {
            G1Xyzz e = T[(uint64_t)(mag - 1) * m];
            if (d & 0x80u) e.y = fq_neg(e.y);
            acc = g1_add(acc, e);
        }
    }
    return acc;
}

__global__ __launch_bounds__(kG1Threads, 2) void k_g1_mul(G1Mul a) {
    __shared__ uint8_t dig[kG1MaxWindows][kG1Threads];
    const uint64_t i = (uint64_t)blockIdx.x * kG1Threads + threadIdx.x;
    if (i >= a.m) return;
    const uint64_t t = a.t0 + i, idx = g1_item_index(a, t);
    if (g1_item_skipped(a, t)) return;                     // the butterfly takes the point itself
    const Fr s = g1_item_scalar(a, t);
    if (!a.twiddle) {
        if (fr_is_zero(s)) atomicAdd(&a.cnt[0], 1ull);
        if (g1_affine_is_identity(a.points[idx])) atomicAdd(&a.cnt[1], 1ull);
    }
    atomicAdd(&a.cnt[3], 1ull);
    a.dst[a.dst_linear ? i : idx] = g1_mul_walk(a.table + i, a.m, s, a.c, a.W, dig, threadIdx.x);
}

// Butterfly t of a stage: (a + p, a - p) over the working array, p the product
// k_g1_mul left in dst, or b itself where the twiddle is 1.
__global__ __launch_bounds__(kG1Threads) void k_g1_butterfly(G1Mul a) {
    const uint64_t i = (uint64_t)blockIdx.x * kG1Threads + threadIdx.x;
    if (i >= a.m) return;
    const uint64_t t = a.t0 + i, idx = g1_item_index(a, t);
    G1Xyzz p = g1_item_skipped(a, t) ? a.work[idx] : a.dst[i];
    G1Xyzz* lo = a.work + (idx - a.offset);
    const G1Xyzz top = *lo;
#pragma unroll 1
    for (int r = 0; r < 2; ++r) {                          // a + p, then a - p
        *lo = g1_add(top, p);
        p.y = fq_neg(p.y);
        lo += a.offset;
    }
}

__global__ __launch_bounds__(kFbThreads) void k_g1_affine(const G1Xyzz* src, uint64_t n, int bases_form, G1Affine* out,
                                                          unsigned long long* cnt) {
    const uint64_t first = (uint64_t)blockIdx.x * (kFbThreads * kFbGroup) + threadIdx.x;
    Fq run = fq_one();
#pragma unroll 1
    for (uint32_t g = 0; g < kFbGroup; ++g) {
        const uint64_t i = first + (uint64_t)g * kFbThreads;
        if (i >= n) break;
        out[i].x = run;                                    // the prefix waits in the output point
        if (!fq_is_zero(src[i].zz)) run = fq_mul(run, src[i].zzz);
    }
    Fq inv = fq_inv(run);                                  // run != 0: a product of non-zero ZZZ
#pragma unroll 1
    for (uint32_t g = kFbGroup; g-- > 0;) {
        const uint64_t i = first + (uint64_t)g * kFbThreads;
        if (i >= n) continue;
        const G1Xyzz acc = src[i];
        G1Affine r;
        if (g1_is_identity(acc)) {
            atomicAdd(&cnt[2], 1ull);
            r.x = r.y = fq_zero();
        } else {
            r = g1_affine_shared_inv(acc, out[i].x, inv, bases_form);
        }
        out[i] = r;
    }
}

__global__ __launch_bounds__(kCommitThreads) void k_g1_fft_first(const G1Affine* in, uint32_t k, int bases_form,
                                                                 G1Xyzz* work, unsigned long long* cnt) {
    const uint64_t t = (uint64_t)blockIdx.x * kCommitThreads + threadIdx.x, half = 1ull << (k - 1);
    if (t >= half) return;
    const uint64_t r = k > 1 ? __brevll(t) >> (65 - k) : 0;   // t reversed over k - 1 bits
    const G1Affine a = g1_affine_to_mont(in[r], bases_form);
    G1Affine b = g1_affine_to_mont(in[r + half], bases_form);
    const unsigned long long ids = (g1_affine_is_identity(a) ? 1 : 0) + (g1_affine_is_identity(b) ? 1 : 0);
    if (ids) atomicAdd(&cnt[1], ids);
    const G1Xyzz top = g1_from_affine(a);
    G1Xyzz* o = work + 2 * t;
#pragma unroll 1
    for (int s = 0; s < 2; ++s) {                          // a + b, then a - b
        o[s] = g1_add_mixed(top, b);
        b.y = fq_neg(b.y);
    }
}

}  // namespace

hipError_t launch_g1_table(const G1Mul& a, hipStream_t st) {
    if (!a.m) return hipSuccess;
    hipLaunchKernelGGL(k_g1_table, dim3(blocks_of(a.m, kG1Threads)), dim3(kG1Threads), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_g1_mul(const G1Mul& a, hipStream_t st) {
    if (!a.m) return hipSuccess;
    hipLaunchKernelGGL(k_g1_mul, dim3(blocks_of(a.m, kG1Threads)), dim3(kG1Threads), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_g1_butterfly(const G1Mul& a, hipStream_t st) {
    if (!a.m) return hipSuccess;
    hipLaunchKernelGGL(k_g1_butterfly, dim3(blocks_of(a.m, kG1Threads)), dim3(kG1Threads), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_g1_affine(const G1Xyzz* src, uint64_t n, int bases_form, G1Affine* out, unsigned long long* cnt,
                            hipStream_t st) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_g1_affine, dim3(blocks_of(n, (uint64_t)kFbThreads * kFbGroup)), dim3(kFbThreads), 0, st, src, n,
                       bases_form, out, cnt);
    return hipGetLastError();
}

hipError_t launch_g1_fft_first(const G1Affine* in, uint32_t k, int bases_form, G1Xyzz* work, unsigned long long* cnt,
                               hipStream_t st) {
    hipLaunchKernelGGL(k_g1_fft_first, dim3(blocks_of(1ull << (k - 1), kCommitThreads)), dim3(kCommitThreads), 0, st, in,
                       k, bases_form, work, cnt);
    return hipGetLastError();
}

}  // namespace svdw
