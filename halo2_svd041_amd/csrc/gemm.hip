// gfx950 (CDNA4) kernels of the exact field product c_s = a * b
// (honest_prover_mat_mul / field_mat_mul, src/matrix/mod.rs:510-568).
//
//  k_to_digits +      balanced base-256 digit planes and the exact signed-integer
//  k_gemm_dot4        GEMM on v_dot4c_i32_i8 over them, one reduction mod p per output
//  k_to_digits_mf +   the same decomposition on the matrix cores
//  k_gemm_mfma(_rt)   (v_mfma_i32_16x16x64_i8); _rt: plane counts decided on the device
//  k_to_residues /    multi-modular (CRT) product: balanced residue planes mod
//  k_residues_f64 +   pairwise coprime m_k <= 256 (crt_tables.hpp), one int8 GEMM
//  k_gemm_crt_* +     per modulus (per-unit, persistent and wide variants), and
//  k_crt_combine_multi  the rebuild of C mod p from its residues
//  k_gemm_mont        generic Montgomery fallback (operands not small integers)
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <type_traits>
#include <string.h>

#include "gemm.hpp"
#include "kernel_common.hpp"
#include "crt_tables.hpp"

namespace svdw {

// ---------------------------------------------------------- digit planes
// Balanced base-256 digits d_l in [-128, 127]: x = sum_l d_l 256^l.
__global__ __launch_bounds__(256) void k_to_digits(const DView x, uint32_t rows, uint32_t kdim,
                                                   int D, uint32_t rows_pad, uint32_t kg_pad,
                                                   uint32_t* __restrict__ out) {
    uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (uint64_t)rows_pad * kg_pad) return;
    uint32_t row = (uint32_t)(idx / kg_pad), kg = (uint32_t)(idx % kg_pad);
    uint32_t words[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    Fr zero = fr_zero();
    Fr half = fr_p();
    {
        uint32_t c = 0;
#pragma unroll
        for (int i = 7; i >= 0; --i) {
            uint32_t nw = (half.w[i] >> 1) | c;
            c = half.w[i] << 31;
            half.w[i] = nw;
        }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        uint32_t k = kg * 4 + t;
        if (row >= rows || k >= kdim) continue;
        Fr v = view_load(x, zero, row, k);
        Fr tmp;
        bool neg = sub256(tmp, half, v) != 0;
        Fr mag = neg ? fr_sub(fr_zero(), v) : v;
        // signed 128-bit value (host guarantees |x| fits D digits, D <= 9)
        __int128 s = (__int128)(((unsigned __int128)mag.w[3] << 96) | ((unsigned __int128)mag.w[2] << 64) |
                                ((unsigned __int128)mag.w[1] << 32) | mag.w[0]);
        if (neg) s = -s;
#pragma unroll
        for (int l = 0; l < 9; ++l) {
            if (l < D) {
                int dg = (int)(uint32_t)(s & 0xff);
                if (dg >= 128) dg -= 256;
                s = (s - dg) >> 8;
                words[l] |= ((uint32_t)dg & 0xffu) << (8 * t);
            }
        }
    }
    uint32_t* o = out + idx * D;
#pragma unroll
    for (int l = 0; l < 9; ++l)
        if (l < D) o[l] = words[l];
}

hipError_t launch_to_digits(const DView& x, uint32_t rows, uint32_t kdim, int D, uint32_t rows_pad,
                            uint32_t kg_pad, uint32_t* out, hipStream_t st) {
    uint64_t n = (uint64_t)rows_pad * kg_pad;
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_to_digits, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x, rows,
                       kdim, D, rows_pad, kg_pad, out);
    return hipGetLastError();
}

// ------------------------------------------------------------- dot4 GEMM
// Block = 256 threads = 16 x 16, each 2 x 2 outputs -> 32 x 32 tile.
// K advances 8 digit-groups (32 k) per LDS stage. acc[.][.][d] is the
// i32 sum of digit products with la + lb = d; |acc| < 9 * 2^14 * K < 2^31
// for K <= 8192 (host-checked).
constexpr int GT = 32;   // tile edge
constexpr int GKC = 8;   // digit groups per K stage

template <int DA, int DB>
__device__ __forceinline__ Fr combine_diagonals(const int (&acc)[DA + DB - 1]) {
    int64_t col[7] = {0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int d = 0; d < DA + DB - 1; ++d) {
        const int sh = 8 * d;
        col[sh >> 5] += (int64_t)acc[d] * ((int64_t)1 << (sh & 31));
    }
    uint32_t w[7];
    int64_t carry = 0;
#pragma unroll
    for (int q = 0; q < 7; ++q) {
        int64_t t = col[q] + carry;
        w[q] = (uint32_t)t;
        carry = t >> 32;
    }
    return fr_from_signed_words<7>(w);
}

template <int DA, int DB, bool SYM>
__global__ __launch_bounds__(256) void k_gemm_dot4(const uint32_t* __restrict__ Ad,
                                                   const uint32_t* __restrict__ Bd, uint32_t N,
                                                   uint32_t M, uint32_t KG, Fr* __restrict__ out,
                                                   int64_t ors, int64_t ocs, uint32_t tiles_m) {
    __shared__ uint32_t As[GKC][DA][GT];
    __shared__ uint32_t Bs[GKC][DB][GT];
    uint32_t bi, bj;
    if (SYM) {
        // blockIdx -> (bi, bj) with bi <= bj over a tiles_m x tiles_m triangle
        uint32_t b = blockIdx.x, r = 0, rowlen = tiles_m;
        while (b >= rowlen) { b -= rowlen; ++r; --rowlen; }
        bi = r; bj = r + b;
    } else {
        bi = blockIdx.x / tiles_m;
        bj = blockIdx.x % tiles_m;
    }
    const uint32_t tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const uint32_t i0 = bi * GT, j0 = bj * GT;
    int acc[2][2][DA + DB - 1];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int d = 0; d < DA + DB - 1; ++d) acc[r][c][d] = 0;

    const uint32_t lrow = tid >> 3, lg = tid & 7;
    for (uint32_t kg0 = 0; kg0 < KG; kg0 += GKC) {
        {
            const uint32_t* src = Ad + ((uint64_t)(i0 + lrow) * KG + kg0 + lg) * DA;
#pragma unroll
            for (int l = 0; l < DA; ++l) As[lg][l][lrow] = src[l];
            const uint32_t* srcb = Bd + ((uint64_t)(j0 + lrow) * KG + kg0 + lg) * DB;
#pragma unroll
            for (int l = 0; l < DB; ++l) Bs[lg][l][lrow] = srcb[l];
        }
        __syncthreads();
#pragma unroll 2
        for (int g = 0; g < GKC; ++g) {
            int a0[DA], a1[DA], b0[DB], b1[DB];
#pragma unroll
            for (int l = 0; l < DA; ++l) {
                uint2 v = *reinterpret_cast<const uint2*>(&As[g][l][2 * ty]);
                a0[l] = (int)v.x; a1[l] = (int)v.y;
            }
#pragma unroll
            for (int l = 0; l < DB; ++l) {
                uint2 v = *reinterpret_cast<const uint2*>(&Bs[g][l][2 * tx]);
                b0[l] = (int)v.x; b1[l] = (int)v.y;
            }
#pragma unroll
            for (int la = 0; la < DA; ++la)
#pragma unroll
                for (int lb = 0; lb < DB; ++lb) {
                    acc[0][0][la + lb] = __builtin_amdgcn_sdot4(a0[la], b0[lb], acc[0][0][la + lb], false);
                    acc[0][1][la + lb] = __builtin_amdgcn_sdot4(a0[la], b1[lb], acc[0][1][la + lb], false);
                    acc[1][0][la + lb] = __builtin_amdgcn_sdot4(a1[la], b0[lb], acc[1][0][la + lb], false);
                    acc[1][1][la + lb] = __builtin_amdgcn_sdot4(a1[la], b1[lb], acc[1][1][la + lb], false);
                }
        }
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const uint32_t i = i0 + 2 * ty + r, j = j0 + 2 * tx + c;
            if (i < N && j < M) {
                Fr v = combine_diagonals<DA, DB>(acc[r][c]);
                st_fr(out + (int64_t)i * ors + (int64_t)j * ocs, v);
                if (SYM && bi != bj) st_fr(out + (int64_t)j * ors + (int64_t)i * ocs, v);
            }
        }
}

template <int DA, int DB>
static hipError_t gemm_dispatch(bool sym, const uint32_t* Ad, const uint32_t* Bd, uint32_t N,
                                uint32_t M, uint32_t kg, Fr* out, int64_t ors, int64_t ocs,
                                hipStream_t st) {
    uint32_t tn = (N + GT - 1) / GT, tm = (M + GT - 1) / GT;
    if (sym) {
        if (DA != DB || N != M) return hipErrorInvalidValue;
        hipLaunchKernelGGL((k_gemm_dot4<DA, DB, true>), dim3(tm * (tm + 1) / 2), dim3(256), 0, st,
                           Ad, Bd, N, M, kg, out, ors, ocs, tm);
    } else {
        hipLaunchKernelGGL((k_gemm_dot4<DA, DB, false>), dim3(tn * tm), dim3(256), 0, st, Ad, Bd,
                           N, M, kg, out, ors, ocs, tm);
    }
    return hipGetLastError();
}

bool gemm_digits_supported(int DA, int DB) {
    auto ok = [](int d) { return d == 5 || d == 8 || d == 9; };
    return ok(DA) && ok(DB);
}

hipError_t launch_gemm_digits(int DA, int DB, bool sym, const uint32_t* Ad, const uint32_t* Bd,
                              uint32_t N, uint32_t M, uint32_t kg, Fr* out, int64_t ors,
                              int64_t ocs, hipStream_t st) {
#define SVDW_G(a, b) \
    if (DA == a && DB == b) return gemm_dispatch<a, b>(sym, Ad, Bd, N, M, kg, out, ors, ocs, st);
    SVDW_G(5, 5) SVDW_G(5, 8) SVDW_G(5, 9) SVDW_G(8, 5) SVDW_G(8, 8) SVDW_G(8, 9)
    SVDW_G(9, 5) SVDW_G(9, 8) SVDW_G(9, 9)
#undef SVDW_G
    return hipErrorInvalidValue;
}

// ------------------------------------------------------------- MFMA GEMM
// Same exact decomposition on the matrix cores: v_mfma_i32_16x16x64_i8 over
// balanced base-256 digit planes. Global digit layout: [row][kc][D][64 B]
// (kc = 64-k chunk; byte b = digit of X(row, 64 kc + b)), rows padded to 32.
// Fragment (one digit, 16 rows x 64 k): lane l holds row (l & 15), bytes
// [16 (l >> 4), +16) of the chunk; A and B use the same k mapping, so the
// product is independent of the hardware's k order inside the chunk.
// C/D (16x16 i32): col = lane & 15, row = 4 (lane >> 4) + reg.
typedef int v4i __attribute__((ext_vector_type(4)));
constexpr int MT = 32;        // block tile (2 x 2 waves of 16 x 16)
constexpr int LROW = 80;      // LDS bytes per (digit, row): 64 + 16 pad

// Digit planes chosen on the device from an operand's bit-length maximum (the
// engine's digits_for_bits + round_digits): 5, 8 or 9 planes, 0 = too wide for
// the digit GEMM (Montgomery fallback).
__device__ __forceinline__ int device_digits(const unsigned* __restrict__ bits) {
    const uint32_t b = *bits;
    const int need = b <= 7 ? 1 : (int)((b + 9) / 8);
    return need <= 5 ? 5 : need <= 8 ? 8 : need <= 9 ? 9 : 0;
}

__global__ __launch_bounds__(256) void k_to_digits_mf(const DView x, uint32_t rows, uint32_t kdim,
                                                      int D, uint32_t rows_pad, uint32_t kcn,
                                                      uint32_t* __restrict__ out,
                                                      const unsigned* __restrict__ dbits) {
    if (dbits) {
        D = device_digits(dbits);
        if (!D) return;
    }
    uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (uint64_t)rows_pad * kcn * 16) return;
    const uint32_t g = (uint32_t)(idx & 15);
    const uint64_t rk = idx >> 4;
    const uint32_t row = (uint32_t)(rk / kcn), kc = (uint32_t)(rk % kcn);
    uint32_t words[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    Fr zero = fr_zero();
    Fr half = fr_p();
    {
        uint32_t c = 0;
#pragma unroll
        for (int i = 7; i >= 0; --i) {
            uint32_t nw = (half.w[i] >> 1) | c;
            c = half.w[i] << 31;
            half.w[i] = nw;
        }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        uint32_t k = kc * 64 + g * 4 + t;
        if (row >= rows || k >= kdim) continue;
        Fr v = view_load(x, zero, row, k);
        Fr tmp;
        bool neg = sub256(tmp, half, v) != 0;
        Fr mag = neg ? fr_sub(fr_zero(), v) : v;
        __int128 s = (__int128)(((unsigned __int128)mag.w[3] << 96) | ((unsigned __int128)mag.w[2] << 64) |
                                ((unsigned __int128)mag.w[1] << 32) | mag.w[0]);
        if (neg) s = -s;
#pragma unroll
        for (int l = 0; l < 9; ++l) {
            if (l < D) {
                int dg = (int)(uint32_t)(s & 0xff);
                if (dg >= 128) dg -= 256;
                s = (s - dg) >> 8;
                words[l] |= ((uint32_t)dg & 0xffu) << (8 * t);
            }
        }
    }
    uint32_t* o = out + rk * (uint64_t)D * 16 + g;
#pragma unroll
    for (int l = 0; l < 9; ++l)
        if (l < D) o[l * 16] = words[l];
}

hipError_t launch_to_digits_mf(const DView& x, uint32_t rows, uint32_t kdim, int D, uint32_t rows_pad,
                               uint32_t kcn, uint32_t* out, hipStream_t st, const unsigned* dbits) {
    uint64_t n = (uint64_t)rows_pad * kcn * 16;
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_to_digits_mf, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x, rows,
                       kdim, D, rows_pad, kcn, out, dbits);
    return hipGetLastError();
}

template <int DA, int DB>
__device__ __forceinline__ Fr combine_diag_reg(const v4i (&acc)[DA + DB - 1], int reg) {
    int a[DA + DB - 1];
#pragma unroll
    for (int d = 0; d < DA + DB - 1; ++d) a[d] = acc[d][reg];
    return combine_diagonals<DA, DB>(a);
}

template <int DA, int DB>
constexpr int gemm_lds_bytes() {
    return (DA + DB) * MT * LROW > MT * MT * 32 ? (DA + DB) * MT * LROW : MT * MT * 32;
}
template <int DA, int DB, bool SYM>
__device__ __forceinline__ void gemm_mfma_body(uint8_t* S, const uint8_t* __restrict__ Ad,
                                               const uint8_t* __restrict__ Bd, uint32_t N,
                                               uint32_t M, uint32_t kcn, Fr* __restrict__ out,
                                               int64_t ors, int64_t ocs, uint32_t tiles_m) {
    // one LDS array: operand slabs during the K loop, the output tile after it
    uint8_t* As = S;
    uint8_t* Bs = S + DA * MT * LROW;
    uint8_t* Ts = S;
    uint32_t bi, bj;
    if (SYM) {
        uint32_t b = blockIdx.x, r = 0, rowlen = tiles_m;
        while (b >= rowlen) { b -= rowlen; ++r; --rowlen; }
        bi = r; bj = r + b;
    } else {
        bi = blockIdx.x / tiles_m;
        bj = blockIdx.x % tiles_m;
    }
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t wr = wave >> 1, wc = wave & 1;
    const uint32_t i0 = bi * MT, j0 = bj * MT;
    v4i acc[DA + DB - 1];
#pragma unroll
    for (int d = 0; d < DA + DB - 1; ++d) acc[d] = v4i{0, 0, 0, 0};

    const uint32_t frow = lane & 15, fk = (lane >> 4) * 16;
    for (uint32_t kc = 0; kc < kcn; ++kc) {
        // stage the A / B slabs: rows x D x 64 B, 16 B per thread-iteration
        for (uint32_t q = tid; q < (uint32_t)(MT * DA * 4); q += 256) {
            const uint32_t row = q / (DA * 4), rem = q % (DA * 4), l = rem >> 2, part = rem & 3;
            const uint4 v = *reinterpret_cast<const uint4*>(
                Ad + (((uint64_t)(i0 + row) * kcn + kc) * DA + l) * 64 + part * 16);
            *reinterpret_cast<uint4*>(As + (l * MT + row) * LROW + part * 16) = v;
        }
        for (uint32_t q = tid; q < (uint32_t)(MT * DB * 4); q += 256) {
            const uint32_t row = q / (DB * 4), rem = q % (DB * 4), l = rem >> 2, part = rem & 3;
            const uint4 v = *reinterpret_cast<const uint4*>(
                Bd + (((uint64_t)(j0 + row) * kcn + kc) * DB + l) * 64 + part * 16);
            *reinterpret_cast<uint4*>(Bs + (l * MT + row) * LROW + part * 16) = v;
        }
        __syncthreads();
        v4i bf[DB];
#pragma unroll
        for (int lb = 0; lb < DB; ++lb)
            bf[lb] = *reinterpret_cast<const v4i*>(Bs + (lb * MT + wc * 16 + frow) * LROW + fk);
#pragma unroll
        for (int la = 0; la < DA; ++la) {
            const v4i af = *reinterpret_cast<const v4i*>(As + (la * MT + wr * 16 + frow) * LROW + fk);
#pragma unroll
            for (int lb = 0; lb < DB; ++lb)
                acc[la + lb] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af, bf[lb], acc[la + lb], 0, 0, 0);
        }
        __syncthreads();
    }
    // Epilogue: reduce the 17 diagonals to canonical Fr, stage the 32 x 32 cell
    // tile (32 KiB) in the (now free) operand LDS, then write whole 1 KiB tile
    // rows — and, for a symmetric off-diagonal tile, the transposed rows too —
    // as contiguous 16 B-per-lane stores.
    {
        const uint32_t tc = wc * 16 + (lane & 15);
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const uint32_t tr = wr * 16 + (lane >> 4) * 4 + reg;
            Fr v = combine_diag_reg<DA, DB>(acc, reg);
            uint4* dst = reinterpret_cast<uint4*>(Ts + (tr * MT + tc) * 32);
            dst[0] = make_uint4(v.w[0], v.w[1], v.w[2], v.w[3]);
            dst[1] = make_uint4(v.w[4], v.w[5], v.w[6], v.w[7]);
        }
    }
    __syncthreads();
    // direct tile: 32 rows x 64 half-cells; thread -> (row, half-cell)
    for (uint32_t q = tid; q < MT * 64; q += 256) {
        const uint32_t tr = q >> 6, hc = q & 63, tc = hc >> 1, h = hc & 1;
        const uint32_t row = i0 + tr, col = j0 + tc;
        if (row < N && col < M)
            reinterpret_cast<uint4*>(out + (int64_t)row * ors + (int64_t)col * ocs)[h] =
                reinterpret_cast<const uint4*>(Ts + (tr * MT + tc) * 32)[h];
    }
    if (SYM && bi != bj) {
        for (uint32_t q = tid; q < MT * 64; q += 256) {
            const uint32_t tc = q >> 6, hc = q & 63, tr = hc >> 1, h = hc & 1;   // out row = j
            const uint32_t row = j0 + tc, col = i0 + tr;
            if (row < M && col < N)
                reinterpret_cast<uint4*>(out + (int64_t)row * ors + (int64_t)col * ocs)[h] =
                    reinterpret_cast<const uint4*>(Ts + (tr * MT + tc) * 32)[h];
        }
    }
}

template <int DA, int DB, bool SYM>
__global__ __launch_bounds__(256) void k_gemm_mfma(const uint8_t* __restrict__ Ad,
                                                   const uint8_t* __restrict__ Bd, uint32_t N,
                                                   uint32_t M, uint32_t kcn, Fr* __restrict__ out,
                                                   int64_t ors, int64_t ocs, uint32_t tiles_m) {
    __shared__ __attribute__((aligned(16))) uint8_t S[gemm_lds_bytes<DA, DB>()];
    gemm_mfma_body<DA, DB, SYM>(S, Ad, Bd, N, M, kcn, out, ors, ocs, tiles_m);
}
// Digit counts read on the device (no host round trip for the operand bounds):
// every (DA, DB) pair is compiled in and the block branches uniformly.
template <bool SYM>
__global__ __launch_bounds__(256) void k_gemm_mfma_rt(const uint8_t* __restrict__ Ad,
                                                      const uint8_t* __restrict__ Bd, uint32_t N,
                                                      uint32_t M, uint32_t kcn, Fr* __restrict__ out,
                                                      int64_t ors, int64_t ocs, uint32_t tiles_m,
                                                      const unsigned* __restrict__ sa,
                                                      const unsigned* __restrict__ sb) {
    __shared__ __attribute__((aligned(16))) uint8_t S[gemm_lds_bytes<9, 9>()];
    const int DA = device_digits(sa), DB = SYM ? DA : device_digits(sb);
#define SVDW_RT(a, b) \
    if (DA == a && DB == b) { gemm_mfma_body<a, b, SYM>(S, Ad, Bd, N, M, kcn, out, ors, ocs, tiles_m); return; }
    if (SYM) {
        SVDW_RT(5, 5) SVDW_RT(8, 8) SVDW_RT(9, 9)
    } else {
        SVDW_RT(5, 5) SVDW_RT(5, 8) SVDW_RT(5, 9) SVDW_RT(8, 5) SVDW_RT(8, 8) SVDW_RT(8, 9)
        SVDW_RT(9, 5) SVDW_RT(9, 8) SVDW_RT(9, 9)
    }
#undef SVDW_RT
}
hipError_t launch_gemm_mfma_rt(bool sym, const uint8_t* Ad, const uint8_t* Bd, uint32_t N,
                               uint32_t M, uint32_t kcn, Fr* out, int64_t ors, int64_t ocs,
                               const unsigned* bits_a, const unsigned* bits_b, hipStream_t st) {
    uint32_t tn = (N + MT - 1) / MT, tm = (M + MT - 1) / MT;
    if (sym) {
        if (N != M) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_gemm_mfma_rt<true>, dim3(tm * (tm + 1) / 2), dim3(256), 0, st, Ad, Ad, N,
                           M, kcn, out, ors, ocs, tm, bits_a, bits_a);
    } else {
        hipLaunchKernelGGL(k_gemm_mfma_rt<false>, dim3(tn * tm), dim3(256), 0, st, Ad, Bd, N, M, kcn,
                           out, ors, ocs, tm, bits_a, bits_b);
    }
    return hipGetLastError();
}

template <int DA, int DB>
static hipError_t gemm_mfma_dispatch(bool sym, const uint8_t* Ad, const uint8_t* Bd, uint32_t N,
                                     uint32_t M, uint32_t kcn, Fr* out, int64_t ors, int64_t ocs,
                                     hipStream_t st) {
    uint32_t tn = (N + MT - 1) / MT, tm = (M + MT - 1) / MT;
    if (sym) {
        if (DA != DB || N != M) return hipErrorInvalidValue;
        hipLaunchKernelGGL((k_gemm_mfma<DA, DB, true>), dim3(tm * (tm + 1) / 2), dim3(256), 0, st,
                           Ad, Bd, N, M, kcn, out, ors, ocs, tm);
    } else {
        hipLaunchKernelGGL((k_gemm_mfma<DA, DB, false>), dim3(tn * tm), dim3(256), 0, st, Ad, Bd, N,
                           M, kcn, out, ors, ocs, tm);
    }
    return hipGetLastError();
}

hipError_t launch_gemm_mfma(int DA, int DB, bool sym, const uint8_t* Ad, const uint8_t* Bd,
                            uint32_t N, uint32_t M, uint32_t kcn, Fr* out, int64_t ors,
                            int64_t ocs, hipStream_t st) {
#define SVDW_G(a, b) \
    if (DA == a && DB == b) return gemm_mfma_dispatch<a, b>(sym, Ad, Bd, N, M, kcn, out, ors, ocs, st);
    SVDW_G(5, 5) SVDW_G(5, 8) SVDW_G(5, 9) SVDW_G(8, 5) SVDW_G(8, 8) SVDW_G(8, 9)
    SVDW_G(9, 5) SVDW_G(9, 8) SVDW_G(9, 9)
#undef SVDW_G
    return hipErrorInvalidValue;
}

// ------------------------------------------- multi-modular (CRT) exact GEMM
// c_s = A * Bt exactly for |A| < 2^ba, |B| < 2^bb (ba, bb <= 128): with n
// pairwise coprime moduli m_k <= 256 whose product Mtot exceeds 2^(ba+bb+lk+2),
// every residue product C mod m_k is one plain int8 GEMM of the balanced
// residue planes (|r| <= 128, K <= 2^17 keeps the i32 sums exact), and C is
// rebuilt from its n residues (crt_tables.hpp). ~19 int8 GEMMs at P = 63
// instead of 72 digit-pair products. n is decided on the device from the
// operand bit-length words, like the digit path.
__device__ __forceinline__ int crt_nmod(uint32_t ba, uint32_t bb, uint32_t lk) {
    if (ba > 128 || bb > 128) return 0;
    const uint32_t need = ba + bb + lk + 2;
    // lane k tests table entry k + 1 (one load per lane; a scalar loop of
    // dependent loads cost ~2 us per call, measured in the GEMM's block
    // prologue). Called with the whole wave active.
    const uint32_t lane = threadIdx.x & 63;
    const bool ok = lane < (uint32_t)kCrtMaxMod && c_crt_cum_bits[lane + 1] >= need;
    const unsigned long long m = __ballot(ok);
    return m ? __ffsll(m) : 0;
}

// Balanced residues bal = ((x + h) mod m) - h, h = floor(m / 2), in [-128, 127],
// of 4 consecutive-k elements x = +-|x| for moduli k < n: one u32 word (4 x
// int8) per plane at o[k * plane]. w: NW u32 words of |x| (< 2^(32 NW)); nm:
// all ones for x < 0. The sign costs one xor per word, since -|x| = ~|x| + 1 -
// 2^(32 NW), plus the AND of the modulus' (1 - 2^(32 NW)) mod m; the sum of the
// bytes times 256^i mod m is one v_dot4_u32_u8 per word and stays < 2^20,
// where the mul_hi quotient by ceil(2^32 / m) is exact.
template <int NW>
__device__ __forceinline__ void residues_emit(const uint32_t (&w)[4][4], const uint32_t (&nm)[4],
                                              uint32_t* __restrict__ o, uint64_t plane, int n) {
    uint32_t x[4][NW];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int j = 0; j < NW; ++j) x[t][j] = w[t][j] ^ nm[t];
    for (int k = 0; k < n; ++k) {
        const uint32_t m = c_crt_mod[k], magic = c_crt_magic[k], h = m >> 1,
                       cn = c_crt_negc[NW - 2][k];
        uint32_t bal[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            uint32_t s0 = nm[t] & cn;
#pragma unroll
            for (int j = 0; j < NW; ++j) s0 = __builtin_amdgcn_udot4(x[t][j], c_crt_p256[k][j], s0, false);
            const uint32_t q = __umulhi(s0 + h, magic);
            bal[t] = s0 - __umul24(q, m);                      // (x + h) mod m - h, two's complement
        }
        const uint32_t lo = __builtin_amdgcn_perm(bal[1], bal[0], 0x0c0c0400u),
                       hi = __builtin_amdgcn_perm(bal[3], bal[2], 0x0c0c0400u);
        o[k * plane] = lo | (hi << 16);
    }
}
// NW words of |x| (|x| < 2^(32 NW)) from canonical Fr cells.
template <int NW>
__device__ __forceinline__ void residues_body(const DView& x, uint32_t rows, uint32_t kdim,
                                              uint32_t rows_pad, uint32_t kw,
                                              uint32_t* __restrict__ out, int n, uint32_t row,
                                              uint32_t kg, const Fr& half) {
    const Fr zero = fr_zero();
    uint32_t w[4][4], nm[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const uint32_t kk = kg * 4 + t;
        Fr v = zero;
        if (row < rows && kk < kdim) v = view_load(x, zero, row, kk);
        Fr tmp;
        const bool neg = sub256(tmp, half, v) != 0;
        const Fr mag = neg ? fr_sub(zero, v) : v;
        nm[t] = neg ? ~0u : 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) w[t][j] = mag.w[j];
    }
    residues_emit<NW>(w, nm, out + (uint64_t)row * kw + kg, (uint64_t)rows_pad * kw, n);
}
// Balanced residue planes: out[k][row][kpad] int8 (= u32 words of 4 consecutive
// k), k < n; rows >= `rows` and columns >= kdim are zero.
__global__ __launch_bounds__(256) void k_to_residues(const DView x, uint32_t rows, uint32_t kdim,
                                                     uint32_t rows_pad, uint32_t kw,
                                                     uint32_t* __restrict__ out,
                                                     const unsigned* __restrict__ bits_a,
                                                     const unsigned* __restrict__ bits_b,
                                                     const unsigned* __restrict__ bits_c,
                                                     uint32_t lk) {
    // planes for the product (a, b) and, when bits_c is given, also for (c, c)
    int n = crt_nmod(*bits_a, *bits_b, lk);
    if (bits_c) n = max(n, crt_nmod(*bits_c, *bits_c, lk));
    if (!n) return;
    const uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (uint64_t)rows_pad * kw) return;
    const uint32_t row = (uint32_t)(idx / kw), kg = (uint32_t)(idx % kw);
    Fr half = fr_p();
    {
        uint32_t c = 0;
#pragma unroll
        for (int i = 7; i >= 0; --i) {
            const uint32_t nw = (half.w[i] >> 1) | c;
            c = half.w[i] << 31;
            half.w[i] = nw;
        }
    }
    const uint32_t bmax = max(max(*bits_a, *bits_b), bits_c ? *bits_c : 0u);
    if (bmax <= 64)
        residues_body<2>(x, rows, kdim, rows_pad, kw, out, n, row, kg, half);
    else if (bmax <= 96)
        residues_body<3>(x, rows, kdim, rows_pad, kw, out, n, row, kg, half);
    else
        residues_body<4>(x, rows, kdim, rows_pad, kw, out, n, row, kg, half);
}
hipError_t launch_to_residues(const DView& x, uint32_t rows, uint32_t kdim, uint32_t rows_pad,
                              uint32_t kpad, uint32_t* out, const unsigned* bits_a,
                              const unsigned* bits_b, uint32_t lk, hipStream_t st,
                              const unsigned* bits_c) {
    const uint64_t n = (uint64_t)rows_pad * (kpad / 4);
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_to_residues, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x, rows,
                       kdim, rows_pad, kpad / 4, out, bits_a, bits_b, bits_c, lk);
    return hipGetLastError();
}

// |x_q| and sign of ZkMatrix::new's quantization (quantize_body: round half away
// of |x| 2^P, u128 saturation, NaN -> 0, sign(x) < 0 -> p - x_q) as u32 words;
// nm = all ones when x_q is negative (-0.0 included: its residues are 0 either way).
__device__ __forceinline__ void quantized_words(double x, double scale, uint32_t (&w)[4], uint32_t& nm) {
    nm = signbit(x) && !isnan(x) ? ~0u : 0u;
    const double s = round(fabs(x) * scale);
    w[0] = w[1] = w[2] = w[3] = 0u;
    if (s >= 340282366920938463463374607431768211456.0) {
        w[0] = w[1] = w[2] = w[3] = 0xffffffffu;
    } else if (s > 0.0) {
        const uint64_t bits = __double_as_longlong(s);
        const int e = (int)((bits >> 52) & 0x7ff) - 1075;
        const uint64_t mant = (bits & 0xfffffffffffffull) | (1ull << 52);
        const unsigned __int128 v = e >= 0 ? ((unsigned __int128)mant << e) : (unsigned __int128)(mant >> -e);
        w[0] = (uint32_t)v; w[1] = (uint32_t)(v >> 32);
        w[2] = (uint32_t)(v >> 64); w[3] = (uint32_t)(v >> 96);
    }
}
// Residue planes straight from the f64 inputs of svd_witness (what k_to_residues
// computes from the quantized cells, without reading the 32 B cells back): up to
// kMaxResSegs matrices in one launch, segment s covering blocks [blk0[s], blk0[s+1]).
__global__ __launch_bounds__(256) void k_residues_f64(const ResSegs q, const unsigned* __restrict__ W,
                                                      double scale) {
    uint32_t s = 0;
#pragma unroll
    for (int k = 1; k < kMaxResSegs; ++k) s += (uint32_t)k < q.nseg && blockIdx.x >= q.blk0[k];
    const ResSeg g = q.seg[s];
    int n = 0;
    uint32_t bmax = 0;
#pragma unroll
    for (int p = 0; p < 2; ++p)
        if (g.wa[p] >= 0) {
            const uint32_t ba = W[g.wa[p]], bb = W[g.wb[p]];
            const int np = crt_nmod(ba, bb, g.lk[p]);
            if (!np) return;                                   // too wide: no CRT product
            n = max(n, np);
            bmax = max(bmax, max(ba, bb));
        }
    if (!n) return;
    const uint64_t idx = (uint64_t)(blockIdx.x - q.blk0[s]) * blockDim.x + threadIdx.x;
    if (idx >= (uint64_t)g.rows_pad * g.kw) return;
    const uint32_t row = g.tr ? (uint32_t)(idx % g.rows_pad) : (uint32_t)(idx / g.kw),
                   kg = g.tr ? (uint32_t)(idx / g.rows_pad) : (uint32_t)(idx % g.kw);
    uint32_t w[4][4], nm[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const uint32_t kk = kg * 4 + t;
        const uint64_t at = g.tr ? (uint64_t)kk * g.ld + row : (uint64_t)row * g.ld + kk;
        const double x = row < g.rows && kk < g.cols ? g.in[at] : 0.0;
        quantized_words(x, scale, w[t], nm[t]);
    }
    uint32_t* o = g.out + (uint64_t)row * g.kw + kg;
    const uint64_t plane = (uint64_t)g.rows_pad * g.kw;
    if (bmax <= 64)
        residues_emit<2>(w, nm, o, plane, n);
    else if (bmax <= 96)
        residues_emit<3>(w, nm, o, plane, n);
    else
        residues_emit<4>(w, nm, o, plane, n);
}
hipError_t launch_residues_f64(const ResSegs& q0, const unsigned* W, int precision_bits,
                               hipStream_t st) {
    ResSegs q = q0;
    if (!q.nseg || q.nseg > (uint32_t)kMaxResSegs) return hipErrorInvalidValue;
    uint32_t blocks = 0;
    for (uint32_t k = 0; k < q.nseg; ++k) {
        ResSeg& g = q.seg[k];
        if (g.kw * 4 < g.cols || g.rows_pad < g.rows || g.ld < (g.tr ? g.rows : g.cols)) return hipErrorInvalidValue;
        q.blk0[k] = blocks;
        blocks += (uint32_t)(((uint64_t)g.rows_pad * g.kw + 255) / 256);
    }
    q.blk0[q.nseg] = blocks;
    if (!blocks) return hipSuccess;
    hipLaunchKernelGGL(k_residues_f64, dim3(blocks), dim3(256), 0, st, q, W,
                       (double)(1ull << precision_bits));
    return hipGetLastError();
}

// f(integral_constant<int, 0>), ..., f(integral_constant<int, N - 1>): an unrolled
// loop whose index is a compile-time constant in the body
template <int I, int N, class F>
__device__ __forceinline__ void static_for_impl(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for_impl<I + 1, N>(f);
    }
}
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) { static_for_impl<0, N>(f); }

static constexpr int CT = CT_TILE;     // CRT GEMM block tile (4 waves of 64 x 64)
// Staged operand rows are 64 B (one k-chunk) with the four 16 B parts XOR-swizzled
// by (row >> 2) & 3: the staging stores (4 rows x 4 parts per 16 lanes) and the
// fragment reads (16 rows x 1 part) both land on 16 distinct 4-bank groups.
static constexpr int CROW = 64;
static constexpr uint32_t kCrtTileBytes = CT * CT;             // residues of one (tile, modulus)
__device__ __forceinline__ uint32_t crt_lds(uint32_t row, uint32_t part) {
    return row * CROW + 16u * (part ^ ((row >> 2) & 3u));
}

// One (128 x 128 tile, modulus) per block: residues of C mod m_k as bytes
// R[k][row][rpad_m] (tile (bi, bj) of the product; SYM: A == B).
// Ar / Br: planes of astride / bstride rows (a row block of a larger operand is
// its planes from row r0 on with the full operand's stride); R is
// [mod][tiles_a * CT][tiles_m * CT]. One 64-k chunk per LDS round, the next
// chunk's global loads in flight under the current chunk's MFMAs.
// Software pipeline, one barrier per 64-k step: LDS is double-buffered (the
// next chunk is stored into the other buffer while this chunk's MFMAs run from
// fragments read before them), two chunks are in flight in registers behind
// that, and the next step's fragment reads overlap the MFMAs still in the
// pipe. (A single buffer with a store / barrier / read / MFMA / barrier chain
// per step took ~1 us per step, ~16 us per tile, against ~0.1 us of MFMA.)
constexpr int crt_lds_bytes() { return 4 * CT * CROW; }
// Residues of the 4 x 4 accumulator tiles of one wave, stored in MFMA order:
// R[mod][tile][wave][a][b][lane][reg] (one u32 per lane and (a, b): a wave store
// is 256 contiguous bytes); the combine reads the same order (crt_combine_elem).
__device__ __forceinline__ void crt_store_residues(const v4i (&acc)[4][4], uint8_t* __restrict__ R,
                                                   uint32_t nblk, uint32_t tile, int mod) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t m = c_crt_mod[mod], magic = c_crt_magic[mod], bias = c_crt_bias[mod];
    uint32_t* Rt = reinterpret_cast<uint32_t*>(R + ((uint64_t)mod * nblk + tile) * kCrtTileBytes) +
                   wave * 1024 + lane;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            uint32_t r[4];
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                // |acc| <= K 2^14 <= 2^27, bias = m ceil(2^27 / m): x < 2^28 + 2^8,
                // where the quotient by magic = ceil(2^32 / m) is floor(x / m) or
                // one more (x (magic m - 2^32) < 2^32 m / 16), so x - q m is in
                // [-m, m) and min_u32(r, r + m) is the residue: five VALU
                // operations (the fp32 quotient with two corrections took twelve)
                const uint32_t x = (uint32_t)acc[a][b][reg] + bias;
                const uint32_t q = __umulhi(x, magic);
                const uint32_t rr = (uint32_t)((int)x - __mul24((int)q, (int)m));
                r[reg] = min(rr, rr + m);
            }
            Rt[(a * 4 + b) * 64] = __builtin_amdgcn_perm(r[1], r[0], 0x0c0c0400u) |
                                   (__builtin_amdgcn_perm(r[3], r[2], 0x0c0c0400u) << 16);
        }
}
__device__ __forceinline__ void crt_gemm_tile(const uint8_t* __restrict__ Ar, const uint8_t* __restrict__ Br,
                                              uint32_t astride, uint32_t bstride, uint32_t kpad,
                                              uint32_t nblk, uint32_t tile, uint8_t* __restrict__ R,
                                              uint32_t bi, uint32_t bj, int mod, uint8_t* __restrict__ S,
                                              uint64_t& tp1, uint64_t& tp2) {
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t wr = wave >> 1, wc = wave & 1;
    const uint8_t* Ap = Ar + ((uint64_t)mod * astride + bi * CT) * kpad;
    const uint8_t* Bp = Br + ((uint64_t)mod * bstride + bj * CT) * kpad;
    // staging map: 512 x 16 B per operand chunk; thread -> (row, part) for q = tid, tid + 256
    const uint32_t r0 = tid >> 2, r1 = (tid + 256) >> 2, part = tid & 3;
    const uint32_t kcn = kpad / 64;
    v4i acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = v4i{0, 0, 0, 0};
    const uint32_t frow = lane & 15, fk = (lane >> 4) * 16;
    // Staging registers per chunk as named variables, loops spelled out by macro
    // (arrays or lambdas over them ended up in scratch). Chunk indices past the
    // end are clamped to the last chunk, so the loads stay unconditional; those
    // chunks are never stored or multiplied.
#define CRT_GLOAD(g, chunk)                                                                   \
    {                                                                                         \
        const uint64_t ko = (uint64_t)min((uint32_t)(chunk), kcn - 1) * 64 + part * 16;     \
        g##a0 = *reinterpret_cast<const uint4*>(Ap + (uint64_t)r0 * kpad + ko);             \
        g##a1 = *reinterpret_cast<const uint4*>(Ap + (uint64_t)r1 * kpad + ko);             \
        g##b0 = *reinterpret_cast<const uint4*>(Bp + (uint64_t)r0 * kpad + ko);             \
        g##b1 = *reinterpret_cast<const uint4*>(Bp + (uint64_t)r1 * kpad + ko);             \
    }
#define CRT_LSTORE(g, buf)                                                                    \
    {                                                                                         \
        uint8_t* Ac = S + (buf) * 2 * CT * CROW;                                              \
        uint8_t* Bc = Ac + CT * CROW;                                                         \
        *reinterpret_cast<uint4*>(Ac + crt_lds(r0, part)) = g##a0;                            \
        *reinterpret_cast<uint4*>(Ac + crt_lds(r1, part)) = g##a1;                            \
        *reinterpret_cast<uint4*>(Bc + crt_lds(r0, part)) = g##b0;                            \
        *reinterpret_cast<uint4*>(Bc + crt_lds(r1, part)) = g##b1;                            \
    }
#define CRT_FRAG(buf)                                                                         \
    {                                                                                         \
        const uint8_t* Ac = S + (buf) * 2 * CT * CROW;                                        \
        const uint8_t* Bc = Ac + CT * CROW;                                                   \
        _Pragma("unroll") for (int a = 0; a < 4; ++a)                                         \
            af[a] = *reinterpret_cast<const v4i*>(Ac + crt_lds(wr * 64 + a * 16 + frow, fk >> 4)); \
        _Pragma("unroll") for (int b = 0; b < 4; ++b)                                         \
            bf[b] = *reinterpret_cast<const v4i*>(Bc + crt_lds(wc * 64 + b * 16 + frow, fk >> 4)); \
    }
#define CRT_MMA()                                                                             \
    {                                                                                         \
        _Pragma("unroll") for (int a = 0; a < 4; ++a)                                         \
            _Pragma("unroll") for (int b = 0; b < 4; ++b)                                     \
                acc[a][b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[a], bf[b], acc[a][b], 0, 0, 0); \
    }
    // chunk c lives in register set g(c mod 4) until it is stored to LDS (at
    // step c - 1); four chunks in flight keep ~64 KB of loads outstanding per
    // CU, what an HBM / Infinity Cache latency needs (at 2 chunks a tile took
    // ~1 us per 64-k step, bound by bytes in flight, not by the MFMAs)
    uint4 g0a0, g0a1, g0b0, g0b1, g1a0, g1a1, g1b0, g1b1;
    uint4 g2a0, g2a1, g2b0, g2b1, g3a0, g3a1, g3b0, g3b1;
    v4i af[4], bf[4];
    CRT_GLOAD(g0, 0);
    CRT_GLOAD(g1, 1);
    CRT_GLOAD(g2, 2);
    CRT_GLOAD(g3, 3);
    CRT_LSTORE(g0, 0);
    CRT_GLOAD(g0, 4);
    __syncthreads();
    tp1 = wall_clock64();
    CRT_FRAG(0);
    // kcn is a multiple of 4 (kpad % 256 == 0): the steps are branch-free, so
    // the compiler's load counters see the four chunks in flight (a branch per
    // step made it drain every load before each LDS store). The last group's
    // stores and fragment reads of chunks >= kcn (clamped loads) are unused.
#define CRT_STEP(g, c)                                                                        \
    {                                                                                         \
        CRT_LSTORE(g, ((c) + 1) & 1);                    /* chunk c + 1 into the other buffer */ \
        CRT_GLOAD(g, (c) + 5);                           /* (c + 5) mod 4 = (c + 1) mod 4 */  \
        CRT_MMA();                                                                            \
        __syncthreads();                                                                      \
        CRT_FRAG(((c) + 1) & 1);                                                              \
    }
    for (uint32_t c0 = 0; c0 < kcn; c0 += 4) {
        CRT_STEP(g1, c0)
        CRT_STEP(g2, c0 + 1)
        CRT_STEP(g3, c0 + 2)
        CRT_STEP(g0, c0 + 3)
    }
    tp2 = wall_clock64();
#undef CRT_STEP
#undef CRT_GLOAD
#undef CRT_LSTORE
#undef CRT_FRAG
#undef CRT_MMA
    crt_store_residues(acc, R, nblk, tile, mod);
}


// Debug timeline of the GEMM's blocks (svdw_debug_trace): per real block its
// start and end on the 100 MHz wall clock and (XCC id << 16 | HW_ID).
__device__ unsigned long long* g_trace = nullptr;
hipError_t set_debug_trace(void* buf) {
    unsigned long long* p = (unsigned long long*)buf;
    return hipMemcpyToSymbol(HIP_SYMBOL(g_trace), &p, sizeof p);
}
__device__ __forceinline__ void trace_block(uint64_t t0, uint64_t t1, uint64_t t2) {
    unsigned long long* tr = g_trace;
    if (!tr || threadIdx.x) return;
    uint32_t xcc, hw;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    tr[5 * blockIdx.x] = t0;
    tr[5 * blockIdx.x + 1] = t1;
    tr[5 * blockIdx.x + 2] = t2;
    tr[5 * blockIdx.x + 3] = wall_clock64();
    tr[5 * blockIdx.x + 4] = ((unsigned long long)xcc << 32) | hw;
}


// tile t of a job (t < nblk; the sequence starts at tile0) -> its (row,
// column) tile (SYM: upper tiles row by row)
__device__ __forceinline__ void crt_tile_rc(const CrtJob& q, uint32_t t, uint32_t* bi, uint32_t* bj) {
    t += q.tile0;
    if (q.sym) {
        uint32_t r = 0, rest = t, rowlen = q.tiles_a;
        while (rest >= rowlen) { rest -= rowlen; ++r; --rowlen; }
        *bi = r; *bj = r + rest;
    } else {
        *bi = t / q.tiles_m;
        *bj = t - *bi * q.tiles_m;
    }
}
// The products of a CrtBatch in one launch, placed modulus-major per XCD: the
// work units (job, modulus < the job's device-decided count n, tile) are laid
// out job-major, modulus-major, and XCD x (blocks x, x + 8, ... on gfx950) takes
// the x-th eighth of them in order, so an XCD streams one modulus's residue
// planes through its own L2 while it computes that modulus's tiles, instead of
// every XCD reading strips of every plane. Blocks past the units exit at once
// (the grid is sized for n = kCrtMaxMod).
// (job, modulus, tile) unit u of the batch in the XCD-modulus-major order of
// the GEMM kernels; false for blocks past the units
__device__ __forceinline__ bool crt_unit(const CrtBatch& b, uint32_t blk, uint32_t* jo, uint32_t* mo,
                                         uint32_t* to) {
    uint32_t cnt[kMaxCrtJobs], total = 0;
#pragma unroll
    for (int j = 0; j < kMaxCrtJobs; ++j) {
        cnt[j] = 0;
        if ((uint32_t)j < b.njobs)
            cnt[j] = (uint32_t)crt_nmod(*b.job[j].bits_a, *b.job[j].bits_b, b.job[j].lk) * b.job[j].nblk;
        total += cnt[j];
    }
    const uint32_t per = (total + 7) / 8, k = blk >> 3;
    if (k >= per) return false;
    uint32_t u = (blk & 7) * per + k;
    if (u >= total) return false;
    uint32_t j = 0;
#pragma unroll
    for (int q = 0; q < kMaxCrtJobs - 1; ++q)
        if (j == (uint32_t)q && u >= cnt[q]) { u -= cnt[q]; ++j; }
    *jo = j;
    *mo = u / b.job[j].nblk;
    *to = u - *mo * b.job[j].nblk;
    return true;
}
__global__ __launch_bounds__(256) void k_gemm_crt_multi(const CrtBatch b) {
    __shared__ __attribute__((aligned(16))) uint8_t S[crt_lds_bytes()];
    const uint64_t t0 = wall_clock64();
    uint32_t j, mod, t;
    if (!crt_unit(b, blockIdx.x, &j, &mod, &t)) return;
    const CrtJob& q = b.job[j];
    uint32_t bi, bj;
    crt_tile_rc(q, t, &bi, &bj);
    uint64_t tp1 = 0, tp2 = 0;
    crt_gemm_tile(q.Ar, q.sym ? q.Ar : q.Br, q.astride, q.sym ? q.astride : q.bstride, q.kpad, q.nblk, t,
                  q.R, bi, bj, (int)mod, S, tp1, tp2);
    trace_block(t0, tp1, tp2);
}
// persistent CRT GEMM blocks per XCD label: two per CU (32 CUs per XCD)
static constexpr uint32_t kCrtPersPerXcd = 64;
// Operand row-tile bases and output place of one (job, modulus, tile) unit.
struct CrtUnitPtr {
    const uint8_t* Ap;
    const uint8_t* Bp;
    uint8_t* R;
    uint32_t nblk, t, mod;
};
__device__ __forceinline__ CrtUnitPtr crt_unit_ptr(const CrtBatch& b, const uint32_t (&cnt)[kMaxCrtJobs],
                                                   uint32_t u) {
    uint32_t j = 0;
#pragma unroll
    for (int q = 0; q < kMaxCrtJobs - 1; ++q)
        if (j == (uint32_t)q && u >= cnt[q]) { u -= cnt[q]; ++j; }
    const CrtJob& q = b.job[j];
    CrtUnitPtr o;
    o.mod = u / q.nblk;
    o.t = u - o.mod * q.nblk;
    o.nblk = q.nblk;
    o.R = q.R;
    uint32_t bi, bj;
    crt_tile_rc(q, o.t, &bi, &bj);
    o.Ap = q.Ar + ((uint64_t)o.mod * q.astride + bi * CT) * q.kpad;
    o.Bp = (q.sym ? q.Ar : q.Br) + ((uint64_t)o.mod * (q.sym ? q.astride : q.bstride) + bj * CT) * q.kpad;
    return o;
}
// The register-staged tile loop of crt_gemm_tile on a persistent grid: block b
// (XCD label b mod 8, slot b / 8 of nb8) takes the units lo + slot, lo + slot +
// nb8, ... of its XCD's eighth [lo, hi) of the batch's units (the order of
// k_gemm_crt_multi), and its chunk pipeline runs on across unit boundaries: the
// loads of the next unit's first chunks are in flight while the current unit's
// last chunks are multiplied and its residues reduced and stored, so a block's
// prologue (3.3 us per 128 x 128 x 1024 unit, gemmprobe timeline) is paid once
// instead of per unit. Needs one kpad for all jobs with at least 8 chunks (a
// load is then at most one unit ahead); launch_gemm_crt_multi checks.
__global__ __launch_bounds__(256, 2) void k_gemm_crt_pers(const CrtBatch b) {
    __shared__ __attribute__((aligned(16))) uint8_t S[crt_lds_bytes()];
    const uint64_t t0 = wall_clock64();
    uint32_t cnt[kMaxCrtJobs], total = 0;
#pragma unroll
    for (int j = 0; j < kMaxCrtJobs; ++j) {
        cnt[j] = 0;
        if ((uint32_t)j < b.njobs)
            cnt[j] = (uint32_t)crt_nmod(*b.job[j].bits_a, *b.job[j].bits_b, b.job[j].lk) * b.job[j].nblk;
        total += cnt[j];
    }
    const uint32_t per = (total + 7) / 8, x = blockIdx.x & 7, slot = blockIdx.x >> 3, nb8 = gridDim.x >> 3;
    const uint32_t lo = x * per, hi = min(lo + per, total);
    if (lo + slot >= hi) return;
    const uint32_t nunits = (hi - lo - slot + nb8 - 1) / nb8;
    const uint32_t kpad = b.job[0].kpad, kcn = kpad / 64;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t wr = wave >> 1, wc = wave & 1;
    const uint32_t r0 = tid >> 2, r1 = (tid + 256) >> 2, part = tid & 3;
    const uint32_t frow = lane & 15, fk = (lane >> 4) * 16;
    const uint64_t o0 = (uint64_t)r0 * kpad + part * 16, o1 = (uint64_t)r1 * kpad + part * 16;
    CrtUnitPtr cur = crt_unit_ptr(b, cnt, lo + slot);
    CrtUnitPtr nxt = nunits > 1 ? crt_unit_ptr(b, cnt, lo + slot + nb8) : cur;
    v4i acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[a][q] = v4i{0, 0, 0, 0};
    // chunk ch of the current unit (ch >= kcn: chunk ch - kcn of the next one,
    // the current unit's last chunk when there is none)
#define CRP_GLOAD(g, ch)                                                                      \
    {                                                                                         \
        const uint32_t c_ = (ch);                                                             \
        const bool nx_ = c_ >= kcn;                                                           \
        const uint8_t* A_ = nx_ ? nxt.Ap : cur.Ap;                                            \
        const uint8_t* B_ = nx_ ? nxt.Bp : cur.Bp;                                            \
        const uint64_t ko = (uint64_t)(nx_ ? c_ - kcn : c_) * 64;                             \
        g##a0 = *reinterpret_cast<const uint4*>(A_ + o0 + ko);                                \
        g##a1 = *reinterpret_cast<const uint4*>(A_ + o1 + ko);                                \
        g##b0 = *reinterpret_cast<const uint4*>(B_ + o0 + ko);                                \
        g##b1 = *reinterpret_cast<const uint4*>(B_ + o1 + ko);                                \
    }
#define CRP_LSTORE(g, buf)                                                                    \
    {                                                                                         \
        uint8_t* Ac = S + (buf) * 2 * CT * CROW;                                              \
        uint8_t* Bc = Ac + CT * CROW;                                                         \
        *reinterpret_cast<uint4*>(Ac + crt_lds(r0, part)) = g##a0;                            \
        *reinterpret_cast<uint4*>(Ac + crt_lds(r1, part)) = g##a1;                            \
        *reinterpret_cast<uint4*>(Bc + crt_lds(r0, part)) = g##b0;                            \
        *reinterpret_cast<uint4*>(Bc + crt_lds(r1, part)) = g##b1;                            \
    }
#define CRP_FRAG(buf)                                                                         \
    {                                                                                         \
        const uint8_t* Ac = S + (buf) * 2 * CT * CROW;                                        \
        const uint8_t* Bc = Ac + CT * CROW;                                                   \
        _Pragma("unroll") for (int a = 0; a < 4; ++a)                                         \
            af[a] = *reinterpret_cast<const v4i*>(Ac + crt_lds(wr * 64 + a * 16 + frow, fk >> 4)); \
        _Pragma("unroll") for (int q = 0; q < 4; ++q)                                         \
            bf[q] = *reinterpret_cast<const v4i*>(Bc + crt_lds(wc * 64 + q * 16 + frow, fk >> 4)); \
    }
#define CRP_MMA()                                                                             \
    {                                                                                         \
        _Pragma("unroll") for (int a = 0; a < 4; ++a)                                         \
            _Pragma("unroll") for (int q = 0; q < 4; ++q)                                     \
                acc[a][q] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[a], bf[q], acc[a][q], 0, 0, 0); \
    }
#define CRP_STEP(g, c)                                                                        \
    {                                                                                         \
        CRP_LSTORE(g, ((c) + 1) & 1);                                                         \
        CRP_GLOAD(g, (c) + 5);                                                                \
        CRP_MMA();                                                                            \
        __syncthreads();                                                                      \
        CRP_FRAG(((c) + 1) & 1);                                                              \
    }
    uint4 g0a0, g0a1, g0b0, g0b1, g1a0, g1a1, g1b0, g1b1;
    uint4 g2a0, g2a1, g2b0, g2b1, g3a0, g3a1, g3b0, g3b1;
    v4i af[4], bf[4];
    CRP_GLOAD(g0, 0);
    CRP_GLOAD(g1, 1);
    CRP_GLOAD(g2, 2);
    CRP_GLOAD(g3, 3);
    CRP_LSTORE(g0, 0);
    CRP_GLOAD(g0, 4);
    __syncthreads();
    const uint64_t tp1 = wall_clock64();
    CRP_FRAG(0);
    for (uint32_t k = 0; k < nunits; ++k) {
        if (k + 1 >= nunits) nxt = cur;
        // (the last unit's loads past its end re-read its first chunks: the
        // stores and fragment reads of those are never multiplied)
        for (uint32_t c0 = 0; c0 < kcn; c0 += 4) {
            CRP_STEP(g1, c0)
            CRP_STEP(g2, c0 + 1)
            CRP_STEP(g3, c0 + 2)
            CRP_STEP(g0, c0 + 3)
        }
        crt_store_residues(acc, cur.R, cur.nblk, cur.t, (int)cur.mod);
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[a][q] = v4i{0, 0, 0, 0};
        cur = nxt;
        if (k + 2 < nunits) nxt = crt_unit_ptr(b, cnt, lo + slot + (k + 2) * nb8);
    }
    trace_block(t0, tp1, wall_clock64());
#undef CRP_STEP
#undef CRP_GLOAD
#undef CRP_LSTORE
#undef CRP_FRAG
#undef CRP_MMA
}
// 256 x 128 block tile: two vertically adjacent 128 x 128 tiles of the job's
// tile grid per (tile pair, modulus) unit, 4 waves of 128 x 64. Per 64-k step a
// wave reads 8 A and 4 B fragments (12 KiB) for 32 MFMAs: half the LDS bytes
// per MFMA of the 64 x 64 wave tiles (16 fragments for 16 MFMAs), which bound
// those near 40 % of the matrix-core rate. 48 KiB of LDS (two 24 KiB buffers),
// two chunks in flight in registers, two blocks per CU. Non-symmetric jobs of
// whole tile grids only (launch_gemm_crt_multi checks); a pair's second tile
// past the last tile row reads clamped rows and stores nothing. Residues go to
// the 128 x 128 tiles' places in the per-unit kernel's MFMA order, so the
// combine is unchanged: wave (wr, wc)'s accumulator rows a < 4 / a >= 4 are the
// per-unit kernel's waves 2 * 0 + wc / 2 * 1 + wc of tile 2 bi2 + wr.
static constexpr int CTW = 2 * CT;
constexpr int crt_wide_lds_bytes() { return 2 * (CTW + CT) * CROW; }
__device__ __forceinline__ uint32_t crt_npairs(const CrtJob& q) { return (q.tiles_a + 1) / 2 * q.tiles_m; }
__device__ __forceinline__ bool crt_unit_wide(const CrtBatch& b, uint32_t blk, uint32_t* jo, uint32_t* mo,
                                              uint32_t* po) {
    uint32_t cnt[kMaxCrtJobs], total = 0;
#pragma unroll
    for (int j = 0; j < kMaxCrtJobs; ++j) {
        cnt[j] = 0;
        if ((uint32_t)j < b.njobs)
            cnt[j] = (uint32_t)crt_nmod(*b.job[j].bits_a, *b.job[j].bits_b, b.job[j].lk) * crt_npairs(b.job[j]);
        total += cnt[j];
    }
    const uint32_t per = (total + 7) / 8, k = blk >> 3;
    if (k >= per) return false;
    uint32_t u = (blk & 7) * per + k;
    if (u >= total) return false;
    uint32_t j = 0;
#pragma unroll
    for (int q = 0; q < kMaxCrtJobs - 1; ++q)
        if (j == (uint32_t)q && u >= cnt[q]) { u -= cnt[q]; ++j; }
    const uint32_t np = crt_npairs(b.job[j]);
    *jo = j;
    *mo = u / np;
    *po = u - *mo * np;
    return true;
}
__global__ __launch_bounds__(256, 2) void k_gemm_crt_wide(const CrtBatch b) {
    __shared__ __attribute__((aligned(16))) uint8_t S[crt_wide_lds_bytes()];
    const uint64_t t0 = wall_clock64();
    uint32_t j, mod, pr;
    if (!crt_unit_wide(b, blockIdx.x, &j, &mod, &pr)) return;
    const CrtJob& q = b.job[j];
    const uint32_t bi2 = pr / q.tiles_m, bj = pr - bi2 * q.tiles_m;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t wr = wave >> 1, wc = wave & 1;
    const uint32_t kpad = q.kpad, kcn = kpad / 64;
    const uint32_t rlast = q.tiles_a * CT - 1;            // staged A rows stay in the job's tile rows
    const uint8_t* Ap = q.Ar + (uint64_t)mod * q.astride * kpad;
    const uint8_t* Bp = q.Br + ((uint64_t)mod * q.bstride + bj * CT) * kpad;
    const uint32_t rr = tid >> 2, part = tid & 3;
    uint64_t ao[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) ao[i] = (uint64_t)min(bi2 * CTW + rr + 64u * i, rlast) * kpad + part * 16;
    const uint64_t bo0 = (uint64_t)rr * kpad + part * 16, bo1 = (uint64_t)(rr + 64) * kpad + part * 16;
    const uint32_t frow = lane & 15, fp = lane >> 4;
    v4i acc[8][4];
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[a][c] = v4i{0, 0, 0, 0};
#define CRW_GLOAD(g, chunk)                                                                   \
    {                                                                                         \
        const uint64_t ko = (uint64_t)min((uint32_t)(chunk), kcn - 1) * 64;                   \
        g##a0 = *reinterpret_cast<const uint4*>(Ap + ao[0] + ko);                             \
        g##a1 = *reinterpret_cast<const uint4*>(Ap + ao[1] + ko);                             \
        g##a2 = *reinterpret_cast<const uint4*>(Ap + ao[2] + ko);                             \
        g##a3 = *reinterpret_cast<const uint4*>(Ap + ao[3] + ko);                             \
        g##b0 = *reinterpret_cast<const uint4*>(Bp + bo0 + ko);                               \
        g##b1 = *reinterpret_cast<const uint4*>(Bp + bo1 + ko);                               \
    }
#define CRW_LSTORE(g, buf)                                                                    \
    {                                                                                         \
        uint8_t* Ac = S + (buf) * (CTW + CT) * CROW;                                          \
        uint8_t* Bc = Ac + CTW * CROW;                                                        \
        *reinterpret_cast<uint4*>(Ac + crt_lds(rr, part)) = g##a0;                            \
        *reinterpret_cast<uint4*>(Ac + crt_lds(rr + 64, part)) = g##a1;                       \
        *reinterpret_cast<uint4*>(Ac + crt_lds(rr + 128, part)) = g##a2;                      \
        *reinterpret_cast<uint4*>(Ac + crt_lds(rr + 192, part)) = g##a3;                      \
        *reinterpret_cast<uint4*>(Bc + crt_lds(rr, part)) = g##b0;                            \
        *reinterpret_cast<uint4*>(Bc + crt_lds(rr + 64, part)) = g##b1;                       \
    }
#define CRW_FRAG(buf)                                                                         \
    {                                                                                         \
        const uint8_t* Ac = S + (buf) * (CTW + CT) * CROW;                                    \
        const uint8_t* Bc = Ac + CTW * CROW;                                                  \
        _Pragma("unroll") for (int a = 0; a < 8; ++a)                                         \
            af[a] = *reinterpret_cast<const v4i*>(Ac + crt_lds(wr * 128 + a * 16 + frow, fp)); \
        _Pragma("unroll") for (int c = 0; c < 4; ++c)                                         \
            bf[c] = *reinterpret_cast<const v4i*>(Bc + crt_lds(wc * 64 + c * 16 + frow, fp));  \
    }
#define CRW_MMA()                                                                             \
    {                                                                                         \
        _Pragma("unroll") for (int a = 0; a < 8; ++a)                                         \
            _Pragma("unroll") for (int c = 0; c < 4; ++c)                                     \
                acc[a][c] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[a], bf[c], acc[a][c], 0, 0, 0); \
    }
    // chunk c + 1 into the other LDS buffer, chunk c + 3 into the registers it
    // came from, chunk c multiplied, then the fragments of chunk c + 1
#define CRW_STEP(g, c)                                                                        \
    {                                                                                         \
        CRW_LSTORE(g, ((c) + 1) & 1);                                                         \
        CRW_GLOAD(g, (c) + 3);                                                                \
        CRW_MMA();                                                                            \
        __syncthreads();                                                                      \
        CRW_FRAG(((c) + 1) & 1);                                                              \
    }
    uint4 g0a0, g0a1, g0a2, g0a3, g0b0, g0b1, g1a0, g1a1, g1a2, g1a3, g1b0, g1b1;
    v4i af[8], bf[4];
    CRW_GLOAD(g0, 0);
    CRW_GLOAD(g1, 1);
    CRW_LSTORE(g0, 0);
    CRW_GLOAD(g0, 2);
    __syncthreads();
    const uint64_t tp1 = wall_clock64();
    CRW_FRAG(0);
    // (kcn is a multiple of 4: whole pairs of steps)
    for (uint32_t c0 = 0; c0 < kcn; c0 += 2) {
        CRW_STEP(g1, c0)
        CRW_STEP(g0, c0 + 1)
    }
    const uint64_t tp2 = wall_clock64();
#undef CRW_STEP
#undef CRW_GLOAD
#undef CRW_LSTORE
#undef CRW_FRAG
#undef CRW_MMA
    const uint32_t ti = bi2 * 2 + wr;                       // this wave's 128 x 128 tile row
    if (ti < q.tiles_a) {
        const uint32_t m = c_crt_mod[mod], magic = c_crt_magic[mod], bias = c_crt_bias[mod];
        uint32_t* Rt = reinterpret_cast<uint32_t*>(q.R + ((uint64_t)mod * q.nblk + ti * q.tiles_m + bj) *
                                                            kCrtTileBytes) + lane;
#pragma unroll
        for (int a = 0; a < 8; ++a)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                uint32_t r[4];
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {           // (crt_store_residues' reduction)
                    const uint32_t x = (uint32_t)acc[a][c][reg] + bias;
                    const uint32_t qq = __umulhi(x, magic);
                    const uint32_t rv = (uint32_t)((int)x - __mul24((int)qq, (int)m));
                    r[reg] = min(rv, rv + m);
                }
                Rt[((a >> 2) * 2 + wc) * 1024 + ((a & 3) * 4 + c) * 64] =
                    __builtin_amdgcn_perm(r[1], r[0], 0x0c0c0400u) |
                    (__builtin_amdgcn_perm(r[3], r[2], 0x0c0c0400u) << 16);
            }
    }
    trace_block(t0, tp1, tp2);
}
// C from its n residues, written as canonical Fr to out[i*ors + j*ocs]: one
// element per thread in the GEMM's tile order (each block one 256-element
// stretch of a tile), so a wave reads 64 consecutive residue bytes per modulus
// (the n loads issued before the first use: one memory latency, not n) and
// writes four rows of 16 consecutive cells. C mod p = sum_k r_k E_k +
// q (-Mtot mod p), q = floor(sum_k r_k inv_k / m_k + 1/2) in f64 (|C| < Mtot / 4
// keeps it exact), accumulated in eight 64-bit accumulators, one per 32-bit
// word of E_k (each sum of n <= 40 products of an 8-bit residue and a 32-bit
// word stays below 2^46: no carries until the end), then one 9-word
// reduction. SYM: elements j >= i of the upper tiles (the GEMM computed upper
// and diagonal 128-tiles), each also stored at (j, i).
__device__ __forceinline__ void crt_combine_elem(const CrtJob& q, uint32_t cblk) {
    const int n = crt_nmod(*q.bits_a, *q.bits_b, q.lk);
    if (!n) return;
    // element e of tile t in the GEMM's MFMA order (wave, a, b, lane, reg)
    constexpr uint32_t BPT = kCrtTileBytes / 256;
    const uint32_t tl = cblk / BPT;
    const uint32_t e = (cblk - tl * BPT) * 256 + threadIdx.x;
    const uint32_t reg = e & 3, ln = (e >> 2) & 63, ab = (e >> 8) & 15, w = e >> 12;
    uint32_t bi, bj;
    crt_tile_rc(q, tl, &bi, &bj);
    const uint32_t i = bi * CT + (w >> 1) * 64 + (ab >> 2) * 16 + (ln >> 4) * 4 + reg;
    const uint32_t j = bj * CT + (w & 1) * 64 + (ab & 3) * 16 + (ln & 15);
    if (i >= q.N || j >= q.M || (q.sym && j < i)) return;
    const uint64_t plane = (uint64_t)q.nblk * kCrtTileBytes;
    const uint8_t* __restrict__ rp = q.R + (uint64_t)tl * kCrtTileBytes + e;
    uint32_t r[kCrtMaxMod];
#pragma unroll
    for (int k = 0; k < kCrtMaxMod; ++k) r[k] = k < n ? rp[k * plane] : 0u;
    const int off = n * (n - 1) / 2;
    // one 64-bit accumulator per 32-bit word of E_k (v_mad_u64_u32): r (8 bit)
    // x word (32 bit) summed over n <= 40 moduli stays below 2^46 -> no carries
    // until the end (half the VALU of 16-bit limbs with 24-bit products)
    uint64_t acc[8];
#pragma unroll
    for (int w = 0; w < 8; ++w) acc[w] = 0;
    double sq = 0.0;
#pragma unroll
    for (int k = 0; k < kCrtMaxMod; ++k) {
        if (k < n) {                                       // (uniform)
            sq = fma((double)r[k], c_crt_frac[off + k], sq);
#pragma unroll
            for (int w = 0; w < 8; ++w) acc[w] += (uint64_t)r[k] * c_crt_ep[off + k][w];
        }
    }
    const uint32_t qq = (uint32_t)floor(sq + 0.5);         // < 2^14
    uint32_t x[9];
    uint64_t t = 0;
#pragma unroll
    for (int w = 0; w < 8; ++w) {
        t += acc[w] + (uint64_t)qq * c_crt_nmp[n][w];       // < 2^47 + carry
        x[w] = (uint32_t)t;
        t >>= 32;
    }
    x[8] = (uint32_t)t;
    const Fr v = reduce9(x);
    // plain stores: the two 16 B halves of a cell (and, for the mirror, the
    // other lanes' cells of a line) meet in L2 and go out as whole lines (the
    // nontemporal form wrote x1.24 the cell bytes, r03_pmc_summary.json)
    st_fr(q.out + (int64_t)i * q.ors + (int64_t)j * q.ocs, v);
    if (q.sym && j > i) st_fr(q.out + (int64_t)j * q.ors + (int64_t)i * q.ocs, v);
}
// Combine blocks of a CrtBatch (cblocks in all, job j from cblk0[j]) dealt
// XCD-contiguously: XCD x takes a contiguous run of the row-major tile
// sequence, so the halves of a 128-byte residue line that neighbouring tiles
// read come through the same L2.
__global__ __launch_bounds__(256) void k_crt_combine_multi(const CrtBatch b, uint32_t cblocks) {
    const uint32_t per = (cblocks + 7) / 8, t = (blockIdx.x & 7) * per + (blockIdx.x >> 3);
    if (t >= cblocks) return;
    uint32_t j = 0;
    for (uint32_t k = 1; k < b.njobs; ++k) j += t >= b.job[k].cblk0;
    crt_combine_elem(b.job[j], t - b.job[j].cblk0);
}

size_t crt_scratch_bytes(uint32_t N, uint32_t M) {
    // kCrtMaxMod planes of whole 128 x 128 tiles
    const uint64_t a = ((uint64_t)N + CT - 1) / CT * CT, m = ((uint64_t)M + CT - 1) / CT * CT;
    return (size_t)(kCrtMaxMod * a * m);
}
// tile / block fields of a batch; units: GEMM blocks for n = kCrtMaxMod, cblocks: combine blocks
static hipError_t prep_crt_batch(CrtBatch& b, uint32_t& units, uint32_t& cblocks) {
    if (b.njobs < 1 || b.njobs > (uint32_t)kMaxCrtJobs) return hipErrorInvalidValue;
    units = 0;
    cblocks = 0;
    for (uint32_t j = 0; j < b.njobs; ++j) {
        CrtJob& q = b.job[j];
        q.tiles_a = (q.N + CT - 1) / CT;
        q.tiles_m = q.sym ? q.tiles_a : (q.M + CT - 1) / CT;
        // every staged row (tiles x CT) lies inside its operand's planes
        if (q.kpad % 256 || q.astride < q.tiles_a * CT || (!q.sym && q.bstride < q.tiles_m * CT))
            return hipErrorInvalidValue;
        if (q.sym && q.N != q.M) return hipErrorInvalidValue;
        q.nblk = q.sym ? q.tiles_a * (q.tiles_a + 1) / 2 : q.tiles_a * q.tiles_m;
        if (q.tcount) {
            if (q.tile0 + q.tcount > q.nblk) return hipErrorInvalidValue;
            q.nblk = q.tcount;
        } else if (q.tile0) {
            return hipErrorInvalidValue;
        }
        units += kCrtMaxMod * q.nblk;                    // upper bound: n = kCrtMaxMod
        q.cblk0 = cblocks;
        cblocks += q.nblk * (kCrtTileBytes / 256);
    }
    return hipSuccess;
}
hipError_t launch_gemm_crt_multi(const CrtBatch& b0, hipStream_t st) {
    CrtBatch b = b0;
    uint32_t units, cblocks;
    const hipError_t pe = prep_crt_batch(b, units, cblocks);
    if (pe != hipSuccess) return pe;
    const dim3 grid((units + 7) / 8 * 8);
    if (b.kern > 3) return hipErrorInvalidValue;
    // wide tiles: non-symmetric jobs over whole tile grids (kern 3: and at
    // least 64 tile pairs, ~1200 units at n = 19, two rounds of two blocks per
    // CU; gemmprobe: 2048^2 m.v^T 209 -> 186 us against the persistent kernel,
    // but 1024^2's 608 units 35 -> 37 us), else the persistent kernel (one
    // kpad of >= 8 chunks for every job), else the per-unit one
    bool wide = b.kern >= 2;
    uint32_t wunits = 0, pairs = 0;
    for (uint32_t j = 0; j < b.njobs; ++j) {
        const CrtJob& q = b.job[j];
        wide = wide && !q.sym && !q.tile0 && !q.tcount;
        pairs += (q.tiles_a + 1) / 2 * q.tiles_m;
    }
    wunits = kCrtMaxMod * pairs;
    if (b.kern == 3 && pairs < 64) wide = false;
    bool pers = b.kern >= 1 && b.job[0].kpad >= 512;
    for (uint32_t j = 1; j < b.njobs; ++j) pers = pers && b.job[j].kpad == b.job[0].kpad;
    if (wide)
        hipLaunchKernelGGL(k_gemm_crt_wide, dim3((wunits + 7) / 8 * 8), dim3(256), 0, st, b);
    else if (pers)
        hipLaunchKernelGGL(k_gemm_crt_pers, dim3(std::min<uint32_t>(grid.x, 8 * kCrtPersPerXcd)), dim3(256), 0,
                           st, b);
    else
        hipLaunchKernelGGL(k_gemm_crt_multi, grid, dim3(256), 0, st, b);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_crt_combine_multi, dim3((cblocks + 7) / 8 * 8), dim3(256), 0, st, b, cblocks);
    return hipGetLastError();
}

hipError_t launch_gemm_crt(bool sym, const uint8_t* Ar, const uint8_t* Br, uint32_t N, uint32_t M,
                           uint32_t astride, uint32_t bstride, uint32_t kpad, uint8_t* R, Fr* out,
                           int64_t ors, int64_t ocs, const unsigned* bits_a,
                           const unsigned* bits_b, uint32_t lk, hipStream_t st, uint32_t kern) {
    if (sym && (N != M || astride != bstride)) return hipErrorInvalidValue;
    CrtBatch b;
    memset(&b, 0, sizeof b);
    b.njobs = 1;
    b.kern = kern;
    CrtJob& q = b.job[0];
    q.Ar = Ar;
    q.Br = sym ? Ar : Br;
    q.R = R;
    q.out = out;
    q.bits_a = bits_a;
    q.bits_b = bits_b;
    q.ors = ors;
    q.ocs = ocs;
    q.astride = astride;
    q.bstride = bstride;
    q.kpad = kpad;
    q.N = N;
    q.M = M;
    q.lk = lk;
    q.sym = sym;
    return launch_gemm_crt_multi(b, st);
}

// -------------------------------------------------------- Montgomery GEMM
__global__ __launch_bounds__(256) void k_gemm_mont(const DView A, const DView B, uint32_t N,
                                                   uint32_t K, uint32_t M, Fr* out, int64_t ors,
                                                   int64_t ocs, const unsigned* __restrict__ sa,
                                                   const unsigned* __restrict__ sb, int crt_lk) {
    if (sa) {   // the digit (crt_lk < 0) or CRT GEMM already produced the product
        if (crt_lk < 0 ? (device_digits(sa) && device_digits(sb)) : crt_nmod(*sa, *sb, crt_lk) > 0)
            return;
    }
    uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (uint64_t)N * M) return;
    uint32_t i = (uint32_t)(e / M), j = (uint32_t)(e % M);
    Fr zero = fr_zero();
    Fr acc = fr_zero();
    for (uint32_t k = 0; k < K; ++k) {
        Fr a = view_load(A, zero, i, k);
        Fr b = view_load(B, zero, k, j);
        acc = fr_add(acc, mont_mul(a, b));   // a * b * R^-1
    }
    st_fr(out + (int64_t)i * ors + (int64_t)j * ocs, mont_mul(acc, fr_r2()));
}

hipError_t launch_gemm_mont(const DView& A, const DView& B, uint32_t N, uint32_t K, uint32_t M,
                            Fr* out, int64_t ors, int64_t ocs, hipStream_t st,
                            const unsigned* bits_a, const unsigned* bits_b, int crt_lk) {
    uint64_t n = (uint64_t)N * M;
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_gemm_mont, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, A, B, N, K,
                       M, out, ors, ocs, bits_a, bits_b, crt_lk);
    return hipGetLastError();
}

}  // namespace svdw
