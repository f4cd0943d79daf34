// Kernels of the decomposition (svd.hpp has the method, the storage and what
// each kernel does). Every kernel runs blocks of kSvdThreads threads; every row
// index is checked against R or L before memory is touched, every column index
// is below Cp = P b by construction (svd_pair gives panels below P).
#include "svd.hpp"

#include <algorithm>

namespace svdw {
namespace {

constexpr double kSvdEps = 0x1p-52;
typedef double svd_d4 __attribute__((ext_vector_type(4)));

// Column `i` (0 .. 2b - 1) of the pair (p, q): p's b columns, then q's.
__device__ inline uint32_t pair_col(uint32_t p, uint32_t q, uint32_t b, uint32_t i) {
    return i < b ? p * b + i : q * b + (i - b);
}

// The block's sum of x in a fixed order (a tree over the thread index).
__device__ inline double block_sum(double x, double* sh) {
    const unsigned t = threadIdx.x;
    sh[t] = x;
    __syncthreads();
    for (unsigned s = kSvdThreads / 2; s > 0; s >>= 1) {
        if (t < s) sh[t] += sh[t + s];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

// Block j: column j of A.
__global__ __launch_bounds__(kSvdThreads) void k_svd_load(SvdArgs a, const double* __restrict__ m, uint32_t N,
                                                          uint32_t M) {
    __shared__ double sh[kSvdThreads];
    const uint32_t j = blockIdx.x;
    double* col = a.A + (uint64_t)j * a.L;
    const bool wide = N <= M;                              // G = m, else G = m^T
    double sq = 0.0;
    unsigned bad = 0;
    for (uint32_t i = threadIdx.x; i < a.L; i += kSvdThreads) {
        double x = 0.0;
        if (i < a.R) {
            if (j < a.C) {
                x = wide ? m[(uint64_t)i * M + j] : m[(uint64_t)j * M + i];
                if (!(fabs(x) <= 1.79769313486231570815e308)) {   // NaN or infinite
                    ++bad;
                    x = 0.0;
                }
                sq = fma(x, x, sq);
            }
        } else {
            x = i - a.R == j ? 1.0 : 0.0;
        }
        col[i] = x;
    }
    if (bad) atomicAdd(&a.words->nonfinite, (unsigned long long)bad);
    const double s = block_sum(sq, sh);
    if (threadIdx.x == 0) a.norms[j] = s;
}

__global__ __launch_bounds__(kSvdThreads) void k_svd_tiny(SvdArgs a) {
    __shared__ double sh[kSvdThreads];
    double s = 0.0;
    for (uint32_t j = threadIdx.x; j < a.C; j += kSvdThreads) s += a.norms[j];
    const double fro2 = block_sum(s, sh);
    if (threadIdx.x == 0) a.words->tiny = kSvdEps * kSvdEps * fro2;
}

template <int B>
__global__ __launch_bounds__(kSvdThreads) void k_svd_gram(SvdArgs a, uint32_t step) {
    uint32_t p, q;
    svd_pair(a.P, step, blockIdx.x, &p, &q);
    const uint32_t r0 = blockIdx.y * kSvdRows;
    double* out = a.gram + ((uint64_t)blockIdx.x * a.gram_chunks + blockIdx.y) * kSvdGramCells;
    const unsigned t = threadIdx.x;
    if constexpr (B == 8) {
        __shared__ double part[4][kSvdGramCells];
        const unsigned lane = t & 63, w = t >> 6;
        const double* src = a.A + (uint64_t)pair_col(p, q, 8, lane & 15) * a.L;
        const uint32_t base = r0 + w * 16 + (lane >> 4) * 4;   // the lane's 4 rows: k slot (lane >> 4) of 4 steps
        svd_d4 acc = {0.0, 0.0, 0.0, 0.0};
        for (uint32_t e = 0; e < 4; ++e) {
            const uint32_t row = base + e;
            const double x = row < a.R ? src[row] : 0.0;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(x, x, acc, 0, 0, 0);
        }
        for (unsigned reg = 0; reg < 4; ++reg) part[w][((lane >> 4) + 4 * reg) * 16 + (lane & 15)] = acc[reg];
        __syncthreads();
        out[t] = ((part[0][t] + part[1][t]) + part[2][t]) + part[3][t];
    } else {
        constexpr unsigned n2 = 2 * B;
        if (t < n2 * n2) {
            const double* ci = a.A + (uint64_t)pair_col(p, q, B, t / n2) * a.L;
            const double* cj = a.A + (uint64_t)pair_col(p, q, B, t % n2) * a.L;
            const uint32_t r1 = min(r0 + kSvdRows, a.R);
            double acc = 0.0;
            for (uint32_t row = r0; row < r1; ++row) acc = fma(ci[row], cj[row], acc);
            out[t] = acc;
        }
    }
}

template <int B>
__global__ __launch_bounds__(kSvdThreads) void k_svd_rotate(SvdArgs a, uint32_t step) {
    constexpr unsigned n2 = 2 * B;
    __shared__ double H[n2][n2 + 1], J[n2][n2];
    __shared__ double rc[n2], rs[n2];
    __shared__ unsigned partner[n2];
    __shared__ unsigned nrot;
    __shared__ unsigned long long offb;
    uint32_t p, q;
    svd_pair(a.P, step, blockIdx.x, &p, &q);
    const unsigned t = threadIdx.x;
    const bool act = t < n2 * n2;
    const unsigned r = act ? t / n2 : 0, cc = act ? t % n2 : 0;
    if (act) {
        const double* g = a.gram + (uint64_t)blockIdx.x * a.gram_chunks * kSvdGramCells + t;
        double h = 0.0;
        for (uint32_t y = 0; y < a.gram_chunks; ++y) h += g[(uint64_t)y * kSvdGramCells];
        H[r][cc] = h;
        J[r][cc] = r == cc ? 1.0 : 0.0;
    }
    if (t == 0) {
        nrot = 0;
        offb = 0;
    }
    const double tiny = a.words->tiny;
    __syncthreads();
#pragma unroll 1
    for (uint32_t sweep = 0; sweep < a.inner; ++sweep) {
        const unsigned before = nrot;
        __syncthreads();                                   // every thread has read nrot before a round adds to it
#pragma unroll 1
        for (unsigned round = 0; round + 1 < n2; ++round) {
            if (t < B) {
                uint32_t i, j;
                svd_pair(n2, round, t, &i, &j);
                const double hii = H[i][i], hjj = H[j][j], hij = H[i][j];
                double c = 1.0, s = 0.0;
                if (fmin(hii, hjj) > tiny) {
                    const double off = fabs(hij) / sqrt(hii * hjj);
                    atomicMax(&offb, (unsigned long long)__double_as_longlong(off));   // off >= 0: ordered as bits
                    if (!(hij * hij <= kSvdEps * kSvdEps * hii * hjj)) {
                        const double z = (hjj - hii) / (2.0 * hij);
                        const double tt = (z >= 0.0 ? 1.0 : -1.0) / (fabs(z) + sqrt(1.0 + z * z));
                        c = 1.0 / sqrt(1.0 + tt * tt);
                        s = c * tt;
                        atomicAdd(&nrot, 1u);
                    }
                }
                rc[i] = rc[j] = c;
                rs[i] = rs[j] = s;
                partner[i] = j;
                partner[j] = i;
            }
            __syncthreads();
            double nh = 0.0, nj = 0.0;
            if (act) {                                     // X <- X Jr for H and J
                const unsigned pc = partner[cc];
                const double c = rc[cc], s = rs[cc];
                const double ha = H[r][cc], hp = H[r][pc], ja = J[r][cc], jp = J[r][pc];
                nh = cc < pc ? c * ha - s * hp : s * hp + c * ha;
                nj = cc < pc ? c * ja - s * jp : s * jp + c * ja;
            }
            __syncthreads();
            if (act) {
                H[r][cc] = nh;
                J[r][cc] = nj;
            }
            __syncthreads();
            if (act) {                                     // H <- Jr^T H
                const unsigned pr = partner[r];
                const double c = rc[r], s = rs[r];
                const double ha = H[r][cc], hp = H[pr][cc];
                nh = r < pr ? c * ha - s * hp : s * hp + c * ha;
                if (cc == pr && s != 0.0) nh = 0.0;        // the rotated entry itself
            }
            __syncthreads();
            if (act) H[r][cc] = nh;
            __syncthreads();
        }
        if (nrot == before) break;                         // (uniform: nrot is read behind a barrier)
    }
    const unsigned nr = nrot;
    if (blockIdx.y == 0 && t == 0) {
        if (nr)
            atomicAdd(&a.words->rotations, (unsigned long long)nr);
        else
            atomicAdd(&a.words->skipped, 1ull);
        atomicMax(&a.words->off_bits, offb);
    }
    if (nr == 0) return;
    if constexpr (B == 8) {
        const unsigned lane = t & 63, w = t >> 6;
        const uint64_t row = (uint64_t)blockIdx.y * kSvdRows + w * 16 + (lane & 15);
        const bool ok = row < a.L;
        svd_d4 acc = {0.0, 0.0, 0.0, 0.0};
        for (unsigned kk = 0; kk < 4; ++kk) {              // D^T = J^T S^T: A operand J[k][lane & 15], B operand S[row][k]
            const unsigned k = kk * 4 + (lane >> 4);
            const double x = ok ? a.A[(uint64_t)pair_col(p, q, 8, k) * a.L + row] : 0.0;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(J[k][lane & 15], x, acc, 0, 0, 0);
        }
        if (ok)
            for (unsigned reg = 0; reg < 4; ++reg)
                a.A[(uint64_t)pair_col(p, q, 8, (lane >> 4) + 4 * reg) * a.L + row] = acc[reg];
    } else {
        const uint64_t row = (uint64_t)blockIdx.y * kSvdRows + (t & 63);
        const unsigned cg = t >> 6;
        const bool ok = row < a.L;
        double x[n2];
#pragma unroll
        for (unsigned k = 0; k < n2; ++k) x[k] = ok ? a.A[(uint64_t)pair_col(p, q, B, k) * a.L + row] : 0.0;
        __syncthreads();                                   // the row's four threads have read it whole
        for (unsigned j = cg; j < n2; j += 4) {
            double acc = 0.0;
#pragma unroll
            for (unsigned k = 0; k < n2; ++k) acc = fma(x[k], J[k][j], acc);
            if (ok) a.A[(uint64_t)pair_col(p, q, B, j) * a.L + row] = acc;
        }
    }
}

__global__ __launch_bounds__(kSvdThreads) void k_svd_norms(SvdArgs a) {
    __shared__ double sh[kSvdThreads];
    const double* col = a.A + (uint64_t)blockIdx.x * a.L;
    double sq = 0.0;
    for (uint32_t i = threadIdx.x; i < a.R; i += kSvdThreads) sq = fma(col[i], col[i], sq);
    const double s = block_sum(sq, sh);
    if (threadIdx.x == 0) a.norms[blockIdx.x] = sqrt(s);
}

// Element e of u (N N of them), then of v (M M), then of d (R).
__global__ __launch_bounds__(kSvdThreads) void k_svd_write(SvdArgs a, const uint32_t* __restrict__ perm, uint32_t N,
                                                           uint32_t M, double floor, double* u, double* d, double* v) {
    const bool wide = N <= M;
    const uint64_t nu = (uint64_t)N * N, nv = (uint64_t)M * M, total = nu + nv + a.R;
    for (uint64_t e = (uint64_t)blockIdx.x * kSvdThreads + threadIdx.x; e < total;
         e += (uint64_t)gridDim.x * kSvdThreads) {
        if (e >= nu + nv) {
            d[e - nu - nv] = a.norms[perm[e - nu - nv]];
            continue;
        }
        const bool is_u = e < nu;
        const uint64_t f = is_u ? e : e - nu;
        const uint32_t n = is_u ? N : M, row = (uint32_t)(f / n), col = (uint32_t)(f % n);
        double x;
        if (is_u == wide) {                                // the R x R factor: u[i][j] or v[j][i] = g_j[i] / d_j
            const uint32_t j = wide ? col : row, i = wide ? row : col, src = perm[j];
            const double nj = a.norms[src];
            x = nj > floor ? a.A[(uint64_t)src * a.L + i] / nj : 0.0;
        } else {                                           // the C x C factor: v[k][i] or u[i][k] = w_k[i]
            const uint32_t k = wide ? row : col, i = wide ? col : row;
            x = a.A[(uint64_t)perm[k] * a.L + a.R + i];
        }
        (is_u ? u : v)[f] = x;
    }
}

template <class K>
hipError_t launched(K&& k) {
    k();
    return hipGetLastError();
}

}  // namespace

hipError_t launch_svd_load(const SvdArgs& a, const double* m, uint32_t N, uint32_t M, hipStream_t st) {
    return launched([&] { k_svd_load<<<a.P * a.b, kSvdThreads, 0, st>>>(a, m, N, M); });
}
hipError_t launch_svd_tiny(const SvdArgs& a, hipStream_t st) {
    return launched([&] { k_svd_tiny<<<1, kSvdThreads, 0, st>>>(a); });
}
hipError_t launch_svd_gram(const SvdArgs& a, uint32_t step, hipStream_t st) {
    const dim3 grid(a.P / 2, a.gram_chunks);
    return launched([&] {
        if (a.b == 8)
            k_svd_gram<8><<<grid, kSvdThreads, 0, st>>>(a, step);
        else if (a.b == 4)
            k_svd_gram<4><<<grid, kSvdThreads, 0, st>>>(a, step);
        else
            k_svd_gram<1><<<grid, kSvdThreads, 0, st>>>(a, step);
    });
}
hipError_t launch_svd_rotate(const SvdArgs& a, uint32_t step, hipStream_t st) {
    const dim3 grid(a.P / 2, a.apply_chunks);
    return launched([&] {
        if (a.b == 8)
            k_svd_rotate<8><<<grid, kSvdThreads, 0, st>>>(a, step);
        else if (a.b == 4)
            k_svd_rotate<4><<<grid, kSvdThreads, 0, st>>>(a, step);
        else
            k_svd_rotate<1><<<grid, kSvdThreads, 0, st>>>(a, step);
    });
}
hipError_t launch_svd_norms(const SvdArgs& a, hipStream_t st) {
    return launched([&] { k_svd_norms<<<a.P * a.b, kSvdThreads, 0, st>>>(a); });
}
hipError_t launch_svd_write(const SvdArgs& a, const uint32_t* perm, uint32_t N, uint32_t M, double floor, double* u,
                            double* d, double* v, hipStream_t st) {
    const uint64_t total = (uint64_t)N * N + (uint64_t)M * M + a.R;
    const unsigned blocks = (unsigned)std::min<uint64_t>((total + kSvdThreads - 1) / kSvdThreads, 65536);
    return launched([&] { k_svd_write<<<blocks, kSvdThreads, 0, st>>>(a, perm, N, M, floor, u, d, v); });
}

}  // namespace svdw
