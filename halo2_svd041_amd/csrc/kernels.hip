// gfx950 (CDNA4) kernels of the SVD-verify witness engine.
//
//  k_quantize      ZkMatrix::new / ZkVector::new cells   (src/matrix/mod.rs:29-40, 230-252)
//  k_stage         every gadget block of check_svd_phase0 / verify_mul except
//                  the GEMM and the inner-product rows: one cell program per
//                  stage (prog.hpp), HBM-write bound, 16 B/lane coalesced stores
//  k_matvec_scan   field_mat_vec_mul rows (src/matrix/mod.rs:574-599): every
//                  prefix sum of the row inner product is a cell -> block Fr scan
// (The exact field product honest_prover_mat_mul / field_mat_mul: gemm.hip.)
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <type_traits>
#include <string.h>

#include "kernels.hpp"
#include "kernel_common.hpp"

namespace svdw {

// ----------------------------------------------------------------- helpers
// (view_load, f64_scale and reduce9: kernel_common.hpp, shared with gemm.hip)
__device__ __forceinline__ uint32_t signed_bits(const Fr& x) {
    // bit length of |x| where x is read as the signed representative in (-p/2, p/2]
    Fr half = fr_p();
    // (p-1)/2
    uint32_t c = 0;
#pragma unroll
    for (int i = 7; i >= 0; --i) {
        uint32_t nw = (half.w[i] >> 1) | c;
        c = half.w[i] << 31;
        half.w[i] = nw;
    }
    Fr t;
    bool neg = sub256(t, half, x) != 0;   // x > (p-1)/2
    Fr mag = neg ? fr_sub(fr_zero(), x) : x;
    uint32_t bits = 0;
#pragma unroll
    for (int i = 7; i >= 0; --i)
        if (bits == 0 && mag.w[i]) bits = 32 * i + 32 - __clz(mag.w[i]);
    return bits;
}

// --------------------------------------------------------------- quantize
// x_q = round_half_away(|x| * 2^P) as u128 (saturating, NaN -> 0);
// sign(x) < 0 (incl. -0.0) -> p - x_q.   [zk_fixed_point_chip quantization,
// SURVEY.md Appendix C.1]
// Fold of the block maxima inside the quantize launch (BitFold), fence-free:
// each block publishes its maximum with an agent-scope atomic exchange and
// arrives on its group's counter (group = blk & 7) only once the exchange has
// returned (the register use below makes the arrival wait for it); the last
// arrival of a group arrives on the global counter, the last of those sees
// every maximum with agent-scope loads. An agent-scope release fence instead
// writes back the whole L2 (the block's cells) per block: 670 us instead of 19.
// Hardware assumption (gfx950, several XCDs with their own L2): agent-scope
// atomics are performed at the device coherence point, not in an XCD's L2, so
// a maximum exchanged before the arrival is what the last block's agent-scope
// load returns; the last arrival's counter update is an acquire besides.
// Called after the block's stores are issued, so its latency overlaps them.
__device__ __forceinline__ void bits_fold(const BitFold& f, uint32_t blk, uint32_t bmax) {
    __shared__ uint32_t last, red[4][4];
    if (threadIdx.x == 0) {
        const uint32_t g = blk & 7, gsize = (f.nblk - g + 7) / 8;
        const uint32_t old = __hip_atomic_exchange(f.bm + blk, bmax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("" ::"v"(old) : "memory");
        bool lst = __hip_atomic_fetch_add(f.cnt + 1 + g, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gsize - 1;
        if (lst) {
            __hip_atomic_store(f.cnt + 1 + g, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const uint32_t ng = min(f.nblk, 8u);
            // acquire on the last arrival only (a cache invalidate, no write-back)
            lst = __hip_atomic_fetch_add(f.cnt, 1u, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) == ng - 1;
        }
        last = lst;
    }
    __syncthreads();
    if (!last) return;
    uint32_t x[3] = {0u, 0u, 0u};
    for (uint32_t k0 = threadIdx.x; k0 < f.nblk; k0 += 8 * blockDim.x) {
        uint32_t v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const uint32_t k = k0 + q * blockDim.x;
            v[q] = k < f.nblk ? __hip_atomic_load(f.bm + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const uint32_t k = k0 + q * blockDim.x;
#pragma unroll
            for (int s = 0; s < 3; ++s)
                if (k >= f.b[s] && k < f.b[s + 1]) x[s] = max(x[s], v[q]);
        }
    }
#pragma unroll
    for (int s = 0; s < 3; ++s) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) x[s] = max(x[s], (uint32_t)__shfl_xor((int)x[s], off));
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][s] = x[s];
    }
    __syncthreads();
    if (threadIdx.x < f.nred) {
        const uint32_t s = threadIdx.x;
        f.wout[s] = max(max(red[0][s], red[1][s]), max(red[2][s], red[3][s]));
    }
    if (threadIdx.x == 0) __hip_atomic_store(f.cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// bit length of |x_q| over a block's values (for the GEMM modulus count):
// thread max -> wave max -> block max (LDS)
template <int PT>
__device__ __forceinline__ uint32_t block_bits(const double (&xv)[PT], double scale) {
    uint32_t bits = 0;
#pragma unroll
    for (int k = 0; k < PT; ++k) {
        const double s = round(fabs(xv[k]) * scale);
        if (s >= 340282366920938463463374607431768211456.0) bits = 128;
        else if (s >= 1.0) bits = max(bits, (uint32_t)ilogb(s) + 1);
    }
    __shared__ uint32_t wmax[4];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) bits = max(bits, (uint32_t)__shfl_xor((int)bits, off));
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = bits;
    __syncthreads();
    return max(max(wmax[0], wmax[1]), max(wmax[2], wmax[3]));
}
// PT * 256 values per block, PT per thread (value blk * PT * 256 + k * 256 +
// tid: each store instruction coalesced), all loads issued first.
template <int PT>
__device__ __forceinline__ void quantize_body(const double* __restrict__ in, uint64_t n,
                                              Fr* __restrict__ out, double scale,
                                              unsigned* __restrict__ blockmax, uint32_t blk,
                                              QuantKeep keep = QuantKeep{0, 0, 0, 0, 0},
                                              const BitFold fold = BitFold{}, uint32_t gblk = 0) {
    const uint64_t i0 = (uint64_t)blk * (PT * 256) + threadIdx.x;
    uint32_t bmax = 0;
    double xv[PT];
#pragma unroll
    for (int k = 0; k < PT; ++k) {
        const uint64_t i = i0 + 256ull * k;
        xv[k] = i < n ? in[i] : 0.0;
    }
    if (blockmax) {
        bmax = block_bits<PT>(xv, scale);
        if (!(fold.wout && gblk < fold.nblk) && threadIdx.x == 0) blockmax[blk] = bmax;
    }
#pragma unroll
    for (int k = 0; k < PT; ++k) {
        const uint64_t i = i0 + 256ull * k;
        if (i >= n) continue;
        if (keep.cols) {                                  // partial store (row-sharded rank)
            const uint32_t r = (uint32_t)(i / keep.cols), cc = (uint32_t)(i - (uint64_t)r * keep.cols);
            if (!((r >= keep.rlo && r < keep.rhi) || (cc >= keep.clo && cc < keep.chi))) continue;
        }
        st_fr(out + i, quantize_fr(xv[k], scale));    // (L2 joins the two halves of a line)
    }
    if (blockmax && fold.wout && gblk < fold.nblk) bits_fold(fold, gblk, bmax);
}
__global__ __launch_bounds__(256) void k_quantize(const double* __restrict__ in, uint64_t n,
                                                  Fr* __restrict__ out, double scale,
                                                  unsigned* __restrict__ blockmax) {
    quantize_body<kQuantPerBlock / 256>(in, n, out, scale, blockmax, blockIdx.x);
}
// m, u, v, d in one launch (their ZkMatrix::new calls are back to back,
// examples/svd_example.rs:138-144): one ramp-up / tail instead of four.
template <int PT>
__global__ __launch_bounds__(256) void k_quantize_multi(const QuantSegs q, double scale) {
    uint32_t s = 0;
#pragma unroll
    for (int k = 1; k < kMaxQuantSegs; ++k) s += (uint32_t)k < q.nseg && blockIdx.x >= q.blk0[k];
    const double* in = q.in[0];
    Fr* out = q.out[0];
    unsigned* bm = q.blockmax[0];
    uint64_t n = q.n[0];
    uint32_t b0 = q.blk0[0];
    QuantKeep keep = q.keep[0];
#pragma unroll
    for (int k = 1; k < kMaxQuantSegs; ++k)      // selects, not a dynamic index into the argument
        if (s == (uint32_t)k) {
            in = q.in[k]; out = q.out[k]; bm = q.blockmax[k]; n = q.n[k]; b0 = q.blk0[k]; keep = q.keep[k];
        }
    quantize_body<PT>(in, n, out, scale, bm, blockIdx.x - b0, keep, q.fold, blockIdx.x);
}
hipError_t launch_quantize_multi(const QuantSegs& q, int p, hipStream_t st) {
    if (!q.nseg || q.nseg > (uint32_t)kMaxQuantSegs || !q.blk0[q.nseg]) return hipErrorInvalidValue;
    const uint32_t pb = q.per_block ? q.per_block : kQuantPerBlock;
    if (pb == kQuantPerBlockSmall)
        hipLaunchKernelGGL(k_quantize_multi<kQuantPerBlockSmall / 256>, dim3(q.blk0[q.nseg]), dim3(256), 0, st, q,
                           (double)(1ull << p));
    else if (pb == kQuantPerBlock)
        hipLaunchKernelGGL(k_quantize_multi<kQuantPerBlock / 256>, dim3(q.blk0[q.nseg]), dim3(256), 0, st, q,
                           (double)(1ull << p));
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_quantize(const double* in, uint64_t n, Fr* out, int p, unsigned* blockmax,
                           hipStream_t st) {
    if (!n) return hipSuccess;
    double scale = (double)(1ull << p);
    hipLaunchKernelGGL(k_quantize, dim3((unsigned)((n + kQuantPerBlock - 1) / kQuantPerBlock)), dim3(256), 0, st, in, n, out,
                       scale, blockmax);
    return hipGetLastError();
}
// block s: out[s] = max(blockmax[seg.begin[s] .. seg.begin[s + 1]))
__global__ __launch_bounds__(256) void k_bits_reduce(const unsigned* __restrict__ blockmax,
                                                     const BitSegs seg, unsigned* __restrict__ out) {
    __shared__ uint32_t wmax[4];
    const uint32_t s = blockIdx.x;
    uint32_t b = 0;
    for (uint32_t i = seg.begin[s] + threadIdx.x; i < seg.begin[s + 1]; i += 256) b = max(b, blockmax[i]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) b = max(b, (uint32_t)__shfl_xor((int)b, off));
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = b;
    __syncthreads();
    if (threadIdx.x == 0) out[s] = max(max(wmax[0], wmax[1]), max(wmax[2], wmax[3]));
}
// Timing aid ("hold_us"): one wave spinning ~us microseconds on the device clock
// (s_memrealtime, 100 MHz) so the host finishes enqueueing before the step runs.
__global__ void k_hold(uint64_t ticks) {
    const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
    while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
}
hipError_t launch_hold(uint32_t us, hipStream_t st) {
    hipLaunchKernelGGL(k_hold, dim3(1), dim3(64), 0, st, (uint64_t)us * 100u);
    return hipGetLastError();
}
hipError_t launch_bits_reduce(const unsigned* blockmax, const BitSegs& seg, uint32_t nseg,
                              unsigned* out, hipStream_t st) {
    if (!nseg || nseg >= (uint32_t)kMaxBitSegs) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_bits_reduce, dim3(nseg), dim3(256), 0, st, blockmax, seg, out);
    return hipGetLastError();
}

// ----------------------------------------------------------- stage kernel
// Phase A: one thread per element (kStageElems = 256 = block size) runs the
// stage's micro-ops, leaving the element's values V[0..nv) (8 words each) in
// LDS. Phase B: the block's E*C advice cells (then E*L lookup cells) are
// produced half a cell (16 B) per lane in stream order, so every wave store
// is 1 KiB contiguous: cell = (V[src] >> lo) & (2^nbits - 1).
constexpr int VW = 8;    // LDS words per value

__device__ __forceinline__ void lds_put(uint32_t* s, const Fr& v) {
    uint4* q = reinterpret_cast<uint4*>(s);
    q[0] = make_uint4(v.w[0], v.w[1], v.w[2], v.w[3]);
    q[1] = make_uint4(v.w[4], v.w[5], v.w[6], v.w[7]);
}
__device__ __forceinline__ Fr lds_get(const uint32_t* s) {
    const uint4* q = reinterpret_cast<const uint4*>(s);
    uint4 a = q[0], b = q[1];
    Fr r;
    r.w[0] = a.x; r.w[1] = a.y; r.w[2] = a.z; r.w[3] = a.w;
    r.w[4] = b.x; r.w[5] = b.y; r.w[6] = b.z; r.w[7] = b.w;
    return r;
}

// Output words [4h, 4h+4) of (S >> lo) & mask(nbits), S = 8 LDS words at s;
// words past the top read as 0 (reads are clamped in-bounds, then masked).
__device__ __forceinline__ uint4 extract_half(const uint32_t* s, uint32_t lo, uint32_t nbits,
                                              uint32_t h) {
    const uint32_t q = (lo >> 5) + 4 * h, r = lo & 31;
    uint32_t x[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const uint32_t w = q + i;
        const uint32_t v = s[w < 8 ? w : 7];
        x[i] = w < 8 ? v : 0u;
    }
    uint32_t o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = __builtin_amdgcn_alignbit(x[i + 1], x[i], r);
    if (nbits) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int keep = (int)nbits - 32 * (4 * (int)h + i);
            const uint32_t m = keep >= 32 ? 0xffffffffu : (keep <= 0 ? 0u : ((1u << keep) - 1u));
            o[i] &= m;
        }
    }
    return make_uint4(o[0], o[1], o[2], o[3]);
}

// LDS carve (bytes, all 16-aligned): consts | element values | slot ops | micro-ops | views

// x / d for x * d < 2^32 via one 32-bit mul_hi (magic = ceil(2^32 / d), d >= 2).
__device__ __forceinline__ uint32_t fastdiv(uint32_t x, uint32_t d, uint32_t magic) {
    return d == 1 ? x : __umulhi(x, magic);
}

// Phase B: per-(slot, half) descriptors and masks prepared once per block
// (half_desc, prog.hpp), so a half-cell costs one descriptor + one mask LDS
// read, five word reads, four alignbit and four and (no per-cell decoding,
// clamping or mask arithmetic). The (element, slot) of the lane's next cell is
// tracked incrementally (the cell index advances by blockDim / 2 per step).
// ALIGN: the block's iterations cover whole (blockDim * 16 B)-aligned address
// windows (the first one partially), so every wave store is one aligned 1 KiB.
// Half-cells [.., hc_end) of the windows from the one holding hc_begin on (hc_begin
// is this lane's first half-cell: lane tid's half-cells are hc_begin + k * blockDim).
__device__ __forceinline__ void stream_cells_run(uint4* __restrict__ out, uint32_t hc_begin, uint32_t hc_end,
                                                 const uint32_t* __restrict__ sHD,
                                                 const uint4* __restrict__ sHM, uint32_t C, uint32_t magic,
                                                 const uint32_t* smem, uint32_t vbase0, uint32_t nv) {
    const uint32_t h = threadIdx.x & 1, step = blockDim.x >> 1;
    const uint32_t dq = step / C, dr = step - dq * C, ev = stage_elem_words(nv);
    uint32_t c = hc_begin >> 1;
    uint32_t el = fastdiv(c, C, magic), slot = c - el * C;
    uint32_t vbase = vbase0 + el * ev;                    // LDS word of this element's values
    for (uint32_t hc = hc_begin; hc < hc_end; hc += blockDim.x) {
        const uint32_t k = 2 * slot + h;
        const uint32_t d = sHD[k];
        const uint4 m = sHM[k];
        const uint32_t wo = ((d & kHalfElem) ? vbase : 0u) + (d & 0xffffu);
        const uint32_t r = (d >> 16) & 31u;
        const uint32_t* x = smem + wo;
        const uint32_t x0 = x[0], x1 = x[1], x2 = x[2], x3 = x[3], x4 = x[4];
        const uint4 v = make_uint4(__builtin_amdgcn_alignbit(x1, x0, r) & m.x,
                                   __builtin_amdgcn_alignbit(x2, x1, r) & m.y,
                                   __builtin_amdgcn_alignbit(x3, x2, r) & m.z,
                                   __builtin_amdgcn_alignbit(x4, x3, r) & m.w);
        out[hc] = v;
        slot += dr;
        vbase += dq * ev;
        if (slot >= C) {
            slot -= C;
            vbase += ev;
        }
    }
}
// rot: the block starts at window rot mod (its window count) and wraps around
// ("stage_rot"), so that blocks started together do not all write the same
// window offset of their chunks at the same time.
template <bool ALIGN>
__device__ __forceinline__ void stream_cells_desc(uint4* __restrict__ out, uint32_t total,
                                                  const uint32_t* __restrict__ sHD,
                                                  const uint4* __restrict__ sHM, uint32_t C,
                                                  uint32_t magic, const uint32_t* smem,
                                                  uint32_t vbase0, uint32_t nv, uint32_t rot = 0) {
    const uint32_t B = blockDim.x, tid = threadIdx.x;
    const uint32_t mis = ALIGN ? (uint32_t)(reinterpret_cast<uintptr_t>(out) >> 4) & (B - 1) : 0u;
    // lane tid's half-cells: tid - mis + k B (k >= 0, >= 0); window k holds
    // [k B - mis, (k + 1) B - mis)
    const uint32_t first = tid >= mis ? tid - mis : tid + B - mis;
    const uint32_t nw = (total + mis + B - 1) / B;
    const uint32_t r = nw > 1 ? rot % nw : 0u;
    if (!r) {
        stream_cells_run(out, first, total, sHD, sHM, C, magic, smem, vbase0, nv);
        return;
    }
    const uint32_t cut = r * B - mis;                     // first half-cell of window r
    stream_cells_run(out, cut + tid, total, sHD, sHM, C, magic, smem, vbase0, nv);
    stream_cells_run(out, first, cut, sHD, sHM, C, magic, smem, vbase0, nv);
}

// Descriptor and masks of half h of a slot (see half_desc).
__device__ __forceinline__ void make_half(const SlotOp op, uint32_t h, uint32_t* d, uint4* m) {
    const uint32_t lo = op.lo;
    uint32_t nb = op.nbits ? op.nbits : 256u;
    nb = min(nb, 256u - lo);
    const bool elem = op.src < KSRC;
    const uint32_t base = (elem ? op.src : op.src - KSRC) * VW;
    *d = half_desc(base + (lo >> 5) + 4 * h, lo & 31u, elem);
    uint32_t w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int keep = (int)nb - 32 * (4 * (int)h + i);
        w[i] = keep >= 32 ? 0xffffffffu : (keep <= 0 ? 0u : ((1u << keep) - 1u));
    }
    *m = make_uint4(w[0], w[1], w[2], w[3]);
}

// a * b mod p for canonical a, b. Fast path when both signed representatives
// (x or x - p) are below 2^128 in magnitude -- quantized cells always are (the
// u128 saturation of ZkMatrix::new), e.g. mat_times_diag_mat's u_ij * d_j:
// an exact 4 x 4-word product (< 2^256 < 6p), a quotient-estimate reduction and
// a conditional negation instead of two full Montgomery products.
__device__ __forceinline__ Fr fr_mul_any(const Fr& a, const Fr& b) {
    Fr na, nb;
    sub256(na, fr_p(), a);                              // p - a
    sub256(nb, fr_p(), b);
    const bool sa = a.w[7] != 0, sb = b.w[7] != 0;     // top word set: the negative side
    uint32_t ma[4], mb[4], hi = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        ma[i] = sa ? na.w[i] : a.w[i];
        mb[i] = sb ? nb.w[i] : b.w[i];
    }
#pragma unroll
    for (int i = 4; i < 8; ++i) hi |= (sa ? na.w[i] : a.w[i]) | (sb ? nb.w[i] : b.w[i]);
    if (__any(hi != 0)) {                               // some lane out of range: generic
        if (hi) return fr_mul(a, b);
    }
    uint32_t t[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) t[i] = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        uint32_t c = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) t[i + j] = mac32(ma[i], mb[j], t[i + j], c);
        t[i + 4] = c;
    }
    const Fr r = reduce9(t);                            // < 2^256 -> mod p
    return (sa != sb) ? fr_neg(r) : r;
}

// Phase A for one element: run the stage's micro-ops, values into myV (LDS).
__device__ __forceinline__ void element_program(const StageArgs& a, uint32_t e, uint32_t* myV,
                                                const uint32_t* sK, const MicroOp* sMo,
                                                const DView* sVw, const Fr& pf0, bool in0,
                                                const Fr& pf1, bool in1) {
    const uint32_t i = e / a.cols, j = e - (e / a.cols) * a.cols;
    for (uint32_t m = 0; m < a.nmo; ++m) {
        const MicroOp op = sMo[m];
        uint32_t* dst = myV + op.dst * VW;
        switch (op.op) {
            case MO_LOAD: {
                if (op.a == 0 && in0) {
                    lds_put(dst, pf0);
                } else if (op.a == 1 && in1) {
                    lds_put(dst, pf1);
                } else {
                    const DView vw = sVw[op.a];
                    if (vw.mode == VIEW_DIAGK)
                        lds_put(dst, lds_get(sK + (i == j ? vw.diag_k : vw.pad_k) * VW));
                    else
                        lds_put(dst, view_load(vw, lds_get(sK + vw.pad_k * VW), i, j));
                }
                break;
            }
            case MO_ADDK:
                lds_put(dst, fr_add(lds_get(myV + op.a * VW), lds_get(sK + op.b * VW)));
                break;
            case MO_SUB:
                lds_put(dst, fr_sub(lds_get(myV + op.a * VW), lds_get(myV + op.b * VW)));
                break;
            case MO_MUL:
                lds_put(dst, fr_mul_any(lds_get(myV + op.a * VW), lds_get(myV + op.b * VW)));
                break;
            case MO_LIMBSHL: {
                const Fr sv = lds_get(myV + op.a * VW);
                // 64-bit window at bit p0 (p0 < 256), masked to p1 bits, << b
                const uint32_t lo = op.p0, q = lo >> 5, r = lo & 31;
                uint32_t w0 = 0, w1 = 0, w2 = 0;
#pragma unroll
                for (int t = 0; t < 8; ++t) {
                    w0 = (t == (int)q) ? sv.w[t] : w0;
                    w1 = (t == (int)q + 1) ? sv.w[t] : w1;
                    w2 = (t == (int)q + 2) ? sv.w[t] : w2;
                }
                const uint64_t w01 = (uint64_t)w0 | ((uint64_t)w1 << 32);
                uint64_t x = r ? ((w01 >> r) | ((uint64_t)w2 << (64 - r))) : w01;
                if (op.p1 < 64) x &= (1ull << op.p1) - 1;
                const uint32_t sh = op.b;
                const uint64_t lo64 = sh < 64 ? (x << sh) : 0;
                const uint64_t hi64 = sh == 0 ? 0 : (sh < 64 ? (x >> (64 - sh)) : (x << (sh - 64)));
                Fr v = fr_zero();
                v.w[0] = (uint32_t)lo64; v.w[1] = (uint32_t)(lo64 >> 32);
                v.w[2] = (uint32_t)hi64; v.w[3] = (uint32_t)(hi64 >> 32);
                lds_put(dst, v);
                break;
            }
            case MO_FDBL: {
                Fr v = lds_get(myV + op.a * VW);
                for (uint32_t t = 0; t < op.b; ++t) v = fr_add(v, v);
                lds_put(dst, v);
                break;
            }
            case MO_ISZERO: {
                const Fr v = lds_get(myV + op.a * VW);
                const bool z = fr_is_zero(v);
                // the exponentiation only where some lane needs it (honest
                // is_equal rows are all zero): a select would always run it
                Fr inv = fr_from_u64(1);
                if (__any(!z)) {
                    // word by word: `inv = z ? inv : t` on whole structs compiled
                    // to a select between two stack copies (scratch, 80 B / lane)
                    const Fr t = fr_inv(v);
#pragma unroll
                    for (int w = 0; w < 8; ++w) inv.w[w] = z ? inv.w[w] : t.w[w];
                }
                lds_put(dst, fr_from_u64(z ? 1 : 0));
                lds_put(dst + VW, inv);
                break;
            }
            case MO_POWK: {
                const uint64_t x = (uint64_t)e + op.p0;       // square-and-multiply over its bits only
                lds_put(dst, fr_pow_u64(lds_get(sK + op.a * VW), x, x ? 64 - __clzll(x) : 1));
                break;
            }
            case MO_ISQRT: {
                // bit by bit from 2^127 down: keep the bit when (y | b)^2 <= v
                const Fr v = lds_get(myV + op.a * VW);
                uint32_t y[4] = {0u, 0u, 0u, 0u};
                for (int bit = 127; bit >= 0; --bit) {
                    uint32_t c[4] = {y[0], y[1], y[2], y[3]};
                    c[bit >> 5] |= 1u << (bit & 31);
                    uint32_t sq[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        uint64_t carry = 0;
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const uint64_t t = (uint64_t)c[i] * c[j] + sq[i + j] + carry;
                            sq[i + j] = (uint32_t)t;
                            carry = t >> 32;
                        }
                        sq[i + 4] = (uint32_t)carry;
                    }
                    bool le = true;                     // sq <= v (lexicographic from the top word)
                    bool decided = false;
#pragma unroll
                    for (int w = 7; w >= 0; --w) {
                        if (!decided && sq[w] != v.w[w]) { le = sq[w] < v.w[w]; decided = true; }
                    }
                    if (le) { y[0] = c[0]; y[1] = c[1]; y[2] = c[2]; y[3] = c[3]; }
                }
                Fr r = fr_zero();
                r.w[0] = y[0]; r.w[1] = y[1]; r.w[2] = y[2]; r.w[3] = y[3];
                lds_put(dst, r);
                break;
            }
            case MO_SHR: {
                const uint32_t* s = myV + op.a * VW;    // words straight from LDS
                const uint32_t q = op.p0 >> 5, r = op.p0 & 31;
                Fr v;
#pragma unroll
                for (uint32_t t = 0; t < 8; ++t) {
                    const uint32_t lo = t + q < 8 ? s[t + q] : 0u;
                    const uint32_t hi = t + q + 1 < 8 ? s[t + q + 1] : 0u;
                    v.w[t] = r ? (lo >> r) | (hi << (32 - r)) : lo;
                }
                lds_put(dst, v);
                break;
            }
            default:
                break;
        }
    }
    }

// LDS carve of a stage block (the same for every block of a program):
// constants | element values | slot ops | micro-ops | views | half descriptors.
struct StageLds {
    uint32_t* sK;
    uint32_t* sV;
    SlotOp* sAdv;
    SlotOp* sLk;
    MicroOp* sMo;
    DView* sVw;
    uint4* sHM;
    uint32_t* sHD;
};
__device__ __forceinline__ StageLds stage_lds(const StageArgs& a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    StageLds L;
    L.sK = smem;
    L.sV = L.sK + kMaxK * VW;
    const uint32_t E = a.E ? a.E : kStageElems;
    L.sAdv = reinterpret_cast<SlotOp*>(L.sV + E * stage_elem_words(a.nv));
    L.sLk = L.sAdv + kMaxAdv;
    L.sMo = reinterpret_cast<MicroOp*>(L.sLk + kMaxLk);
    L.sVw = reinterpret_cast<DView*>(L.sMo + kMaxMicro);
    // (stage_lds_bytes counts 48 B per view, >= sizeof(DView) + the alignment slack)
    static_assert(sizeof(DView) <= 40, "DView grew: recheck stage_lds_bytes");
    // (word offsets from smem, not integer casts: a cast pointer would lose its
    // LDS address space and every table read would become a flat load)
    const uint32_t hm_off = ((uint32_t)(reinterpret_cast<uint32_t*>(L.sVw + kMaxViews) - smem) + 3u) & ~3u;
    L.sHM = reinterpret_cast<uint4*>(smem + hm_off);
    L.sHD = reinterpret_cast<uint32_t*>(L.sHM + 2 * (a.C + a.L));
    return L;
}
// A block's tables: constants, slot ops, micro-ops, views and the per (slot,
// half) descriptors and masks (no barrier).
__device__ __forceinline__ void stage_setup(const StageArgs& a, const StageLds& L,
                                            const MicroOp* __restrict__ mo, const SlotOp* __restrict__ adv,
                                            const SlotOp* __restrict__ lk, const Fr* __restrict__ K) {
    const uint32_t tid = threadIdx.x;
    for (uint32_t k = tid; k < a.nk; k += blockDim.x) lds_put(L.sK + k * VW, K[k]);
    for (uint32_t k = tid; k < a.C; k += blockDim.x) L.sAdv[k] = adv[k];
    for (uint32_t k = tid; k < a.L; k += blockDim.x) L.sLk[k] = lk[k];
    for (uint32_t k = tid; k < a.nmo; k += blockDim.x) L.sMo[k] = mo[k];
    if (tid < kMaxViews) L.sVw[tid] = a.view[tid];
    for (uint32_t k = tid; k < 2 * (a.C + a.L); k += blockDim.x) {
        const uint32_t sl = k >> 1;
        make_half(sl < a.C ? adv[sl] : lk[sl - a.C], k & 1, L.sHD + k, L.sHM + k);
    }
}
// This thread's in-bounds strided view loads of block blk's element.
struct Prefetch {
    Fr v0, v1;
    bool in0, in1;
};
__device__ __forceinline__ Prefetch stage_loads(const StageArgs& a, uint32_t blk) {
    const uint32_t E = a.E ? a.E : kStageElems;
    const uint32_t e0 = a.e_begin + blk * E;
    const uint32_t ne = min(E, a.e_end - e0), e = e0 + threadIdx.x;
    Prefetch f{fr_zero(), fr_zero(), false, false};
    if (threadIdx.x < ne) {
        const uint32_t pi = e / a.cols, pj = e - pi * a.cols;
        const DView& v0 = a.view[0];
        if (v0.ptr && v0.mode == VIEW_STRIDED && pi < v0.rows && pj < v0.cols) {
            f.v0 = ld_fr(v0.ptr + (int64_t)pi * v0.rs + (int64_t)pj * v0.cs);
            f.in0 = true;
        } else if (v0.ptr && v0.mode == VIEW_F64 && pi < v0.rows && pj < v0.cols) {
            f.v0 = quantize_fr(reinterpret_cast<const double*>(v0.ptr)[(int64_t)pi * v0.rs + (int64_t)pj * v0.cs],
                               f64_scale(v0));
            f.in0 = true;
        }
        const DView& v1 = a.view[1];
        if (v1.ptr && v1.mode == VIEW_STRIDED && pi < v1.rows && pj < v1.cols) {
            f.v1 = ld_fr(v1.ptr + (int64_t)pi * v1.rs + (int64_t)pj * v1.cs);
            f.in1 = true;
        } else if (v1.ptr && v1.mode == VIEW_F64 && pi < v1.rows && pj < v1.cols) {
            f.v1 = quantize_fr(reinterpret_cast<const double*>(v1.ptr)[(int64_t)pi * v1.rs + (int64_t)pj * v1.cs],
                               f64_scale(v1));
            f.in1 = true;
        }
    }
    return f;
}
// Phase A and phase B of block blk (tables set up; one barrier in between).
__device__ __forceinline__ void stage_chunk(const StageArgs& a, const StageLds& L, uint32_t blk,
                                            const Prefetch& f) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    const uint32_t nv = a.nv, tid = threadIdx.x;
    const uint32_t E = a.E ? a.E : kStageElems;
    const uint32_t e0 = a.e_begin + blk * E;
    const uint32_t ne = min(E, a.e_end - e0), e = e0 + tid;
    // ---- phase A: per-element micro-ops (constants / ops / views read from LDS:
    // dynamic indexing into the by-value kernel argument would go to scratch)
    if (tid < ne)
        element_program(a, e, L.sV + tid * stage_elem_words(nv), L.sK, L.sMo, L.sVw, f.v0, f.in0, f.v1, f.in1);
    __syncthreads();

    // ---- phase B: advice cells, then lookup cells
    uint4* outA = reinterpret_cast<uint4*>(a.out_adv + (uint64_t)e0 * a.C);
    uint4* outL = a.L ? reinterpret_cast<uint4*>(a.out_lk + (uint64_t)e0 * a.L) : nullptr;
    const uint32_t vb0 = (uint32_t)(L.sV - smem);
    const uint32_t rot = (a.flags & STAGE_ROT) ? blk * 37u : 0u;
    stream_cells_desc<true>(outA, 2 * ne * a.C, L.sHD, L.sHM, a.C, a.cdiv_magic, smem, vb0, nv, rot);
    if (a.L)
        stream_cells_desc<true>(outL, 2 * ne * a.L, L.sHD + 2 * a.C, L.sHM + 2 * a.C, a.L, a.ldiv_magic, smem,
                                vb0, nv, rot);
}

// One block of a stage: `a` supplies the scalar fields and the views (StageArgs
// up to `mo`), the tables come from mo / adv / lk / K (the by-value kernel
// argument of k_stage, or a record of a k_stage_multi batch); blk is the
// block's index within the stage. The view loads are issued before the table
// set-up so their latency overlaps it.
__device__ __forceinline__ void stage_block(const StageArgs& a, const MicroOp* __restrict__ mo,
                                            const SlotOp* __restrict__ adv,
                                            const SlotOp* __restrict__ lk, const Fr* __restrict__ K,
                                            uint32_t blk) {
    const StageLds L = stage_lds(a);
    const Prefetch f = stage_loads(a, blk);
    stage_setup(a, L, mo, adv, lk, K);
    __syncthreads();
    stage_chunk(a, L, blk, f);
}

__global__ __launch_bounds__(256) void k_stage(const StageArgs a) {
    stage_block(a, a.mo, a.adv, a.lk, a.K, blockIdx.x);
}

// the program of batch block g (m.blk0 ascending)
__device__ __forceinline__ uint32_t multi_prog(const StageMulti& m, uint32_t g) {
    uint32_t p = 0;
    for (uint32_t k = 1; k < m.nprog; ++k) p += g >= m.blk0[k];
    return p;
}
struct Rec {
    const StageArgs* a;
    const MicroOp* mo;
    const SlotOp* adv;
    const SlotOp* lk;
    const Fr* K;
};
__device__ __forceinline__ Rec multi_rec(const StageMulti& m, uint32_t p) {
    const uint8_t* r = m.data + m.off[p];
    Rec q;
    q.a = reinterpret_cast<const StageArgs*>(r);                     // fields up to `mo` only
    q.mo = reinterpret_cast<const MicroOp*>(r + kRecHead);
    q.adv = reinterpret_cast<const SlotOp*>(q.mo + q.a->nmo);
    q.lk = q.adv + q.a->C;
    q.K = reinterpret_cast<const Fr*>(q.lk + q.a->L);
    return q;
}

// Several independent stages in one launch (k_stage_multi): block b runs block
// b - blk0[p] of program p, whose compact record (stage_record, prog.hpp) is at
// data + off[p] -- so the small stages of a witness (single cells, d checks,
// gamma powers, is_equal rows, ...) and the phase-0 stages that read only the
// loaded matrices share one launch (one tail, one dispatch).
__global__ __launch_bounds__(256) void k_stage_multi(const StageMulti m) {
    const uint32_t p = multi_prog(m, blockIdx.x);
    const Rec q = multi_rec(m, p);
    stage_block(*q.a, q.mo, q.adv, q.lk, q.K, blockIdx.x - m.blk0[p]);
}
// Profiled stage launches (set_launch_events): the kernel's own dispatch
// records the profiler's events (hipExtLaunchKernelGGL: start on the first
// launch of the scope, stop re-recorded by every launch, so the last one's end
// counts) instead of event records between the launches, which cost a few us
// of stream time each.
static thread_local hipEvent_t tl_ev0 = nullptr, tl_ev1 = nullptr;
static thread_local bool tl_used = false;
void set_launch_events(hipEvent_t e0, hipEvent_t e1) {
    tl_ev0 = e0;
    tl_ev1 = e1;
    tl_used = false;
}
bool launch_events_used() {
    const bool u = tl_used;
    tl_ev0 = tl_ev1 = nullptr;
    tl_used = false;
    return u;
}
template <class K, class... Args>
static void launch_ev(K kernel, dim3 grid, dim3 block, uint32_t lds, hipStream_t st, Args... args) {
    if (!tl_ev1) {
        hipLaunchKernelGGL(kernel, grid, block, lds, st, args...);
        return;
    }
    hipExtLaunchKernelGGL(kernel, grid, block, lds, st, tl_used ? nullptr : tl_ev0, tl_ev1, 0, args...);
    tl_used = true;
}
hipError_t launch_stage(const StageArgs& a, hipStream_t st) {
    if (a.e_end <= a.e_begin) return hipSuccess;
    const uint32_t n = a.e_end - a.e_begin;
    const uint32_t E = a.E ? a.E : kStageElems;
    if (E > kStageElems) return hipErrorInvalidValue;
    const uint32_t lds = stage_lds_bytes(a.nv ? a.nv : 1, E, a.C + a.L);
    const uint32_t grid = (n + E - 1) / E;
    launch_ev(k_stage, dim3(grid), dim3(256), lds, st, a);
    return hipGetLastError();
}
bool stage_multi_fits(const StageArgs& a) {
    return stage_record_bytes(a.nmo, a.C, a.L, a.nk) <= kMultiBytes && (a.E ? a.E : kStageElems) <= kStageElems;
}
hipError_t launch_stage_multi(const StageArgs* const* progs, int n, hipStream_t st) {
    StageMulti m;
    uint32_t used = 0, blocks = 0, lds = 0;
    m.nprog = 0;
    const StageArgs* single = nullptr;
    // launch what is packed (a single program as a plain k_stage launch)
    auto flush = [&]() -> hipError_t {
        hipError_t e = hipSuccess;
        if (m.nprog == 1) {
            e = launch_stage(*single, st);
        } else if (m.nprog > 1) {
            m.blk0[m.nprog] = blocks;
            launch_ev(k_stage_multi, dim3(blocks), dim3(256), lds, st, m);
            e = hipGetLastError();
        }
        m.nprog = 0;
        used = blocks = lds = 0;
        return e;
    };
    for (int i = 0; i < n; ++i) {
        const StageArgs& a = *progs[i];
        if (a.e_end <= a.e_begin) continue;
        const uint32_t E = a.E ? a.E : kStageElems;
        if (E > kStageElems) return hipErrorInvalidValue;
        const uint32_t rb = stage_record_bytes(a.nmo, a.C, a.L, a.nk);
        if (rb > kMultiBytes) return hipErrorInvalidValue;
        if (m.nprog == (uint32_t)kMaxMulti || used + rb > kMultiBytes) {
            const hipError_t e = flush();
            if (e != hipSuccess) return e;
        }
        uint8_t* r = m.data + used;
        memcpy(r, &a, kRecHead);
        uint8_t* q = r + kRecHead;
        memcpy(q, a.mo, 8 * a.nmo);
        q += 8 * a.nmo;
        memcpy(q, a.adv, 4 * a.C);
        q += 4 * a.C;
        memcpy(q, a.lk, 4 * a.L);
        q += 4 * a.L;
        memcpy(q, a.K, 32 * a.nk);
        m.off[m.nprog] = used;
        m.blk0[m.nprog] = blocks;
        ++m.nprog;
        if (m.nprog == 1) single = &a;
        used += rb;
        blocks += (a.e_end - a.e_begin + E - 1) / E;
        lds = lds > stage_lds_bytes(a.nv ? a.nv : 1, E, a.C + a.L) ? lds : stage_lds_bytes(a.nv ? a.nv : 1, E, a.C + a.L);
    }
    return flush();
}

// ----------------------------------------------------------------- maxbits
__global__ __launch_bounds__(256) void k_maxbits(const DView v, uint32_t rows, uint32_t cols,
                                                 unsigned* out) {
    uint64_t n = (uint64_t)rows * cols;
    uint32_t best = 0;
    Fr zero = fr_zero();
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n;
         e += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t i = (uint32_t)(e / cols), j = (uint32_t)(e % cols);
        Fr x = view_load(v, zero, i, j);
        best = max(best, signed_bits(x));
    }
    __shared__ uint32_t wmax[4];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) best = max(best, (uint32_t)__shfl_xor((int)best, off));
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = max(max(wmax[0], wmax[1]), max(wmax[2], wmax[3]));
}

hipError_t launch_maxbits(const DView& v, uint32_t rows, uint32_t cols, unsigned* out,
                          hipStream_t st) {
    uint64_t n = (uint64_t)rows * cols;
    if (!n) return hipSuccess;
    unsigned blocks = (unsigned)((n + 255) / 256 < kMaxBitBlocks ? (n + 255) / 256 : kMaxBitBlocks);
    hipLaunchKernelGGL(k_maxbits, dim3(blocks), dim3(256), 0, st, v, rows, cols, out);
    return hipGetLastError();
}

// ---------------------------------------------------------- checker
// svdw_check_gates: the MockProver-style constraint check of a generated
// witness on the device (halo2-base's basic gate q * (a + b*c - d) = 0 at every
// enabled offset, and the lookup table [0, 2^lb)); copy constraints are not
// checked here. One thread per (unit, gate); counts via one atomic per wave.
// Checker kernels: grid-stride, per-thread counts reduced in LDS, one global
// atomic per block and counter (per-wave atomics on one address serialise).
__device__ __forceinline__ void block_flush(const uint32_t (&v)[4], unsigned long long* c0,
                                            unsigned long long* c1) {
    __shared__ unsigned long long s[4];
    if (threadIdx.x < 4) s[threadIdx.x] = 0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (v[k]) atomicAdd(&s[k], (unsigned long long)v[k]);
    __syncthreads();
    if (threadIdx.x < 2 && c0 && s[threadIdx.x]) atomicAdd(c0 + threadIdx.x, s[threadIdx.x]);
    if (threadIdx.x >= 2 && threadIdx.x < 4 && c1 && s[threadIdx.x])
        atomicAdd(c1 + threadIdx.x - 2, s[threadIdx.x]);
}
static inline unsigned check_grid(uint64_t n) {
    const uint64_t b = (n + 255) / 256;
    return (unsigned)(b < 4096 ? b : 4096);
}
__global__ __launch_bounds__(256) void k_check_cells(const Fr* __restrict__ adv, uint64_t u0, uint64_t nunits,
                                                     uint32_t unit, uint32_t cols,
                                                     const uint32_t* __restrict__ words, uint32_t nw,
                                                     ChkView v0, ChkView v1, unsigned long long* cnt) {
    uint32_t v[4] = {0, 0, 0, 0};   // gates checked / failed, copies checked / failed
    const uint64_t n = nunits * nw;
    for (uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n;
         idx += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t u = idx / nw;
        const uint32_t w = words[idx - u * nw];
        const Fr* q = adv + u * unit;
        if (chk_kind(w) == CHK_GATE) {
            const Fr* g = q + w;
            ++v[0];
            v[1] += !fr_eq(fr_add(ld_fr(g), fr_mul(ld_fr(g + 1), ld_fr(g + 2))), ld_fr(g + 3));
        } else if (chk_kind(w) == CHK_COPY) {
            ++v[2];
            v[3] += !fr_eq(ld_fr(q + chk_a(w)), ld_fr(q + chk_b(w)));
        } else {
            const ChkView vw = chk_a(w) ? v1 : v0;
            const uint64_t i = (u0 + u) / cols, j = (u0 + u) - i * cols;
            if (vw.ptr && i < vw.rows && j < vw.cols) {
                ++v[2];
                v[3] += !fr_eq(ld_fr(vw.ptr + (int64_t)i * vw.rs + (int64_t)j * vw.cs), ld_fr(q + chk_b(w)));
            }
        }
    }
    block_flush(v, cnt, cnt + 4);
}
hipError_t launch_check_cells(const Fr* adv, uint64_t u0, uint64_t nunits, uint32_t unit, uint32_t cols,
                              const uint32_t* words, uint32_t nw, ChkView v0, ChkView v1,
                              unsigned long long* cnt, hipStream_t st) {
    const uint64_t n = nunits * nw;
    if (!n) return hipSuccess;
    if (!cols) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_check_cells, dim3(check_grid(n)), dim3(256), 0, st, adv, u0,
                       nunits, unit, cols, words, nw, v0, v1, cnt);
    return hipGetLastError();
}
__global__ __launch_bounds__(256) void k_gate_bits(uint32_t* qb, uint64_t off, uint64_t n,
                                                   uint64_t unit, const uint8_t* __restrict__ ubits) {
    const uint64_t w = off / 32 + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w * 32 >= off + n) return;
    uint32_t bits = 0;
    const uint64_t i0 = w * 32;
    uint64_t o = i0 >= off ? (i0 - off) % unit : 0;
    for (int b = 0; b < 32; ++b) {
        const uint64_t i = i0 + b;
        if (i >= off && i < off + n) {
            if (ubits[o]) bits |= 1u << b;
            if (++o == unit) o = 0;
        }
    }
    if (bits) atomicOr(qb + w, bits);
}
hipError_t launch_gate_bits(uint32_t* qb, uint64_t off, uint64_t n, uint64_t unit, const uint8_t* ubits,
                            hipStream_t st) {
    if (!n) return hipSuccess;
    if (!unit) return hipErrorInvalidValue;
    const uint64_t nw = (off + n + 31) / 32 - off / 32;
    hipLaunchKernelGGL(k_gate_bits, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, st, qb, off, n, unit,
                       ubits);
    return hipGetLastError();
}
// 4 selector bytes per thread
__global__ __launch_bounds__(256) void k_selectors(uint8_t* q, const uint32_t* __restrict__ qb,
                                                   uint64_t start, uint64_t len, uint64_t rows,
                                                   bool clear_last) {
    const uint64_t r0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (r0 >= rows) return;
    uint32_t v = 0;
    for (int b = 0; b < 4; ++b) {
        const uint64_t r = r0 + b;
        if (r < len && !(clear_last && r + 1 == len)) {
            const uint64_t i = start + r;
            v |= ((qb[i >> 5] >> (i & 31)) & 1u) << (8 * b);
        }
    }
    *reinterpret_cast<uint32_t*>(q + r0) = v;
}
hipError_t launch_selectors(uint8_t* q, const uint32_t* qb, uint64_t start, uint64_t len, uint64_t rows,
                            bool clear_last, hipStream_t st) {
    if ((rows & 3) || ((uintptr_t)q & 3)) return hipErrorInvalidValue;
    if (len && !qb) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_selectors, dim3((unsigned)((rows / 4 + 255) / 256)), dim3(256), 0, st, q, qb, start,
                       len, rows, clear_last);
    return hipGetLastError();
}
__global__ __launch_bounds__(256) void k_check_physical(const Fr* __restrict__ cols,
                                                        const uint8_t* __restrict__ q, uint64_t rows,
                                                        uint32_t ncols, unsigned long long* cnt) {
    uint32_t v[4] = {0, 0, 0, 0};
    const uint64_t n = rows * ncols;
    for (uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n;
         idx += (uint64_t)gridDim.x * blockDim.x) {
        if (!q[idx]) continue;
        const uint64_t col = idx / rows, r = idx - col * rows;
        const Fr* g = cols + idx;
        ++v[0];
        v[1] += r + 3 >= rows ||
                !fr_eq(fr_add(ld_fr(g), fr_mul(ld_fr(g + 1), ld_fr(g + 2))), ld_fr(g + 3));
    }
    block_flush(v, cnt, nullptr);
}
// the break cell of column c (row bp[c]) == row 0 of column c + 1
__global__ __launch_bounds__(256) void k_check_breaks(const Fr* __restrict__ cols, uint64_t rows,
                                                      const uint64_t* __restrict__ bp, uint32_t nb,
                                                      unsigned long long* cnt) {
    uint32_t v[4] = {0, 0, 0, 0};
    for (uint32_t c = blockIdx.x * blockDim.x + threadIdx.x; c < nb; c += gridDim.x * blockDim.x) {
        ++v[0];
        v[1] += bp[c] >= rows || !fr_eq(ld_fr(cols + c * rows + bp[c]), ld_fr(cols + (c + 1) * rows));
    }
    block_flush(v, cnt, nullptr);
}
hipError_t launch_check_breaks(const Fr* cols, uint64_t rows, const uint64_t* bp, uint32_t nb,
                               unsigned long long* cnt, hipStream_t st) {
    if (!nb) return hipSuccess;
    hipLaunchKernelGGL(k_check_breaks, dim3((nb + 255) / 256), dim3(256), 0, st, cols, rows, bp, nb, cnt);
    return hipGetLastError();
}
hipError_t launch_check_physical(const Fr* cols, const uint8_t* q, uint64_t rows, uint32_t ncols,
                                 unsigned long long* cnt, hipStream_t st) {
    const uint64_t n = rows * ncols;
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_check_physical, dim3(check_grid(n)), dim3(256), 0, st, cols, q, rows,
                       ncols, cnt);
    return hipGetLastError();
}
__global__ __launch_bounds__(256) void k_check_lookups(const Fr* __restrict__ lk, uint64_t n,
                                                       uint32_t lb, unsigned long long* cnt) {
    uint32_t v[4] = {0, 0, 0, 0};
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const Fr x = ld_fr(lk + i);
        bool bad = false;
#pragma unroll
        for (int w = 0; w < 8; ++w) {
            const int keep = (int)lb - 32 * w;
            const uint32_t m = keep >= 32 ? 0u : (keep <= 0 ? 0xffffffffu : ~((1u << keep) - 1u));
            bad |= (x.w[w] & m) != 0;
        }
        ++v[0];
        v[1] += bad;
    }
    block_flush(v, cnt, nullptr);
}
// Equality lists (svdw_check_equalities) on cell stores: pair i = (source | its
// store << 62, destination); store 2 is the external value `ext` (init_rand).
// Constants: 5 words per record, (destination, canonical value).
__global__ __launch_bounds__(256) void k_check_copies(const Fr* __restrict__ s0, const Fr* __restrict__ s1,
                                                      const Fr* __restrict__ dst,
                                                      const uint64_t* __restrict__ pairs, uint64_t n,
                                                      const Fr ext, unsigned long long* cnt) {
    uint32_t v[4] = {0, 0, 0, 0};
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t src = pairs[2 * i], d = pairs[2 * i + 1];
        const uint32_t st = (uint32_t)(src >> 62);
        const uint64_t so = src & ((1ull << 62) - 1);
        const Fr a = st == 2 ? ext : ld_fr((st ? s1 : s0) + so);
        const Fr b = ld_fr(dst + d);
        ++v[0];
        v[1] += !fr_eq(a, b);
    }
    block_flush(v, cnt, nullptr);
}
__global__ __launch_bounds__(256) void k_check_consts(const Fr* __restrict__ dst,
                                                      const uint64_t* __restrict__ recs, uint64_t n,
                                                      unsigned long long* cnt) {
    uint32_t v[4] = {0, 0, 0, 0};
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t* r = recs + 5 * i;
        const Fr b = ld_fr(dst + r[0]);
        Fr k;
#pragma unroll
        for (int w = 0; w < 4; ++w) { k.w[2 * w] = (uint32_t)r[1 + w]; k.w[2 * w + 1] = (uint32_t)(r[1 + w] >> 32); }
        ++v[0];
        v[1] += !fr_eq(k, b);
    }
    block_flush(v, cnt, nullptr);
}
hipError_t launch_check_copies(const Fr* s0, const Fr* s1, const Fr* dst, const uint64_t* pairs,
                               uint64_t n, const Fr& ext, unsigned long long* cnt, hipStream_t st) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_check_copies, dim3(check_grid(n)), dim3(256), 0, st, s0, s1, dst, pairs, n,
                       ext, cnt);
    return hipGetLastError();
}
// the copy source of a region's view (engine.cpp eq_src_cell, same cases)
__device__ __forceinline__ uint64_t eq_src_dev(const EqSrcDev& e, uint64_t i, uint64_t j, uint64_t t,
                                               unsigned* err) {
    if (e.kind == 2) {                          // EQS_CHAIN
        if (t == 0) return e.first | (uint64_t)e.first_phase << 62;
        return (e.off + (t - 1) * (uint64_t)e.rs) | (uint64_t)e.phase << 62;
    }
    if (e.kind == 1) {                          // EQS_MAT
        if (e.diag_phase >= 0 && i == j) return e.diag_off | (uint64_t)e.diag_phase << 62;
        if (i < e.rows && j < e.cols)
            return (uint64_t)((int64_t)e.off + (int64_t)i * e.rs + (int64_t)j * e.cs) | (uint64_t)e.phase << 62;
        if (e.pad_phase >= 0) return e.pad_off | (uint64_t)e.pad_phase << 62;
    }
    atomicOr(err, 1u);
    return 0;
}
__global__ __launch_bounds__(256) void k_eq_records(const EqRegionDev* __restrict__ R, uint32_t nreg,
                                                    uint64_t nitems, const uint32_t* __restrict__ words,
                                                    const Fr* __restrict__ konst, uint32_t phase,
                                                    uint64_t ext_off, uint64_t* __restrict__ copies,
                                                    uint64_t* __restrict__ consts, unsigned* __restrict__ err) {
    const uint64_t me = (uint64_t)phase << 62;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < nitems;
         g += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t lo = 0, hi = nreg;                 // region: the last with item0 <= g
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (R[mid].item0 <= g) lo = mid; else hi = mid;
        }
        const EqRegionDev& r = R[lo];
        const uint64_t e = g - r.item0;
        if (r.scan) {                               // [C(0), E(a_j), E(v_j), W(s_j), ...]
            const uint64_t i = e / r.L, j = e - i * r.L, base = r.off + i * r.unit;
            if (j == 0) {
                uint64_t* k = consts + 5 * (r.const0 + i);
                k[0] = base;
                k[1] = k[2] = k[3] = k[4] = 0;
            }
            uint64_t* c = copies + 2 * (r.copy0 + 2 * (i * r.L + j));
            c[0] = eq_src_dev(r.src[0], i, j, 0, err);
            c[1] = base + 1 + 3 * j;
            c[2] = eq_src_dev(r.src[1], 0, 0, j, err);
            c[3] = base + 2 + 3 * j;
            continue;
        }
        const uint64_t base = r.off + e * r.unit, i = e / r.cols, j = e - i * r.cols;
        uint64_t* c = copies + 2 * (r.copy0 + e * r.ncw);
        uint64_t* k = consts + 5 * (r.const0 + e * r.nkw);
        for (uint32_t q = 0; q < r.nw; ++q) {
            const uint32_t w = words[r.w0 + q], a = eq_a(w), at = eq_slot(w);
            switch (eq_kind(w)) {
            case EQ_CONST: {
                const Fr v = konst[r.k0 + a];
                k[0] = base + at;
                for (int t = 0; t < 4; ++t) k[1 + t] = (uint64_t)v.w[2 * t] | (uint64_t)v.w[2 * t + 1] << 32;
                k += 5;
                break;
            }
            case EQ_LOCAL: c[0] = (base + a) | me; c[1] = base + at; c += 2; break;
            case EQ_VIEW: c[0] = eq_src_dev(r.src[a], i, j, i, err); c[1] = base + at; c += 2; break;
            default: c[0] = ext_off | 2ull << 62; c[1] = base + at; c += 2; break;   // init_rand
            }
        }
    }
}
__device__ __forceinline__ uint64_t phys_dev(const uint64_t* st, uint32_t ncol, uint32_t k, uint64_t v) {
    uint32_t lo = 0, hi = ncol;                     // upper_bound(st, v) - 1
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (st[mid] <= v) lo = mid + 1; else hi = mid;
    }
    uint32_t col = lo ? lo - 1 : 0;
    if (col > 0 && v == st[col]) --col;             // break cell: its row in the column before
    return ((uint64_t)col << k) + (v - st[col]);
}
__global__ __launch_bounds__(256) void k_eq_phys(uint64_t* __restrict__ copies, uint64_t nc,
                                                 uint64_t* __restrict__ consts, uint64_t nk,
                                                 const uint64_t* __restrict__ s0, uint32_t n0,
                                                 const uint64_t* __restrict__ s1, uint32_t n1, uint32_t phase,
                                                 uint32_t k) {
    const uint64_t* sp = phase ? s1 : s0;
    const uint32_t np = phase ? n1 : n0;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < nc + nk;
         g += (uint64_t)gridDim.x * blockDim.x) {
        if (g < nc) {
            const uint64_t src = copies[2 * g];
            const uint32_t st = (uint32_t)(src >> 62);
            if (st < 2)
                copies[2 * g] = phys_dev(st ? s1 : s0, st ? n1 : n0, k, src & ((1ull << 62) - 1)) | (uint64_t)st << 62;
            copies[2 * g + 1] = phys_dev(sp, np, k, copies[2 * g + 1]);
        } else {
            consts[5 * (g - nc)] = phys_dev(sp, np, k, consts[5 * (g - nc)]);
        }
    }
}
hipError_t launch_eq_records(const EqRegionDev* regions, uint32_t nreg, uint64_t nitems,
                             const uint32_t* words, const Fr* konst, uint32_t phase, uint64_t ext_off,
                             uint64_t* copies, uint64_t* consts, unsigned* err, hipStream_t st) {
    if (!nitems || !nreg) return hipSuccess;
    hipLaunchKernelGGL(k_eq_records, dim3(check_grid(nitems)), dim3(256), 0, st, regions, nreg, nitems, words,
                       konst, phase, ext_off, copies, consts, err);
    return hipGetLastError();
}
hipError_t launch_eq_phys(uint64_t* copies, uint64_t nc, uint64_t* consts, uint64_t nk,
                          const uint64_t* start0, uint32_t ncol0, const uint64_t* start1, uint32_t ncol1,
                          uint32_t phase, uint32_t k, hipStream_t st) {
    if (!nc && !nk) return hipSuccess;
    hipLaunchKernelGGL(k_eq_phys, dim3(check_grid(nc + nk)), dim3(256), 0, st, copies, nc, consts, nk, start0,
                       ncol0, start1, ncol1, phase, k);
    return hipGetLastError();
}
hipError_t launch_check_consts(const Fr* dst, const uint64_t* recs, uint64_t n,
                               unsigned long long* cnt, hipStream_t st) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_check_consts, dim3(check_grid(n)), dim3(256), 0, st, dst, recs, n, cnt);
    return hipGetLastError();
}
hipError_t launch_check_lookups(const Fr* lk, uint64_t n, uint32_t lb, unsigned long long* cnt,
                                hipStream_t st) {
    if (!n) return hipSuccess;
    if ((n + 255) / 256 > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_check_lookups, dim3(check_grid(n)), dim3(256), 0, st, lk, n,
                       lb, cnt);
    return hipGetLastError();
}

// ------------------------------------------------------------ vectors
// grid (ceil(L / 256), 1 + kTabSlots): y = 0 the canonical copy, y = 1 + s the
// table slot s (one Montgomery product per thread).
__device__ __forceinline__ void tab_store(Fr* wc, Fr* tab, uint32_t L, uint32_t j, uint32_t y,
                                          const Fr& v, const ScaleTab& f) {
    if (y == 0) {
        if (wc) st_fr(wc + j, v);
        return;
    }
    const uint32_t s = y - 1;
    const Fr x = mont_mul(v, f.f[s]);
    Fr* base = tab + 2ull * s * L;
    st_fr(base + j, x);
    if (s < kTabSlots - 1) st_fr(base + L + j, fr_neg(x));
}
__global__ __launch_bounds__(256) void k_vec_prep(const DView w, uint32_t L, Fr* wc, Fr* tab,
                                                  const ScaleTab f) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= L) return;
    const Fr v = view_load(w, fr_zero(), 0, j);
    tab_store(wc, tab, L, j, blockIdx.y, v, f);
}
hipError_t launch_vec_prep(const DView& w, uint32_t L, Fr* wc, Fr* tab, const ScaleTab& f,
                           hipStream_t st) {
    if (!L) return hipSuccess;
    hipLaunchKernelGGL(k_vec_prep, dim3((L + 255) / 256, 1 + kTabSlots), dim3(256), 0, st, w, L, wc,
                       tab, f);
    return hipGetLastError();
}
// g^j from the host's three Montgomery tables (depth: three products, then the
// slot's): no per-element square-and-multiply chain.
__global__ __launch_bounds__(256) void k_gamma_prep(const GammaTab g, uint32_t L, Fr* wc, Fr* tab,
                                                    const ScaleTab f, const PowCells pc) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= L) return;
    const Fr v = fr_from_mont(mont_mul(mont_mul(g.t[j & 15], g.t[16 + ((j >> 4) & 15)]), g.t[32 + (j >> 8)]));
    tab_store(wc, tab, L, j, blockIdx.y, v, f);
    if (pc.one && blockIdx.y == 0 && j < pc.d) {          // v_j = gamma^j: v_0 is the one cell
        if (j == 0) st_fr(pc.one, v);
        if (j >= 1) {                                      // element j - 1: [0, v_(j-1), gamma, v_j]
            Fr* e = pc.pows + 4ull * (j - 1);
            st_fr(e, fr_zero());
            st_fr(e + 2, pc.gamma);
            st_fr(e + 3, v);
        }
        if (j + 1 < pc.d) st_fr(pc.pows + 4ull * j + 1, v); // v_j as element j's v_(i-1)
    }
}
hipError_t launch_gamma_prep(const GammaTab& g, uint32_t L, Fr* wc, Fr* tab, const ScaleTab& f,
                             hipStream_t st, const PowCells* pc) {
    if (!L) return hipSuccess;
    if ((L + 255) / 256 > g.nhi || g.nhi > (uint32_t)kGammaTab - 32) return hipErrorInvalidValue;
    PowCells p;
    memset(&p, 0, sizeof p);
    if (pc) {
        if (pc->d > L || !pc->d) return hipErrorInvalidValue;
        p = *pc;
    }
    hipLaunchKernelGGL(k_gamma_prep, dim3((L + 255) / 256, 1 + kTabSlots), dim3(256), 0, st, g, L,
                       wc, tab, f, p);
    return hipGetLastError();
}

// -------------------------------------------------------- row inner products
// One 256-thread block per row. Chunks of 256 terms: Montgomery products
// a_j * w_j, wave shuffle scan + cross-wave LDS combine (Fr addition is
// associative, so the prefix values are exact whatever the order), cells
// [a_j, w_j, s_j] staged in LDS and written as coalesced 16 B half-cells.
__device__ __forceinline__ Fr shfl_up_fr(const Fr& v, int d) {
    Fr r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.w[i] = (uint32_t)__shfl_up((int)v.w[i], d);
    return r;
}

// Row handled by block b of a row scan. Blocks are dealt round-robin to the 8
// XCDs (b % 8); give each XCD a contiguous run of rows so that a column-strided
// view (row r of a transposed matrix = column r) finds its neighbours' 128 B
// lines in the same L2 instead of every XCD fetching them separately.
__device__ __forceinline__ uint32_t scan_row(uint32_t b, uint32_t nb) {
    return (nb & 7) ? b : (b & 7) * (nb >> 3) + (b >> 3);
}

// Inclusive wave64 scan of Fr values with DPP lane moves (GFX9 row_shr 1/2/4/8
// inside 16-lane rows, then row_bcast:15 / row_bcast:31 across rows); lanes
// without a source receive 0 (bound_ctrl / row_mask), and adding 0 is a no-op.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ Fr dpp_fr(const Fr& v) {
    Fr r;
#pragma unroll
    for (int i = 0; i < 8; ++i)
        r.w[i] = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v.w[i], CTRL, ROW_MASK, 0xf, true);
    return r;
}
__device__ __forceinline__ Fr wave_scan_fr(Fr s) {
    s = fr_add(s, dpp_fr<0x111, 0xf>(s));   // row_shr:1
    s = fr_add(s, dpp_fr<0x112, 0xf>(s));   // row_shr:2
    s = fr_add(s, dpp_fr<0x114, 0xf>(s));   // row_shr:4
    s = fr_add(s, dpp_fr<0x118, 0xf>(s));   // row_shr:8
    s = fr_add(s, dpp_fr<0x142, 0xa>(s));   // row_bcast:15 -> rows 1, 3
    s = fr_add(s, dpp_fr<0x143, 0xc>(s));   // row_bcast:31 -> rows 2, 3
    return s;
}

// Unreduced 9-word sums (values < 2^288, exact integers) for the scan network.
struct U9 {
    uint32_t w[9];
};
__device__ __forceinline__ U9 u9_from(const Fr& a) {
    U9 r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.w[i] = a.w[i];
    r.w[8] = 0;
    return r;
}
__device__ __forceinline__ U9 u9_add(const U9& a, const U9& b) {
    U9 r;
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) r.w[i] = addc32(a.w[i], b.w[i], c);
    return r;
}
__device__ __forceinline__ U9 u9_sub(const U9& a, const U9& b) {   // a >= b
    U9 r;
    uint32_t br = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) r.w[i] = subb32(a.w[i], b.w[i], br);
    return r;
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ U9 dpp_u9(const U9& v) {
    U9 r;
#pragma unroll
    for (int i = 0; i < 9; ++i)
        r.w[i] = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v.w[i], CTRL, ROW_MASK, 0xf, true);
    return r;
}
// inclusive wave scan without modular reduction (64 terms < 2^b -> < 2^(b+6))
__device__ __forceinline__ U9 wave_scan_u9(U9 s) {
    s = u9_add(s, dpp_u9<0x111, 0xf>(s));
    s = u9_add(s, dpp_u9<0x112, 0xf>(s));
    s = u9_add(s, dpp_u9<0x114, 0xf>(s));
    s = u9_add(s, dpp_u9<0x118, 0xf>(s));
    s = u9_add(s, dpp_u9<0x142, 0xa>(s));
    s = u9_add(s, dpp_u9<0x143, 0xc>(s));
    return s;
}

// T terms per thread, DPP scan. The cells go through a 24 KB LDS stage (768
// cells) in T rounds -- round q stages the 3T cells of threads [q*256/T,
// (q+1)*256/T) and the whole block writes them as coalesced 16 B half-cells --
// so four blocks fit a CU and N = 1024 rows run as one wave of blocks.
// NA < 8: |signed a| < 2^(32 NA) and wm = w * 2^(32 NA) (fr_mul_small_signed);
// NA = 8: wm is Montgomery form (any field elements).
// One launch serves up to kMaxScanJobs independent scans (blocks [blk0, blk0 + rows)
// of the grid belong to job q), so the scans of several verify_mul calls share
// one wave of blocks.
// Words of the small operand from a bit bound (host: scan_na): 8 = full Montgomery.
__device__ __forceinline__ int na_of_bits(uint32_t b) {
    if (b > 192) return 8;
    return b ? (int)((b + 31) / 32) : 1;
}
__device__ __forceinline__ int spec_na(const NaSpec& sp, const unsigned* __restrict__ W) {
    if (sp.wa == -2) return na_of_bits(sp.lk);            // host-known bound
    if (sp.wa < 0 || !W) return 8;
    uint32_t b = W[sp.wa];
    if (sp.wb >= 0) b += W[sp.wb] + sp.lk;
    return na_of_bits(b);
}
// the launch's na: the template's, or (NA = 0) the max over the jobs' specs
template <int NA>
__device__ __forceinline__ int batch_na(const ScanBatch& B) {
    if constexpr (NA != 0) {
        return NA;
    } else {
        int na = 1;
#pragma unroll
        for (int q = 0; q < kMaxScanJobs; ++q)
            if ((uint32_t)q < B.njobs) na = max(na, spec_na(B.job[q].spec, B.bitw));
        return na;
    }
}
__device__ __forceinline__ const Fr* tab_slot(const Fr* tab, uint32_t L, int na) {
    return tab + 2ull * (na >= 8 ? kTabSlots - 1 : na - 1) * L;
}
// a_j * w_j: |signed a| < 2^(32 NA): a negative value p - x has a non-zero top
// word; multiply |a| (NA words) by w * 2^(32 NA) or by its negation. NA = 8:
// Montgomery product with w's Montgomery form.
template <int NA>
__device__ __forceinline__ Fr scan_prod(const Fr& a, const Fr* __restrict__ wm,
                                        const Fr* __restrict__ wn, uint32_t j) {
    if constexpr (NA == 8) {
        return mont_mul(a, ld_fr(wm + j));
    } else {
        const bool neg = a.w[7] != 0;
        Fr mag = fr_zero();
        uint32_t br = 0;
#pragma unroll
        for (int q = 0; q < NA; ++q) {
            const uint32_t t = subb32(p_word(q), a.w[q], br);
            mag.w[q] = neg ? t : a.w[q];
        }
        return mont_mul_small<NA>(mag, ld_fr((neg ? wn : wm) + j));
    }
}
template <int NA>
__device__ __forceinline__ Fr scan_prod_rt(int na, const Fr& a, const Fr* __restrict__ wm,
                                           const Fr* __restrict__ wn, uint32_t j) {
    if constexpr (NA != 0) {
        return scan_prod<NA>(a, wm, wn, j);
    } else {
        switch (na) {          // uniform over the launch
        case 1: return scan_prod<1>(a, wm, wn, j);
        case 2: return scan_prod<2>(a, wm, wn, j);
        case 3: return scan_prod<3>(a, wm, wn, j);
        case 4: return scan_prod<4>(a, wm, wn, j);
        case 5: return scan_prod<5>(a, wm, wn, j);
        case 6: return scan_prod<6>(a, wm, wn, j);
        default: return scan_prod<8>(a, wm, wn, j);
        }
    }
}

// scan_prod with the table entries already loaded (wmv = w * 2^(32 NA) or its
// Montgomery form for NA = 8, wnv = -wmv)
template <int NA>
__device__ __forceinline__ Fr scan_prod_v(const Fr& a, const Fr& wmv, const Fr& wnv) {
    if constexpr (NA == 8) {
        return mont_mul(a, wmv);
    } else {
        const bool neg = a.w[7] != 0;
        Fr mag = fr_zero(), wv;
        uint32_t br = 0;
#pragma unroll
        for (int q = 0; q < NA; ++q) {
            const uint32_t t = subb32(p_word(q), a.w[q], br);
            mag.w[q] = neg ? t : a.w[q];
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) wv.w[q] = neg ? wnv.w[q] : wmv.w[q];
        return mont_mul_small<NA>(mag, wv);
    }
}
template <int NA>
__device__ __forceinline__ Fr scan_prod_pre(int na, const Fr& a, const Fr& wmv, const Fr& wnv) {
    if constexpr (NA != 0) {
        return scan_prod_v<NA>(a, wmv, wnv);
    } else {
        switch (na) {          // uniform over the launch
        case 1: return scan_prod_v<1>(a, wmv, wnv);
        case 2: return scan_prod_v<2>(a, wmv, wnv);
        case 3: return scan_prod_v<3>(a, wmv, wnv);
        case 4: return scan_prod_v<4>(a, wmv, wnv);
        case 5: return scan_prod_v<5>(a, wmv, wnv);
        case 6: return scan_prod_v<6>(a, wmv, wnv);
        default: return scan_prod_v<8>(a, wmv, wnv);
        }
    }
}

template <int T, int NA>
__global__ __launch_bounds__(256) void k_matvec_scan_dpp(const ScanBatch B) {
    static_assert(256 % T == 0, "T divides the block");
    constexpr uint32_t TPR = 256 / T;                     // threads staged per round
    // a staging thread's 3T cells, padded by 16 B: a lane stride of 6T + 1
    // (odd) 16 B units keeps each b128 store pass on distinct bank groups
    constexpr uint32_t RS = 6 * T + 1;
    __shared__ __attribute__((aligned(16))) uint4 stage[TPR * RS];
    __shared__ U9 wtot[4], wpre[4];
    __shared__ Fr carry_s;
    ScanJob J = B.job[0];
#pragma unroll
    for (int q = 1; q < kMaxScanJobs; ++q)
        if ((uint32_t)q < B.njobs && blockIdx.x >= B.job[q].blk0) J = B.job[q];
    const DView& A = J.A;
    const uint32_t L = J.L;
    const int na = batch_na<NA>(B);
    const Fr* __restrict__ wc = J.wc;
    const Fr* __restrict__ wm = tab_slot(J.tab, J.tl, na);
    const Fr* __restrict__ wn = wm + J.tl;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t lb = blockIdx.x - J.blk0;
    const uint32_t rb = (J.blk0 & 7) ? lb : scan_row(lb, J.rows), r = J.r_begin + rb;
    Fr* rowout = J.out + (uint64_t)rb * (3ull * L + 1);
    const Fr zero = fr_zero();
    Fr eqy = zero;                                        // is_equal's y, loaded ahead
    if (tid == 0) {
        st_fr(rowout, zero);
        carry_s = zero;
        if (J.eq_out) eqy = ld_fr(J.eq_y + (uint64_t)r * J.eq_ys);
    }
    for (uint32_t c0 = 0; c0 < L; c0 += 256 * T) {
        const uint32_t j0 = c0 + tid * T;
        // every load of the chunk issued together (the row operand, both table
        // entries, the vector's canonical cell): one memory round trip per
        // chunk instead of three dependent ones, which beside a saturating cell
        // stream cost microseconds each
        Fr a[T], w[T], tm[T], tn[T], s[T];
#pragma unroll
        for (int i = 0; i < T; ++i) {
            const uint32_t j = j0 + i;
            const bool in = j < L;
            a[i] = in ? view_load(A, zero, r, j) : zero;
            w[i] = in ? ld_fr(wc + j) : zero;
            tm[i] = in ? ld_fr(wm + j) : zero;
            tn[i] = in && na < 8 ? ld_fr(wn + j) : zero;
        }
#pragma unroll
        for (int i = 0; i < T; ++i) s[i] = j0 + i < L ? scan_prod_pre<NA>(na, a[i], tm[i], tn[i]) : zero;
        // local inclusive sums (< T p), the wave scan and the prefixes stay
        // unreduced (exact, < 2^265); each output is reduced once
        U9 loc[T];
        loc[0] = u9_from(s[0]);
#pragma unroll
        for (int i = 1; i < T; ++i) loc[i] = u9_add(loc[i - 1], u9_from(s[i]));
        const U9 tot = wave_scan_u9(loc[T - 1]);
        if (lane == 63) wtot[wave] = tot;
        __syncthreads();
        if (tid == 0) {                                   // wave prefixes and the running carry
            U9 acc = u9_from(carry_s);
#pragma unroll
            for (int w2 = 0; w2 < 4; ++w2) {
                wpre[w2] = acc;
                acc = u9_add(acc, wtot[w2]);
            }
            carry_s = reduce9(acc.w);
        }
        __syncthreads();
        const U9 pre = u9_add(u9_sub(tot, loc[T - 1]), wpre[wave]);
#pragma unroll
        for (int q = 0; q < T; ++q) {
            const uint32_t t0 = c0 + q * 256;                 // first term of this round
            if (t0 >= L) break;
            if (tid / TPR == (uint32_t)q) {
#pragma unroll
                for (int i = 0; i < T; ++i) {
                    const Fr si = reduce9(u9_add(loc[i], pre).w);
                    uint4* st3 = stage + (tid % TPR) * RS + i * 6;
                    st3[0] = make_uint4(a[i].w[0], a[i].w[1], a[i].w[2], a[i].w[3]);
                    st3[1] = make_uint4(a[i].w[4], a[i].w[5], a[i].w[6], a[i].w[7]);
                    st3[2] = make_uint4(w[i].w[0], w[i].w[1], w[i].w[2], w[i].w[3]);
                    st3[3] = make_uint4(w[i].w[4], w[i].w[5], w[i].w[6], w[i].w[7]);
                    st3[4] = make_uint4(si.w[0], si.w[1], si.w[2], si.w[3]);
                    st3[5] = make_uint4(si.w[4], si.w[5], si.w[6], si.w[7]);
                }
            }
            __syncthreads();
            const uint32_t ncell = 3 * min(256u, L - t0);
            uint4* o = reinterpret_cast<uint4*>(rowout + 1 + 3ull * t0);
            for (uint32_t hc = tid; hc < 2 * ncell; hc += 256) o[hc] = stage[hc + hc / (6 * T)];
            __syncthreads();
        }
    }
    // row-end epilogues on the row total carry_s (written before the last barrier)
    if (J.pc && tid < 1 + kTabSlots) {
        const Fr v = carry_s;
        if (tid == 0) {
            st_fr(J.pc + r, v);
        } else {
            const uint32_t sl = tid - 1;
            const Fr x = mont_mul(v, B.f.f[sl]);
            Fr* base = J.ptab + 2ull * sl * J.plen;
            st_fr(base + r, x);
            if (sl < kTabSlots - 1) st_fr(base + J.plen + r, fr_neg(x));
        }
    }
    if (J.eq_out) {
        if (tid == 0) {
            const Fr x = carry_s, y = eqy;
            const Fr d = fr_sub(x, y), one = fr_from_u64(1);
            const bool z = fr_is_zero(d);
            const Fr zf = z ? one : zero;
            Fr inv = one;
            if (!z) inv = fr_inv(d);
            const Fr cell[12] = {d, y, one, x, zf, d, inv, one, zero, d, zf, zero};
#pragma unroll
            for (int k = 0; k < 12; ++k) {
                stage[2 * k] = make_uint4(cell[k].w[0], cell[k].w[1], cell[k].w[2], cell[k].w[3]);
                stage[2 * k + 1] = make_uint4(cell[k].w[4], cell[k].w[5], cell[k].w[6], cell[k].w[7]);
            }
        }
        __syncthreads();
        if (tid < 24) reinterpret_cast<uint4*>(J.eq_out + 12ull * r)[tid] = stage[tid];
    }
}

// out[r] = sum_j A(r, j) w_j mod p for rows [0, R) (values only, no cells): the
// row-sharded witness needs every entry of b.g while it emits the b.g scan
// cells of its own rows only. One block per row; products as in the scan.
// Batched like the scans: job q owns blocks [blk0, blk0 + rows) of the grid.
template <int NA>
__global__ __launch_bounds__(256) void k_matvec_values(const ScanBatch B) {
    __shared__ U9 part[256];
    ScanJob J = B.job[0];
#pragma unroll
    for (int q = 1; q < kMaxScanJobs; ++q)
        if ((uint32_t)q < B.njobs && blockIdx.x >= B.job[q].blk0) J = B.job[q];
    const DView& A = J.A;
    const uint32_t L = J.L;
    const int na = batch_na<NA>(B);
    const Fr* __restrict__ wm = tab_slot(J.tab, J.tl, na);
    const Fr* __restrict__ wn = wm + J.tl;
    Fr* __restrict__ out = J.out;
    // rows dealt XCD-contiguously (as the scans): a transposed b's neighbouring
    // rows are neighbouring columns, one 128 B line per 4 rows in one L2
    const uint32_t lb = blockIdx.x - J.blk0;
    const uint32_t r = (J.blk0 & 7) ? lb : scan_row(lb, J.rows), tid = threadIdx.x;
    const Fr zero = fr_zero();
    U9 acc = u9_from(zero);
    for (uint32_t j = tid; j < L; j += 256) {
        const Fr a = view_load(A, zero, r, j);
        const Fr s = scan_prod_rt<NA>(na, a, wm, wn, j);
        acc = u9_add(acc, u9_from(s));                     // <= 2^13 terms of < p: < 2^267
    }
    part[tid] = acc;
    __syncthreads();
    for (uint32_t h = 128; h > 0; h >>= 1) {
        if (tid < h) part[tid] = u9_add(part[tid], part[tid + h]);
        __syncthreads();
    }
    if (tid == 0) st_fr(out + r, reduce9(part[0].w));
}
hipError_t launch_matvec_values(const ScanBatch& b0, int na, hipStream_t st) {
    ScanBatch b = b0;
    uint32_t blocks = 0;
    for (uint32_t q = 0; q < b.njobs; ++q) {
        if (b.job[q].L > 8192 || b.job[q].tl < b.job[q].L) return hipErrorInvalidValue;
        b.job[q].blk0 = blocks;
        blocks += b.job[q].L ? b.job[q].rows : 0;
        if (!b.job[q].L) b.job[q].rows = 0;
    }
    if (!blocks) return hipSuccess;
    const dim3 g(blocks), blk(256);
    switch (na) {
    case 0: hipLaunchKernelGGL(k_matvec_values<0>, g, blk, 0, st, b); break;
    case 1: hipLaunchKernelGGL(k_matvec_values<1>, g, blk, 0, st, b); break;
    case 2: hipLaunchKernelGGL(k_matvec_values<2>, g, blk, 0, st, b); break;
    case 3: hipLaunchKernelGGL(k_matvec_values<3>, g, blk, 0, st, b); break;
    case 4: hipLaunchKernelGGL(k_matvec_values<4>, g, blk, 0, st, b); break;
    case 5: hipLaunchKernelGGL(k_matvec_values<5>, g, blk, 0, st, b); break;
    case 6: hipLaunchKernelGGL(k_matvec_values<6>, g, blk, 0, st, b); break;
    default: hipLaunchKernelGGL(k_matvec_values<8>, g, blk, 0, st, b); break;
    }
    return hipGetLastError();
}

// b.g for b = X^T with X an f64 input of svd_witness (the row-sharded witness's
// b.g vector, every entry): (b.g)_i = sum_j q(X[j][i]) g^j, q = ZkMatrix::new's
// quantization done in registers (the cells of X need not exist on this rank).
// Column-parallel: thread = column i, block = (256 columns, one slice of
// rows), so every wave load is 2 KiB of one row of X (k_matvec_values reads a
// transposed view: one 32 B cell per lane, each from a different row). The
// slices' partial sums land in part[job][slice][C]; k_vec_prep_sum adds them.
__device__ __forceinline__ void quantize_mag(double x, double scale, Fr& mag, bool& neg) {
    const double s = round(fabs(x) * scale);
    mag = fr_zero();
    if (s >= 340282366920938463463374607431768211456.0) {
        mag.w[0] = mag.w[1] = mag.w[2] = mag.w[3] = 0xffffffffu;
    } else if (s > 0.0) {
        const uint64_t bits = __double_as_longlong(s);
        const int e = (int)((bits >> 52) & 0x7ff) - 1075;
        const uint64_t mant = (bits & 0xfffffffffffffull) | (1ull << 52);
        const unsigned __int128 v = e >= 0 ? ((unsigned __int128)mant << e) : (unsigned __int128)(mant >> -e);
        mag.w[0] = (uint32_t)v; mag.w[1] = (uint32_t)(v >> 32);
        mag.w[2] = (uint32_t)(v >> 64); mag.w[3] = (uint32_t)(v >> 96);
    }
    // -0.0 and negatives quantizing to 0 are the cell 0 (quantize_body)
    neg = signbit(x) && !isnan(x) && s > 0.0;
}
// Beside a saturating cell stream a memory round trip costs microseconds, so
// the kernel has three: the block's slice of the g table into LDS, every f64
// of the thread issued at once, the partial-sum store. Block = 32 columns x 8
// sub-slices of kColRows rows (one slice of 8 kColRows rows); the sub-slices
// are added in LDS, so a column has ceil(R / (8 kColRows)) partial sums.
template <int NA>
__device__ __forceinline__ U9 colsum_rows(const double (&x)[kColRows], uint32_t jl0, double scale,
                                          const Fr* sWm, const Fr* sWn) {
    U9 acc = u9_from(fr_zero());
#pragma unroll
    for (int t = 0; t < kColRows; ++t) {
        Fr mag;
        bool neg;
        quantize_mag(x[t], scale, mag, neg);
        const uint32_t jl = jl0 + t;
        Fr s;
        if constexpr (NA == 8) s = mont_mul(neg ? fr_neg(mag) : mag, sWm[jl]);
        else s = mont_mul_small<NA>(mag, neg ? sWn[jl] : sWm[jl]);
        acc = u9_add(acc, u9_from(s));                    // kColRows * 8 terms of < p
    }
    return acc;
}
__global__ __launch_bounds__(256) void k_colsum_f64(const ColBatch B, double scale) {
    constexpr uint32_t SR = 8 * kColRows;                 // rows per block
    __shared__ Fr sWm[SR], sWn[SR];
    __shared__ U9 sPart[256];
    const ColJob J = B.job[blockIdx.y];
    const uint32_t ncb = (J.C + 31) / 32, cb = blockIdx.x % ncb, sg = blockIdx.x / ncb;
    if (sg * SR >= J.R) return;                           // (grid sized for the longest job)
    const uint32_t tid = threadIdx.x, col = tid & 31, sub = tid >> 5;
    const uint32_t i = cb * 32 + col, jb = sg * SR, jl0 = sub * kColRows;
    int na = spec_na(J.spec, B.bitw);
    if (na > 4) na = 8;                                   // (quantized: <= 128 bits)
    const Fr* __restrict__ wm = tab_slot(B.tab, B.tl, na);
    const Fr* __restrict__ wn = wm + B.tl;
    double x[kColRows];
#pragma unroll
    for (int t = 0; t < kColRows; ++t) {
        const uint32_t j = jb + jl0 + t;
        x[t] = i < J.C && j < J.R ? J.x[(uint64_t)j * J.ld + i] : 0.0;
    }
    for (uint32_t k = tid; k < SR; k += 256) {            // rows past R read as 0 (x = 0 there)
        const uint32_t j = min(jb + k, J.R - 1);
        sWm[k] = ld_fr(wm + j);
        sWn[k] = na == 8 ? fr_zero() : ld_fr(wn + j);
    }
    __syncthreads();
    U9 acc;
    switch (na) {                                         // uniform over the launch
    case 1: acc = colsum_rows<1>(x, jl0, scale, sWm, sWn); break;
    case 2: acc = colsum_rows<2>(x, jl0, scale, sWm, sWn); break;
    case 3: acc = colsum_rows<3>(x, jl0, scale, sWm, sWn); break;
    case 4: acc = colsum_rows<4>(x, jl0, scale, sWm, sWn); break;
    default: acc = colsum_rows<8>(x, jl0, scale, sWm, sWn); break;
    }
    sPart[tid] = acc;
    __syncthreads();
    if (sub == 0 && i < J.C) {
#pragma unroll
        for (int k = 1; k < 8; ++k) acc = u9_add(acc, sPart[tid + 32 * k]);   // < 2^267 + 2^264
        st_fr(J.part + (uint64_t)sg * J.C + i, reduce9(acc.w));
    }
}
uint32_t colsum_slices(uint32_t R) { return (R + 8 * kColRows - 1) / (8 * kColRows); }
hipError_t launch_colsum_f64(const ColBatch& b, int precision_bits, hipStream_t st) {
    if (!b.njobs || b.njobs > (uint32_t)kMaxColJobs) return hipErrorInvalidValue;
    uint32_t blocks = 0;
    for (uint32_t q = 0; q < b.njobs; ++q) {
        const ColJob& j = b.job[q];
        if (!j.R || j.R > b.tl || j.R > 8192 || j.ld < j.C) return hipErrorInvalidValue;
        blocks = max(blocks, (j.C + 31) / 32 * colsum_slices(j.R));
    }
    if (!blocks) return hipSuccess;
    hipLaunchKernelGGL(k_colsum_f64, dim3(blocks, b.njobs), dim3(256), 0, st, b,
                       (double)(1ull << precision_bits));
    return hipGetLastError();
}
// w_j = sum_s part[s L + j] -> canonical copy and scaled table (as k_vec_prep);
// a thread's loads are issued kColPartBatch at a time
__global__ __launch_bounds__(256) void k_vec_prep_sum(const Fr* __restrict__ part, uint32_t S, uint32_t L,
                                                      Fr* wc, Fr* tab, const ScaleTab f) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= L) return;
    Fr v = fr_zero();
    for (uint32_t s0 = 0; s0 < S; s0 += kColPartBatch) {
        Fr p[kColPartBatch];
#pragma unroll
        for (int s = 0; s < kColPartBatch; ++s)
            p[s] = s0 + s < S ? ld_fr(part + (uint64_t)(s0 + s) * L + j) : fr_zero();
#pragma unroll
        for (int s = 0; s < kColPartBatch; ++s) v = fr_add(v, p[s]);
    }
    tab_store(wc, tab, L, j, blockIdx.y, v, f);
}
// k_vec_prep_sum over the jobs of a batch (block x: job by blk0 ranges)
__global__ __launch_bounds__(256) void k_vec_prep_sum_multi(const VecPrepBatch b, const ScaleTab f) {
    uint32_t q = 0;
#pragma unroll
    for (int k = 1; k < kMaxColJobs; ++k) q += (uint32_t)k < b.njobs && blockIdx.x >= b.job[k].blk0;
    const Fr* part = b.job[0].part;
    uint32_t S = b.job[0].S, L = b.job[0].L, b0 = b.job[0].blk0;
    Fr* wc = b.job[0].wc;
    Fr* tab = b.job[0].tab;
#pragma unroll
    for (int k = 1; k < kMaxColJobs; ++k)                 // selects, not a dynamic index into the argument
        if (q == (uint32_t)k) {
            part = b.job[k].part; S = b.job[k].S; L = b.job[k].L; b0 = b.job[k].blk0; wc = b.job[k].wc;
            tab = b.job[k].tab;
        }
    const uint32_t j = (blockIdx.x - b0) * blockDim.x + threadIdx.x;
    if (j >= L) return;
    Fr v = fr_zero();
    for (uint32_t s0 = 0; s0 < S; s0 += kColPartBatch) {
        Fr p[kColPartBatch];
#pragma unroll
        for (int s = 0; s < kColPartBatch; ++s)
            p[s] = s0 + s < S ? ld_fr(part + (uint64_t)(s0 + s) * L + j) : fr_zero();
#pragma unroll
        for (int s = 0; s < kColPartBatch; ++s) v = fr_add(v, p[s]);
    }
    tab_store(wc, tab, L, j, blockIdx.y, v, f);
}
hipError_t launch_vec_prep_sum_multi(const VecPrepBatch& b0, const ScaleTab& f, hipStream_t st) {
    if (!b0.njobs || b0.njobs > (uint32_t)kMaxColJobs) return hipErrorInvalidValue;
    VecPrepBatch b = b0;
    uint32_t blocks = 0;
    for (uint32_t q = 0; q < b.njobs; ++q) {
        if (!b.job[q].S) return hipErrorInvalidValue;
        b.job[q].blk0 = blocks;
        blocks += (b.job[q].L + 255) / 256;
    }
    for (uint32_t q = b.njobs; q < (uint32_t)kMaxColJobs; ++q) b.job[q].blk0 = ~0u;
    if (!blocks) return hipSuccess;
    hipLaunchKernelGGL(k_vec_prep_sum_multi, dim3(blocks, 1 + kTabSlots), dim3(256), 0, st, b, f);
    return hipGetLastError();
}
hipError_t launch_vec_prep_sum(const Fr* part, uint32_t S, uint32_t L, Fr* wc, Fr* tab, const ScaleTab& f,
                               hipStream_t st) {
    if (!L) return hipSuccess;
    if (!S) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_vec_prep_sum, dim3((L + 255) / 256, 1 + kTabSlots), dim3(256), 0, st, part, S, L,
                       wc, tab, f);
    return hipGetLastError();
}

hipError_t launch_scan_batch(const ScanBatch& b0, int na, hipStream_t st) {
    ScanBatch b = b0;
    uint32_t blocks = 0;
    for (uint32_t q = 0; q < b.njobs; ++q) {
        if (b.job[q].tl < b.job[q].L) return hipErrorInvalidValue;
        b.job[q].blk0 = blocks;
        blocks += b.job[q].L ? b.job[q].rows : 0;
        if (!b.job[q].L) b.job[q].rows = 0;
    }
    if (!blocks) return hipSuccess;
    const dim3 g(blocks), blk(256);
    switch (na) {                      // two terms per thread (T = 2)
    case 0: hipLaunchKernelGGL((k_matvec_scan_dpp<2, 0>), g, blk, 0, st, b); break;
    case 1: hipLaunchKernelGGL((k_matvec_scan_dpp<2, 1>), g, blk, 0, st, b); break;
    case 2: hipLaunchKernelGGL((k_matvec_scan_dpp<2, 2>), g, blk, 0, st, b); break;
    case 3: hipLaunchKernelGGL((k_matvec_scan_dpp<2, 3>), g, blk, 0, st, b); break;
    case 4: hipLaunchKernelGGL((k_matvec_scan_dpp<2, 4>), g, blk, 0, st, b); break;
    case 5: hipLaunchKernelGGL((k_matvec_scan_dpp<2, 5>), g, blk, 0, st, b); break;
    case 6: hipLaunchKernelGGL((k_matvec_scan_dpp<2, 6>), g, blk, 0, st, b); break;
    default: hipLaunchKernelGGL((k_matvec_scan_dpp<2, 8>), g, blk, 0, st, b); break;
    }
    return hipGetLastError();
}
hipError_t launch_matvec_scan(const DView& A, uint32_t r_begin, uint32_t r_end, uint32_t L,
                              const Fr* wc, const Fr* tab, uint32_t tl, Fr* out, int na, hipStream_t st) {
    if (r_end <= r_begin || !L) return hipSuccess;
    if (tl < L) return hipErrorInvalidValue;
    ScanBatch b;
    memset(&b, 0, sizeof b);
    b.njobs = 1;
    b.job[0] = ScanJob{A, wc, tab, tl, out, L, r_end - r_begin, 0, r_begin, NaSpec{-1, -1, 0, 0}};
    b.bitw = nullptr;
    return launch_scan_batch(b, na, st);
}

}  // namespace svdw
