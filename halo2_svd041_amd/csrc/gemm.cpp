// Host side of the exact field product c_s = a * b (field_mat_mul, kernels: gemm.hip):
// which kernels a product runs, the plane geometry they share and the launches.
// engine.cpp keeps the cells, a witness call's bookkeeping and every scheduling decision.
#include <math.h>

#include <algorithm>

#include "engine_internal.hpp"
#include "gemm.hpp"

// Largest inner dimension of the integer GEMMs: |acc| <= K 2^14 <= 2^27 (int8 products;
// the bias in k_gemm_crt and the nine digit diagonals of an i32 sum rest on it).
const uint32_t kCrtMaxK = 8192;

// ------------------------------------------------------------------- rules
bool crt_product(const svdw_ctx* c, uint32_t K) { return c->opt.gemm_crt && K <= kCrtMaxK; }
bool crt_product_f64(const svdw_ctx* c, uint32_t K) {
    return c->opt.res_f64 && c->opt.gemm_impl == SVDW_GEMM_MFMA && crt_product(c, K);
}
bool products_on_cell_stream(const svdw_ctx* c) {
    return c->opt.prod_cell > 0 || (c->opt.prod_cell < 0 && sharded(c));
}
// CrtBatch::kern; "gemm_kern" -1: wide tiles or the persistent grid for a product
// queued on its own (gemm_solo, never set inside a witness call), else one block per unit
static uint32_t crt_kern(const svdw_ctx* c) {
    return c->opt.gemm_kern >= 0 ? (uint32_t)c->opt.gemm_kern : (c->gemm_solo ? 3u : 0u);
}
// Balanced base-256 digits needed for |x| < 2^bits.
static int digits_for_bits(uint32_t bits) {
    for (int D = 1; D <= 16; ++D) {
        // max representable magnitude 127 * (256^D - 1) / 255 >= 2^bits - 1 ?
        long double maxv = 127.0L * (powl(256.0L, D) - 1.0L) / 255.0L;
        if (maxv >= powl(2.0L, bits) - 1.0L) return D;
    }
    return 99;
}
static int round_digits(int need) {
    if (need <= 5) return 5;
    if (need <= 8) return 8;
    if (need <= 9) return 9;
    return 0;
}
bool is_transpose_of(const svdw_mat& b, const svdw_mat& a) {
    return a.phase == b.phase && a.off == b.off && a.rows == b.cols && a.cols == b.rows &&
           a.rs == b.cs && a.cs == b.rs;
}
std::vector<uint32_t> maxbits_many(svdw_ctx* c, const std::vector<svdw_mat>& ms) {
    std::vector<uint32_t> out(ms.size(), 0);
    if (c->dry || ms.empty()) return out;
    settle(c);                                  // a pipelined witness's row scans read c->bits
    const size_t words = ms.size() * kMaxBitBlocks;
    ensure_buf(c, c->bits, words * sizeof(unsigned));
    std::vector<uint32_t> nb(ms.size());
    for (size_t i = 0; i < ms.size(); ++i) {
        const uint64_t n = (uint64_t)ms[i].rows * ms[i].cols;
        nb[i] = (uint32_t)std::min<uint64_t>((n + 255) / 256, kMaxBitBlocks);
        hipck(launch_maxbits(view_of(c, ms[i]), ms[i].rows, ms[i].cols,
                             (unsigned*)c->bits.p + i * kMaxBitBlocks, c->st), "k_maxbits");
    }
    std::vector<unsigned> h(words);
    hipck(hipMemcpyAsync(h.data(), c->bits.p, words * sizeof(unsigned), hipMemcpyDeviceToHost,
                         c->st), "D2H");
    sync(c);
    for (size_t i = 0; i < ms.size(); ++i)
        for (uint32_t b = 0; b < nb[i]; ++b) out[i] = std::max(out[i], h[i * kMaxBitBlocks + b]);
    return out;
}

// ---------------------------------------------------------------- geometry
// Residue planes of an operand of `rows` rows and inner dimension K:
// [kCrtMaxResidues][rows_pad][kpad] int8, whole 128-row tiles (plus the caller's
// slack rows) of whole groups of four 64-k chunks.
struct CrtGeom { uint32_t kpad, rows_pad, lk; size_t bytes; };
static CrtGeom crt_geom(uint32_t rows, uint32_t K, uint32_t slack_rows = 0) {
    const uint32_t kpad = ceil_to(K, 256), rp = ceil_to(rows, 128) + slack_rows;
    return CrtGeom{kpad, rp, clog2(K), (size_t)kCrtMaxResidues * rp * kpad};
}
// One matrix of a k_residues_f64 launch: rows x cols of `in` (row pitch ld; tr:
// its transpose) into `out`, covering the products (W[wa], W[wb], K <= 2^lk) of `pairs`.
struct ResPair { int wa, wb; uint32_t lk; };
static void add_res_seg(ResSegs& q, const double* in, uint32_t rows, uint32_t cols, uint32_t ld, uint32_t tr,
                        const CrtGeom& geom, const DBuf& out, std::initializer_list<ResPair> pairs) {
    ResSeg& g = q.seg[q.nseg++];
    g.in = in; g.out = (uint32_t*)out.p;
    g.rows = rows; g.cols = cols; g.ld = ld; g.rows_pad = geom.rows_pad; g.kw = geom.kpad / 4; g.tr = tr;
    g.wa[0] = g.wa[1] = g.wb[0] = g.wb[1] = -1;
    int k = 0;
    for (const ResPair& pr : pairs) { g.wa[k] = (int16_t)pr.wa; g.wb[k] = (int16_t)pr.wb; g.lk[k] = pr.lk; ++k; }
}
// The step every path starts with: planes of a (digA), then planes of b^T (bb)
// unless the product is symmetric, where a's serve both sides. make(x, buf, side)
// sizes buf and queues the planes of x's rows (side 1: the b operand).
// a_in_bb / b_ready: those planes are in bb already (the CRT path's reuse).
struct Planes { const void *a, *b; };
template <class Make>
static Planes operand_planes(svdw_ctx* c, const svdw_mat& a, const svdw_mat& b, bool sym, DBuf& bb, Make&& make,
                             bool a_in_bb = false, bool b_ready = false) {
    if (!a_in_bb) make(a, c->digA, 0);
    const void* pa = a_in_bb ? bb.p : c->digA.p;
    if (sym) return Planes{pa, pa};
    if (!b_ready) make(transposed(b), bb, 1);
    return Planes{pa, bb.p};
}

// ------------------------------------------------------- gemm_exec's paths
// Multi-modular path: residue planes, one int8 GEMM per modulus, CRT.
static void gemm_crt(svdw_ctx* c, hipStream_t s, const svdw_mat& a, const svdw_mat& b, bool sym, Fr* out,
                     const unsigned* sa, const unsigned* sb, bool quantized, const unsigned* b_cover,
                     bool a_from_b, DBuf& BB, bool b_ready) {
    const uint32_t N = a.rows, K = a.cols, M = b.cols;
    const CrtGeom ga = crt_geom(N, K), gb = crt_geom(M, K);
    const uint32_t lk = ga.lk;
    ensure_buf(c, c->crtR, crt_scratch_bytes(N, M));
    const Planes p = operand_planes(c, a, b, sym, BB, [&](const svdw_mat& x, DBuf& buf, int side) {
        const CrtGeom& g = side ? gb : ga;
        ensure_buf(c, buf, g.bytes);
        ProfScope ps(c, s, "k_to_residues", 32.0 * x.rows * K, 0);
        hipck(launch_to_residues(view_of(c, x), x.rows, K, g.rows_pad, g.kpad, (uint32_t*)buf.p, sa,
                                 side || !sym ? sb : sa, lk, s, side ? b_cover : nullptr), "k_to_residues");
    }, a_from_b && sym, b_ready);
    {
        ProfScope ps(c, s, std::string("k_gemm_crt") + (sym ? ":s" : ""), 32.0 * N * M, (double)N * M * K);
        hipck(launch_gemm_crt(sym, (const uint8_t*)p.a, (const uint8_t*)p.b, N, M, ga.rows_pad,
                              sym ? ga.rows_pad : gb.rows_pad, ga.kpad, (uint8_t*)c->crtR.p, out, M, 1, sa,
                              sym ? sa : sb, lk, s, crt_kern(c)), "k_gemm_crt");
    }
    if (!quantized)
        hipck(launch_gemm_mont(view_of(c, a), view_of(c, b), N, K, M, out, M, 1, s, sa,
                               sym ? sa : sb, (int)lk), "k_gemm_mont");
}
// Balanced base-256 digit planes, DA x DB of them, on the matrix cores (mfma: a
// row is 64-k chunks of 64 B per plane) or on v_dot4c_i32_i8 (groups of 4 k in
// a u32, eight per stage). sa, sb (both or neither; mfma): the plane counts are
// decided on the device from these words, nine planes sized, and the Montgomery
// kernel takes over, on the device's word too, when an operand needs more.
static void gemm_digits(svdw_ctx* c, hipStream_t s, const svdw_mat& a, const svdw_mat& b, bool sym, Fr* out,
                        bool mfma, int DA, int DB, const unsigned* sa = nullptr, const unsigned* sb = nullptr) {
    const uint32_t N = a.rows, K = a.cols, M = b.cols, npad = ceil_to(N, 32), mpad = ceil_to(M, 32);
    const uint32_t ku = mfma ? (K + 63) / 64 : ceil_to((K + 3) / 4, 8);   // a row's units, of ub bytes per plane
    const double ub = mfma ? 64.0 : 4.0;
    const char* planes = mfma ? "k_to_digits_mf" : "k_to_digits";
    const Planes p = operand_planes(c, a, b, sym, c->digB, [&](const svdw_mat& x, DBuf& buf, int side) {
        const uint32_t rp = side ? mpad : npad;
        const int D = side ? DB : DA;
        ensure_buf(c, buf, (size_t)rp * ku * D * (size_t)ub);
        ProfScope ps(c, s, planes, 32.0 * x.rows * K + ub * rp * ku * D, 0);
        hipck(mfma ? launch_to_digits_mf(view_of(c, x), x.rows, K, D, rp, ku, (uint32_t*)buf.p, s, side ? sb : sa)
                   : launch_to_digits(view_of(c, x), x.rows, K, D, rp, ku, (uint32_t*)buf.p, s), planes);
    });
    if (sa) {
        {
            ProfScope ps(c, s, std::string("k_gemm_mfma:rt") + (sym ? "s" : ""), 32.0 * N * M, (double)N * M * K);
            hipck(launch_gemm_mfma_rt(sym, (const uint8_t*)p.a, (const uint8_t*)p.b, N, M, ku, out, M, 1, sa,
                                      sym ? sa : sb, s), "k_gemm_mfma_rt");
        }
        hipck(launch_gemm_mont(view_of(c, a), view_of(c, b), N, K, M, out, M, 1, s, sa, sym ? sa : sb), "k_gemm_mont");
        return;
    }
    ProfScope ps(c, s, std::string(mfma ? "k_gemm_mfma:" : "k_gemm_dot4:") + std::to_string(DA) + "x" +
                           std::to_string(DB) + (sym ? "s" : ""),
                 ub * ku * ((double)npad * DA + (sym ? 0.0 : (double)mpad * DB)) + 32.0 * N * M, (double)N * M * K);
    hipck(mfma ? launch_gemm_mfma(DA, DB, sym, (const uint8_t*)p.a, (const uint8_t*)p.b, N, M, ku, out, M, 1, s)
               : launch_gemm_digits(DA, DB, sym, (const uint32_t*)p.a, (const uint32_t*)p.b, N, M, ku, out, M, 1, s),
          mfma ? "k_gemm_mfma" : "k_gemm_dot4");
}
// field_mat_mul (src/matrix/mod.rs:510-537) on stream `s`: c_s = a * b written
// as canonical cells at `out` (row-major). Exact: residue or balanced base-256
// digit planes and integer GEMMs when the entries are small, else Montgomery
// per MAC. With device bit-length words (sa, sb: one word each) the modulus or
// digit counts are read by the kernels themselves and the host needs no operand
// bounds. quantized: both operands are ZkMatrix::new cells (|x| < 2^128 by the
// u128 saturation), so the CRT path always applies and no fallback is queued.
// CRT path residue reuse (prelaunched products of check_svd_phase0): b_cover
// makes b's planes (kept in digB) also valid for the product (b, b); a_from_b
// takes a's planes from digB (a is that b) instead of recomputing them.
// bbuf: where b's planes live (default digB); b_ready: they are already there
// (row-sharded v.v^T after m.v^T: same b, planes built with b_cover).
void gemm_exec(svdw_ctx* c, hipStream_t s, const svdw_mat& a, const svdw_mat& b, Fr* out,
               uint32_t bits_a, uint32_t bits_b, const unsigned* sa, const unsigned* sb, bool quantized,
               const unsigned* b_cover, bool a_from_b, DBuf* bbuf, bool b_ready) {
    const uint32_t N = a.rows, K = a.cols, M = b.cols;
    const bool sym = is_transpose_of(b, a);
    if (!sa && !sb && crt_product(c, K) && c->opt.gemm_impl == SVDW_GEMM_MFMA && bits_a <= 128 &&
        bits_b <= 128 && !c->dry) {
        // host-known bounds: hand them to the CRT kernels as device words
        // (stream-ordered memsets, one pair per stream)
        const int slot = s == c->st2 ? 2 : 0;
        ensure_buf(c, c->gbits, 4 * sizeof(unsigned));
        unsigned* w = (unsigned*)c->gbits.p + slot;
        hipck(hipMemsetD32Async((hipDeviceptr_t)w, bits_a, 1, s), "hipMemsetD32Async");
        hipck(hipMemsetD32Async((hipDeviceptr_t)(w + 1), bits_b, 1, s), "hipMemsetD32Async");
        sa = w;
        sb = w + 1;
    }
    if (sa && sb && crt_product(c, K))
        return gemm_crt(c, s, a, b, sym, out, sa, sb, quantized, b_cover, a_from_b, bbuf ? *bbuf : c->digB, b_ready);
    if (sa && sb && K <= kCrtMaxK) return gemm_digits(c, s, a, b, sym, out, true, 9, 9, sa, sb);
    const int DA = round_digits(digits_for_bits(bits_a)), DB = round_digits(digits_for_bits(bits_b));
    if (DA && DB && K <= kCrtMaxK && gemm_digits_supported(DA, DB))
        return gemm_digits(c, s, a, b, sym, out, c->opt.gemm_impl == SVDW_GEMM_MFMA, DA, DB);
    ProfScope ps(c, s, "k_gemm_mont", 32.0 * ((double)N * K + (double)K * M + (double)N * M), (double)N * M * K);
    hipck(launch_gemm_mont(view_of(c, a), view_of(c, b), N, K, M, out, M, 1, s), "k_gemm_mont");
}

// -------------------------------- the three products of check_svd_phase0
// A[g] * B[g] (B = transposes; m.v^T, u.u^T, v.v^T) from residue planes built in
// one k_residues_f64 launch over svd_witness's f64 inputs: m (this rank's rows)
// into digA, v into digB (covering m.v^T and v.v^T), u into digC. Planes of v
// and u carry 128 rows of slack so a row block (sharded rank) reads its A tiles
// as a slice of the full planes.
struct SvdPlanes { uint64_t r0[3], r1[3]; CrtGeom g[3]; };   // this rank's rows of product g; planes of m's rows, u, v
static SvdPlanes svd_planes(const svdw_ctx* c, const svdw_mat (&A)[3]) {
    const uint32_t N = A[0].rows, M = A[0].cols;
    SvdPlanes p;
    for (int g = 0; g < 3; ++g) {
        p.r0[g] = 0; p.r1[g] = A[g].rows;
        if (sharded(c)) shard_rows(c, A[g].rows, &p.r0[g], &p.r1[g]);
    }
    p.g[0] = crt_geom(std::max((uint32_t)(p.r1[0] - p.r0[0]), 1u), M);
    p.g[1] = crt_geom(N, N, 128);
    p.g[2] = crt_geom(M, M, 128);
    return p;
}
// The residue planes; W: the device bit-length words of m, u, v.
void svd_residues_f64(svdw_ctx* c, const svdw_mat (&A)[3], const unsigned* W, hipStream_t pst) {
    const uint32_t N = A[0].rows, M = A[0].cols;
    const SvdPlanes p = svd_planes(c, A);
    const uint32_t rows_m = (uint32_t)(p.r1[0] - p.r0[0]), lkM = p.g[2].lk, lkN = p.g[1].lk;
    ensure_buf(c, c->digA, p.g[0].bytes);
    ensure_buf(c, c->digB, p.g[2].bytes);
    ensure_buf(c, c->digC, p.g[1].bytes);
    ResSegs q;
    memset(&q, 0, sizeof q);
    if (rows_m) add_res_seg(q, c->call.svd_f64[0] + p.r0[0] * M, rows_m, M, M, 0, p.g[0], c->digA, {{0, 2, lkM}});
    add_res_seg(q, c->call.svd_f64[2], M, M, M, 0, p.g[2], c->digB, {{0, 2, lkM}, {2, 2, lkM}});
    add_res_seg(q, c->call.svd_f64[1], N, N, N, 0, p.g[1], c->digC, {{1, 1, lkN}});
    ProfScope ps(c, pst, "k_residues_f64", 8.0 * ((double)rows_m * M + (double)M * M + (double)N * N), 0);
    hipck(launch_residues_f64(q, W, (int)c->P, pst), "k_residues_f64");
}
// The three GEMMs in one launch and the three combines in one (each product
// its own residue scratch): one step of the chain instead of three (512^2 P=32
// 0.43 -> 0.41 ms, 1024^2 P=63 2.10 -> 2.07 ms; row-sharded ranks too). log[g]:
// the products' stream offsets.
void svd_products_f64(svdw_ctx* c, const svdw_mat (&A)[3], const svdw_mat (&B)[3],
                      const std::vector<uint64_t>& log, uint32_t phase, const unsigned* W, hipStream_t pst) {
    const SvdPlanes p = svd_planes(c, A);
    const uint8_t* P[3] = {(const uint8_t*)c->digA.p, (const uint8_t*)c->digC.p,
                           (const uint8_t*)c->digB.p};                 // A planes of m, u, v
    const int wa[3] = {0, 1, 2}, wb[3] = {2, 1, 2};
    CrtBatch b;
    memset(&b, 0, sizeof b);
    size_t rbytes[3], rtot = 0;
    for (int g = 0; g < 3; ++g) {
        rbytes[g] = crt_scratch_bytes(std::max<uint32_t>((uint32_t)(p.r1[g] - p.r0[g]), 1), B[g].cols);
        rtot += rbytes[g];
    }
    ensure_buf(c, c->crtR, rtot);
    size_t roff = 0;
    double bytes = 0, ops = 0;
    for (int g = 0; g < 3; ++g) {
        const uint32_t rows = (uint32_t)(p.r1[g] - p.r0[g]), cols = B[g].cols;
        if (rows) {
            const CrtGeom& ga = p.g[g];
            CrtJob& q = b.job[b.njobs++];
            q.Ar = P[g] + (g == 0 ? 0 : p.r0[g] * (uint64_t)ga.kpad);
            q.Br = g == 0 ? (const uint8_t*)c->digB.p : P[g];
            q.R = (uint8_t*)c->crtR.p + roff;
            q.out = cellp(c, phase, log[g] + p.r0[g] * cols);
            q.bits_a = W + wa[g]; q.bits_b = W + wb[g];
            q.ors = cols; q.ocs = 1;
            q.astride = ga.rows_pad; q.bstride = g == 0 ? p.g[2].rows_pad : ga.rows_pad;
            q.kpad = ga.kpad; q.N = rows; q.M = cols; q.lk = ga.lk;
            q.sym = !sharded(c) && g > 0;
            bytes += 32.0 * rows * cols;
            ops += (double)rows * cols * A[g].cols;
        }
        roff += rbytes[g];
    }
    b.kern = crt_kern(c);
    if (b.njobs) {
        ProfScope ps(c, pst, "k_gemm_crt:multi", bytes, ops);
        hipck(launch_gemm_crt_multi(b, pst), "k_gemm_crt_multi");
    }
}

// ------------------------------------------ verify_mul_witness's product
// c_s = a * b (N x K by K x M, row-major f64 inputs on the device): residue
// planes of a and b^T straight from them (one launch), then the GEMM and
// combine, all on `s`. dbits: the device bit-length words of a and b.
void product_f64(svdw_ctx* c, hipStream_t s, const double* a, const double* b, uint32_t N, uint32_t K,
                 uint32_t M, Fr* out, const unsigned* dbits) {
    const CrtGeom ga = crt_geom(N, K), gb = crt_geom(M, K);
    ensure_buf(c, c->digA, ga.bytes);
    ensure_buf(c, c->digB, gb.bytes);
    ensure_buf(c, c->crtR, crt_scratch_bytes(N, M));
    ResSegs q;
    memset(&q, 0, sizeof q);
    add_res_seg(q, a, N, K, K, 0, ga, c->digA, {{0, 1, ga.lk}});
    add_res_seg(q, b, M, K, M, 1, gb, c->digB, {{0, 1, ga.lk}});   // b^T(j, k) = b[k * M + j]
    {
        ProfScope ps(c, s, "k_residues_f64", 8.0 * ((double)N * K + (double)K * M), 0);
        hipck(launch_residues_f64(q, dbits, (int)c->P, s), "k_residues_f64");
    }
    ProfScope ps(c, s, "k_gemm_crt", 32.0 * N * M, (double)N * M * K);
    hipck(launch_gemm_crt(false, (const uint8_t*)c->digA.p, (const uint8_t*)c->digB.p, N, M, ga.rows_pad,
                          gb.rows_pad, ga.kpad, (uint8_t*)c->crtR.p, out, M, 1, dbits, dbits + 1, ga.lk, s,
                          crt_kern(c)), "k_gemm_crt");
}
