// Host-side launchers for the exact field product kernels in gemm.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fr.hpp"
#include "prog.hpp"

namespace svdw {

// Balanced base-256 digit planes of X (rows x kdim): out[row][kg][D] int32 words,
// each packing the digit of 4 consecutive k. rows_pad/kg_pad are zero-filled.
hipError_t launch_to_digits(const DView& x, uint32_t rows, uint32_t kdim, int D,
                            uint32_t rows_pad, uint32_t kg_pad, uint32_t* out, hipStream_t st);
// c_s[i][j] = sum_k A[i][k] * Bt[j][k] exactly, written as canonical Fr to
// out[i*ors + j*ocs]. sym: A == Bt (upper tiles + mirror).
hipError_t launch_gemm_digits(int DA, int DB, bool sym, const uint32_t* Ad, const uint32_t* Bd,
                              uint32_t N, uint32_t M, uint32_t kg_pad, Fr* out, int64_t ors,
                              int64_t ocs, hipStream_t st);
bool gemm_digits_supported(int DA, int DB);
// Matrix-core variant: digit planes laid out [row][kc][D][64 B] (kc = 64-k chunks).
// dbits (nullable, one word): take D from this device-side bit-length maximum
// instead (5 / 8 / 9 planes; nothing written when wider than 9 digits).
hipError_t launch_to_digits_mf(const DView& x, uint32_t rows, uint32_t kdim, int D, uint32_t rows_pad,
                               uint32_t kcn, uint32_t* out, hipStream_t st,
                               const unsigned* dbits = nullptr);
hipError_t launch_gemm_mfma(int DA, int DB, bool sym, const uint8_t* Ad, const uint8_t* Bd,
                            uint32_t N, uint32_t M, uint32_t kcn, Fr* out, int64_t ors,
                            int64_t ocs, hipStream_t st);
// Same product with DA / DB decided on the device from bit-length words (planes
// laid out for those counts by launch_to_digits_mf with the same words); a
// no-op when either operand is wider than 9 digits.
hipError_t launch_gemm_mfma_rt(bool sym, const uint8_t* Ad, const uint8_t* Bd, uint32_t N,
                               uint32_t M, uint32_t kcn, Fr* out, int64_t ors, int64_t ocs,
                               const unsigned* bits_a, const unsigned* bits_b, hipStream_t st);
// Generic Montgomery GEMM (any field elements): out = A(NxK) * B(KxM). With
// bit-length words, a no-op unless an operand is too wide for the digit GEMM.
// crt_lk >= 0: the skip test is the CRT GEMM's (ceil(log2 K) = crt_lk).
hipError_t launch_gemm_mont(const DView& A, const DView& B, uint32_t N, uint32_t K, uint32_t M,
                            Fr* out, int64_t ors, int64_t ocs, hipStream_t st,
                            const unsigned* bits_a = nullptr, const unsigned* bits_b = nullptr,
                            int crt_lk = -1);
// Multi-modular exact GEMM (device-decided modulus count from bits_a / bits_b,
// no-op when an operand exceeds 128 bits). Residue planes of X: out =
// [kCrtMaxResidues][rows_pad][kpad] int8 (rows_pad % 128 == 0, kpad % 64 == 0).
// bits_c (nullable): also cover the product (c, c), so the planes can be reused.
hipError_t launch_to_residues(const DView& x, uint32_t rows, uint32_t kdim, uint32_t rows_pad,
                              uint32_t kpad, uint32_t* out, const unsigned* bits_a,
                              const unsigned* bits_b, uint32_t lk, hipStream_t st,
                              const unsigned* bits_c = nullptr);
// Residue planes of up to kMaxResSegs f64 matrices (row-major, row pitch ld),
// each as k_to_residues would build them from its quantized cells: planes
// [n][rows_pad][kw] u32 words (4 x int8 per word, kw * 4 >= cols), rows >= rows
// and k >= cols zero; n = max over the segment's pairs p (wa[p] >= 0) of the CRT
// modulus count of a product with operand bits W[wa[p]], W[wb[p]] and K <= 2^lk[p].
static constexpr int kMaxResSegs = 4;
// tr: element (row, k) is in[k * ld + row] (the planes of a transposed operand:
// b^T of verify_mul_witness's b), threads laid along rows so the reads coalesce.
struct ResSeg {
    const double* in;
    uint32_t* out;
    uint32_t rows, cols, ld, rows_pad, kw;
    int16_t wa[2], wb[2];
    uint32_t lk[2];
    uint32_t tr;
};
struct ResSegs {
    ResSeg seg[kMaxResSegs];
    uint32_t blk0[kMaxResSegs + 1];   // set by the launcher
    uint32_t nseg;
};
hipError_t launch_residues_f64(const ResSegs& q, const unsigned* W, int precision_bits,
                               hipStream_t st);
// c_s = A * Bt from residue planes Ar (plane stride astride rows, from the A rows'
// first row) and Br (bstride): N x M; R is the residue scratch
// (crt_scratch_bytes(N, M) bytes).
hipError_t launch_gemm_crt(bool sym, const uint8_t* Ar, const uint8_t* Br, uint32_t N, uint32_t M,
                           uint32_t astride, uint32_t bstride, uint32_t kpad, uint8_t* R, Fr* out,
                           int64_t ors, int64_t ocs, const unsigned* bits_a,
                           const unsigned* bits_b, uint32_t lk, hipStream_t st, uint32_t kern = 0);
// Debug: record the CRT GEMM's block timeline into buf (3 u64 per block; null: off).
hipError_t set_debug_trace(void* buf);
static constexpr int kCrtMaxResidues = 40;   // = kCrtMaxMod (crt_tables.hpp)
// Several CRT products in one GEMM launch and one combine launch (the three
// products of check_svd_phase0; launch_gemm_crt is the one-job case). The GEMM's
// (job, modulus, tile) units are placed modulus-major per XCD. Per job the caller sets Ar, Br,
// astride, bstride, kpad, R (its own residue scratch), out, ors, ocs, N, M,
// bits_a, bits_b, lk and sym (A == B: upper tiles + mirror); the launcher
// fills the tile and block fields.
static constexpr int kMaxCrtJobs = 3;
static constexpr uint32_t CT_TILE = 128;   // CRT GEMM output tile edge (gemm.hip CT)
struct CrtJob {
    const uint8_t* Ar;
    const uint8_t* Br;
    uint8_t* R;
    Fr* out;
    const unsigned* bits_a;
    const unsigned* bits_b;
    int64_t ors, ocs;
    uint32_t astride, bstride, kpad, N, M, lk, sym;
    uint32_t tiles_a, tiles_m, nblk, cblk0;
    // tiles [tile0, tile0 + tcount) of the job's tile sequence only (tcount 0:
    // all): a row block of a product (SYM: the upper tiles of rows of tiles
    // [b0, b1), whose mirrors land in later rows)
    uint32_t tile0, tcount;
};
struct CrtBatch {
    CrtJob job[kMaxCrtJobs];
    uint32_t njobs;
    // GEMM kernel (bit-identical): 0 one block per (tile, modulus) unit
    // (k_gemm_crt_multi), 1 a persistent grid whose blocks' chunk pipelines
    // run across their units (k_gemm_crt_pers; jobs of one kpad >= 512), 2
    // 256 x 128 tiles (k_gemm_crt_wide; non-symmetric whole jobs), 3 wide
    // from 64 tile pairs on, else persistent (products queued on their own)
    uint32_t kern;
};
// R sized crt_scratch_bytes per job
hipError_t launch_gemm_crt_multi(const CrtBatch& b, hipStream_t st);
// residue scratch R one CRT product of N x M needs
size_t crt_scratch_bytes(uint32_t N, uint32_t M);

}  // namespace svdw
