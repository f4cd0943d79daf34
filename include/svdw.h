/*
 * svdw.h — C ABI of the MI355X-native SVD-verify witness engine.
 *
 * Drop-in boundary for the witness path of neilcouture/halo2-svd041: every
 * entry point replaces one reference function that appends BN254-Fr cells to
 * a halo2-base `Context` (citations: reference repo paths). Values are the
 * canonical little-endian 32-byte cells (halo2curves `Fr::to_repr`), stored
 * device-resident in per-phase advice / lookup streams owned by the context.
 * Handles (svdw_mat / svdw_vec) are plain views (offset + strides) into a
 * phase's advice stream, valid for the context's lifetime — the analogue of
 * `Vec<Vec<AssignedValue<F>>>` (src/matrix/mod.rs:219-223), with transpose a
 * stride swap (src/matrix/mod.rs:408-419).
 *
 * Errors: every call returns SVDW_OK or a negative code and never aborts; the
 * reference panics (assert!/assert_eq!) on the same conditions
 * (src/matrix/mod.rs:86,142,175,239,307-310,515,580,616; src/svd/mod.rs:50-61).
 * svdw_last_error() gives the thread-local message of the last failure.
 * Threading: one context = one `&mut Context` per phase; not thread safe.
 * Work is enqueued on the context's HIP stream; svdw_sync() waits for it.
 */
#ifndef SVDW_H
#define SVDW_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SVDW_OK 0
#define SVDW_EINVAL -1   /* shape / argument mismatch (reference: assert! panic) */
#define SVDW_ERANGE -2   /* unsupported precision / lookup bits / bound */
#define SVDW_EDEVICE -3  /* HIP runtime error */
#define SVDW_ENOMEM -4

typedef struct svdw_ctx svdw_ctx;

typedef struct {
    int device;               /* HIP device ordinal (-1: host-only planning context) */
    uint32_t precision_bits;  /* FixedPointChip041 PRECISION_BITS, 1..63 */
    uint32_t lookup_bits;     /* RangeChip lookup_bits (LOOKUP_BITS env), 8..63 */
} svdw_params;

/* View of cells of one phase's advice stream:
 * cell(i, j) = stream[phase][off + i*rs + j*cs]. */
typedef struct {
    uint32_t phase;
    uint32_t rows, cols;
    uint64_t off;
    int64_t rs, cs;
} svdw_mat;

typedef struct {
    uint32_t phase;
    uint32_t len;
    uint64_t off;
    int64_t stride;
} svdw_vec;

/* check_svd_phase0's return tuple (src/svd/mod.rs:42-48,115). */
typedef struct {
    svdw_mat u_t, v_t, m_times_vt, u_times_ut, v_times_vt;
} svdw_svd_payload;

/* Constants of the example caller (examples/svd_example.rs:115-118,149,160). */
typedef struct {
    double max_norm;    /* MAX_NORM = 100.0 */
    double eps_svd;     /* EPS_SVD = 1e-10 */
    double eps_u;       /* EPS_U = 1e-10 */
    uint32_t max_bits_d;/* 30 */
} svdw_svd_config;

/* Cell totals of one SVD witness (phase 0 + phase 1). */
typedef struct {
    uint64_t advice0, advice1, lookup0, lookup1;
} svdw_counts;

/* ---------------------------------------------------------------- context */
int svdw_ctx_create(const svdw_params* params, svdw_ctx** out);
int svdw_ctx_destroy(svdw_ctx* ctx);
/* Drop all cells of both phases (allocations are kept). */
int svdw_ctx_reset(svdw_ctx* ctx);
/* Pre-size a phase's advice / lookup streams (cells). */
int svdw_reserve(svdw_ctx* ctx, uint32_t phase, uint64_t advice_cells, uint64_t lookup_cells);
int svdw_sync(svdw_ctx* ctx);
/* Stream ordering with the caller's own HIP stream (hipStream_t as void*; e.g.
 * torch.cuda.current_stream().cuda_stream). The context runs on streams of its
 * own and does NOT see work queued elsewhere: device memory an on_device call
 * reads (f64 inputs, device text) or writes (parse outputs) must be complete
 * / free when the call's work starts. Either synchronize the producing stream
 * first, or call svdw_stream_wait(ctx, producer) before the call: the
 * context's streams then wait (on the device, no host wait) for everything
 * queued on `stream` so far. svdw_stream_signal(ctx, consumer) after a call
 * makes `stream` wait for everything the context has queued (its outputs).
 * The Python layer (halo2_svd041_amd.zk) does both around every on-device call
 * with torch's current stream.
 *
 * Lifetime of device inputs. An on_device call returns before the device has
 * read its inputs: with "pipeline" (svd_witness) the call's stage kernels and
 * row scans read m, u, v, d straight from the f64 buffers after it returned,
 * and with "lanes" (verify_mul_witness) the call runs beside the next one. The
 * caller must keep every input buffer allocated and unmodified until the
 * call's work has completed: svdw_sync(), or svdw_query() returning 1, or any
 * stream ordered after svdw_stream_signal(ctx, stream) (a caching allocator
 * that frees on that stream). The Python layer holds a reference to every
 * device input tensor until a completion mark (svdw_mark, below) after its
 * call, or sync / reset / close, shows the work done. */
int svdw_stream_wait(svdw_ctx* ctx, void* stream);
/* 1 when everything queued on the context (both lanes) has completed, 0 while
 * some of it still runs (no host wait), < 0 on error. */
int svdw_query(svdw_ctx* ctx);
/* Completion marks: svdw_mark records how far the context's work is queued
 * (an event on each of its streams behind what is queued there; no stream
 * waits) and returns a ticket. svdw_mark_done(ticket) is 1 once everything
 * queued before the mark has completed, 0 while some of it runs (no host
 * wait), < 0 on error; svdw_mark_wait(ticket) waits for it on the host. The
 * last 16 marks are kept; an older ticket is answered by the mark that reused
 * its slot (done implies done; otherwise 0). (svdw_stream_signal onto a side
 * stream does the same job, but with 4 hardware queues per process that
 * stream may share a queue with one of the context's streams, whose later
 * work then waits behind the side stream's wait.) */
int svdw_mark(svdw_ctx* ctx, uint64_t* ticket);
int svdw_mark_done(svdw_ctx* ctx, uint64_t ticket);
int svdw_mark_wait(svdw_ctx* ctx, uint64_t ticket);
/* Debug: the CRT GEMM's block timeline into device buffer buf (3 u64 per block:
 * start and end on the 100 MHz wall clock, XCC id << 32 | HW_ID); null: off. */
int svdw_debug_trace(void* buf);
int svdw_stream_signal(svdw_ctx* ctx, void* stream);
const char* svdw_last_error(void);

/* ------------------------------------------------------ stream access */
uint64_t svdw_advice_len(const svdw_ctx* ctx, uint32_t phase);
uint64_t svdw_lookup_len(const svdw_ctx* ctx, uint32_t phase);
/* Device pointers to the canonical 32-byte cells (valid until the next append). */
const void* svdw_advice_device_ptr(const svdw_ctx* ctx, uint32_t phase);
const void* svdw_lookup_device_ptr(const svdw_ctx* ctx, uint32_t phase);
/* Copy cells [off, off+n) to host memory (4 x u64 little endian per cell); syncs. */
int svdw_copy_advice(svdw_ctx* ctx, uint32_t phase, uint64_t off, uint64_t n, uint64_t* out);
int svdw_copy_lookup(svdw_ctx* ctx, uint32_t phase, uint64_t off, uint64_t n, uint64_t* out);

/* ------------------------------------------------------------- read-out
 * Cells in the form the consumer holds them, converted on the device while
 * they are read (no host pass over the witness). These calls read the cells
 * the handle currently shows (the latest call's set under "pipeline", the
 * latest state under "lanes"), as svdw_copy_advice does, and work on a
 * row-sharded context (they export whatever the range holds). SVDW_EINVAL: a
 * null pointer, an unknown form, a range outside the stream, a view outside its
 * phase's stream, a planning context ("planning context has no cells"). */
#define SVDW_FORM_CANONICAL  0   /* Fr::to_repr, what the streams hold */
#define SVDW_FORM_MONTGOMERY 1   /* halo2curves' in-memory Fr([u64;4]): x * 2^256 mod p, 4 LE u64 */
/* Cells [off, off+n) of the advice (lookup = 0) or lookup (1) stream of `phase`,
 * in `form`, into DEVICE memory dst (n * 32 B). Queued on the context behind
 * everything queued so far, no host wait; order the consumer with
 * svdw_stream_signal or a mark. */
int svdw_export_cells(svdw_ctx* ctx, uint32_t phase, int lookup, uint64_t off, uint64_t n, int form,
                      void* dst);
/* The same into HOST memory; waits. Staged through at most 2 x 64 MiB of device
 * scratch whatever n is (chunk k + 1 converts while chunk k copies out); a
 * canonical range is copied straight from the stream. */
int svdw_copy_cells(svdw_ctx* ctx, uint32_t phase, int lookup, uint64_t off, uint64_t n, int form,
                    uint64_t* out);
/* Gather a view, row-major dense (rows*cols resp. len cells of 32 B), into
 * device memory (on_device: queued, no host wait) or host memory (waits).
 * Negative strides are allowed; a transpose is a stride swap. */
int svdw_export_mat(svdw_ctx* ctx, const svdw_mat* a, int form, void* dst, int on_device);
int svdw_export_vec(svdw_ctx* ctx, const svdw_vec* v, int form, void* dst, int on_device);
/* ZkMatrix::dequantize / ZkVector::dequantize (src/matrix/mod.rs:50-58,257-270):
 * rows*cols resp. len f64, row-major, FixedPointChip041::dequantization of every
 * cell for the context's PRECISION_BITS. The chip's source (zk_fixed_point_chip,
 * git HEAD) is not available offline, so the construction is PARITY UNPINNED:
 *   x is negative iff x > (p-1)/2; mag = x, or p - x when negative;
 *   m = mag mod 2^128 (get_lower_128); S = 2^P;
 *   result = +-((m / S as f64) + (m % S as f64) / (S as f64)),
 * every `as f64` being Rust's u128 -> f64 (round to nearest even), the sum one
 * f64 addition; zero gives +0.0. Host and device agree bit for bit. */
int svdw_dequantize_mat(svdw_ctx* ctx, const svdw_mat* a, double* out, int on_device);
int svdw_dequantize_vec(svdw_ctx* ctx, const svdw_vec* v, double* out, int on_device);
/* Host helpers, no context, no GPU: n values between forms (in may equal out;
 * an input >= p in either form is SVDW_EINVAL and nothing is written), and the
 * chip's scalar quantization (ZkMatrix::new's: round half away of |x| 2^P as
 * u128, saturating, NaN -> 0, negative -> p - x_q) / dequantization (above) for
 * P = precision_bits in [1, 63] (else SVDW_ERANGE). */
int svdw_fr_convert(const uint64_t* in, uint64_t n, int from, int to, uint64_t* out);
int svdw_quantization(double x, uint32_t precision_bits, uint64_t out[4]);
int svdw_dequantization(const uint64_t value[4], uint32_t precision_bits, double* out);

/* ------------------------------------------- ZkMatrix / ZkVector (matrix/mod.rs) */
/* ZkMatrix::new (src/matrix/mod.rs:230-252): quantize + load_witness, row-major.
 * data: rows*cols f64 (host memory, or device memory if on_device). */
int svdw_zkmatrix_new(svdw_ctx* ctx, uint32_t phase, const double* data, uint32_t rows,
                      uint32_t cols, int on_device, svdw_mat* out);
/* ZkVector::new (src/matrix/mod.rs:29-40). */
int svdw_zkvector_new(svdw_ctx* ctx, uint32_t phase, const double* data, uint32_t len,
                      int on_device, svdw_vec* out);
/* ZkMatrix::transpose_matrix (src/matrix/mod.rs:408-419): no cells. */
int svdw_transpose_matrix(const svdw_mat* a, svdw_mat* out);
/* Context::load_witness / load_constant of one canonical value (halo2-base). */
int svdw_load_witness(svdw_ctx* ctx, uint32_t phase, const uint64_t value[4], svdw_vec* out);
int svdw_load_constant(svdw_ctx* ctx, uint32_t phase, const uint64_t value[4], svdw_vec* out);

/* ZkVector::entries_less_than (src/matrix/mod.rs:185-194). */
int svdw_entries_less_than(svdw_ctx* ctx, const svdw_vec* d, uint32_t max_bits);
/* ZkVector::entries_in_desc_order (src/matrix/mod.rs:199-215). */
int svdw_entries_in_desc_order(svdw_ctx* ctx, const svdw_vec* d, uint32_t max_bits);

/* check_mat_entries_bounded (src/matrix/mod.rs:490-501): |a_ij| < bnd.
 * bnd: unsigned 256-bit little endian (BigUint). */
int svdw_check_mat_entries_bounded(svdw_ctx* ctx, const svdw_mat* a, const uint64_t bnd[4]);
/* check_mat_diff (src/matrix/mod.rs:441-457): |a_ij - b_ij| < tol. */
int svdw_check_mat_diff(svdw_ctx* ctx, const svdw_mat* a, const svdw_mat* b,
                        const uint64_t tol[4]);
/* check_mat_id (src/matrix/mod.rs:461-483): |a_ij - scalar_id*I_ij| < tol. */
int svdw_check_mat_id(svdw_ctx* ctx, const svdw_mat* a, const svdw_vec* scalar_id,
                      const uint64_t tol[4]);
/* mat_times_diag_mat (src/matrix/mod.rs:610-627): a[i][j]*v[j], j < len(v). */
int svdw_mat_times_diag_mat(svdw_ctx* ctx, const svdw_mat* a, const svdw_vec* v, svdw_mat* out);
/* FixedPointChip041::signed_div_scale constants. The chip's source
 * (zk_fixed_point_chip, git HEAD) is not available offline, so its layout is
 * PARITY UNPINNED; the engine emits the parameterised construction
 *   add(x, 2^S) ; RangeChip::div_mod(t, 2^P, NB) ; sub(q, 2^(S-P))
 * (div_mod = [r, 2^P, q, t] + check_big_less_than_safe(q, 2^NB/2^P + 1)
 *  + check_big_less_than_safe(r, 2^P)), i.e. floor(x / 2^P) for |x| < 2^S.
 * Zero fields (or a null pointer) select S = 3P (the domain rescale_matrix's
 * doc states, src/matrix/mod.rs:350-353) and NB = max(4P + 1, S + 1) (NB = S + 1
 * is the tightest sound choice; a shift alone never makes the default NB
 * invalid). NB = 4P + 1 is the choice that reproduces the
 * reference's own cell counts: 90 cells per element at P = 32, LOOKUP_BITS = 12
 * ("#CONSTRAINTS = 90", src/matrix/mod.rs:102; "~94 (when lookup_bits = 12)",
 * :348) and 60-90 for P = 32 across LOOKUP_BITS 12-24, more for P > 32
 * (README.md:51: "60N^2 - 100N^2, depends on LB; higher for P>32"); NB = 3P + 1
 * gives 72 at P = 32, LB = 12. Both stay parity unpinned. */
typedef struct {
    uint32_t shift_bits;
    uint32_t num_bits;
} svdw_div_scale;
/* ZkMatrix::rescale_matrix (src/matrix/mod.rs:354-375): signed_div_scale of
 * every c_s entry, row-major, into c_s's phase; out = the quotient cells. */
int svdw_rescale_matrix(svdw_ctx* ctx, const svdw_mat* c_s, const svdw_div_scale* cfg,
                        svdw_mat* out);
/* ZkVector::inner_product (src/matrix/mod.rs:79-106): gate.inner_product(x, self)
 * then signed_div_scale; out = 1-element vector. */
int svdw_zkvector_inner_product(svdw_ctx* ctx, uint32_t phase, const svdw_vec* self,
                                const svdw_vec* x, const svdw_div_scale* cfg, svdw_vec* out);
/* ZkVector::_norm_square (src/matrix/mod.rs:112-119) = inner_product(self, self);
 * ZkVector::_dist_square (src/matrix/mod.rs:135-148): per-entry qsub (gate.sub)
 * then _norm_square of the differences. */
int svdw_zkvector_norm_square(svdw_ctx* ctx, uint32_t phase, const svdw_vec* self,
                              const svdw_div_scale* cfg, svdw_vec* out);
int svdw_zkvector_dist_square(svdw_ctx* ctx, uint32_t phase, const svdw_vec* self,
                              const svdw_vec* x, const svdw_div_scale* cfg, svdw_vec* out);
/* ZkVector::norm / dist (src/matrix/mod.rs:124-131, 156-164): _norm_square /
 * _dist_square then FixedPointChip041::qsqrt. The chip (zk_fixed_point_chip,
 * git HEAD) is not available, so qsqrt is a parameterised, constraint-checked
 * construction, PARITY UNPINNED: y = floor(sqrt(a 2^P)) for a in [0, 2^B)
 * (B = sqrt_bits, 0 -> 2P): load_witness(y), range_check(y, ny), t = mul(a, 2^P),
 * d = sub(t, mul(y, y)), range_check(d, ny + 1), f = sub(mul(y, 2), d),
 * range_check(f, ny + 1), ny = ceil((B + P) / 2) + 1; out = the y cell. */
int svdw_zkvector_norm(svdw_ctx* ctx, uint32_t phase, const svdw_vec* self, const svdw_div_scale* cfg,
                       uint32_t sqrt_bits, svdw_vec* out);
int svdw_zkvector_dist(svdw_ctx* ctx, uint32_t phase, const svdw_vec* self, const svdw_vec* x,
                       const svdw_div_scale* cfg, uint32_t sqrt_bits, svdw_vec* out);
/* ZkVector::mul (src/matrix/mod.rs:169-182): inner_product with every row of a. */
int svdw_zkvector_mul(svdw_ctx* ctx, uint32_t phase, const svdw_vec* self, const svdw_mat* a,
                      const svdw_div_scale* cfg, svdw_vec* out);
/* honest_prover_mat_mul (src/matrix/mod.rs:546-568): c_s = a*b over Fr, loaded row-major. */
int svdw_honest_prover_mat_mul(svdw_ctx* ctx, uint32_t phase, const svdw_mat* a,
                               const svdw_mat* b, svdw_mat* c_s);
/* field_mat_vec_mul (src/matrix/mod.rs:574-599): one inner_product per row of a;
 * out = the row results (last cell of each row block). */
int svdw_field_mat_vec_mul(svdw_ctx* ctx, uint32_t phase, const svdw_mat* a, const svdw_vec* v,
                           svdw_vec* out);
/* ZkMatrix::verify_mul (src/matrix/mod.rs:299-342), Freivalds with v = (1, g, g^2, ...);
 * gamma: canonical init_rand value (rlc.gamma_pow_cached()[0]). */
int svdw_verify_mul(svdw_ctx* ctx, uint32_t phase, const svdw_mat* a, const svdw_mat* b,
                    const svdw_mat* c_s, const uint64_t gamma[4]);

/* ------------------------------------------------------------ svd (svd/mod.rs) */
/* err_calc (src/svd/mod.rs:155-163). */
int svdw_err_calc(uint32_t p, uint64_t size, double max_norm, double eps_svd, double eps_u,
                  double* err_svd, double* err_u);
/* check_svd_phase0 (src/svd/mod.rs:32-116), appending to phase 0. */
int svdw_check_svd_phase0(svdw_ctx* ctx, const svdw_mat* m, const svdw_mat* u, const svdw_mat* v,
                          const svdw_vec* d, double err_svd, double err_u, uint32_t max_bits_d,
                          svdw_svd_payload* out);
/* check_svd_phase1 (src/svd/mod.rs:127-144), appending to phase 1. */
int svdw_check_svd_phase1(svdw_ctx* ctx, const svdw_mat* m, const svdw_mat* u, const svdw_mat* v,
                          const svdw_svd_payload* payload, const uint64_t gamma[4]);

/* Whole SVD-verify witness of examples/svd_example.rs:98-200 (intended
 * one-context semantics): reset, ZkMatrix::new(m,u,v), ZkVector::new(d),
 * err_calc(P, max(N,M), ...), check_svd_phase0 into phase 0, then
 * check_svd_phase1 into phase 1. m: N x M, u: N x N, v: M x M, d: min(N,M),
 * all row-major f64 (device memory if on_device). */
int svdw_svd_witness(svdw_ctx* ctx, const double* m, const double* u, const double* v,
                     const double* d, uint32_t N, uint32_t M, int on_device,
                     const svdw_svd_config* cfg, const uint64_t gamma[4], svdw_counts* counts);
/* The README.md:32-46 recipe as one call (BASELINE config 2): reset,
 * ZkMatrix::new(a) (N x K), ZkMatrix::new(b) (K x M), c_s =
 * honest_prover_mat_mul(a, b) into phase 0, ZkMatrix::verify_mul(a, b, c_s,
 * gamma) (src/matrix/mod.rs:299-342) into phase 1; the same cells as those four
 * modular calls, without host waits. a, b row-major f64 (device memory if
 * on_device). */
int svdw_verify_mul_witness(svdw_ctx* ctx, const double* a, const double* b, uint32_t N, uint32_t K,
                            uint32_t M, int on_device, const uint64_t gamma[4], svdw_counts* counts);
/* svdw_verify_mul_witness with device inputs, ordered after the work queued
 * so far on the caller's stream `stream` (svdw_stream_wait inside the call, on
 * the context state that runs it -- with "lanes" 2 the other one): one call
 * and one hand-off wait instead of two calls and a wait per state. */
int svdw_verify_mul_witness_on(svdw_ctx* ctx, void* stream, const double* a, const double* b, uint32_t N,
                               uint32_t K, uint32_t M, const uint64_t gamma[4], svdw_counts* counts);
/* Exact integer GEMM of honest_prover_mat_mul (the integer sum of quantized
 * products, reduced mod p once). Matrix-core paths (SVDW_GEMM_MFMA, default):
 *   - multi-modular / CRT (option "gemm_crt" 1, default): balanced residues
 *     modulo n pairwise coprime moduli <= 256 (n from the operand bit lengths:
 *     19 for m.v^T at P = 63), one int8 v_mfma_i32_16x16x64_i8 GEMM per
 *     modulus, CRT reconstruction; operands up to 2^128, K <= 8192;
 *   - balanced base-256 digit planes with i32 digit-pair diagonal sums
 *     ("gemm_crt" 0), operands up to ~2^71.
 * SVDW_GEMM_VALU: the digit planes on v_dot4c_i32_i8. All paths are
 * bit-identical; wider operands use a Montgomery GEMM. The environment
 * variable SVDW_GEMM=valu selects the VALU path at create. */
#define SVDW_GEMM_MFMA 0
#define SVDW_GEMM_VALU 1
int svdw_set_gemm_impl(svdw_ctx* ctx, int impl);
/* Options (svdw_set_option; 22 names; any other name is SVDW_EINVAL). Tuning
 * knobs, bit-identical results
 * for every value, defaults first:
 *   "gemm_impl" 0 | 1; "gemm_crt" 1 | 0 (CRT or digit-plane matrix-core GEMM);
 *   "overlap" 1 | 0 (the three check_svd_phase0 products run ahead on a second
 *   stream); "phase1_overlap" 1 | 2 | 0 (svd_witness: phase 1 runs on the
 *   second stream behind the products / on a third stream from quantization
 *   on, its c_s scans waiting for the products / after phase 0; 1 acts as 2 on
 *   a row-sharded context and when max(N, M) < 1024); "p1_at" -1 | 0 | 1 | 2 | 3
 *   (with phase 1 on the third stream: queued after the first 0 / 1 / 2
 *   phase-0 stages, 3 after all of phase 0; -1: 0 on a rank of a >= 4-way shard, 3 of a
 *   2-3-way shard, else 1);
 *   "stage_elems" 256 (elements per stage block, multiple of 16 in [16, 256]);
 *   "commit_window_bits" 0 | 2..16 (svdw_commit's window instead of
 *   svdw_commit_plan's, a tuning aid; the result reports what was used);
 *   "commit_scratch_mib" 1024 | 1..65536 (svdw_commit's workspace cap per batch
 *   of (column, window) tasks, MiB; one task always runs; svdw_fixed_base_mul
 *   and svdw_srs_setup size their pieces by it too, and so do svdw_g1_mul
 *   and the stages of svdw_g1_fft, whose planned window also depends on it);
 *   "g1_window_bits" 0 | 2..6 (svdw_g1_fft's window instead of the planned one,
 *   a tuning aid; the result reports what was used);
 *   "srs_chunk_rows" 0 | 1..2^28 (svdw_srs_setup works through that many rows
 *   at a time instead of what fits "commit_scratch_mib", a testing aid; the
 *   result reports what was used);
 *   "place_trials" 6 | 0..8 (a cell stream of >= 256 MiB allocated from now on
 *   is chosen among that many placements in HBM by timing the stage kernels'
 *   store pattern on each; 0 or 1: the first one);
 *   "stage_rot" 1 | 0 (a stage block writes its chunk of cells from a
 *   block-dependent 4 KiB window on, wrapping around, instead of from its
 *   start, so that blocks started together write different window offsets);
 *   "f64_views" 1 | 0 (svd_witness / verify_mul_witness with device inputs:
 *   stages and row scans read the loaded matrices from the f64 inputs,
 *   quantized in registers, instead of waiting for the quantized cells);
 *   "res_f64" 1 | 0 (svd_witness with inputs in HBM: the CRT residue planes of
 *   m, u, v built from the f64 inputs in one launch, or from the quantized cells);
 *   "stage_batch" 1 | 0 (independent stages share k_stage_multi launches: the
 *   u / v bounds and u.d, the d checks and constant cells, verify_mul's one cells
 *   and gamma powers, the is_equal rows; split automatically where a stage reads
 *   cells a pending one writes); "prod_cell" 1 | 0 | -1 (svd_witness with
 *   device inputs: the products on the cell stream and the u / v bounds and u.d
 *   beside them; -1 on row-sharded contexts only);
 *   "pipeline" 1 | 0 (svd_witness with device inputs on the f64 CRT product
 *   path with the products on the cell stream, when the second cell set is
 *   already allocated or its growth fits in the device's free memory with 10 %
 *   of the device to spare -- else the call runs unpipelined and the second set
 *   is released, as it is by "pipeline" 0: consecutive calls overlap -- a call returns with its
 *   u.d / bound / diff stages and its phase-1 row scans still running on the
 *   second and third streams, and the next call's gamma tables, quantization
 *   and products start on the cell stream beside them, into the other cell
 *   set and tables; any other call on the context, a copy and svdw_sync wait
 *   for that tail);
 *   "lanes" 2 | 1 (svdw_verify_mul_witness with device inputs: 2 alternates
 *   between two complete context states, exchanged behind the handle at each
 *   call, so consecutive calls run beside each other on separate streams; the
 *   handle always shows the latest call's cells; svdw_sync, stream_wait /
 *   _signal, graph_stats and destroy cover both states; a call stays on the
 *   current state when the other one would have to grow beyond the device's
 *   free memory less 10 % of the device);
 *   "graph" 1 | 0: svdw_verify_mul_witness with device inputs replays a HIP graph
 *   of its launch sequence. The second call of a key (N, K, M, the input
 *   pointers, no allocation or option change since) is captured, later calls
 *   of the key replay it with one hipGraphLaunch; k_gamma_prep (gamma's tables,
 *   and the one / gamma-power cells) is queued on the context stream ahead of
 *   the graph, so gamma is never part of it. Off while profiling or hold_us is
 *   set; "gamma_at" -1 | 0 | 1 and "dchk_at" 0 | 1 | 2 (pipelined svd_witness:
 *   k_gamma_prep at the head of the cell stream (0) or of the third stream (1;
 *   -1: the third on a row-sharded rank, else the cell stream); the d checks
 *   on the cell stream behind the products (0), on the second stream with the
 *   bounds and u.d (1) or on the third ahead of phase 1 (2)); "vm_linear" 1 | 0 (the captured sequence is queued on the context
 *   stream alone, a linear graph, instead of forking to the second stream);
 *   "gemm_kern" -1 | 0 | 1 | 2 (CRT GEMM: 0 one block per (128 x 128 tile,
 *   modulus) unit, 1 a persistent grid whose blocks' chunk pipelines run on
 *   across their units (jobs of one K >= 512), 2 256 x 128 tiles (non-symmetric
 *   products; others as 1); -1: for a product queued on its own
 *   (svdw_honest_prover_mat_mul) 2 from 64 tile pairs of 256 x 128 on, else 1,
 *   and 0 inside the witness calls);
 *   "res_wait" -1 | 0 | 1 (pipelined svd_witness reading its loads from the f64
 *   inputs: the second stream's stages wait for the residue planes (1) or not
 *   (0); -1: 1 on a row-sharded context, else 0).
 * Layout option (changes the phase-1 stream): "rlc_prefix" 0 | 1 (svd_witness:
 *   phase 1 starts with the two ctx_gate constant cells [1, 0] that
 *   examples/svd_example.rs:183's rlc.load_rlc_cache(.., 1) appends as recalled
 *   from axiom-eth's RlcChip, parity unpinned; init_rand is then RLC cell 2).
 * Test hook: "hold_us" 0 | us (svd_witness, verify_mul_witness: the step's
 *   streams wait behind a kernel spinning that long, so the GPU schedule is
 *   measured without host gaps and a missing cross-stream dependency shows).
 * Fixed since round 4 (measured, no longer options): products batched into one
 *   GEMM and one combine launch, residue planes before the stages beside them,
 *   the d checks and constant cells on the second stream, m, u, v, d quantized
 *   in one launch with the bit-length words folded inside it, b.g of a
 *   row-sharded rank from the f64 inputs, 4 KiB-aligned stage store windows,
 *   GEMM sizes decided on the device.
 * ABI version 2 removed the options ABI 1 had retired as no-ops ("bits_fold",
 *   "bounds_after", "colsum", "d_checks_aside", "dep_values", "fused_quantize",
 *   "gemm_batch", "gemm_priority", "gemm_rt", "prelaunch_at", "prod_blocks",
 *   "prod_first", "res_first", "stage_align", "stage_priority", "stage_probe",
 *   "stage_nt") and the persistent front streamer with its options
 *   ("stage_occ", "stage_front_all", and "stage_diag", a timing diagnostic
 *   whose cells were wrong): they are unknown names now (SVDW_EINVAL). */
int svdw_set_option(svdw_ctx* ctx, const char* name, int64_t value);
/* SVDW_ABI_VERSION of the library (callers compare it with the header's). */
#define SVDW_ABI_VERSION 2
int svdw_abi_version(void);
/* Captures and replays of the verify_mul_witness graph ("graph") so far. */
int svdw_graph_stats(svdw_ctx* ctx, uint64_t* captures, uint64_t* replays);

/* ----------------------------------------------------------- profiling */
/* Per-kernel statistics from HIP events recorded around every launch on the
 * context stream. bytes / ops: algorithmic HBM bytes / MACs of the launches
 * (cells x 32 B written + input cells read; GEMM MACs = N*M*K). */
typedef struct {
    char name[48];
    uint64_t launches;
    double total_ms, max_ms;
    double bytes, ops;
} svdw_kstat;
/* Enable (1) / disable (0) event recording; drops pending records. */
int svdw_profile_enable(svdw_ctx* ctx, int on);
/* Record only launches whose kernel name starts with `prefix` ("" / NULL = all):
 * each recorded launch adds two event packets to the stream. */
int svdw_profile_filter(svdw_ctx* ctx, const char* prefix);
/* Synchronize, aggregate pending records by kernel name (up to cap entries
 * written to out; *n = number of distinct names) and drop them. */
int svdw_profile_collect(svdw_ctx* ctx, svdw_kstat* out, uint32_t cap, uint32_t* n);

/* ---------------------------------------------- row-block sharding
 * One witness split over `world` contexts (one per GPU, no data exchange):
 * after svdw_set_shard(ctx, rank, world), svdw_svd_witness / check_svd_phase0/1
 * compute on this context only the rows [R*rank/world, R*(rank+1)/world) of
 * every row-parallel stage (R = the stage's row count: N or M), writing them
 * at their global offsets of full-size streams; the shared operands (quantized
 * m, u, v, d, single constants, the Freivalds b.g vector values) are computed
 * by every rank. svdw_shard_segments lists the cell ranges this rank is the
 * source of; over all ranks they tile every stream exactly once, so the global
 * witness is the union (a gather to one device, or kept sharded-resident).
 * Works on planning contexts too (segments without cells). world = 1: off. */
typedef struct {
    uint32_t phase;     /* 0 / 1 */
    uint32_t lookup;    /* 0: advice stream, 1: lookup stream */
    uint64_t off, n;    /* cells [off, off + n) */
} svdw_segment;
int svdw_set_shard(svdw_ctx* ctx, uint32_t rank, uint32_t world);
/* Virtual layout of the last witness: every cell region in append order (the
 * order halo2-base's Context receives them), tagged with the gadget / function
 * that appended it. rows > 1: the region is `rows` equal runs of cells, one per
 * row of a row-parallel stage (the unit of svdw_set_shard). Works on planning
 * contexts. Up to cap regions into out; *n = total count. */
typedef struct {
    uint32_t phase;
    uint32_t _pad;
    uint64_t off, n;      /* advice cells [off, off + n) */
    uint64_t loff, nl;    /* lookup cells [loff, loff + nl) */
    uint64_t rows;
    char tag[40];
} svdw_region;
int svdw_layout(const svdw_ctx* ctx, svdw_region* out, uint64_t cap, uint64_t* n);
/* ctx_rlc of the last svd_witness run with "rlc_prefix" 1: the RLC context of
 * examples/svd_example.rs:181-184 (rlc.load_rlc_cache((ctx_gate, ctx_rlc),
 * gate, 1); gamma_pow_cached()[0]), as recalled from axiom-eth's RlcChip
 * (un-vendored: PARITY UNPINNED). An empty cache loads gamma as
 * compute_rlc_fixed_len(ctx_rlc, [one, zero]): ctx_rlc holds
 * [E(one), E(zero), W(gamma)], whose cell 2 is the init_rand every phase-1
 * gamma cell copies. cells: 3 x 4 u64 (canonical LE); copies[k]: the source of
 * ctx_rlc cell k < 2 (phase << 62 | offset in that phase's advice stream, the
 * two ctx_gate constants at the head of phase 1). *n = 3, or 0 when the last
 * witness had no RLC prefix (cells / copies untouched). Host memory, no GPU. */
int svdw_rlc_trace(const svdw_ctx* ctx, uint64_t* cells, uint64_t* copies, uint32_t* n);

/* Constraint check of the last witness on the device, the MockProver-style
 * verification of an (unsharded) context: every halo2-base basic gate
 * a + b*c = d at the offsets the reference's gadgets enable (assign_region's
 * gate offsets; the row-scan inner products), every lookup cell against the
 * [0, 2^lookup_bits) table, and the copy constraints of the gadget blocks: a
 * value's repeated cells, a loaded operand against its source cell, and
 * range_check's last running sum against the checked value. Not checked: the
 * copies of the row scans' operands and of constant cells. An honest witness
 * has no failures; an SVD that violates a bound fails range-check copies
 * (README.md:93 "matrix-wrong", from P = 42 on). A row-sharded context
 * (svdw_set_shard) checks the cells it owns (svdw_shard_segments): summed over
 * the ranks, the counts equal those of the unsharded witness. */
typedef struct {
    uint64_t gates_checked, gate_failures;
    uint64_t lookups_checked, lookup_failures;
    uint64_t copies_checked, copy_failures;
} svdw_check_result;
int svdw_check_gates(svdw_ctx* ctx, svdw_check_result* out);

/* Virtual -> physical layout of the last witness (the
 * halo2-base 0.4.1 keygen assignment, restated from memory -- parity unpinned,
 * see DESIGN.md): basic-gate advice columns of max_rows = 2^k - minimum_rows
 * usable rows (BaseCircuitBuilder::calculate_params, src/scaffold/mod.rs:245-247
 * MINIMUM_ROWS default 20). A column breaks at the cell whose gate would cross
 * max_rows, or at row max_rows - 1; the break cell is repeated at row 0 of the
 * next column and its selector enabled there only. Lookup cells fill lookup
 * advice columns max_rows at a time. num_advice is calculate_params' estimate
 * ceil(cells / max_rows); columns_used is what the assignment needs (more than
 * num_advice: the reference's keygen panics "NOT ENOUGH ADVICE COLUMNS"). */
typedef struct {
    uint32_t k, minimum_rows;
    uint64_t max_rows;
    uint32_t num_advice[2], columns_used[2], num_lookup_advice[2];
    uint32_t num_fixed;
    uint64_t constants;    /* distinct constant cell values (fixed column cells) */
} svdw_physical_params;
int svdw_physical_layout(svdw_ctx* ctx, uint32_t k, uint32_t minimum_rows, svdw_physical_params* out);
/* each column but the last: the row of its break cell (halo2-base break_points) */
int svdw_break_points(const svdw_ctx* ctx, uint32_t phase, uint64_t* out, uint64_t cap, uint64_t* n);
/* Materialise phase `phase` on the device, column-major, 2^k rows per column
 * (rows past the used ones zero): advice = columns_used x 2^k cells, selectors
 * = columns_used x 2^k q_enable bytes, lookup = num_lookup_advice x 2^k cells;
 * any may be NULL. Fails with SVDW_ERANGE when columns_used > num_advice. */
int svdw_assign_columns(svdw_ctx* ctx, uint32_t phase, void* advice, uint8_t* selectors, void* lookup);
/* svdw_assign_columns with the advice and lookup columns in `form` (SVDW_FORM_*;
 * selectors unchanged; padding rows stay zero, which is zero in both forms):
 * Montgomery columns are converted while they are written, one pass over the
 * cells. form 0 == svdw_assign_columns. */
int svdw_assign_columns_form(svdw_ctx* ctx, uint32_t phase, int form, void* advice, uint8_t* selectors,
                             void* lookup);
/* The basic gate at every enabled (column, row) of assigned columns, and each
 * break cell against row 0 of the next column (copies_*). */
int svdw_check_physical(svdw_ctx* ctx, uint32_t phase, const void* advice, const uint8_t* selectors,
                        uint32_t ncols, svdw_check_result* out);
/* Copy-constraint (equality) lists of phase `phase` of the last witness: the
 * records halo2-base 0.4.1's copy manager holds after the same calls, in assign
 * order -- every QuantumCell::Existing cell against its source cell, every
 * Constant cell (and assert_is_const) against its value, range_check's
 * constrain_equal(a, last running sum) -- so keygen / MockProver can run on
 * the engine's columns. Replaces Context's copy manager (advice_equalities,
 * constant_equalities) consumed by raw_synthesize_phase0/1
 * (src/utils/executor.rs:100-102,116-118; src/scaffold/mod.rs:93-106).
 * copies: 2 words per record, (source cell | source phase << 62, destination
 * cell of `phase`); source phase 2 = the external init_rand cell of verify_mul
 * (RLC context). consts: 5 words per record, (cell, 4 canonical LE words).
 * Works on dry (planner) contexts. Null buffers: counts only. */
int svdw_equalities(const svdw_ctx* ctx, uint32_t phase, uint64_t* copies, uint64_t copies_cap,
                    uint64_t* n_copies, uint64_t* consts, uint64_t consts_cap, uint64_t* n_consts);
typedef struct {
    uint64_t copies_checked, copy_failures;
    uint64_t consts_checked, const_failures;
} svdw_eq_check;
/* Check every equality record of `phase` on the device: on the virtual cell
 * streams (columns0 = columns1 = NULL), or on assigned physical columns
 * (svdw_assign_columns output of phase 0, and of phase 1 for phase 1), each
 * cell at its first placement. External sources compare with the last init_rand. */
int svdw_check_equalities(svdw_ctx* ctx, uint32_t phase, const void* columns0, const void* columns1,
                          svdw_eq_check* out);
/* ------------------------------------------------------ lookup argument
 * What a halo2 prover computes next from a lookup advice column: the permuted
 * input column A' and permuted table column S' of
 * halo2_proofs' plonk::lookup::prover::permute_expression_pair, for RangeChip's
 * table T = [0, 1, .., 2^lookup_bits - 1, 0, 0, ..] (padded with its first
 * value), and the table-value multiplicities a logUp-style prover takes
 * instead. halo2_proofs' source is not available offline, so the rule is
 * restated from memory: PARITY UNPINNED. With usable = 2^k - unusable_rows
 * (unusable_rows = halo2's blinding_factors + 1) and only rows [0, usable)
 * taking part:
 *   A' = A[:usable] sorted by the canonical integer;
 *   walking A' in row order, the first row of each run of equal values gets
 *   S' = A' (one copy of the value leaves the table multiset; a value not in
 *   it fails the lookup), every other row is pushed on a list of repeated rows;
 *   the table entries left over, ascending, each go to the row popped off the
 *   END of that list (ascending leftovers fill the repeated rows in
 *   descending row order);
 *   rows >= usable are the prover's blinding rows: the engine writes zero.
 * Every honest cell is < 2^lookup_bits, so the device does this with a
 * histogram, scans over the 2^lookup_bits bins and a fill.
 *
 * Input columns: columns == NULL reads the lookup stream of `phase` through
 * the physical layout (column c = stream cells [c max_rows, min((c + 1)
 * max_rows, len)) then zeros; nothing is materialised; ncols must equal
 * num_lookup_advice[phase]); else a canonical ncols x 2^k DEVICE array,
 * column-major, e.g. svdw_assign_columns' lookup output. The calls need a prior
 * svdw_physical_layout (k, max_rows) and return after the device has finished.
 * SVDW_EINVAL: a planning or row-sharded context, no layout, unusable_rows >
 * the layout's minimum_rows (an assigned row would be a blinding row), ncols
 * mismatch. SVDW_ERANGE: k > 31, 2^lookup_bits > usable (the table does not
 * fit: halo2's not-enough-rows), more than 65535 columns. ncols == 0: SVDW_OK,
 * nothing is touched (phase 1 of an SVD witness has no lookup cells). */
/* mult[c * 2^lookup_bits + v] = the cells equal to v in rows [0, usable) of
 * column c (unassigned rows count as zeros); a cell >= 2^lookup_bits is counted
 * nowhere. mult: DEVICE array of ncols x 2^lookup_bits uint32_t. */
int svdw_lookup_multiplicities(svdw_ctx* ctx, uint32_t phase, uint32_t unusable_rows, const void* columns,
                               uint32_t ncols, uint32_t* mult);
typedef struct {
    uint32_t columns, _pad;
    uint64_t usable_rows;
    uint64_t out_of_table;   /* cells >= 2^lookup_bits in usable rows */
    uint64_t distinct;       /* distinct values per column, summed over the columns */
} svdw_lookup_result;
/* permuted_input / permuted_table: DEVICE arrays of ncols x 2^k cells,
 * column-major as svdw_assign_columns, in `form` (SVDW_FORM_*). If any cell of a
 * usable row is >= 2^lookup_bits (any bit above lookup_bits set, the test of
 * svdw_check_gates' lookup check) the call returns SVDW_OK with out_of_table =
 * their count and leaves the outputs untouched: halo2's ConstraintSystemFailure. */
int svdw_lookup_permute(svdw_ctx* ctx, uint32_t phase, uint32_t unusable_rows, int form, const void* columns,
                        uint32_t ncols, void* permuted_input, void* permuted_table, svdw_lookup_result* result);
typedef struct {
    uint64_t adjacency_checked, adjacency_failures;   /* usable rows */
    uint64_t multiset_checked, multiset_failures;     /* 2 x 2^lookup_bits bins per column */
    uint64_t padding_checked, padding_failures;       /* cells of A' and S' in rows >= usable */
} svdw_lookup_check;
/* The lookup argument's own constraints on permuted columns in `form`, on the
 * device: adjacency (A'[0] == S'[0]; A'[r] == S'[r] or A'[r] == A'[r - 1] for
 * 1 <= r < usable), multisets (the histogram of A' equals that of A[:usable],
 * that of S' equals that of T[:usable]; a cell of A, A' or S' outside the table
 * is a failure of its own), padding (rows >= usable are zero). `phase` selects
 * the stream when columns == NULL. */
int svdw_check_lookup_argument(svdw_ctx* ctx, uint32_t phase, uint32_t unusable_rows, int form,
                               const void* columns, uint32_t ncols, const void* permuted_input,
                               const void* permuted_table, svdw_lookup_check* result);
/* The lookup argument's grand-product column Z of halo2_proofs'
 * plonk::lookup::prover::Permuted::commit_product, the one thing a prover
 * computes from A' and S' after committing to them. Restated from memory like
 * the permute: PARITY UNPINNED. One argument per lookup advice column, the
 * compressed expressions are the columns themselves (no theta). With A the
 * input column (zero where unassigned), T[r] = r for r < 2^lookup_bits, else 0,
 * usable = 2^k - unusable_rows, inv0(x) = 1 / x and inv0(0) = 0 (ff's
 * batch_invert leaves a zero zero):
 *   f[r]     = (A[r] + beta)(T[r] + gamma) inv0((A'[r] + beta)(S'[r] + gamma))
 *   Z[0]     = 1,  Z[r + 1] = Z[r] f[r]        0 <= r < usable
 *   Z[r]     = 0                               usable < r < 2^k
 * Rows above `usable` are the prover's random blinding rows: the engine writes
 * zero. Z[usable] == 1 exactly when the two products agree, as they do for an
 * honest (A', S'); Z is 0 from the row after the first zero denominator on.
 * beta and gamma are inputs (canonical, 4 little-endian words, as gamma of
 * svdw_svd_witness; >= p is SVDW_EINVAL): deriving them from the transcript,
 * the commitments and the blinding rows' randomness stay with the prover.
 * All arithmetic is exact mod p. columns / ncols / phase / unusable_rows as for
 * svdw_lookup_permute, with the same errors, and SVDW_ERANGE for
 * unusable_rows == 0 (Z[usable] would be row 2^k). The checks of the arguments
 * alone come first, in this order: an unknown form (SVDW_EINVAL), beta or
 * gamma >= p (SVDW_EINVAL), unusable_rows == 0 (SVDW_ERANGE); then those of the
 * context as svdw_lookup_permute makes them. Cells are taken as field
 * elements: the table range is svdw_lookup_permute's to validate.
 * permuted_input, permuted_table, z: DEVICE arrays of ncols x 2^k cells,
 * column-major, all in `form`. ncols == 0: SVDW_OK, nothing is touched. */
typedef struct {
    uint32_t columns, _pad;
    uint64_t usable_rows;
    uint64_t zero_denominators;   /* rows r < usable with (A'[r] + beta)(S'[r] + gamma) == 0, all columns */
    uint64_t final_not_one;       /* columns with Z[usable] != 1 */
} svdw_lookup_product_result;
int svdw_lookup_product(svdw_ctx* ctx, uint32_t phase, uint32_t unusable_rows, int form, const void* columns,
                        uint32_t ncols, const void* permuted_input, const void* permuted_table,
                        const uint64_t beta[4], const uint64_t gamma[4], void* z,
                        svdw_lookup_product_result* result);
typedef struct {
    uint64_t recurrence_checked, recurrence_failures;  /* rows r < usable, per column */
    uint64_t boundary_checked, boundary_failures;      /* Z[0] == 1 and Z[usable] in {0, 1}: 2 per column */
    uint64_t padding_checked, padding_failures;        /* Z rows > usable are zero */
} svdw_lookup_product_check;
/* The product's own constraints on a column Z in `form`, on the device, in the
 * division-free form Z[r + 1] (A'[r] + beta)(S'[r] + gamma) ==
 * Z[r] (A[r] + beta)(T[r] + gamma) for r < usable; it shares no inversion and no
 * scan with svdw_lookup_product. */
int svdw_check_lookup_product(svdw_ctx* ctx, uint32_t phase, uint32_t unusable_rows, int form, const void* columns,
                              uint32_t ncols, const void* permuted_input, const void* permuted_table,
                              const uint64_t beta[4], const uint64_t gamma[4], const void* z,
                              svdw_lookup_product_check* result);
/* ----------------------------------------------------- permutation argument
 * The copy-constraint argument's grand-product columns Z of halo2_proofs'
 * plonk::permutation::prover::Argument::commit. Restated from memory like the
 * two lookup steps: PARITY UNPINNED. These calls need no witness and no
 * physical layout; k is an argument, 1 <= k <= 28.
 *
 * Constants of BN254 Fr as in halo2curves: delta = 7^(2^28), omega_k =
 * 7^((p - 1) / 2^k), the generator of the 2^k rows. Inputs: ncols columns v_j
 * of 2^k cells in the order of cs.permutation.columns (the caller's business),
 * their permutation columns sigma_j (pk.permutation.permutations in Lagrange
 * form: sigma_j[r] = delta^j' omega^r' of the cell that (j, r) maps to), beta,
 * gamma, chunk_len = cs_degree - 2 >= 1 and unusable_rows >= 1, usable =
 * 2^k - unusable_rows. Set s holds the columns [s chunk_len, min((s + 1)
 * chunk_len, ncols)), nsets = ceil(ncols / chunk_len); j counts over all
 * columns, not within the set; inv0(0) = 0 (ff's batch_invert):
 *   D_s[r]   = prod_{j in set s} (v_j[r] + beta sigma_j[r] + gamma)
 *   N_s[r]   = prod_{j in set s} (v_j[r] + beta delta^j omega^r + gamma)
 *   Z_0[0]   = 1,  Z_s[0] = Z_{s-1}[usable]                 s > 0
 *   Z_s[r+1] = Z_s[r] N_s[r] inv0(D_s[r])                   0 <= r < usable
 *   Z_s[r]   = 0                                            usable < r < 2^k
 * Rows above `usable` are the prover's random blinding rows: the engine writes
 * zero. For an honest sigma only the last set ends at 1. A zero denominator
 * makes Z zero from the next row on, and in every later set. Deriving beta and
 * gamma, the blinding randomness and the commitments stay with the caller.
 *
 * Sigma itself comes from the copy constraints by keygen's cycle merge, on the
 * device (svdw_permutation_cycles below), in its order-independent form:
 *   cells    total_cols columns of 2^k rows, a cell written col << 32 | row as
 *            svdw_permutation_values takes it;
 *   classes  the connected components of the graph whose edges are the copy
 *            constraints, over the cells of rows < usable;
 *   sigma    links the cells of each class in ascending (col, row) into one
 *            cycle: every cell maps to the next one of its class, the last to
 *            the first; a cell alone in its class and every cell of a row >=
 *            usable maps to itself.
 * halo2's serial Assembly::copy gives a sigma that depends on the order of its
 * calls, which no parallel merge reproduces. The classes here are the partition
 * that merge produces, so Z closes for exactly the same witnesses; only the
 * order inside a cycle differs, and a verifying key made from this sigma
 * differs from one made by halo2's serial keygen on the same circuit. It is
 * believed to be what halo2's thread-safe-region keygen builds: restated from
 * memory, PARITY UNPINNED like the rest. The mapping is the same bits from run
 * to run and for any order or repetition of the edges. */
/* delta and omega_k, canonical, 4 little-endian words each. Host only.
 * k outside 1..28: SVDW_ERANGE. */
int svdw_permutation_constants(uint32_t k, uint64_t delta[4], uint64_t omega[4]);
/* Sigma cells on the device: out (DEVICE, ncols x 2^k cells in `form`,
 * column-major) cell i = delta^col omega^row of mapping[i] = col << 32 | row
 * (DEVICE array of ncols x 2^k uint64_t, the entries of the columns written).
 * mapping == NULL: the identity for the columns first_col .. first_col + ncols.
 * An entry with col >= total_cols or row >= 2^k is written as zero and counted
 * in *out_of_range. Checks in this order: form (SVDW_EINVAL), k outside 1..28
 * (SVDW_ERANGE), a planning context (SVDW_EINVAL), ncols or total_cols > 65535
 * (SVDW_ERANGE); ncols == 0: SVDW_OK, nothing is touched. */
int svdw_permutation_values(svdw_ctx* ctx, uint32_t k, int form, const uint64_t* mapping, uint32_t first_col,
                            uint32_t ncols, uint32_t total_cols, void* out, uint64_t* out_of_range);
typedef struct {
    uint32_t columns, sets;
    uint64_t usable_rows;
    uint64_t zero_denominators;   /* rows r < usable with D_s[r] == 0, all sets */
    uint32_t final_not_one, _pad; /* 1: the last set's Z[usable] != 1 */
} svdw_permutation_product_result;
/* columns, sigma: HOST arrays of ncols DEVICE pointers, each to 2^k cells in
 * `form` (the caller's columns live in several allocations). z: DEVICE array
 * of nsets x 2^k cells, column-major, in `form`. All arithmetic is exact mod p;
 * cells are taken as field elements below p. The checks of the arguments come
 * first, before anything touches the device, in this order: an unknown form
 * (SVDW_EINVAL), beta or gamma >= p (SVDW_EINVAL), unusable_rows == 0 or
 * >= 2^k (SVDW_ERANGE), chunk_len == 0 (SVDW_EINVAL), k outside 1..28
 * (SVDW_ERANGE), a planning context (SVDW_EINVAL), more than 65535 columns
 * (SVDW_ERANGE), null pointers (SVDW_EINVAL). ncols == 0: SVDW_OK, sets = 0,
 * nothing is touched. */
int svdw_permutation_product(svdw_ctx* ctx, uint32_t k, uint32_t unusable_rows, int form,
                             const void* const* columns, const void* const* sigma, uint32_t ncols,
                             uint32_t chunk_len, const uint64_t beta[4], const uint64_t gamma[4], void* z,
                             svdw_permutation_product_result* result);
typedef struct {
    uint64_t recurrence_checked, recurrence_failures;  /* rows r < usable, per set: nsets * usable */
    uint64_t boundary_checked, boundary_failures;      /* Z_0[0] == 1, Z_s[0] == Z_{s-1}[usable], the last
                                                          Z[usable] in {0, 1}: nsets + 1 */
    uint64_t padding_checked, padding_failures;        /* Z rows > usable are zero: nsets * (unusable_rows - 1) */
} svdw_permutation_product_check;
/* The product's own constraints on Z in `form`, on the device, in the
 * division-free form Z_s[r + 1] D_s[r] == Z_s[r] N_s[r] for r < usable with the
 * raw N and D; it shares no inversion and no scan with
 * svdw_permutation_product. Arguments and their checks as for the product. */
int svdw_check_permutation_product(svdw_ctx* ctx, uint32_t k, uint32_t unusable_rows, int form,
                                   const void* const* columns, const void* const* sigma, uint32_t ncols,
                                   uint32_t chunk_len, const uint64_t beta[4], const uint64_t gamma[4],
                                   const void* z, svdw_permutation_product_check* result);
typedef struct {
    uint64_t cells, edges;
    uint64_t out_of_range;    /* edges with an end outside the columns, the 2^k rows or the usable rows: skipped */
    uint64_t self_edges;      /* in-range edges whose two ends are one cell: skipped */
    uint64_t classes, linked_cells, largest_class;   /* of the classes of two or more cells */
    uint32_t sort_passes, _pad;                      /* 8-bit digits that hold every cell id */
} svdw_permutation_cycles_result;
/* The mapping of sigma, by the rule above, from an edge list. edges: DEVICE
 * array of n_edges x 2 cells col << 32 | row; mapping: DEVICE array of
 * total_cols x 2^k uint64_t, every entry written, in the form
 * svdw_permutation_values takes. An edge with an end outside the columns,
 * outside the 2^k rows or in a row >= usable is halo2's bounds failure: it is
 * counted in out_of_range and skipped, for the caller to treat as an error.
 * Cell ids are 32-bit: total_cols << k above 2^32 is SVDW_ERANGE, which leaves
 * out the witness of a 4096 x 4096 matrix. Needs no witness and no physical
 * layout; any edge list does, so a caller who has further copies (those between
 * lookup advice columns and the advice cells they repeat, which the engine does
 * not list) appends them. Checks in this order: null ctx or result
 * (SVDW_EINVAL), k outside 1..28 (SVDW_ERANGE), unusable_rows >= 2^k
 * (SVDW_ERANGE), a planning context (SVDW_EINVAL), total_cols > 65535 or
 * total_cols << k above 2^32 (SVDW_ERANGE); total_cols == 0: SVDW_OK, nothing
 * is touched; then a null mapping, null edges with n_edges > 0, a mapping that
 * overlaps the edges (SVDW_EINVAL). n_edges == 0 gives the identity. Returns
 * after the device has finished. */
int svdw_permutation_cycles(svdw_ctx* ctx, uint32_t k, uint32_t unusable_rows, uint32_t total_cols,
                            const uint64_t* edges, uint64_t n_edges, uint64_t* mapping,
                            svdw_permutation_cycles_result* result);
typedef struct {
    uint64_t cells_checked;
    uint64_t not_permutation;   /* cells not hit exactly once, and entries out of range */
    uint64_t order_failures;    /* cycles of two or more cells whose descents mapping[i] < i are not exactly 1 */
    uint64_t padding_failures;  /* non-identity entries in rows >= usable */
    uint64_t edges_checked;     /* edges with both ends in range */
    uint64_t edge_failures;     /* of those, the edges whose ends lie in different cycles */
    uint64_t cycles;            /* cycles of two or more cells */
} svdw_permutation_mapping_check;
/* A mapping against the rule and the edges, on the device, a debug aid: hit
 * counts by one scatter pass, the minimum of every cycle by pointer doubling
 * over the mapping, descents per cycle, the ends of every edge against the
 * minima. It shares no union-find and no sort with svdw_permutation_cycles. It
 * cannot see that the cycles are no coarser than the classes: two classes
 * linked into one ascending cycle pass (compare `cycles` with `classes`, or the
 * mapping with a host restatement as the tests do). Arguments and their checks
 * as for svdw_permutation_cycles; the mapping is only read. */
int svdw_check_permutation_mapping(svdw_ctx* ctx, uint32_t k, uint32_t unusable_rows, uint32_t total_cols,
                                   const uint64_t* edges, uint64_t n_edges, const uint64_t* mapping,
                                   svdw_permutation_mapping_check* result);
typedef struct {
    uint32_t k, advice[2], fixed, external, total_cols;   /* columns: advice per phase, fixed, external (0 or 1) */
    uint64_t edges, break_edges, copy_edges, const_edges, external_edges;
    uint64_t constants;       /* distinct constant values = svdw_physical_params.constants */
} svdw_permutation_layout;
/* The copy constraints of the last witness as the edge list
 * svdw_permutation_cycles takes, after svdw_physical_layout. The argument's
 * columns, in this order: the advice columns of phase 0 (columns_used[0]), those
 * of phase 1 (columns_used[1]), num_fixed fixed columns, and one external column
 * if and only if a record has source phase 2 (or the witness has the rlc_prefix):
 * it holds the RLC context's cells, gamma at row 0, or at row 2 behind the
 * prefix's two cells. The edges, in this order:
 *   1. per phase, each break cell against row 0 of the next column;
 *   2. the copy records of phase 0, then of phase 1, whose source is an advice
 *      cell, (source, destination) at their first placement, in the order of
 *      svdw_equalities;
 *   3. the constant records of phase 0, then of phase 1, (cell, the fixed cell
 *      of its value);
 *   4. the records of source phase 2 of phase 0, then of phase 1, (external
 *      cell, destination); with the rlc_prefix then the two copies of
 *      svdw_rlc_trace, (advice cell, external row 0), (advice cell, external
 *      row 1).
 * The constants: the distinct values in the order of their first occurrence
 * over the constant records of phase 0 and then of phase 1; constant i goes to
 * fixed column i % num_fixed, row i / num_fixed (halo2-base's round-robin as
 * recalled, PARITY UNPINNED); every other fixed cell is zero. A constant whose
 * row would be one of the layout's minimum_rows last rows: SVDW_ERANGE.
 * edges == NULL: the counts alone, also on a planning context. Else edges is a
 * DEVICE array of cap x 2 cells, cap >= the layout's edges (else SVDW_EINVAL),
 * on a device context. SVDW_EINVAL without a layout and on a row-sharded
 * context; SVDW_ERANGE for k > 28 or more than 65535 columns. Copies between
 * lookup advice columns and the advice cells they repeat are not listed: the
 * lookup stream keeps no origin cell (svdw_equalities does not list them
 * either); a caller who has them appends them. */
int svdw_permutation_edges(svdw_ctx* ctx, uint64_t* edges, uint64_t cap, svdw_permutation_layout* layout);
/* The fixed columns of that placement: fixed is a DEVICE array of num_fixed x
 * 2^k cells in `form`, column-major. Needs a svdw_permutation_edges call with an
 * edge list since the last svdw_physical_layout (it finds the order of the
 * constants); SVDW_EINVAL otherwise, for an unknown form and on a planning
 * context. No constants: SVDW_OK, nothing is touched. */
int svdw_assign_fixed(svdw_ctx* ctx, int form, void* fixed);
/* ------------------------------------------------------ domain transforms
 * halo2_proofs' poly::EvaluationDomain conversions of columns of BN254 Fr cells
 * on the device, eval_polynomial for a batch, and a check of a transform by
 * direct evaluation. Restated from memory like the lookup and permutation
 * steps: PARITY UNPINNED. These calls need no witness and no physical layout.
 * omega = omega_k of svdw_permutation_constants; all arithmetic is exact mod p;
 * cells are taken as field elements below p. Indices are in natural order on
 * both sides: the caller never sees a bit reversal.
 *
 * One transform, svdw_ntt, of ncols columns of 2^k_in cells into ncols columns
 * of 2^k cells, 1 <= k_in <= k <= 28, shift != 0 (NULL: 1):
 *   forward (inverse == 0):  b[i] = in[i] shift^i for i < 2^k_in, 0 above;
 *                            out[j] = sum_i b[i] omega^(i j)
 *   inverse (inverse == 1, k_in == k):
 *                            c[i] = 2^-k sum_j in[j] omega^(-i j);
 *                            out[i] = c[i] shift^i
 * EvaluationDomain's calls are
 *   lagrange_to_coeff   inverse, shift NULL
 *   coeff_to_lagrange   forward, shift NULL
 *   coeff_to_extended   forward, k = extended_k, shift = Fr::ZETA
 *                       (distribute_powers_zeta: g^i with g^3 = 1)
 *   extended_to_coeff   inverse, k_in = k = extended_k, shift = ZETA^2 =
 *                       ZETA^-1; the caller keeps the prefix it needs
 * ZETA is the caller's input: the engine bakes in no cube root. The gates'
 * expressions on the extended domain, the commitments and deriving the
 * evaluation point stay with the caller. */
typedef struct {
    uint32_t columns, passes;     /* passes: svdw_ntt_passes(k) */
    uint64_t rows_in, rows_out;   /* 2^k_in, 2^k */
} svdw_ntt_result;
/* Host only: the passes over global memory of a size-2^k transform (1 for
 * k <= 10, 2 for k <= 20, 3 above). */
uint32_t svdw_ntt_passes(uint32_t k);
/* in: HOST array of ncols DEVICE pointers, each to 2^k_in cells in `form`. out:
 * DEVICE array of ncols x 2^k cells, column-major, in `form`. shift: 4
 * little-endian words, canonical. The checks of the arguments come first,
 * before anything touches the device, in this order: an unknown form
 * (SVDW_EINVAL), shift >= p or shift == 0 (SVDW_EINVAL), inverse not 0 or 1
 * (SVDW_EINVAL), k outside 1..28 (SVDW_ERANGE), k_in outside 1..k or an inverse
 * with k_in != k (SVDW_ERANGE), a planning context (SVDW_EINVAL), more than
 * 65535 columns (SVDW_ERANGE), null pointers or an out that overlaps an input
 * column (SVDW_EINVAL). ncols == 0: SVDW_OK, nothing is touched. The call is
 * queued on the context's streams like svdw_permutation_product, with no host
 * wait; scratch (a second buffer of ncols x 2^k cells for k > 10) is the
 * engine's. */
int svdw_ntt(svdw_ctx* ctx, uint32_t k_in, uint32_t k, int form, int inverse, const uint64_t shift[4],
             const void* const* in, uint32_t ncols, void* out, svdw_ntt_result* result);
/* eval_polynomial for a batch: out (DEVICE, ncols x npoints cells in `form`)
 * cell c npoints + q = sum_i coeffs_c[i] x_q^i over the 2^k coefficients of
 * column c (coeffs: HOST array of ncols DEVICE pointers, cells in `form`).
 * points: HOST, npoints x 4 words, canonical; no relation between x_q and omega
 * is needed. Checks in this order: form (SVDW_EINVAL), a point >= p
 * (SVDW_EINVAL), k outside 1..28 (SVDW_ERANGE), a planning context
 * (SVDW_EINVAL), more than 65535 columns (SVDW_ERANGE), null pointers
 * (SVDW_EINVAL). ncols == 0 or npoints == 0: SVDW_OK, nothing is touched. */
int svdw_eval_polynomial(svdw_ctx* ctx, uint32_t k, int form, const void* const* coeffs, uint32_t ncols,
                         const uint64_t* points, uint32_t npoints, void* out);
typedef struct {
    uint64_t rows_checked, row_failures;   /* summed over the columns */
} svdw_ntt_check;
/* A transform's output against its input on S = 2^log_samples sampled rows per
 * column, each re-derived by direct evaluation with the kernels of
 * svdw_eval_polynomial; it shares no butterfly and no twiddle schedule with
 * svdw_ntt.
 *   forward:  out[j] == sum_i in[i] (shift omega^j)^i
 *   inverse:  in[j] == sum_i out[i] (omega^j shift^-1)^i   (this pins 2^-k too)
 * The rows are stratified: with q = 2^k / S, sample s < S is row
 *   j_s = s q + ((seed + s 0x9E3779B1) mod q);
 * log_samples == k checks every row. Arguments and their checks as for
 * svdw_ntt, log_samples > k with rule 5 (SVDW_ERANGE). */
int svdw_check_ntt(svdw_ctx* ctx, uint32_t k_in, uint32_t k, int form, int inverse, const uint64_t shift[4],
                   const void* const* in, uint32_t ncols, const void* out, uint32_t log_samples, uint64_t seed,
                   svdw_ntt_check* result);
/* ---------------------------------------------------------------- quotient
 * The quotient polynomial h(X) of halo2_proofs' plonk::evaluation::evaluate_h
 * on the extended domain, for the circuit shape this engine assigns:
 * halo2-base's vertical gate per advice column, the permutation argument and
 * one lookup argument per lookup column. Restated from memory like the steps
 * above: PARITY UNPINNED. These calls need no witness and no physical layout.
 *
 * n = 2^k, N = 2^extended_k, E = N / n, omega = omega_k, omega_e =
 * omega_extended_k, usable = n - unusable_rows. l_0, l_last and l_active are the
 * polynomials whose Lagrange columns are e_0, e_usable and (1 on the rows below
 * usable, 0 from usable on) = 1 - (l_last + l_blind). Extended row j is the
 * point X_j = shift omega_e^j, shift the caller's ZETA as for coeff_to_extended;
 * a rotation by r rows of the original domain, f(omega^r X), is extended row
 * (j + r E) mod N. With y the caller's challenge, h starts at 0 and every
 * expression e below does h <- h y + e, in this order:
 *
 *  1. Gates, one per (advice column a_i, its selector q_i), i < n_gate:
 *       q_i(X) (a_i(X) + a_i(omega X) a_i(omega^2 X) - a_i(omega^3 X))
 *  2. Permutation (n_perm > 0), sets of chunk_len columns; Z_s, sigma_j, delta,
 *     the set layout and j counting over all columns exactly as in the
 *     permutation section above, last = nsets - 1:
 *       l_0 (1 - Z_0)
 *       l_last (Z_last^2 - Z_last)
 *       for s = 1 .. nsets - 1:  l_0 (Z_s(X) - Z_{s-1}(omega^usable X))
 *       for every set s:         l_active (Z_s(omega X) prod_{j in s} (v_j + beta sigma_j + gamma)
 *                                          - Z_s(X) prod_{j in s} (v_j + beta delta^j X + gamma))
 *  3. Lookups, per argument i < n_lookup with the input column A and the table
 *     column T given as columns:
 *       l_0 (1 - Z)
 *       l_last (Z^2 - Z)
 *       l_active (Z(omega X) (A' + beta) (S' + gamma) - Z(X) (A + beta) (T + gamma))
 *       l_0 (A' - S')
 *       l_active (A' - S') (A'(X) - A'(omega^-1 X))
 *
 * Finally h_ext[j] = h (X_j^n - 1)^-1. The divisor takes E distinct values,
 * shift^n (omega_e^n)^(j mod E) - 1, inverted once per call. For an honest
 * witness with the zero blinding rows the engine writes every expression
 * vanishes on all n rows, the division is exact, and the coefficients of h
 * (extended_to_coeff of h_ext) are zero above index D (n - 1) - n, D = max(3
 * with gates, 4 with lookups, 2 + the columns of the largest set), 0 without
 * any family. Deriving y, beta, gamma, the blinding rows' randomness, cutting h
 * into pieces and the commitments stay with the caller.
 *
 * Every array is a HOST array of DEVICE column pointers (as svdw_ntt takes
 * them). For svdw_quotient each column is 2^extended_k cells in `form`, already
 * on the coset (the caller ran coeff_to_extended with the same shift); for
 * svdw_check_quotient each is the 2^k coefficients of the same polynomial. */
typedef struct {
    uint32_t k, extended_k, unusable_rows;
    int form;
    uint64_t shift[4], beta[4], gamma[4], y[4];   /* canonical */
    const void* const* advice;                    /* [n_gate] */
    const void* const* selectors;                 /* [n_gate], cells */
    uint32_t n_gate;
    uint32_t n_perm, chunk_len, n_lookup;
    const void* const* perm_columns;              /* [n_perm], the v_j */
    const void* const* sigma;                     /* [n_perm] */
    const void* const* perm_z;                    /* [ceil(n_perm / chunk_len)] */
    const void* const* lookup_input;              /* A, [n_lookup] each */
    const void* const* lookup_table;              /* T */
    const void* const* permuted_input;            /* A' */
    const void* const* permuted_table;            /* S' */
    const void* const* lookup_z;
} svdw_quotient_args;
typedef struct {
    uint64_t gate_expressions, permutation_expressions, lookup_expressions;   /* folded */
    uint64_t rows;          /* 2^extended_k */
    uint32_t extension;     /* E */
    uint32_t degree;        /* D */
} svdw_quotient_result;
/* h_ext: DEVICE, one column of 2^extended_k cells in `form`. All arithmetic is
 * exact mod p; cells are taken as field elements below p. Any family may be
 * empty; with all three empty the call returns SVDW_OK and touches nothing. The
 * checks of the arguments come first, before anything touches the device, in
 * this order: an unknown form (SVDW_EINVAL), shift, beta, gamma or y >= p or
 * shift == 0 (SVDW_EINVAL), unusable_rows == 0 or >= 2^k (SVDW_ERANGE),
 * chunk_len == 0 with n_perm > 0 (SVDW_EINVAL), k outside 1..28 or extended_k
 * outside k..28 (SVDW_ERANGE), a degree that does not fit, D > E + 1
 * (SVDW_ERANGE), shift^n an E-th root of unity, which makes a divisor zero
 * (SVDW_EINVAL), a planning context (SVDW_EINVAL), more than 65535 columns in a
 * family (SVDW_ERANGE), null pointers (SVDW_EINVAL), h_ext overlapping an input
 * column (SVDW_EINVAL). The call is queued on the context's streams like
 * svdw_ntt, with no host wait; scratch is the engine's. The engine builds the
 * extended columns of l_0, l_last and l_active itself, from their Lagrange
 * columns through its own inverse and coset transforms, and keeps them on the
 * context for the next call of the same (k, extended_k, unusable_rows, shift);
 * they are held in Montgomery form whatever `form` is, as multipliers are. */
int svdw_quotient(svdw_ctx* ctx, const svdw_quotient_args* args, void* h_ext, svdw_quotient_result* result);
typedef struct {
    uint64_t lhs[4];              /* h(x) (x^n - 1), canonical */
    uint64_t rhs[4];              /* the fold at x, canonical */
    uint64_t identity_failures;   /* 0 or 1: lhs != rhs */
    uint64_t tail_checked;        /* coefficients of h above D (n - 1) - n: N - 1 - (D (n - 1) - n) */
    uint64_t tail_nonzero;        /* those that are not zero */
} svdw_quotient_check;
/* The verifier's identity h(x) (x^n - 1) == fold(x) at a caller-chosen point x
 * (canonical, >= p: SVDW_EINVAL, checked with the challenges). coeffs: the
 * arguments of svdw_quotient with every column in coefficient form, 2^k cells;
 * h_coeffs: DEVICE, 2^extended_k cells in `form`. Every polynomial is evaluated
 * at x omega^r for r in {0, 1, 2, 3, -1, usable} with the kernels of
 * svdw_eval_polynomial, h at x; l_0(x), l_last(x) and l_active(x) come from the
 * closed form l_i(x) = omega^i (x^n - 1) / (n (x - omega^i)) on the host, and
 * the fold is redone on those few values there: it shares nothing with the
 * extended-domain kernel. The tail is counted on the device. Arguments and
 * their checks as for svdw_quotient (there is no output to overlap); it writes
 * to neither side and returns after the device has finished. Without any
 * family: SVDW_OK, nothing is evaluated and the result is zero. */
int svdw_check_quotient(svdw_ctx* ctx, const svdw_quotient_args* coeffs, const void* h_coeffs,
                        const uint64_t x[4], svdw_quotient_check* result);
/* ------------------------------------------------------------- commitments
 * KZG commitments of columns on the device: for each column of 2^k BN254 Fr
 * cells s_i the multi-scalar multiplication sum_i s_i P_i over 2^k shared G1
 * bases, as halo2_proofs' ParamsKZG::commit_lagrange (bases = g_lagrange, the
 * column in Lagrange form) and ::commit (bases = g, coefficient form) compute
 * with best_multiexp. Restated from memory like the steps above (PARITY
 * UNPINNED for the calls; the SRS layout below is pinned by the reference's
 * params/kzg_bn254_8.srs, tests/golden). No blinding term is added: as far as
 * recalled commit_lagrange ignores its Blind argument (unpinned). These calls
 * need no witness and no physical layout.
 *
 * A G1 point is 64 bytes: x then y, each a 32-byte little-endian Fq
 * (q = 21888242871839275222246405745257275088696311157297823662689037894645226208583),
 * on y^2 = x^3 + 3; (0, 0) is the identity. bases_form says how the
 * coordinates of the bases and of the commitments are held:
 * SVDW_FORM_MONTGOMERY is halo2curves' in-memory G1Affine (x 2^256 mod q), which
 * is what an SRS file holds (u32 k, 2^k points g, 2^k points g_lagrange, G2);
 * SVDW_FORM_CANONICAL the plain integers. `form` is the cells' form as
 * everywhere else. Cells are taken as integers below p; identity bases and
 * zero cells are skipped. */
typedef struct {
    uint32_t columns;
    uint32_t window_bits, windows;   /* svdw_commit_plan(k) */
    uint64_t rows;                   /* 2^k */
    uint64_t zero_scalars;           /* cells equal to 0, over the columns */
    uint64_t identity_bases;         /* bases equal to (0, 0) */
    uint64_t identity_outputs;       /* commitments that are the identity, written as (0, 0) */
} svdw_commit_result;
/* Host only: the Pippenger window of a size-2^k commitment (k clamped to
 * 1..28): window_bits = c, non-decreasing in k, and windows = ceil(255 / c)
 * signed digits per cell. Either pointer may be null. */
void svdw_commit_plan(uint32_t k, uint32_t* window_bits, uint32_t* windows);
/* bases: DEVICE, 2^k points in bases_form. cols: HOST array of ncols DEVICE
 * pointers, each to 2^k cells in `form`. out: DEVICE, ncols points in
 * bases_form. The checks of the arguments come first, before anything touches
 * the device, in this order: an unknown form or bases_form (SVDW_EINVAL), k
 * outside 1..28 (SVDW_ERANGE), a planning context (SVDW_EINVAL), more than 65535
 * columns (SVDW_ERANGE), null pointers (SVDW_EINVAL), an out that overlaps the
 * bases or an input column (SVDW_EINVAL). ncols == 0: SVDW_OK, nothing is
 * touched (window_bits, windows and rows are still reported). Every kernel is
 * queued on the context's streams like svdw_ntt, with no host wait between
 * them; like the grand products the call returns once the three counters of
 * the result have been read back. Scratch is the engine's: the window sums
 * and one batch of (column, window) tasks at a time, a batch kept under
 * 1 GiB (option "commit_scratch_mib") unless a single task needs more: about
 * 21 B per row and 140 B per bucket, 2^(window_bits - 1) buckets, per task. */
int svdw_commit(svdw_ctx* ctx, uint32_t k, int form, int bases_form, const void* bases, const void* const* cols,
                uint32_t ncols, void* out, svdw_commit_result* result);
typedef struct {
    uint64_t columns_checked, commit_failures;
    uint64_t bases_checked, bases_off_curve;   /* neither (0, 0) nor on y^2 = x^3 + 3, or a coordinate >= q */
} svdw_commit_check;
/* commitments (DEVICE, ncols points in bases_form) against the same inputs,
 * independently of svdw_commit: no windows, no sort, no buckets. For each of
 * the 254 bits b the bases whose cell has bit b set are tree-summed, Horner
 * over the bits (one doubling each) gives the sum, and it is compared with the
 * given affine point cross-multiplied, without a division. Arguments and
 * their checks as for svdw_commit (there is no output to overlap); it writes
 * to none of its inputs and returns after the device has finished. */
int svdw_check_commit(svdw_ctx* ctx, uint32_t k, int form, int bases_form, const void* bases,
                      const void* const* cols, uint32_t ncols, const void* commitments, svdw_commit_check* result);
/* A measurement probe (tools/commit_bench.py): `threads` device threads each
 * add one of the npoints Montgomery affine points (DEVICE) `reps` times into a
 * register-resident accumulator; *seconds is the launch's device time. */
int svdw_commit_add_probe(svdw_ctx* ctx, const void* points, uint32_t npoints, uint64_t threads, uint32_t reps,
                          double* seconds);
/* --------------------------------------------------------------------- SRS
 * The bases of the commitments above, made on the device: what halo2-base's
 * gen_srs(k) obtains from ParamsKZG::setup(k, rng), which draws one secret s
 * and writes g[i] = [s^i] G and g_lagrange[i] = [l_i(s)] G for i < n = 2^k,
 * G = (1, 2) and l_i the Lagrange basis of the domain of omega_k:
 * l_i(s) = (s^n - 1) omega^i / (n (s - omega^i)). PARITY PINNED BY THE
 * REFERENCE'S FILE: with the secret gen_srs draws (ChaCha20Rng from the zero
 * seed, Fr::random; halo2_svd041_amd.srs.default_secret) the two arrays are,
 * byte for byte, those of the reference's params/kzg_bn254_8.srs
 * (tests/golden). The G2 half of a file ([1] G2 and [s] G2) is one scalar
 * multiplication on the host (halo2_svd041_amd/srs.py) and not part of this
 * interface. These calls need no witness and no physical layout.
 *
 * All of it is multiplication of ONE base by many unrelated scalars, which is
 * not Pippenger's problem: svdw_fixed_base_mul looks every signed digit of a
 * scalar up in a table of the base's multiples. Points, forms and the digits
 * (c bits, W = ceil(255 / c) windows, digits in (-2^(c-1), 2^(c-1)] with
 * carry) are those of the commitments section. */
typedef struct {
    uint32_t window_bits, windows;   /* c and W = ceil(255 / c) as used */
    uint64_t points;                 /* n */
    uint64_t zero_scalars;           /* scalars equal to 0 */
    uint64_t identity_outputs;       /* outputs that are the identity, written as (0, 0) */
} svdw_fixed_base_result;
/* out[i] = [scalars[i]] base for i < n. base: HOST, one point (64 bytes) in
 * base_form, (0, 0) allowed. scalars: DEVICE, n cells in `form`, taken as
 * integers below p. out: DEVICE, n points in base_form; exactly n points are
 * written. window_bits: 0 for the planned window (the c <= 12 with the fewest
 * field products for n outputs; at c = 12 the table of W 2^(c-1) = 45056
 * points, 2.75 MiB, stays in one XCD's L2), or 2..16. The table is built on
 * the device on the first use of (base, base_form, window_bits) and kept on
 * the context, four tables at the most, the oldest replaced. The checks of the
 * arguments come first, before anything touches the device, in this order:
 * null ctx, base or result (SVDW_EINVAL), an unknown form or base_form
 * (SVDW_EINVAL), a base coordinate >= q or a base that is neither (0, 0) nor
 * on the curve (SVDW_EINVAL), window_bits outside {0, 2..16} (SVDW_ERANGE), a
 * planning context (SVDW_EINVAL), n > 0 with a null scalars or out, or an out
 * that overlaps the scalars (SVDW_EINVAL). n == 0: SVDW_OK, nothing is touched
 * (window_bits and windows are still reported). Queued on the context's
 * stream with no host wait between the kernels; the call returns once its two
 * counters have been read back. Scratch is the engine's, 160 B per output,
 * in pieces kept under the option "commit_scratch_mib". */
int svdw_fixed_base_mul(svdw_ctx* ctx, int form, int base_form, const void* base, const void* scalars, uint64_t n,
                        uint32_t window_bits, void* out, svdw_fixed_base_result* result);
typedef struct {
    uint32_t k;
    uint32_t window_bits, windows;   /* of the fixed-base multiplications */
    uint32_t chunks;                 /* pieces of chunk_rows rows (the last may be shorter) */
    uint64_t rows, chunk_rows;       /* 2^k; rows of a full piece */
    uint64_t g_zero_scalars, g_identity_outputs;                 /* over g: s^i == 0; [s^i] G == identity */
    uint64_t lagrange_zero_scalars, lagrange_identity_outputs;   /* over g_lagrange */
    uint32_t secret_in_domain;       /* s^n == 1: g_lagrange is G at the i with omega^i == s, the identity elsewhere */
    uint32_t _pad;
} svdw_srs_result;
/* ParamsKZG::setup(k, .) for the secret s (4 little-endian words, canonical):
 * g (DEVICE, 2^k points in bases_form, or NULL) and g_lagrange (likewise) as
 * defined above; either may be NULL and the other is still written. The two
 * scalar columns are made on the device, s^i from a two-level power table of s,
 * omega^i from the context's domain table, the inverses of s - omega^i by
 * Montgomery's trick over Fr, and both go through svdw_fixed_base_mul's kernel
 * with the planned window. A secret in the domain (s^n = 1, where the formula
 * is 0 / 0) and s = 0 (g = G, identity, ...; g_lagrange = [1 / n] G throughout)
 * are ordinary inputs. Rows are worked through in pieces of what fits the
 * option "commit_scratch_mib" at 192 B per row and array (option
 * "srs_chunk_rows": that many rows instead, a testing aid); the two columns
 * of a piece share one launch of the multiplication. Checks in this order: null ctx, s or
 * result (SVDW_EINVAL), an unknown bases_form (SVDW_EINVAL), s >= p
 * (SVDW_EINVAL), k outside 1..28 (SVDW_ERANGE), a planning context
 * (SVDW_EINVAL), g and g_lagrange overlapping (SVDW_EINVAL). Both NULL:
 * SVDW_OK, nothing is touched. Queued and finished like svdw_fixed_base_mul. */
int svdw_srs_setup(svdw_ctx* ctx, uint32_t k, const uint64_t s[4], int bases_form, void* g, void* g_lagrange,
                   svdw_srs_result* result);
typedef struct {
    uint64_t points_checked, points_off_curve;   /* over both arrays; off the curve as svdw_commit_check counts it */
    uint32_t g_failed;                /* sum_i rho^i g[i] != [((rho s)^n - 1) / (rho s - 1)] G */
    uint32_t lagrange_failed;         /* sum_i rho^i g_lagrange[i] != [sum_i rho^i l_i(s)] G */
} svdw_srs_check;
/* g and g_lagrange (DEVICE, 2^k points in bases_form each, both required)
 * against the secret s, independently of svdw_fixed_base_mul and of the
 * setup's scalar columns: no table, no digits of s^i, no l_i. Every point is
 * tested for the curve; then, with the column rho^i for a caller-chosen rho
 * (canonical, like every challenge of this interface), svdw_commit's Pippenger
 * path gives the two sums above, and each must be one multiple of G, which the
 * host computes bit by bit with the laws of g1.hpp. The first scalar is the
 * geometric sum (n when rho s = 1). The second is the value at s of the
 * polynomial that takes rho^i at omega^i: svdw_ntt (inverse) of the column,
 * then svdw_eval_polynomial at s. A single wrong point passes for at most n of
 * the p choices of rho. Checks in this order: null ctx, s, rho or result
 * (SVDW_EINVAL), an unknown bases_form (SVDW_EINVAL), s or rho >= p
 * (SVDW_EINVAL), k outside 1..28 (SVDW_ERANGE), a planning context
 * (SVDW_EINVAL), a null g or g_lagrange (SVDW_EINVAL). It writes to none of its
 * inputs and returns after the device has finished. Scratch: two columns. */
int svdw_check_srs(svdw_ctx* ctx, uint32_t k, int bases_form, const void* g, const void* g_lagrange,
                   const uint64_t s[4], const uint64_t rho[4], svdw_srs_check* result);
/* ----------------------------------------------------------- G1 transforms
 * What a ceremony's SRS needs, whose secret nobody knows and whose file fixes
 * k at the ceremony's size: halo2_proofs' ParamsKZG::downsize(k) keeps the
 * first 2^k points of g and recomputes the Lagrange half with g_to_lagrange,
 * an inverse FFT over G1: g_lagrange[i] = [1 / n] sum_j [omega^(-i j)] g[j].
 * PARITY PINNED BY THE REFERENCE'S FILE: params/kzg_bn254_8.srs holds both
 * halves, and svdw_g1_fft (inverse) of its g is its g_lagrange byte for byte
 * (tests/golden), no secret involved. halo2_svd041_amd.srs has g_to_lagrange
 * and downsize on top of it. These calls need no witness and no physical
 * layout. Points, forms and the digits are those of the commitments section.
 *
 * An FFT over a group is, per butterfly and stage, one multiplication of an
 * unrelated point by an unrelated scalar, which neither Pippenger's buckets
 * nor svdw_fixed_base_mul's table of one base provide: svdw_g1_mul builds a
 * table of every point's own small multiples and keeps the doublings. */
typedef struct {
    uint32_t window_bits, windows;        /* c and W = ceil(255 / c) as used */
    uint64_t points;                      /* n */
    uint64_t zero_scalars;                /* scalars equal to 0 */
    uint64_t identity_inputs;             /* points equal to (0, 0) */
    uint64_t identity_outputs;            /* outputs that are the identity, written as (0, 0) */
} svdw_g1_mul_result;
/* out[i] = [scalars[i]] points[i] for i < n. points, out: DEVICE, n affine
 * points in bases_form each, (0, 0) the identity; coordinates are taken as
 * svdw_commit takes its bases. scalars: DEVICE, n cells in `form`, taken as
 * integers below p as svdw_fixed_base_mul takes them (a canonical cell may hold
 * r itself: the digits are the integer's). Exactly n points are written.
 * window_bits: 0 for the planned window, or 2..6. Per point a table [d] P,
 * 1 <= d <= 2^(c-1), is built in scratch; the digits are walked top first, c
 * doublings and at most one complete add per window. The planned window is
 * the c <= 4 with the fewest field products (4: 3298 a multiplication) whose
 * scratch for 2^17 points fits the option "commit_scratch_mib"; 5 has 2 % fewer
 * products and twice the table, and measured slower at 2^20. The checks of the arguments come
 * first, before anything touches the device, in this order: null ctx or result
 * (SVDW_EINVAL), an unknown form or bases_form (SVDW_EINVAL), window_bits
 * outside {0, 2..6} (SVDW_ERANGE), a planning context (SVDW_EINVAL), n > 0 with
 * a null points, scalars or out, or an out that overlaps the points or the
 * scalars (SVDW_EINVAL). n == 0: SVDW_OK, nothing is touched (window_bits and
 * windows are still reported). Queued on the context's stream with no host
 * wait between the kernels; the call returns once its counters have been read
 * back. Scratch is the engine's, (2^(c-1) + 1) 128 B per point, worked through
 * in pieces kept under the option "commit_scratch_mib". */
int svdw_g1_mul(svdw_ctx* ctx, int form, int bases_form, const void* points, const void* scalars, uint64_t n,
                uint32_t window_bits, void* out, svdw_g1_mul_result* result);
typedef struct {
    uint32_t k, stages;                   /* stages == k */
    uint32_t window_bits, windows;        /* of the twiddle multiplications (the planned window) */
    uint64_t rows;                        /* 2^k */
    uint64_t multiplications;             /* twiddle multiplications done; a twiddle of 1 is not multiplied */
    uint64_t identity_inputs, identity_outputs;
} svdw_g1_fft_result;
/* The FFT over G1 of size n = 2^k, natural order on both sides:
 *   forward  out[i] = sum_j [omega_k^(i j)] points[j]
 *   inverse  out[i] = [2^-k] sum_j [omega_k^(-i j)] points[j]   (g_to_lagrange)
 * points, out: DEVICE, 2^k affine points in bases_form each; they must not
 * overlap. Radix 2, decimation in time: the bit reversal and the first stage
 * (twiddle 1) in one kernel, then one stage at a time over a working array of
 * 2^k XYZZ points, a butterfly (a + [w] b, a - [w] b) with w from the
 * context's domain table and [w] b by svdw_g1_mul's kernels; a butterfly whose
 * twiddle is 1 multiplies nothing. The inverse folds 2^-k into its last stage,
 * [c] a +- [c w] b, which costs n / 2 multiplications more where a scaling
 * pass would cost n: multiplications = k n / 2 - n + 1 forward and
 * k n / 2 - n / 2 + 2 inverse, counted on the device. Checks in this order: null
 * ctx or result (SVDW_EINVAL), an unknown bases_form (SVDW_EINVAL), k outside
 * 1..28 (SVDW_ERANGE), a planning context (SVDW_EINVAL), a null points or out,
 * or an out that overlaps the points (SVDW_EINVAL). Queued and finished like
 * svdw_g1_mul. Scratch: the working array, 128 B 2^k, outside the option
 * "commit_scratch_mib" (a transform has no pieces; SVDW_ENOMEM when it cannot
 * be had), and the tables of a stage, in pieces under that option. */
int svdw_g1_fft(svdw_ctx* ctx, uint32_t k, int bases_form, int inverse, const void* points, void* out,
                svdw_g1_fft_result* result);
typedef struct {
    uint64_t points_checked, points_off_curve;   /* over both arrays; off the curve as svdw_commit_check counts it */
    uint32_t failed;                  /* sum_i rho^i g_lagrange[i] != sum_j c_j g[j] */
    uint32_t _pad;
} svdw_lagrange_check;
/* g_lagrange against g (DEVICE, 2^k points in bases_form each, both required)
 * without a secret and independently of svdw_g1_fft: no butterfly, no
 * variable-base multiplication. Every point is tested for the curve; then,
 * with the column v_i = rho^i for a caller-chosen rho (canonical) and its
 * coefficients c = svdw_ntt (inverse) of v, svdw_commit's Pippenger path gives
 * sum_i v_i g_lagrange[i] and sum_j c_j g[j], which the host compares. When
 * g_lagrange is the inverse transform of g the two are equal for every rho; a
 * single wrong point passes for at most n of the p choices of rho. rho = 0
 * sees row 0 of g_lagrange alone. It proves that the two halves agree. It does
 * NOT prove that g is a sequence of powers [s^j] G of one secret: that needs
 * the G2 half and a pairing, which stay with the caller. It is also what to
 * run on a file one was handed. Checks in this order: null ctx, rho or result
 * (SVDW_EINVAL), an unknown bases_form (SVDW_EINVAL), rho >= p (SVDW_EINVAL), k
 * outside 1..28 (SVDW_ERANGE), a planning context (SVDW_EINVAL), a null g or
 * g_lagrange (SVDW_EINVAL). It writes to none of its inputs and returns after
 * the device has finished. Scratch: two columns. */
int svdw_check_lagrange(svdw_ctx* ctx, uint32_t k, int bases_form, const void* g, const void* g_lagrange,
                        const uint64_t rho[4], svdw_lagrange_check* result);
/* ---------------------------------------------------------------- openings
 * The quotient polynomials of halo2_proofs' poly::kzg::multiopen::shplonk
 * prover (ProverSHPLONK::create_proof) for polynomials held as coefficient
 * columns on the device. Restated from memory like the steps above: PARITY
 * UNPINNED; the rule below is the specification. These calls need no witness
 * and no physical layout. All arithmetic is exact mod p; cells are taken as
 * field elements below p.
 *
 * ncols polynomials p_j of n = 2^k coefficients each (cols: HOST array of DEVICE
 * pointers, cells in `form`, as svdw_ntt takes them). set_of[j] < nsets assigns
 * p_j to a rotation set; set i holds npoints[i] points S_i, 1 <= npoints[i] <= 8,
 * canonical and pairwise distinct, nsets <= 255. points: HOST, nsets x 8 x 4
 * words, the points of set i in slots 8 i .. 8 i + npoints[i] - 1 (the other
 * slots are not read). Every set holds a polynomial. T is the union of the S_i
 * as field elements, Z_A(X) = prod_{s in A} (X - s). The challenges y, v, u are
 * the caller's (canonical), as beta, gamma, y and x are everywhere else.
 *
 *  1. Fold per set:  F_i(X) = Horner in y over the polynomials of set i in
 *     index order: acc starts at 0 and acc <- acc y + p_j.
 *  2. Quotient per set:  Q_i = the Euclidean quotient of F_i by Z_{S_i}, which
 *     equals (F_i - r_i) / Z_{S_i} with r_i the interpolant of F_i on S_i:
 *     successive synthetic divisions by (X - s), s in S_i in the order given,
 *     each remainder dropped. No evaluation is needed.
 *  3. First quotient:  h1(X) = Horner in v over the sets in index order: acc
 *     starts at 0 and acc <- acc v + Q_i. The caller commits h1 (svdw_commit on
 *     g) and derives u.
 *  4. Second quotient:  z_i = Z_{T \ S_i}(u), c_i = z_i / z_0,
 *       G(X) = (Horner in v of c_i F_i(X)) - Z_{S_0}(u) h1(X),
 *     h2 = the Euclidean quotient of G by (X - u). The dropped remainder G(u)
 *     equals the same Horner in v of c_i r_i(u), the verifier's constant, when
 *     h1 is step 3's; the call reports the remainder and does not subtract the
 *     constant.
 *
 * What stays with the caller: the transcript, deriving y, v, u (and x),
 * blinding, the commitments of h1 and h2 (svdw_commit), G2 and the pairing. */
typedef struct {
    uint32_t columns, sets;
    uint32_t points;          /* |T| */
    uint32_t passes;          /* divisions by one (X - s): sum of npoints (quotient), 1 (linearise) */
    uint64_t rows;            /* 2^k */
    uint64_t remainder[4];    /* svdw_open_linearise: G(u), canonical; else zero */
} svdw_open_result;
/* h1_out: DEVICE, 2^k cells in `form`; the top min_i |S_i| cells are written as
 * zero (the degree of Q_i is n - 1 - |S_i|, that of h1 the largest of them). The checks of the arguments come
 * first, before anything touches the device, in this order: an unknown form
 * (SVDW_EINVAL); y or v >= p, then a point >= p, then two equal points in a set,
 * then a set_of[j] >= nsets, then a set without a polynomial (all SVDW_EINVAL;
 * of the sets at most 256 and of each at most 8 points are looked at here); k
 * outside 1..28
 * (SVDW_ERANGE); a planning context (SVDW_EINVAL); more than 65535 columns, then
 * nsets outside 1..255 or an npoints[i] outside 1..8 (SVDW_ERANGE); null
 * pointers (SVDW_EINVAL); h1_out overlapping an input column (SVDW_EINVAL).
 * ncols == 0: SVDW_OK, nothing is touched. The call is queued on the context's
 * streams like svdw_ntt, with no host wait; scratch (one column of 2^k cells,
 * the tile carries and a power table per point) is the engine's. */
int svdw_open_quotient(svdw_ctx* ctx, uint32_t k, int form, const void* const* cols, uint32_t ncols,
                       const uint32_t* set_of, const uint64_t* points, const uint32_t* npoints, uint32_t nsets,
                       const uint64_t y[4], const uint64_t v[4], void* h1_out, svdw_open_result* result);
/* h2 from the same arguments, u and h1 (DEVICE, 2^k cells in `form`): h2_out
 * (DEVICE, 2^k cells in `form`; its top cell is written as zero) and
 * result->remainder = G(u), read back as the grand products read their
 * counters. Checks as for svdw_open_quotient with u >= p beside y and v, and
 * u in T (SVDW_EINVAL: z_0 or a divisor would be zero) after the empty set;
 * h2_out overlapping an input column or h1 (SVDW_EINVAL). */
int svdw_open_linearise(svdw_ctx* ctx, uint32_t k, int form, const void* const* cols, uint32_t ncols,
                        const uint32_t* set_of, const uint64_t* points, const uint32_t* npoints, uint32_t nsets,
                        const uint64_t y[4], const uint64_t v[4], const uint64_t u[4], const void* h1, void* h2_out,
                        svdw_open_result* result);
typedef struct {
    uint64_t lhs1[4], rhs1[4];    /* h1(t) Z_T(t); Horner in v of Z_{T \ S_i}(t) (F_i(t) - r_i(t)) */
    uint64_t lhs2[4], rhs2[4];    /* G(t) - constant; h2(t) (t - u) */
    uint64_t constant[4];         /* Horner in v of c_i r_i(u) */
    uint64_t identity1_failures;  /* 0 or 1: lhs1 != rhs1 */
    uint64_t identity2_failures;  /* 0 or 1: lhs2 != rhs2 */
    uint64_t h1_top_checked, h1_top_nonzero;   /* the top min_i |S_i| cells of h1 */
    uint64_t h2_top_checked, h2_top_nonzero;   /* the top cell of h2 */
} svdw_open_check;
/* The independent check of h1 and h2 (DEVICE, 2^k cells in `form`) at a
 * caller-chosen point t (canonical; >= p: SVDW_EINVAL, with the challenges). It
 * shares no fold and no scan with the two calls above: every column is
 * evaluated at its set's points and at t, h1 and h2 at t, with the kernels of
 * svdw_eval_polynomial; the host folds the evaluations with y, interpolates each
 * r_i (Lagrange on at most 8 points) and tests
 *   h1(t) Z_T(t) == Horner in v of Z_{T \ S_i}(t) (F_i(t) - r_i(t)),
 *   G(t) - constant == h2(t) (t - u),   constant = Horner in v of c_i r_i(u).
 * evals_out: HOST, ncols x 8 x 4 words, canonical: slot q of column j is
 * p_j(S_{set_of[j]}[q]), the evals the transcript takes; unused slots zero.
 * Arguments and their checks as for svdw_open_linearise (there is no output
 * to overlap); it writes to none of its device inputs and returns after the
 * device has finished. */
int svdw_check_open(svdw_ctx* ctx, uint32_t k, int form, const void* const* cols, uint32_t ncols,
                    const uint32_t* set_of, const uint64_t* points, const uint32_t* npoints, uint32_t nsets,
                    const uint64_t y[4], const uint64_t v[4], const uint64_t u[4], const void* h1, const void* h2,
                    const uint64_t t[4], uint64_t* evals_out, svdw_open_check* result);
/* out[r] = sum_j scalars[j] cols[j][r] over ncols columns of 2^k cells in
 * `form` (cols as above; scalars: HOST, ncols x 4 words, canonical; out:
 * DEVICE, 2^k cells in `form`): the fold kernel of the opening by itself.
 * create_proof opens the pieces of h as the one polynomial sum_i x^(n i) h_i,
 * which is this call on the pieces with the scalars x^(n i). Checks in this
 * order: form (SVDW_EINVAL), a scalar >= p (SVDW_EINVAL), k outside 1..28
 * (SVDW_ERANGE), a planning context (SVDW_EINVAL), more than 65535 columns
 * (SVDW_ERANGE), null pointers (SVDW_EINVAL), out overlapping an input column
 * (SVDW_EINVAL). ncols == 0: SVDW_OK, nothing is touched. Queued with no host
 * wait. */
int svdw_linear_combination(svdw_ctx* ctx, uint32_t k, int form, const void* const* cols, uint32_t ncols,
                            const uint64_t* scalars, void* out);
/* Up to cap segments of the last witness into out; *n = total count. */
int svdw_shard_segments(const svdw_ctx* ctx, svdw_segment* out, uint64_t cap, uint64_t* n);

/* ------------------------------------------------------------ input ingest
 * Parse the example's input file (data/matrix.in of input-creator.py:23-44;
 * read by examples/svd_example.rs:326-330 with serde_json::from_str) into
 * row-major f64 arrays. mode SVDW_PARSE_SERDE reproduces serde_json's default
 * float parse (u64 significand x / / 10^|e| in f64; 1 ulp off correct rounding
 * on ~10 % of the values, which changes quantized cells), SVDW_PARSE_CORRECT
 * rounds correctly. Call with null arrays to get the shapes, then again with
 * arrays of those sizes. */
#define SVDW_PARSE_SERDE 0
#define SVDW_PARSE_CORRECT 1
typedef struct {
    uint32_t m_rows, m_cols, u_rows, u_cols, v_rows, v_cols, d_len;
} svdw_input_dims;
int svdw_parse_svd_input(const char* text, uint64_t len, int mode, svdw_input_dims* dims,
                         double* m, double* u, double* d, double* v);
/* The same parse of text already in device memory, on the context's device
 * (serde mode only): m, u, d, v are DEVICE pointers (null: dims only), ready for
 * svdw_svd_witness(on_device = 1). Replaces examples/svd_example.rs:326-330
 * (read_to_string + serde_json::from_str) for a file staged to HBM; the values
 * are identical to svdw_parse_svd_input's (SVDW_PARSE_SERDE) on every input, and
 * malformed text is rejected (SVDW_EINVAL). Synchronous. */
int svdw_parse_svd_input_device(svdw_ctx* ctx, const void* text, uint64_t len, int mode,
                                svdw_input_dims* dims, double* m, double* u, double* d, double* v);

/* ----------------------------------------------------------- decomposition
 * The singular value decomposition itself, m = u diag(d) v, on the device in
 * f64: what input-creator.py:30 (`u, d, v = lin.svd(m)`) asks of LAPACK, so that
 * a witness needs no host linear algebra. The circuit is the specification of
 * a good factorisation (check_svd_phase0: d non-negative and descending, the
 * entries of u and v inside (-1, 1), |u d - m v^T| < err_svd, |u u^T - I| and
 * |v v^T - I| < err_u after quantization), and svdw_check_gates on the witness
 * made from the factors is its acceptance test. NO PARITY WITH LAPACK: singular
 * vectors are unique up to sign (and up to a rotation among equal singular
 * values), and the method differs; d agrees to rounding.
 *
 * Blocked one-sided (Hestenes) Jacobi. With R = min(N, M), C = max(N, M) it works
 * on G = m (N <= M) or m^T (N > M), R x C, and W = I (C x C): columns of G and W
 * are rotated together until G's columns are mutually orthogonal. Columns go in
 * panels of b; a sweep is the round-robin tournament over panel pairs; per pair
 * the 2b x 2b Gram matrix (b = 8: one v_mfma_f64_16x16x4_f64 tile), `inner`
 * cyclic Jacobi sweeps on it, and the product of the rotations applied to the
 * pair's columns (matrix cores at b = 8). A rotation of columns i, j is skipped
 * when h_ij^2 <= eps^2 h_ii h_jj or min(h_ii, h_jj) <= (eps |m|_F)^2, eps = 2^-52;
 * a sweep without a rotation ends the iteration. No floating-point atomics: the
 * result is the same bytes from run to run. Then d = the column norms sorted
 * descending (stable), the R x R factor the normalised columns, the C x C factor
 * W. A column j < R whose norm is <= C eps d_0 (rank deficiency; d_0 = 0 is the
 * zero matrix) keeps its norm as d_j and gets its vector by completion on the
 * host: unit vectors orthogonalised twice against all other columns. The zero
 * matrix gives d = 0, u = I, v = I. */
typedef struct {
    uint32_t panel;        /* columns per panel b: 1, 4 or 8; 0 = default (8) */
    uint32_t inner;        /* sweeps of the in-block eigen solve; 0 = default (2) */
    uint32_t max_sweeps;   /* 0 = default (40) */
} svdw_svd_opts;
typedef struct {
    uint32_t sweeps, converged, completed;   /* completed: u / v columns made by completion */
    uint64_t rotations;
    double off;            /* largest |h_ij| / sqrt(h_ii h_jj) seen in the last sweep */
    uint64_t pairs;        /* panel pairs visited: sweeps (P - 1) P / 2 for P panels (padded to even) */
    uint64_t skipped_pairs; /* of those, pairs whose solve made no rotation: their apply is skipped */
} svdw_svd_info;
/* u (N x N), d (min(N, M)) and v (M x M, the rows of V^T as numpy's third output
 * and the reference's v) from m (N x M); all row-major f64, all four in host
 * memory (on_device = 0) or all four in DEVICE memory (on_device = 1, then
 * svdw_svd_witness(on_device = 1) reads u, d, v where they lie). opts and info
 * may be null. Checks in this order, the first six before anything touches the
 * device: null ctx (SVDW_EINVAL), N or M == 0 (SVDW_EINVAL), a null m, u, d or v
 * (SVDW_EINVAL), an output that overlaps m or another output (SVDW_EINVAL), a
 * panel other than 0, 1, 4, 8 or a dimension above 2^20 (SVDW_ERANGE), a planning
 * context (SVDW_EINVAL, as svdw_ntt refuses it); workspace that cannot be had
 * (SVDW_ENOMEM); an entry of m that is NaN or infinite (SVDW_EINVAL: found by the
 * kernel that loads m, and u, d, v are not written). Not converged within
 * max_sweeps is SVDW_OK with converged = 0 and the factors of the last sweep:
 * the caller decides. Synchronous, like svdw_parse_svd_input_device: it waits
 * for the context's queued work (and what svdw_stream_wait ordered it after),
 * reads one counter back per sweep and returns when u, d, v are written, so a
 * witness call that follows on the same context needs nothing in between.
 * Workspace is the engine's, kept on the context: 8 (R + C) C bytes for G
 * stacked on W, plus m, u, d, v staged when they are the host's. */
int svdw_svd_decompose(svdw_ctx* ctx, const double* m, uint32_t N, uint32_t M, int on_device,
                       const svdw_svd_opts* opts, double* u, double* d, double* v, svdw_svd_info* info);

/* Closed-form cell counts of svdw_svd_witness without touching a device. */
int svdw_plan_svd(uint32_t N, uint32_t M, uint32_t precision_bits, uint32_t lookup_bits,
                  const svdw_svd_config* cfg, svdw_counts* counts);

#ifdef __cplusplus
}
#endif
#endif /* SVDW_H */
