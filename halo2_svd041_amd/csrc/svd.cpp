// The decomposition call of the C ABI (include/svdw.h, "decomposition"; kernels:
// svd.hip, the method: svd.hpp): svdw_svd_decompose. It checks its arguments in
// the order the header documents, sizes its workspace on the context ahead of
// the first launch, queues every kernel on the context's stream and reads the
// sweep's counters back once per sweep through pinned memory. The sort of the norms and the
// completion of columns that cannot be normalised are the host's: O(C log C)
// and O(R^2) per such column and try (svd_complete). Of the context this file
// uses the stream, the profiler, sync, ensure_buf and its own SvdState.
#include <string.h>

#include <algorithm>
#include <cmath>
#include <numeric>

#include "engine_internal.hpp"
#include "svd.hpp"

static constexpr uint32_t kSvdDefaultPanel = 8, kSvdDefaultInner = 2, kSvdDefaultSweeps = 40;
static constexpr uint32_t kSvdMaxDim = 1u << 20;           // L = R + C and the chunk counts stay far inside 32 bits
static constexpr double kSvdHostEps = 0x1p-52;

static bool svd_overlap(const void* a, uint64_t abytes, const void* b, uint64_t bbytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return !(a0 + abytes <= b0 || b0 + bbytes <= a0);
}

// Vectors `missing` of the R x R factor q (element i of vector j at q[j sj + i si]) from unit vectors,
// orthogonalised twice (modified Gram-Schmidt) against every other vector. A unit vector is taken when it
// keeps 1 / (2 R) of its square (one of those not yet tried keeps 1 / R, their average). The search goes on
// from the unit vector after the last one taken, wrapping, and never goes back: a unit vector taken lies in the
// span of what the factor holds from then on and would only fail again. A try costs O(R) per vector held:
// O(R^2) a column when its first try is taken, as it is when the held vectors leave the next unit vector
// alone (the zero matrix, where completion gives the identity), and O(R^2) more per failed try, at most R
// tries a column. Restarting every column at the first unit vector made j - 1 failed tries for column j.
static void svd_complete(double* q, uint32_t R, size_t si, size_t sj, const std::vector<uint32_t>& missing) {
    std::vector<char> have(R, 1);
    for (uint32_t j : missing) have[j] = 0;
    // the vectors held, gathered contiguous once: a pass then streams them
    std::vector<double> held;
    held.reserve((size_t)R * R);
    for (uint32_t o = 0; o < R; ++o)
        if (have[o])
            for (uint32_t i = 0; i < R; ++i) held.push_back(q[o * sj + i * si]);
    std::vector<double> x(R);
    uint32_t k = 0;                                         // the next unit vector to try
    for (uint32_t j : missing) {
        for (uint32_t tries = 0; tries < R; ++tries, k = (k + 1) % R) {
            std::fill(x.begin(), x.end(), 0.0);
            x[k] = 1.0;
            const size_t n = held.size() / R;
            for (int pass = 0; pass < 2; ++pass)
                for (size_t o = 0; o < n; ++o) {
                    const double* qo = held.data() + o * R;
                    double dot = 0.0;
                    for (uint32_t i = 0; i < R; ++i) dot += qo[i] * x[i];
                    for (uint32_t i = 0; i < R; ++i) x[i] -= dot * qo[i];
                }
            double nn = 0.0;
            for (uint32_t i = 0; i < R; ++i) nn += x[i] * x[i];
            if (nn >= 1.0 / (2.0 * R)) {
                const double s = std::sqrt(nn);
                for (uint32_t i = 0; i < R; ++i) {
                    x[i] /= s;
                    q[j * sj + i * si] = x[i];
                }
                held.insert(held.end(), x.begin(), x.end());
                k = (k + 1) % R;
                break;
            }
        }
    }
}

int svdw_svd_decompose(svdw_ctx* c, const double* m, uint32_t N, uint32_t M, int on_device, const svdw_svd_opts* opts,
                       double* u, double* d, double* v, svdw_svd_info* info) {
    return guarded([&] {
        const std::string f = "svdw_svd_decompose";
        REQUIRE(c, f + ": null ctx");
        REQUIRE(N >= 1 && M >= 1, f + ": empty matrix");
        REQUIRE(m && u && d && v, f + ": null argument");
        const uint32_t R = std::min(N, M), C = std::max(N, M);
        const uint64_t mb = (uint64_t)N * M * 8, ub = (uint64_t)N * N * 8, vb = (uint64_t)M * M * 8, db = (uint64_t)R * 8;
        REQUIRE(!svd_overlap(u, ub, m, mb) && !svd_overlap(d, db, m, mb) && !svd_overlap(v, vb, m, mb),
                f + ": an output overlaps m");
        REQUIRE(!svd_overlap(u, ub, d, db) && !svd_overlap(u, ub, v, vb) && !svd_overlap(d, db, v, vb),
                f + ": the outputs overlap each other");
        const uint32_t b = opts && opts->panel ? opts->panel : kSvdDefaultPanel;
        if (b != 1 && b != 4 && b != 8) fail(SVDW_ERANGE, f + ": panel must be 0, 1, 4 or 8");
        if (C > kSvdMaxDim) fail(SVDW_ERANGE, f + ": a dimension above 2^20");
        need_device(c, f);
        const uint32_t inner = opts && opts->inner ? opts->inner : kSvdDefaultInner;
        const uint32_t max_sweeps = opts && opts->max_sweeps ? opts->max_sweeps : kSvdDefaultSweeps;
        if (info) memset(info, 0, sizeof *info);
        sync(c);
        SvdArgs a{};
        a.R = R;
        a.C = C;
        a.L = R + C;
        a.b = b;
        a.P = (C + b - 1) / b;
        a.P += a.P & 1;
        a.inner = inner;
        a.gram_chunks = (R + kSvdRows - 1) / kSvdRows;
        a.apply_chunks = (a.L + kSvdRows - 1) / kSvdRows;
        const uint64_t Cp = (uint64_t)a.P * b;
        // everything that may allocate comes ahead of the first launch
        const uint64_t a_bytes = Cp * a.L * 8, g_bytes = (uint64_t)(a.P / 2) * a.gram_chunks * kSvdGramCells * 8,
                       n_bytes = Cp * 8, p_bytes = (Cp * 4 + 7) / 8 * 8;
        ensure_buf(c, c->svd.ws, a_bytes + g_bytes + n_bytes + p_bytes + sizeof(SvdWords));
        if (!on_device) ensure_buf(c, c->svd.io, mb + ub + vb + db);
        if (!c->svd.pinned && hipHostMalloc((void**)&c->svd.pinned, 64, hipHostMallocDefault) != hipSuccess) {
            c->svd.pinned = nullptr;
            fail(SVDW_ENOMEM, f + ": pinned host allocation failed");
        }
        unsigned long long* pin = c->svd.pinned;
        char* ws = (char*)c->svd.ws.p;
        a.A = (double*)ws;
        a.gram = (double*)(ws + a_bytes);
        a.norms = (double*)(ws + a_bytes + g_bytes);
        uint32_t* perm = (uint32_t*)(ws + a_bytes + g_bytes + n_bytes);
        a.words = (SvdWords*)(ws + a_bytes + g_bytes + n_bytes + p_bytes);
        const double* dm = m;
        double *du = u, *dd = d, *dv = v;
        if (!on_device) {
            char* io = (char*)c->svd.io.p;
            dm = (const double*)io;
            du = (double*)(io + mb);
            dv = (double*)(io + mb + ub);
            dd = (double*)(io + mb + ub + vb);
            hipck(hipMemcpyAsync(io, m, mb, hipMemcpyHostToDevice, c->st), "H2D");
        }
        hipck(hipMemsetAsync(a.words, 0, sizeof(SvdWords), c->st), "hipMemsetAsync");
        profiled(c, "k_svd_load", (double)(mb + a_bytes), [&] { return launch_svd_load(a, dm, N, M, c->st); });
        profiled(c, "k_svd_tiny", (double)n_bytes, [&] { return launch_svd_tiny(a, c->st); });
        hipck(hipMemcpyAsync(pin, &a.words->nonfinite, 8, hipMemcpyDeviceToHost, c->st), "D2H");
        hipck(hipStreamSynchronize(c->st), "hipStreamSynchronize");
        REQUIRE(pin[0] == 0, f + ": m has an entry that is not finite");
        uint32_t sweeps = 0, converged = 0;
        uint64_t rotations = 0, skipped = 0;
        double off = 0.0;
        const double g_step = (double)Cp * R * 8, r_step = 2.0 * (double)Cp * a.L * 8;
        while (sweeps < max_sweeps) {
            hipck(hipMemsetAsync(&a.words->rotations, 0, 24, c->st), "hipMemsetAsync");
            for (uint32_t step = 0; step + 1 < a.P; ++step) {
                profiled(c, "k_svd_gram", g_step, [&] { return launch_svd_gram(a, step, c->st); });
                profiled(c, "k_svd_rotate", r_step, [&] { return launch_svd_rotate(a, step, c->st); });
            }
            hipck(hipMemcpyAsync(pin, &a.words->rotations, 24, hipMemcpyDeviceToHost, c->st), "D2H");
            hipck(hipStreamSynchronize(c->st), "hipStreamSynchronize");
            ++sweeps;
            rotations += pin[0];
            skipped += pin[2];
            memcpy(&off, &pin[1], 8);
            if (pin[0] == 0) {
                converged = 1;
                break;
            }
        }
        // the norms, their order, d's floor and the columns below it
        profiled(c, "k_svd_norms", (double)Cp * R * 8, [&] { return launch_svd_norms(a, c->st); });
        std::vector<double> norms(C);
        hipck(hipMemcpyAsync(norms.data(), a.norms, (size_t)C * 8, hipMemcpyDeviceToHost, c->st), "D2H");
        hipck(hipStreamSynchronize(c->st), "hipStreamSynchronize");
        std::vector<uint32_t> order(C);
        std::iota(order.begin(), order.end(), 0u);
        std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return norms[x] > norms[y]; });
        const double floor = (double)C * kSvdHostEps * norms[order[0]];
        std::vector<uint32_t> missing;
        for (uint32_t j = 0; j < R; ++j)
            if (!(norms[order[j]] > floor)) missing.push_back(j);
        hipck(hipMemcpyAsync(perm, order.data(), (size_t)C * 4, hipMemcpyHostToDevice, c->st), "H2D");
        profiled(c, "k_svd_write", (double)(ub + vb) * 2, [&] { return launch_svd_write(a, perm, N, M, floor, du, dd, dv, c->st); });
        // the R x R factor: u's columns (N <= M) or v's rows
        const bool wide = N <= M;
        double* const host_q = wide ? u : v;
        double* const dev_q = wide ? du : dv;
        const size_t si = wide ? R : 1, sj = wide ? 1 : R;
        if (!on_device) {
            hipck(hipMemcpyAsync(u, du, ub, hipMemcpyDeviceToHost, c->st), "D2H");
            hipck(hipMemcpyAsync(v, dv, vb, hipMemcpyDeviceToHost, c->st), "D2H");
            hipck(hipMemcpyAsync(d, dd, db, hipMemcpyDeviceToHost, c->st), "D2H");
            hipck(hipStreamSynchronize(c->st), "hipStreamSynchronize");
            if (!missing.empty()) svd_complete(host_q, R, si, sj, missing);
        } else {
            hipck(hipStreamSynchronize(c->st), "hipStreamSynchronize");
            if (!missing.empty()) {
                std::vector<double> q((size_t)R * R);
                hipck(hipMemcpy(q.data(), dev_q, q.size() * 8, hipMemcpyDeviceToHost), "D2H");
                svd_complete(q.data(), R, si, sj, missing);
                hipck(hipMemcpy(dev_q, q.data(), q.size() * 8, hipMemcpyHostToDevice), "H2D");
            }
        }
        if (info) {
            info->sweeps = sweeps;
            info->converged = converged;
            info->completed = (uint32_t)missing.size();
            info->rotations = rotations;
            info->off = off;
            info->pairs = (uint64_t)sweeps * (a.P - 1) * (a.P / 2);
            info->skipped_pairs = skipped;
        }
    });
}
