// Text ingest of data/matrix.in: the host parser (ingest.hpp) and the device
// parser (ingest_dev.hpp) behind the C ABI.
#include <stdio.h>
#include <stdlib.h>

#include "engine_internal.hpp"
#include "ingest.hpp"
#include "ingest_dev.hpp"

extern "C" {

int svdw_parse_svd_input(const char* text, uint64_t len, int mode, svdw_input_dims* dims,
                         double* m, double* u, double* d, double* v) {
    return guarded([&] {
        REQUIRE(text && dims, "null argument");
        REQUIRE(mode == SVDW_PARSE_SERDE || mode == SVDW_PARSE_CORRECT, "parse mode: 0 or 1");
        svdw_ingest::SvdInput in;
        std::string err;
        svdw_ingest::Parser ps(text, len, mode);
        if (!ps.parse(in, err)) fail(SVDW_EINVAL, "svd input: " + err);
        REQUIRE(in.d.rows == 0 && in.m.rows && in.u.rows && in.v.rows,
                "svd input: m, u, v must be matrices and d a vector");
        *dims = svdw_input_dims{in.m.rows, in.m.cols, in.u.rows, in.u.cols, in.v.rows, in.v.cols,
                                in.d.cols};
        const std::pair<double*, const svdw_ingest::Array*> outs[4] = {
            {m, &in.m}, {u, &in.u}, {d, &in.d}, {v, &in.v}};
        for (const auto& o : outs)
            if (o.first) memcpy(o.first, o.second->v.data(), o.second->v.size() * sizeof(double));
    });
}
// Device ingest of data/matrix.in (ingest_dev.hip): three passes over the text
// on the device, then the few top-level keys and the arrays' number ranges on
// the host (small reads), then a device check of depths, separators and row
// lengths of m, u, v, d and device-to-device copies of their values.
namespace {
struct DevText {                  // small host reads of the device text
    svdw_ctx* c;
    const uint8_t* t;
    uint64_t n;
    std::vector<uint8_t> get(uint64_t at, uint64_t len) {
        len = std::min(len, at < n ? n - at : 0);
        std::vector<uint8_t> b(len);
        if (len) hipck(hipMemcpy(b.data(), t + at, len, hipMemcpyDeviceToHost), "D2H");
        return b;
    }
    // byte i of the text (-1 past its end), read forward in 256-byte pieces
    // that str and next_nonws share
    uint64_t w0 = 0;
    std::vector<uint8_t> w;
    int byte(uint64_t i) {
        if (i >= n) return -1;
        if (i < w0 || i >= w0 + w.size()) { w = get(i, 256); w0 = i; }
        return w[i - w0];
    }
    // the string starting with the quote at `at`: its content (escapes as the
    // host parser reads them) and the position just past the closing quote
    bool str(uint64_t at, std::string* s, uint64_t* end) {
        bool esc = false;
        for (uint64_t p = at + 1;; ++p) {
            const int b = byte(p);
            if (b < 0) return false;
            if (esc) { s->push_back((char)b); esc = false; continue; }
            if (b == '\\') { esc = true; continue; }
            if (b == '"') { *end = p + 1; return true; }
            s->push_back((char)b);
        }
    }
    int next_nonws(uint64_t at, uint64_t* pos = nullptr) {
        for (;; ++at) {
            const int b = byte(at);
            if (b < 0) return -1;
            if (!(b == ' ' || b == '\n' || b == '\r' || b == '\t')) {
                if (pos) *pos = at;
                return b;
            }
        }
    }
    // the last non-blank byte before `at` (0: none), walking back as next_nonws walks
    // forward. Its copies are its own (the shared piece holds bytes read forward only):
    // one per depth-1 string, more only behind a blank run of 256 bytes or longer
    int prev_nonws(uint64_t at) {
        while (at > 0) {
            const uint64_t lo = at >= 256 ? at - 256 : 0;
            std::vector<uint8_t> b = get(lo, at - lo);
            for (size_t q = b.size(); q-- > 0;)
                if (!(b[q] == ' ' || b[q] == '\n' || b[q] == '\r' || b[q] == '\t')) return b[q];
            at = lo;
        }
        return 0;
    }
};
}  // namespace
int svdw_parse_svd_input_device(svdw_ctx* c, const void* text, uint64_t len, int mode,
                                svdw_input_dims* dims, double* m, double* u, double* d, double* v) {
    namespace ig = svdw_ingest_dev;
    return guarded([&] {
        REQUIRE(c && text && dims, "null argument");
        need_device(c, "device ingest");
        REQUIRE(mode == SVDW_PARSE_SERDE,
                "device ingest: serde mode only (correct rounding: svdw_parse_svd_input)");
        REQUIRE(len > 0, "svd input: empty text");
        const uint8_t* t = (const uint8_t*)text;
        const uint64_t nc64 = (len + ig::kChunk - 1) / ig::kChunk;
        REQUIRE(nc64 < (1ull << 31), "svd input: text too large");
        const uint32_t nc = (uint32_t)nc64;
        IngestState& g = c->ingest;
        hipStream_t s = c->st;
        sync(c);
        if (!g.pow10.p) {                       // serde's POW10 table (correctly rounded 10^k)
            std::vector<double> p10(309);
            char buf[16];
            for (int i = 0; i <= 308; ++i) { snprintf(buf, sizeof buf, "1e%d", i); p10[i] = strtod(buf, nullptr); }
            ensure_buf(c, g.pow10, sizeof(double) * 309);
            // on st, complete before p10 goes out of scope (a null-stream copy
            // is not ordered against the parse launches on st)
            hipck(hipMemcpyAsync(g.pow10.p, p10.data(), sizeof(double) * 309, hipMemcpyHostToDevice, s), "H2D");
            hipck(hipStreamSynchronize(s), "hipStreamSynchronize");
        }
        ensure_buf(c, g.xfer, sizeof(ig::Xfer) * nc);
        ensure_buf(c, g.entry, sizeof(ig::Entry) * (nc + 1));
        ensure_buf(c, g.counts, sizeof(ig::Counts) * (nc + 1));
        ig::Xfer* X = (ig::Xfer*)g.xfer.p;
        ig::Entry* E = (ig::Entry*)g.entry.p;
        ig::Counts* C = (ig::Counts*)g.counts.p;
        hipck(ig::launch_pass1(t, len, X, s), "ingest pass 1");
        hipck(ig::launch_scan1(X, nc, E, s), "ingest scan 1");
        hipck(ig::launch_pass2(t, len, E, C, s), "ingest pass 2");
        hipck(ig::launch_scan2(C, nc, s), "ingest scan 2");
        ig::Entry fin;
        ig::Counts tot;
        hipck(hipMemcpyAsync(&fin, E + nc, sizeof fin, hipMemcpyDeviceToHost, s), "D2H");
        hipck(hipMemcpyAsync(&tot, C + nc, sizeof tot, hipMemcpyDeviceToHost, s), "D2H");
        hipck(hipStreamSynchronize(s), "hipStreamSynchronize");
        REQUIRE(fin.state == 0, "svd input: unterminated string");
        REQUIRE(fin.depth == 0, "svd input: unbalanced brackets");
        const uint32_t nn = tot.num, nr = tot.row, nk = tot.key;
        ensure_buf(c, g.values, sizeof(double) * std::max(nn, 1u));
        ensure_buf(c, g.num_pos, sizeof(uint64_t) * std::max(nn, 1u));
        ensure_buf(c, g.num_depth, std::max(nn, 1u));
        ensure_buf(c, g.row_pos, sizeof(uint64_t) * std::max(nr, 1u));
        ensure_buf(c, g.key_pos, sizeof(uint64_t) * std::max(nk, 1u));
        ensure_buf(c, g.errors, sizeof(uint64_t) * 264);
        unsigned long long* slist = (unsigned long long*)g.errors.p;          // [0] count, [1..255]
        unsigned long long* verr = slist + 256;
        hipck(hipMemsetAsync(slist, 0, sizeof(uint64_t), s), "memset");
        hipck(hipMemsetAsync(verr, 0xff, sizeof(uint64_t), s), "memset");
        hipck(ig::launch_pass3(t, len, E, C, (const double*)g.pow10.p, (double*)g.values.p,
                               (uint64_t*)g.num_pos.p, (uint8_t*)g.num_depth.p, (uint64_t*)g.row_pos.p,
                               (uint64_t*)g.key_pos.p, slist, s), "ingest pass 3");
        std::vector<uint64_t> kpos(nk), sl(256);
        if (nk) hipck(hipMemcpyAsync(kpos.data(), g.key_pos.p, sizeof(uint64_t) * nk, hipMemcpyDeviceToHost, s), "D2H");
        hipck(hipMemcpyAsync(sl.data(), slist, sizeof(uint64_t) * 256, hipMemcpyDeviceToHost, s), "D2H");
        hipck(hipStreamSynchronize(s), "hipStreamSynchronize");
        auto at = [](uint64_t p) { return " (at byte " + std::to_string(p) + ")"; };
        // members: depth-1 strings followed by ':' are keys (host parser: str, ws, ':')
        DevText dt{c, t, len};
        struct Member { uint64_t pos; std::string key; };
        std::vector<Member> mem;
        for (uint32_t j = 0; j < nk; ++j) {
            std::string k;
            uint64_t end = 0;
            REQUIRE(dt.str(kpos[j], &k, &end), "svd input: unterminated string" + at(kpos[j]));
            uint64_t colon = 0;
            const int nx = dt.next_nonws(end, &colon);
            // a key follows '{' or ','; a string value follows ':' and is not followed by ':'
            const int pv = dt.prev_nonws(kpos[j]);
            if (pv == ':') {
                REQUIRE(nx != ':', "svd input: expected ',' or '}'" + at(end));
                continue;
            }
            REQUIRE(nx == ':', "svd input: expected ':'" + at(end));
            // m, u, v, d hold arrays (host parser: array() expects '['); a literal or a
            // string there has no number and would pass for an empty d
            if (k == "m" || k == "u" || k == "v" || k == "d")
                REQUIRE(dt.next_nonws(colon + 1) == '[', "svd input: expected '['" + at(colon + 1));
            mem.push_back({kpos[j], k});
        }
        const uint64_t nsl = sl[0];
        REQUIRE(nsl <= 255, "svd input: too many structural irregularities for the device parser");
        for (const char* want : {"m", "u", "v", "d"}) {
            int cnt = 0;
            for (const auto& x : mem) cnt += x.key == want;
            REQUIRE(cnt <= 1, std::string("svd input: duplicate key \"") + want + "\"");
            REQUIRE(cnt == 1, "svd input: missing one of the keys m, u, v, d");
        }
        // number / row-open ranges of every member
        std::vector<uint64_t> q;
        for (const auto& x : mem) q.push_back(x.pos);
        q.push_back(len);
        ensure_buf(c, g.queries, (sizeof(uint64_t) + 2 * sizeof(uint32_t)) * q.size());
        uint32_t* rg = (uint32_t*)((uint64_t*)g.queries.p + q.size());
        hipck(hipMemcpyAsync(g.queries.p, q.data(), sizeof(uint64_t) * q.size(), hipMemcpyHostToDevice, s), "H2D");
        hipck(ig::launch_ranges((const uint64_t*)g.num_pos.p, nn, (const uint64_t*)g.row_pos.p, nr,
                                (const uint64_t*)g.queries.p, (uint32_t)q.size(), rg, s), "ingest ranges");
        std::vector<uint32_t> r(2 * q.size());
        hipck(hipMemcpyAsync(r.data(), rg, sizeof(uint32_t) * r.size(), hipMemcpyDeviceToHost, s), "D2H");
        hipck(hipStreamSynchronize(s), "hipStreamSynchronize");
        for (uint64_t k = 0; k < nsl; ++k) {       // structural errors: object level, or inside m/u/v/d
            const uint64_t p = sl[1 + k] & ~(1ull << 63);
            REQUIRE(!(sl[1 + k] >> 63), "svd input: malformed JSON object" + at(p));
            for (size_t j = 0; j < mem.size(); ++j) {
                const bool known = mem[j].key == "m" || mem[j].key == "u" || mem[j].key == "v" || mem[j].key == "d";
                REQUIRE(!(known && p >= q[j] && p < q[j + 1]), "svd input: malformed array" + at(p));
            }
        }
        struct Arr { uint32_t lo, hi, r0, rows, cols; };
        auto arr = [&](const char* key, bool matrix) {
            size_t j = 0;
            while (mem[j].key != key) ++j;
            Arr a{r[2 * j], r[2 * j + 2], r[2 * j + 1], r[2 * j + 3] - r[2 * j + 1], 0};
            const uint32_t total = a.hi - a.lo;
            if (matrix) {
                REQUIRE(a.rows >= 1, "svd input: m, u, v must be matrices and d a vector");
                REQUIRE(total % a.rows == 0, std::string("svd input: ragged matrix rows (") + key + ")");
                a.cols = total / a.rows;
            } else {
                REQUIRE(a.rows == 0, "svd input: m, u, v must be matrices and d a vector");
                a.cols = total;
            }
            hipck(ig::launch_validate((const uint8_t*)g.num_depth.p, a.lo, a.hi, matrix ? 3 : 2,
                                      (const uint64_t*)g.num_pos.p, nn, (const uint64_t*)g.row_pos.p,
                                      a.r0, a.rows, a.cols, verr, s), "ingest validate");
            return a;
        };
        const Arr am = arr("m", true), au = arr("u", true), av = arr("v", true), ad = arr("d", false);
        unsigned long long ve = 0;
        hipck(hipMemcpyAsync(&ve, verr, sizeof ve, hipMemcpyDeviceToHost, s), "D2H");
        hipck(hipStreamSynchronize(s), "hipStreamSynchronize");
        if (ve != ~0ull) {
            static const char* what[] = {"", "expected a number", "significand beyond u64 (serde's overflow path is not emulated)",
                                         "number out of range", "expected ',' or ']'", "unexpected nesting",
                                         "ragged matrix rows"};
            const uint32_t code = (uint32_t)(ve >> 48);
            fail(SVDW_EINVAL, std::string("svd input: ") + (code < 7 ? what[code] : "malformed") +
                              at(ve & ((1ull << 48) - 1)));
        }
        *dims = svdw_input_dims{am.rows, am.cols, au.rows, au.cols, av.rows, av.cols, ad.cols};
        const std::pair<double*, const Arr*> outs[4] = {{m, &am}, {u, &au}, {d, &ad}, {v, &av}};
        for (const auto& o : outs)
            if (o.first && o.second->hi > o.second->lo)
                hipck(hipMemcpyAsync(o.first, (const double*)g.values.p + o.second->lo,
                                     sizeof(double) * (o.second->hi - o.second->lo), hipMemcpyDeviceToDevice, s),
                      "D2D");
        hipck(hipStreamSynchronize(s), "hipStreamSynchronize");
    });
}

}  // extern "C"
