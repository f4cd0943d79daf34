// The calls of the C ABI (include/svdw.h) that turn a finished witness into
// circuit inputs: its checker, the physical layout with its columns and checks,
// the equality records, the permutation argument's edge list, the fixed columns,
// and the getters of what a witness left behind. Of a context they read that and
// the cell streams; what their kernels read is staged like the prover calls'
// (stage, engine_internal.hpp), and their own buffers are CircuitState's.
#include <algorithm>

#include "engine_internal.hpp"
#include "export.hpp"
#include "permutation_cycles.hpp"

// ------------------------------------------------------- regions and gates
// A region is `rows` inner-product rows [C(0), E(a_0), E(v_0), W(s_0), E(a_1), ...]
// (a scan; RegionChecks::scan, set with the "scan" tag of its layout entry) or
// elements of a cell program. Its unit is one row, or one element.
static uint64_t unit_cells(const svdw_region& r, const RegionChecks& rc) { return rc.scan ? r.n / r.rows : rc.unit; }
// bit[o]: does a basic gate a + b c = d start at offset o of a unit? In a scan
// row at every third cell except the last, in a program where its check words say.
static std::vector<uint8_t> gate_starts(const svdw_region& r, const RegionChecks& rc) {
    const uint64_t unit = unit_cells(r, rc);
    std::vector<uint8_t> bit(unit, 0);
    if (rc.scan) {
        for (uint64_t o = 0; o + 3 < unit; o += 3) bit[o] = 1;
    } else {
        for (uint32_t w : rc.words)
            if (chk_kind(w) == CHK_GATE) bit[w] = 1;
    }
    return bit;
}
// The parts of [off, off + n) of a phase's advice (lookup) stream this context
// holds: all of it, or for a row-sharded rank the intersection with its owned
// segments (whole row blocks).
static std::vector<std::pair<uint64_t, uint64_t>> held(const svdw_ctx* c, uint32_t phase, bool lookup,
                                                       uint64_t off, uint64_t n) {
    std::vector<std::pair<uint64_t, uint64_t>> out;
    if (!n) return out;
    if (!sharded(c)) {
        out.emplace_back(off, n);
        return out;
    }
    for (const auto& o : c->owned) {
        if (o.phase != phase || (o.lookup != 0) != lookup) continue;
        const uint64_t b = std::max(off, o.off), e = std::min(off + n, o.off + o.n);
        if (b < e) out.emplace_back(b, e - b);
    }
    return out;
}
// The six counters of the checkers' kernels (gates, lookups, copies: checked, failed) into their result.
static void read_check_result(svdw_ctx* c, const unsigned long long* cnt, svdw_check_result* out) {
    unsigned long long h[6];
    read_counters(c, cnt, h, 6);
    out->gates_checked = h[0];
    out->gate_failures = h[1];
    out->lookups_checked = h[2];
    out->lookup_failures = h[3];
    out->copies_checked = h[4];
    out->copy_failures = h[5];
}
int svdw_check_gates(svdw_ctx* c, svdw_check_result* out) {
    return guarded([&] {
        REQUIRE(c && out, "null argument");
        need_device(c, "svdw_check_gates");
        sync(c);
        memset(out, 0, sizeof *out);
        // every region's check words, back to back in one upload (a scan's: its gates); region k's from w0[k] on
        std::vector<uint32_t> words;
        std::vector<size_t> w0(1, 0);
        for (size_t k = 0; k < c->wit.layout.size(); ++k) {
            const RegionChecks& rc = c->wit.layout_chk[k];
            if (!rc.scan) words.insert(words.end(), rc.words.begin(), rc.words.end());
            const std::vector<uint8_t> bit = rc.scan ? gate_starts(c->wit.layout[k], rc) : std::vector<uint8_t>();
            for (size_t o = 0; o < bit.size(); ++o)
                if (bit[o]) words.push_back(chk_gate((uint32_t)o));
            w0.push_back(words.size());
        }
        const Staged d = stage_bytes(c, words.data(), words.size() * sizeof(uint32_t));
        for (size_t k = 0; k < c->wit.layout.size(); ++k) {
            const svdw_region& r = c->wit.layout[k];
            const RegionChecks& rc = c->wit.layout_chk[k];
            for (const auto& sg : held(c, r.phase, true, r.loff, r.nl))
                hipck(launch_check_lookups(c->ph[r.phase].lk + sg.first, sg.second, c->LB, d.cnt + 2, c->st),
                      "k_check_lookups");
            const uint64_t unit = unit_cells(r, rc);
            const uint32_t nw = (uint32_t)(w0[k + 1] - w0[k]);
            if (!nw || !unit || !r.n) continue;
            ChkView v[kMaxViews];
            for (int q = 0; q < kMaxViews; ++q) {
                const RegionChecks::Src& s = rc.src[q];
                v[q] = s.phase < 0 ? ChkView{nullptr, 0, 0, 0, 0}
                                   : ChkView{c->ph[s.phase].adv + s.off, s.rs, s.cs, s.rows, s.cols};
            }
            for (const auto& sg : held(c, r.phase, false, r.off, r.n)) {
                if ((sg.first - r.off) % unit || sg.second % unit)
                    fail(SVDW_EINVAL, "svdw_check_gates: owned segment is not whole elements");
                hipck(launch_check_cells(c->ph[r.phase].adv + sg.first, (sg.first - r.off) / unit, sg.second / unit,
                                         (uint32_t)unit, rc.scan ? 1 : rc.cols, (const uint32_t*)d.cells + w0[k], nw,
                                         v[0], v[1], d.cnt, c->st), "k_check_cells");
            }
        }
        read_check_result(c, d.cnt, out);
    });
}
// ------------------------------------------------- physical layout
// Virtual -> physical assignment of a phase's cells (halo2-base 0.4.1, recalled;
// oracle/pyoracle.py physical_layout): basic-gate advice columns of max_rows =
// 2^k - minimum_rows usable rows. A column ends at a cell whose gate would
// cross max_rows (q && row + 4 > max_rows) or at row max_rows - 1; that cell is
// repeated at row 0 of the next column (copy-constrained) and its selector is
// enabled there only.
namespace {
struct GateIndex {               // q(i): does a basic gate start at virtual cell i
    struct Reg {
        uint64_t off, n;
        std::vector<uint8_t> bit;    // gate_starts: per offset of a unit
    };
    std::vector<Reg> regs;       // the regions with gates, ascending offsets
    GateIndex(const svdw_ctx* c, uint32_t phase) {
        for (size_t k = 0; k < c->wit.layout.size(); ++k) {
            const svdw_region& r = c->wit.layout[k];
            if (r.phase != phase || !r.n) continue;
            Reg g{r.off, r.n, gate_starts(r, c->wit.layout_chk[k])};
            if (std::find(g.bit.begin(), g.bit.end(), 1) != g.bit.end()) regs.push_back(std::move(g));
        }
    }
    bool q(uint64_t i) const {
        auto it = std::upper_bound(regs.begin(), regs.end(), i,
                                   [](uint64_t x, const Reg& r) { return x < r.off; });
        if (it == regs.begin()) return false;
        const Reg& r = *--it;
        return i < r.off + r.n && r.bit[(i - r.off) % r.bit.size()] != 0;
    }
};
}  // namespace
int svdw_physical_layout(svdw_ctx* c, uint32_t k, uint32_t minimum_rows, svdw_physical_params* out) {
    return guarded([&] {
        REQUIRE(c && out, "null argument");
        REQUIRE(k >= 3 && k <= 40, "svdw_physical_layout: k out of range");
        REQUIRE(!sharded(c), "svdw_physical_layout: the witness of a sharded context is partial");
        REQUIRE((1ull << k) > (uint64_t)minimum_rows + 4, "svdw_physical_layout: minimum_rows >= 2^k - 4");
        const uint64_t R = (1ull << k) - minimum_rows;
        auto& P = c->phys;
        P.valid = false;
        P.fixed_ready = false;
        P.fixed.clear();
        P.k = k;
        P.min_rows = minimum_rows;
        P.R = R;
        memset(out, 0, sizeof *out);
        out->k = k;
        out->minimum_rows = minimum_rows;
        out->max_rows = R;
        for (uint32_t ph = 0; ph < 2; ++ph) {
            const uint64_t T = c->ph[ph].n, TL = c->ph[ph].nl;
            P.start[ph].clear();
            P.bp[ph].clear();
            const GateIndex gi(c, ph);
            for (uint64_t s = 0; T && true;) {
                P.start[ph].push_back(s);
                // the first of rows R-3, R-2 (gate crossing max_rows) or R-1 (last row)
                uint64_t r = R - 3;
                for (; r < R - 1; ++r)
                    if (s + r < T && gi.q(s + r)) break;
                if (s + r >= T) break;                     // the phase ends in this column
                P.bp[ph].push_back(r);
                s += r;
            }
            out->num_advice[ph] = (uint32_t)((T + R - 1) / R);
            out->columns_used[ph] = (uint32_t)P.start[ph].size();
            out->num_lookup_advice[ph] = (uint32_t)((TL + R - 1) / R);
        }
        out->constants = c->wit.consts.size();
        out->num_fixed = (uint32_t)((c->wit.consts.size() + (1ull << k) - 1) >> k);
        P.valid = true;
    });
}
int svdw_break_points(const svdw_ctx* c, uint32_t phase, uint64_t* out, uint64_t cap, uint64_t* n) {
    return guarded([&] {
        REQUIRE(c && n && phase < 2, "bad argument");
        REQUIRE(c->phys.valid, "svdw_break_points: call svdw_physical_layout after the witness");
        const auto& b = c->phys.bp[phase];
        *n = b.size();
        for (uint64_t i = 0; i < cap && i < b.size() && out; ++i) out[i] = b[i];
    });
}
// One column's cells: the stream range [s, s + len) then zero rows up to `rows`.
// Canonical: a device copy and a memset; Montgomery: converted while it is
// written (k_export pads the column itself), no second pass over the column.
static void assign_column(svdw_ctx* c, int form, const Fr* stream, uint64_t s, uint64_t len, uint64_t rows, Fr* dst) {
    if (form == SVDW_FORM_MONTGOMERY) {
        hipck(launch_export(ExportSrc{stream, s, len, 0, 0, 0, 0}, form, dst, rows - len, c->st), "k_export");
        return;
    }
    hipck(hipMemcpyAsync(dst, stream + s, len * sizeof(Fr), hipMemcpyDeviceToDevice, c->st), "D2D");
    if (len < rows) hipck(hipMemsetAsync(dst + len, 0, (rows - len) * sizeof(Fr), c->st), "hipMemsetAsync");
}
int svdw_assign_columns(svdw_ctx* c, uint32_t phase, void* advice, uint8_t* selectors, void* lookup) {
    return svdw_assign_columns_form(c, phase, SVDW_FORM_CANONICAL, advice, selectors, lookup);
}
int svdw_assign_columns_form(svdw_ctx* c, uint32_t phase, int form, void* advice, uint8_t* selectors, void* lookup) {
    return guarded([&] {
        REQUIRE(c && phase < 2, "bad argument");
        check_form(form);
        need_device(c, "svdw_assign_columns");
        REQUIRE(c->phys.valid, "svdw_assign_columns: call svdw_physical_layout after the witness");
        sync(c);
        const auto& P = c->phys;
        const uint64_t rows = 1ull << P.k, T = c->ph[phase].n, TL = c->ph[phase].nl;
        const size_t ncols = P.start[phase].size();
        REQUIRE(ncols <= (T + P.R - 1) / P.R,
                "NOT ENOUGH ADVICE COLUMNS IN PHASE (columns_used > num_advice: raise k)");
        DBuf& gateq = c->circuit.gateq[phase];
        if (selectors && T) {                              // q bits of the virtual stream
            const GateIndex gi(c, phase);
            std::vector<uint8_t> tables;                   // every region's bit table, back to back in one upload
            for (const auto& r : gi.regs) tables.insert(tables.end(), r.bit.begin(), r.bit.end());
            const Staged d = stage_bytes(c, tables.data(), tables.size());
            const uint64_t nw = (T + 31) / 32;
            ensure_buf(c, gateq, nw * 4);
            uint32_t* qb = (uint32_t*)gateq.p;
            hipck(hipMemsetAsync(qb, 0, nw * 4, c->st), "hipMemsetAsync");
            const uint8_t* table = (const uint8_t*)d.cells;
            for (const auto& r : gi.regs) {
                hipck(launch_gate_bits(qb, r.off, r.n, r.bit.size(), table, c->st), "k_gate_bits");
                table += r.bit.size();
            }
        }
        for (size_t col = 0; col < ncols; ++col) {
            const uint64_t s = P.start[phase][col];
            const bool last = col + 1 == ncols;
            const uint64_t len = last ? T - s : P.bp[phase][col] + 1;
            if (advice) assign_column(c, form, c->ph[phase].adv, s, len, rows, (Fr*)advice + col * rows);
            if (selectors)
                hipck(launch_selectors(selectors + col * rows, (const uint32_t*)gateq.p, s, len, rows, !last, c->st),
                      "k_selectors");
        }
        if (lookup) {
            const uint64_t nl = (TL + P.R - 1) / P.R;
            for (uint64_t col = 0; col < nl; ++col) {
                const uint64_t s = col * P.R, len = std::min(P.R, TL - s);
                assign_column(c, form, c->ph[phase].lk, s, len, rows, (Fr*)lookup + col * rows);
            }
        }
        hipck(hipStreamSynchronize(c->st), "hipStreamSynchronize");
    });
}
int svdw_check_physical(svdw_ctx* c, uint32_t phase, const void* advice, const uint8_t* selectors,
                        uint32_t ncols, svdw_check_result* out) {
    return guarded([&] {
        REQUIRE(c && advice && selectors && out && phase < 2, "bad argument");
        need_device(c, "svdw_check_physical");
        REQUIRE(c->phys.valid, "svdw_check_physical: call svdw_physical_layout first");
        memset(out, 0, sizeof *out);
        settle(c);
        const auto& bp = c->phys.bp[phase];
        const uint32_t nb = (uint32_t)std::min<uint64_t>(bp.size(), ncols ? ncols - 1 : 0);
        const Staged d = stage_bytes(c, bp.data(), nb * sizeof(uint64_t));
        hipck(launch_check_physical((const Fr*)advice, selectors, 1ull << c->phys.k, ncols, d.cnt, c->st),
              "k_check_physical");
        if (nb)
            hipck(launch_check_breaks((const Fr*)advice, 1ull << c->phys.k, (const uint64_t*)d.cells, nb, d.cnt + 4,
                                      c->st), "k_check_breaks");
        read_check_result(c, d.cnt, out);                  // (no lookups: those counters stay zero)
    });
}
// ------------------------------------------------------ equality lists
// halo2-base's equality records of a phase (svdw_equalities), in assign order,
// from the layout table: per region its element program's eq words (PB::eq) or
// the inner-product row pattern, with the source cells of the loaded values
// (RegionChecks::esrc). copies: (source | store << 62, destination) pairs,
// store 2 = the external init_rand cell; consts: (cell, 4 canonical words).
static EqSrcDev eqsrc_dev(const RegionChecks::EqSrc& e) {
    EqSrcDev d;
    memset(&d, 0, sizeof d);
    d.kind = e.kind; d.phase = (int32_t)e.phase; d.pad_phase = e.pad_phase; d.diag_phase = e.diag_phase;
    d.first_phase = (int32_t)e.first_phase; d.off = e.off; d.pad_off = e.pad_off; d.diag_off = e.diag_off;
    d.first = e.first; d.rs = e.rs; d.cs = e.cs; d.rows = e.rows; d.cols = e.cols;
    return d;
}
namespace {
// A phase's regions with records, in layout order, as k_eq_records reads them (a
// scan's rows of L terms, 2 L copies and the constant 0 each; a program's elements,
// ncw copies and nkw constants each), the programs' eq words and constants back to
// back, and the record counts: closed-form, so a record's place in its list is fixed.
struct EqRegions {
    std::vector<EqRegionDev> regs;
    std::vector<size_t> at;                                // their places in layout / layout_chk
    std::vector<uint32_t> words;
    std::vector<Fr> konst;
    uint64_t items = 0, copies = 0, consts = 0, external = 0;   // external: the copies whose source is init_rand
};
}  // namespace
static EqRegions eq_regions(const svdw_ctx* c, uint32_t phase) {
    EqRegions all;
    for (size_t k = 0; k < c->wit.layout.size(); ++k) {
        const svdw_region& r = c->wit.layout[k];
        const RegionChecks& rc = c->wit.layout_chk[k];
        if (r.phase != phase || !r.n) continue;
        EqRegionDev d;
        memset(&d, 0, sizeof d);
        d.off = r.off;
        d.item0 = all.items;
        d.copy0 = all.copies;
        d.const0 = all.consts;
        d.src[0] = eqsrc_dev(rc.esrc[0]);
        d.src[1] = eqsrc_dev(rc.esrc[1]);
        d.unit = (uint32_t)unit_cells(r, rc);
        if (rc.scan) {
            d.scan = 1;
            d.L = (d.unit - 1) / 3;
            d.nitems = (uint64_t)r.rows * d.L;
            all.copies += (uint64_t)r.rows * 2 * d.L;
            all.consts += r.rows;
        } else {
            if (rc.eq.empty() || !d.unit) continue;
            d.nitems = r.n / d.unit;
            d.cols = rc.cols ? rc.cols : 1;
            d.w0 = (uint32_t)all.words.size();
            d.nw = (uint32_t)rc.eq.size();
            d.k0 = (uint32_t)all.konst.size();
            for (uint32_t w : rc.eq) {
                (eq_kind(w) == EQ_CONST ? d.nkw : d.ncw) += 1;
                if (eq_kind(w) == EQ_EXT) all.external += d.nitems;
            }
            all.words.insert(all.words.end(), rc.eq.begin(), rc.eq.end());
            all.konst.insert(all.konst.end(), rc.eqk.begin(), rc.eqk.end());
            all.copies += d.nitems * d.ncw;
            all.consts += d.nitems * d.nkw;
        }
        all.items += d.nitems;
        all.regs.push_back(d);
        all.at.push_back(k);
    }
    return all;
}
static uint64_t eq_src_cell(const RegionChecks::EqSrc& e, uint64_t i, uint64_t j, uint64_t t) {
    if (e.kind == EQS_CHAIN) {
        if (t == 0) return e.first | (uint64_t)e.first_phase << 62;
        return (e.off + (t - 1) * (uint64_t)e.rs) | (uint64_t)e.phase << 62;
    }
    if (e.kind == EQS_MAT) {
        if (e.diag_phase >= 0 && i == j) return e.diag_off | (uint64_t)e.diag_phase << 62;
        if (i < e.rows && j < e.cols)
            return (uint64_t)((int64_t)e.off + (int64_t)i * e.rs + (int64_t)j * e.cs) | (uint64_t)e.phase << 62;
        if (e.pad_phase >= 0) return e.pad_off | (uint64_t)e.pad_phase << 62;
    }
    fail(SVDW_EINVAL, "svdw_equalities: a region's copy source is not in the cell streams");
    return 0;
}
// The records on the host (a planning context).
static void eq_lists(const svdw_ctx* c, uint32_t phase, const EqRegions& all, std::vector<uint64_t>* copies,
                     std::vector<uint64_t>* consts) {
    auto konst = [&](uint64_t dst, const Fr& v) {
        uint64_t w[4];
        fr_store_words(v, w);
        consts->push_back(dst);
        consts->insert(consts->end(), w, w + 4);
    };
    const uint64_t me = (uint64_t)phase << 62;
    for (size_t q = 0; q < all.regs.size(); ++q) {
        const EqRegionDev& g = all.regs[q];
        const RegionChecks& rc = c->wit.layout_chk[all.at[q]];
        const uint64_t units = g.scan ? c->wit.layout[all.at[q]].rows : g.nitems;
        for (uint64_t e = 0; e < units; ++e) {
            const uint64_t base = g.off + e * g.unit;
            if (g.scan) {
                konst(base, fr_zero());
                for (uint64_t t = 0; t < g.L; ++t) {
                    copies->push_back(eq_src_cell(rc.esrc[0], e, t, 0));
                    copies->push_back(base + 1 + 3 * t);
                    copies->push_back(eq_src_cell(rc.esrc[1], 0, 0, t));
                    copies->push_back(base + 2 + 3 * t);
                }
                continue;
            }
            const uint64_t i = e / g.cols, j = e % g.cols;
            for (uint32_t w : rc.eq) {
                const uint32_t a = eq_a(w), at = eq_slot(w);
                switch (eq_kind(w)) {
                case EQ_CONST: konst(base + at, rc.eqk.at(a)); break;
                case EQ_LOCAL: copies->push_back((base + a) | me); copies->push_back(base + at); break;
                case EQ_VIEW:
                    copies->push_back(eq_src_cell(rc.esrc[a], i, j, i));
                    copies->push_back(base + at);
                    break;
                default:                                  // EQ_EXT: init_rand's RLC cell
                    copies->push_back(c->wit.ext_off | 2ull << 62); copies->push_back(base + at); break;
                }
            }
        }
    }
}
// The same records generated on the device (k_eq_records) into eq_cp / eq_ks, in eq_lists' order. Called
// from inside other calls, so it leaves the staged scratch alone: its input goes up in one copy to eq_in.
static void eq_gen_device(svdw_ctx* c, uint32_t phase, const EqRegions& all) {
    for (const EqRegionDev& d : all.regs) REQUIRE(!d.scan || d.L >= 1, "internal: empty scan rows");
    std::vector<char> in(32, 0);                           // the err word, then each part 32-byte aligned
    auto put = [&](const void* p, size_t bytes) {
        const size_t at = in.size();
        in.insert(in.end(), (const char*)p, (const char*)p + bytes);
        in.resize((in.size() + 31) / 32 * 32, 0);
        return at;
    };
    const size_t o_reg = put(all.regs.data(), all.regs.size() * sizeof(EqRegionDev)),
                 o_w = put(all.words.data(), all.words.size() * 4),
                 o_k = put(all.konst.data(), all.konst.size() * sizeof(Fr)), bytes = in.size();
    CircuitState& cs = c->circuit;
    ensure_buf(c, cs.eq_cp, std::max<uint64_t>(all.copies, 1) * 16);
    ensure_buf(c, cs.eq_ks, std::max<uint64_t>(all.consts, 1) * 40);
    ensure_buf(c, cs.eq_in, bytes);
    char* dev = (char*)cs.eq_in.p;
    hipck(hipMemcpyAsync(dev, in.data(), bytes, hipMemcpyHostToDevice, c->st), "H2D");
    hipck(launch_eq_records((const EqRegionDev*)(dev + o_reg), (uint32_t)all.regs.size(), all.items,
                            (const uint32_t*)(dev + o_w), (const Fr*)(dev + o_k), phase, c->wit.ext_off,
                            (uint64_t*)cs.eq_cp.p, (uint64_t*)cs.eq_ks.p, (unsigned*)dev, c->st), "k_eq_records");
    unsigned long long err = 0;                            // (the word and the zeros behind it)
    read_counters(c, (const unsigned long long*)dev, &err, 1);
    REQUIRE(!err, "svdw_equalities: a region's copy source is not in the cell streams");
}
// phys.start[0] then phys.start[1] (each column's first virtual cell) as a staged call uploads them, and
// k_eq_phys over the records of `phase` with their device copy `st`: virtual cells become physical indices.
static std::vector<uint64_t> starts(const svdw_ctx::Phys& P) {
    std::vector<uint64_t> s(P.start[0]);
    s.insert(s.end(), P.start[1].begin(), P.start[1].end());
    return s;
}
static void eq_to_physical(svdw_ctx* c, uint32_t phase, const EqRegions& all, const uint64_t* st) {
    const uint32_t n0 = (uint32_t)c->phys.start[0].size(), n1 = (uint32_t)c->phys.start[1].size();
    hipck(launch_eq_phys((uint64_t*)c->circuit.eq_cp.p, all.copies, (uint64_t*)c->circuit.eq_ks.p, all.consts, st, n0,
                         st + n0, n1, phase, c->phys.k, c->st), "k_eq_phys");
}
// virtual cell -> column-major physical index (the first placement of a break cell)
static uint64_t phys_index(const svdw_ctx* c, uint32_t phase, uint64_t v) {
    const auto& st = c->phys.start[phase];
    size_t col = std::upper_bound(st.begin(), st.end(), v) - st.begin();
    REQUIRE(col > 0, "internal: cell before column 0");
    --col;
    if (col > 0 && v == st[col]) --col;                   // break cell: its row in the column before
    return ((uint64_t)col << c->phys.k) + (v - st[col]);
}
int svdw_equalities(const svdw_ctx* c, uint32_t phase, uint64_t* copies, uint64_t copies_cap,
                    uint64_t* n_copies, uint64_t* consts, uint64_t consts_cap, uint64_t* n_consts) {
    return guarded([&] {
        REQUIRE(c && phase < 2 && n_copies && n_consts, "bad argument");
        const EqRegions all = eq_regions(c, phase);
        *n_copies = all.copies;
        *n_consts = all.consts;
        if (!c->dry) {                       // generated on the device, copied out up to the caps
            svdw_ctx* m = const_cast<svdw_ctx*>(c);
            sync(m);
            eq_gen_device(m, phase, all);
            const CircuitState& cs = c->circuit;
            if (copies && copies_cap)
                hipck(hipMemcpy(copies, cs.eq_cp.p, std::min(copies_cap, all.copies) * 16, hipMemcpyDeviceToHost), "D2H");
            if (consts && consts_cap)
                hipck(hipMemcpy(consts, cs.eq_ks.p, std::min(consts_cap, all.consts) * 40, hipMemcpyDeviceToHost), "D2H");
            return;
        }
        std::vector<uint64_t> cp, cs;
        eq_lists(c, phase, all, &cp, &cs);
        if (copies) memcpy(copies, cp.data(), std::min<uint64_t>(copies_cap, cp.size() / 2) * 16);
        if (consts) memcpy(consts, cs.data(), std::min<uint64_t>(consts_cap, cs.size() / 5) * 40);
    });
}
int svdw_check_equalities(svdw_ctx* c, uint32_t phase, const void* columns0, const void* columns1,
                          svdw_eq_check* out) {
    return guarded([&] {
        REQUIRE(c && phase < 2 && out, "bad argument");
        need_device(c, "svdw_check_equalities");
        // a record's source and destination cells may lie in other ranks' rows,
        // which this context never wrote (svdw_check_gates checks a rank's own)
        REQUIRE(!sharded(c), "svdw_check_equalities: not on a row-sharded context (its streams hold "
                             "this rank's rows only; check the reassembled witness, or use svdw_check_gates)");
        const bool phys = columns0 || columns1;
        REQUIRE(!phys || (c->phys.valid && (phase == 0 ? columns0 != nullptr : columns0 && columns1)),
                "svdw_check_equalities: physical columns need svdw_physical_layout and phase 0's "
                "columns (and phase 1's for phase 1)");
        memset(out, 0, sizeof *out);
        sync(c);
        const EqRegions all = eq_regions(c, phase);
        eq_gen_device(c, phase, all);
        const std::vector<uint64_t> st = phys ? starts(c->phys) : std::vector<uint64_t>();
        const Staged d = stage_bytes(c, st.data(), st.size() * 8);
        if (phys) eq_to_physical(c, phase, all, (const uint64_t*)d.cells);   // records onto the assigned columns
        const Fr* s0 = phys ? (const Fr*)columns0 : c->ph[0].adv;
        const Fr* s1 = phys ? (const Fr*)columns1 : c->ph[1].adv;
        const Fr* dst = phase ? s1 : s0;
        const CircuitState& cs = c->circuit;
        hipck(launch_check_copies(s0, s1, dst, (const uint64_t*)cs.eq_cp.p, all.copies, c->ext_gamma, d.cnt, c->st),
              "k_check_copies");
        hipck(launch_check_consts(dst, (const uint64_t*)cs.eq_ks.p, all.consts, d.cnt + 2, c->st), "k_check_consts");
        unsigned long long h[4];
        read_counters(c, d.cnt, h, 4);
        out->copies_checked = h[0];
        out->copy_failures = h[1];
        out->consts_checked = h[2];
        out->const_failures = h[3];
    });
}
// ---- the permutation argument's edge list and fixed columns of the witness
// (include/svdw.h, svdw_permutation_edges; kernels: permutation_cycles.hpp)
static uint64_t perm_cell(uint32_t col, uint64_t row) { return (uint64_t)col << 32 | row; }
int svdw_permutation_edges(svdw_ctx* c, uint64_t* edges, uint64_t cap, svdw_permutation_layout* out) {
    return guarded([&] {
        REQUIRE(c && out, "null argument");
        REQUIRE(c->phys.valid, "svdw_permutation_edges: call svdw_physical_layout after the witness");
        REQUIRE(!sharded(c), "svdw_permutation_edges: the witness of a sharded context is partial");
        REQUIRE(!edges || !c->dry, "svdw_permutation_edges: the edge list needs a device context");
        auto& P = c->phys;
        const uint32_t k = P.k;
        if (k > 28) fail(SVDW_ERANGE, "svdw_permutation_edges: k > 28");
        const EqRegions n[2] = {eq_regions(c, 0), eq_regions(c, 1)};
        const uint64_t D = c->wit.consts.size(), rows = 1ull << k;
        memset(out, 0, sizeof *out);
        out->k = k;
        out->advice[0] = (uint32_t)P.start[0].size();
        out->advice[1] = (uint32_t)P.start[1].size();
        out->fixed = (uint32_t)((D + rows - 1) >> k);
        out->break_edges = P.bp[0].size() + P.bp[1].size();
        out->copy_edges = n[0].copies - n[0].external + n[1].copies - n[1].external;
        out->const_edges = n[0].consts + n[1].consts;
        out->external_edges = n[0].external + n[1].external + (c->rlc.n ? 2 : 0);
        out->external = out->external_edges ? 1 : 0;
        out->total_cols = out->advice[0] + out->advice[1] + out->fixed + out->external;
        out->edges = out->break_edges + out->copy_edges + out->const_edges + out->external_edges;
        out->constants = D;
        // constant i sits in row i / fixed: the last one has to lie above the blinding rows
        if (D && (D - 1) / out->fixed >= P.R)
            fail(SVDW_ERANGE, "svdw_permutation_edges: a constant's fixed row is not usable (raise k)");
        need_columns("svdw_permutation_edges", out->total_cols);
        if (!edges) return;
        REQUIRE(cap >= out->edges, "svdw_permutation_edges: cap is below the number of edges");
        sync(c);
        const uint32_t base[2] = {0, out->advice[0]}, fixed_col = out->advice[0] + out->advice[1],
                       ext_col = fixed_col + out->fixed;
        const PcColumns w{k, {base[0], base[1]}, ext_col};
        // 1. the break cells, and the last edges of 4.: ctx_rlc's two copies (host)
        std::vector<uint64_t> head, tail;
        for (uint32_t ph = 0; ph < 2; ++ph)
            for (size_t j = 0; j < P.bp[ph].size(); ++j) {
                head.push_back(perm_cell(base[ph] + (uint32_t)j, P.bp[ph][j]));
                head.push_back(perm_cell(base[ph] + (uint32_t)j + 1, 0));
            }
        for (uint32_t i = 0; c->rlc.n && i < 2; ++i) {
            const uint32_t ph = (uint32_t)(c->rlc.src[i] >> 62);
            REQUIRE(ph < 2, "internal: ctx_rlc copies a cell outside the streams");
            const uint64_t p = phys_index(c, ph, c->rlc.src[i] & ((1ull << 62) - 1));
            tail.push_back(perm_cell(base[ph] + (uint32_t)(p >> k), p & (rows - 1)));
            tail.push_back(perm_cell(ext_col, i));
        }
        uint64_t *o_copy = edges + 2 * out->break_edges, *o_const = o_copy + 2 * out->copy_edges,
                 *o_ext = o_const + 2 * out->const_edges;
        if (!head.empty()) hipck(hipMemcpyAsync(edges, head.data(), head.size() * 8, hipMemcpyHostToDevice, c->st), "H2D");
        if (!tail.empty())
            hipck(hipMemcpyAsync(o_ext + 2 * (n[0].external + n[1].external), tail.data(), tail.size() * 8,
                                 hipMemcpyHostToDevice, c->st), "H2D");
        // the distinct constants, ascending as numbers, and per value the first record that holds it
        std::vector<std::array<uint64_t, 4>> table;
        for (const auto& v : c->wit.consts) {
            Fr x;
            memcpy(x.w, v.data(), sizeof x.w);
            fr_store_words(x, table.emplace_back().data());
        }
        std::sort(table.begin(), table.end(), [](const std::array<uint64_t, 4>& a, const std::array<uint64_t, 4>& b) {
            for (int q = 3; q >= 0; --q)
                if (a[q] != b[q]) return a[q] < b[q];
            return false;
        });
        // staged: counter 0 is the err word; the cells are the start arrays, then the table; free holds first
        // (all ones), rank and the tile sums of k_pcw_split
        std::vector<uint64_t> up = starts(P);
        up.resize((up.size() + 15) / 16 * 16);             // (each part on a 128-byte line of its own)
        const size_t o_tab = up.size(), o_rank = (D * 8 + 127) / 128 * 128, o_bsum = o_rank + (D * 4 + 127) / 128 * 128;
        for (const auto& t : table) up.insert(up.end(), t.begin(), t.end());
        up.resize((up.size() + 15) / 16 * 16);
        const uint64_t tiles = std::max<uint64_t>(pc_tiles(std::max(n[0].copies, n[1].copies)), 1);
        const Staged d = stage_bytes(c, up.data(), up.size() * 8, o_bsum + tiles * 8);
        const uint64_t *st = (const uint64_t*)d.cells, *dtable = st + o_tab;
        unsigned long long* first = (unsigned long long*)d.free;
        uint32_t *drank = (uint32_t*)(d.free + o_rank), *err = (unsigned*)d.cnt;
        uint64_t* bsum = (uint64_t*)(d.free + o_bsum);
        if (D) hipck(hipMemsetAsync(first, 0xff, D * 8, c->st), "hipMemsetAsync");
        // 2. - 4. per phase: the records (k_eq_records), onto the columns (k_eq_phys), into their groups
        uint64_t g0 = 0;
        for (uint32_t ph = 0; ph < 2; ++ph) {
            const uint64_t nc = n[ph].copies, nk = n[ph].consts, nx = n[ph].external;
            eq_gen_device(c, ph, n[ph]);
            eq_to_physical(c, ph, n[ph], st);
            profiled(c, "k_pcw_split", 32.0 * (double)nc, [&] {
                return launch_pcw_split((const uint64_t*)c->circuit.eq_cp.p, nc, w, ph, bsum, o_copy, nc - nx, o_ext, nx,
                                        err, c->st);
            });
            profiled(c, "k_pcw_consts", 56.0 * (double)nk, [&] {
                return launch_pcw_consts((const uint64_t*)c->circuit.eq_ks.p, nk, dtable, (uint32_t)D, g0, w, ph, first,
                                         o_const, err, c->st);
            });
            o_copy += 2 * (nc - nx);
            o_ext += 2 * nx;
            o_const += 2 * nk;
            g0 += nk;
            hipck(hipStreamSynchronize(c->st), "hipStreamSynchronize");   // the records are the next phase's too
        }
        // the constants in the order of their first record (one without a record: after the others)
        std::vector<unsigned long long> hfirst(D);
        unsigned long long herr = 0;
        if (D) hipck(hipMemcpyAsync(hfirst.data(), first, D * 8, hipMemcpyDeviceToHost, c->st), "D2H");
        read_counters(c, d.cnt, &herr, 1);
        REQUIRE(!(herr & 2), "internal: the external copy records differ from their count");
        REQUIRE(!herr, "svdw_permutation_edges: a constant record's value is not among the context's constants");
        std::vector<uint32_t> order(D), rank(D);
        for (uint32_t i = 0; i < D; ++i) order[i] = i;
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return hfirst[a] < hfirst[b]; });
        P.fixed.assign(D, fr_zero());
        for (uint32_t i = 0; i < D; ++i) {
            rank[order[i]] = i;
            P.fixed[i] = fr_raw_words(table[order[i]].data());
        }
        P.fixed_ready = true;
        if (D) hipck(hipMemcpyAsync(drank, rank.data(), D * 4, hipMemcpyHostToDevice, c->st), "H2D");
        hipck(launch_pcw_place(edges + 2 * (out->break_edges + out->copy_edges), out->const_edges, drank, (uint32_t)D,
                               fixed_col, out->fixed, c->st), "k_pcw_place");
        hipck(hipStreamSynchronize(c->st), "hipStreamSynchronize");
    });
}
int svdw_assign_fixed(svdw_ctx* c, int form, void* fixed) {
    return guarded([&] {
        REQUIRE(c, "null argument");
        check_form(form);
        need_device(c, "svdw_assign_fixed");
        auto& P = c->phys;
        REQUIRE(P.valid && P.fixed_ready,
                "svdw_assign_fixed: call svdw_permutation_edges with an edge list after svdw_physical_layout");
        const uint64_t D = P.fixed.size(), rows = 1ull << P.k, F = (D + rows - 1) >> P.k;
        if (!F) return;
        REQUIRE(fixed, "null output");
        sync(c);
        // column j holds the constants j, j + F, ... from row 0 on
        std::vector<Fr> cells(D);
        std::vector<size_t> at(F + 1, 0);
        for (uint64_t j = 0; j < F; ++j) at[j + 1] = at[j] + (D - j + F - 1) / F;
        for (uint64_t i = 0; i < D; ++i)
            cells[at[i % F] + i / F] = form == SVDW_FORM_MONTGOMERY ? fr_to_mont(P.fixed[i]) : P.fixed[i];
        hipck(hipMemsetAsync(fixed, 0, F * rows * sizeof(Fr), c->st), "hipMemsetAsync");
        for (uint64_t j = 0; j < F; ++j)
            if (at[j + 1] > at[j])
                hipck(hipMemcpyAsync((Fr*)fixed + j * rows, cells.data() + at[j], (at[j + 1] - at[j]) * sizeof(Fr),
                                     hipMemcpyHostToDevice, c->st), "H2D");
        hipck(hipStreamSynchronize(c->st), "hipStreamSynchronize");
    });
}
// ---- what a witness left behind, as it is
int svdw_rlc_trace(const svdw_ctx* c, uint64_t* cells, uint64_t* copies, uint32_t* n) {
    return guarded([&] {
        REQUIRE(c && n, "null argument");
        *n = c->rlc.n;
        if (!c->rlc.n) return;
        REQUIRE(cells && copies, "null output");
        for (uint32_t k = 0; k < c->rlc.n; ++k) fr_store_words(c->rlc.cells[k], cells + 4 * k);
        copies[0] = c->rlc.src[0];
        copies[1] = c->rlc.src[1];
    });
}
int svdw_layout(const svdw_ctx* c, svdw_region* out, uint64_t cap, uint64_t* n) {
    return guarded([&] {
        REQUIRE(c && n, "null argument");
        *n = c->wit.layout.size();
        for (uint64_t i = 0; i < cap && i < c->wit.layout.size(); ++i) out[i] = c->wit.layout[i];
    });
}
int svdw_shard_segments(const svdw_ctx* c, svdw_segment* out, uint64_t cap, uint64_t* n) {
    return guarded([&] {
        REQUIRE(c && n, "null argument");
        *n = c->owned.size();
        for (uint64_t i = 0; i < c->owned.size() && i < cap && out; ++i)
            out[i] = svdw_segment{c->owned[i].phase, c->owned[i].lookup, c->owned[i].off, c->owned[i].n};
    });
}
