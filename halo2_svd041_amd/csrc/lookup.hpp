// The lookup argument's permuted columns on the device (lookup.hip): halo2's
// lookup::prover::permute_expression_pair for RangeChip's table
// T = [0, 1, .., 2^LB - 1, 0, 0, ..], restated from memory (PARITY UNPINNED,
// include/svdw.h). Every honest input cell is below B = 2^LB, so the sort of a
// column is a histogram, the BTreeMap walk two scans over the B bins, and the
// hand-out of the leftover table entries an index computation:
//
//  k_lk_hist      cnt[v] of the usable rows of each column (cells validated)
//  k_lk_scan_*    start = exclusive scan of cnt, pincl = inclusive scan of
//                 (cnt > 0), absent = ascending v >= 1 with cnt[v] == 0
//  k_lk_fill      row r of the run of v: A'[r] = v; S'[r] = v at r == start[v],
//                 else L[usable - D - 1 - (r - pincl[v])] with L = z0 zeros
//                 then absent, z0 = 1 + usable - B - (cnt[0] > 0), D = pincl[B-1]
//  k_lk_adjacent, k_lk_compare   the argument's own constraints (a check)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fr.hpp"

namespace svdw {

// Input columns: cell (c, r) is p[c * stride + r] where r < span and
// c * stride + r < total, zero elsewhere. A lookup stream read through the
// physical layout is (stride = span = max_rows, total = the stream's cells);
// assigned columns are (stride = span = 2^k, total = ncols * 2^k).
struct LkSrc {
    const Fr* p;
    uint64_t stride, span, total;
};

// Scratch of one permute, in 32-bit words; ncols columns of B bins each.
struct LkScratch {
    uint32_t* cnt;      // [ncols][B]
    uint32_t* start;    // [ncols][B]
    uint32_t* pincl;    // [ncols][B]
    uint32_t* absent;   // [ncols][B]
    uint32_t* bsum;     // [ncols][nblk][2]: block sums of cnt, of present; then their exclusive scans
    uint32_t* tot;      // [ncols]: D
};
static constexpr uint32_t kLkScanTile = 1024;   // bins per block of the scans
inline uint64_t lk_scan_blocks(uint64_t B) { return (B + kLkScanTile - 1) / kLkScanTile; }

// cnt[c][v] += the cells equal to v in rows [0, usable) of column c, cells in
// `form`; oot[0] += the cells >= 2^lb (not binned). cnt is not cleared here.
hipError_t launch_lk_hist(const LkSrc& src, int form, uint32_t ncols, uint64_t usable, uint32_t lb,
                          uint32_t* cnt, unsigned long long* oot, hipStream_t st);
// start, pincl, absent, tot from cnt.
hipError_t launch_lk_scans(const LkScratch& s, uint32_t ncols, uint32_t lb, hipStream_t st);
// A' and S' (ncols x rows cells, in `form`) from the scans; rows >= usable zero.
hipError_t launch_lk_fill(const LkScratch& s, uint32_t ncols, uint64_t rows, uint64_t usable, uint32_t lb,
                          int form, Fr* pin, Fr* ptab, hipStream_t st);
// cnt[0..1] += adjacency rows checked / failed, cnt[2..3] += padding cells checked / failed.
hipError_t launch_lk_adjacent(const Fr* pin, const Fr* ptab, uint32_t ncols, uint64_t rows, uint64_t usable,
                              unsigned long long* cnt, hipStream_t st);
// cnt[0..1] += bins compared / differing: ha against hpin, htab against the table's histogram.
hipError_t launch_lk_compare(const uint32_t* ha, const uint32_t* hpin, const uint32_t* htab, uint32_t ncols,
                             uint64_t usable, uint32_t lb, unsigned long long* cnt, hipStream_t st);

}  // namespace svdw
