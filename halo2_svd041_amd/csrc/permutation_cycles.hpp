// Sigma from the copy constraints on the device (permutation_cycles.hip):
// keygen's cycle merge in its order-independent form (include/svdw.h,
// "permutation argument"; PARITY UNPINNED). The cells of total_cols columns of
// 2^k rows get the flat id col << k | row, a uint32_t; an edge joins two cells
// of rows < usable. The classes are the connected components, and sigma links
// the cells of each class in ascending id into one cycle.
//
// The builder, one launch each unless said otherwise, in stream order:
//
//  k_pc_init      parent[i] = i
//  k_pc_union     one edge per thread: both roots by find with path halving, a
//                 device-scope CAS hangs the larger root under the smaller,
//                 a lost CAS goes on from what it read. parent[x] <= x always,
//                 and whatever a thread reads of parent is an ancestor, so every
//                 step of every loop moves to a smaller id or ends
//  k_pc_flatten   parent[i] = root(i)
//  k_pc_flag      flag[root] = 1 for every root with a child
//  k_pc_sum, k_pc_carry, k_pc_apply
//                 the scan in three kernels (tiles, one block over the tile sums,
//                 the tiles again) over member(i) = the class of i has two or
//                 more cells; apply writes the (root, cell) pairs compacted in
//                 ascending cell
//  k_pc_hist, the scan again, k_pc_scatter     per 8-bit digit of the root, least
//                 significant first, over the digits the ids need: a stable
//                 counting sort; ranks within a wave come from ballots, the
//                 waves of a block and the blocks from the scanned table
//  k_pc_link      the root is its class's smallest id and so heads its segment:
//                 mapping[cell_j] = root_{j+1} == root_j ? cell_{j+1} : root_j;
//                 a segment's last thread finds its head by bisection: classes
//                 and the largest class
//  k_pc_identity  every cell that is no member maps to itself
//
// No block waits for another one; the result does not depend on which CAS wins,
// as the root of a class is its smallest cell whatever the order: the mapping
// is the same bits for any order or repetition of the edges.
//
// The checker shares none of this: a scatter of hit counts (k_pm_hits), the
// minimum of every sigma-cycle by pointer doubling over (next, min) pairs
// (k_pm_double, ceil(log2 cells) launches between two buffers), descents per
// cycle (k_pm_descents, k_pm_cycles) and the edges' ends against the minima
// (k_pm_edges).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace svdw {

constexpr uint32_t kPcThreads = 256;
constexpr uint32_t kPcItems = 8;                           // cells per thread of a scan tile
constexpr uint32_t kPcTile = kPcThreads * kPcItems;
constexpr uint32_t kPcSortIters = 16;                      // wave-wide steps of a sort block
constexpr uint32_t kPcSortTile = kPcThreads * kPcSortIters;

// cells = total_cols << k <= 2^32; usable <= rows = 2^k.
struct PcShape {
    uint32_t k, total_cols;
    uint64_t rows, usable, cells;
};
inline uint64_t pc_tiles(uint64_t n) { return (n + kPcTile - 1) / kPcTile; }
inline uint64_t pc_sort_blocks(uint64_t m) { return (m + kPcSortTile - 1) / kPcSortTile; }
// 8-bit digits that hold every id below cells.
inline uint32_t pc_sort_passes(uint64_t cells) {
    uint32_t bits = 1;
    while (bits < 32 && (1ull << bits) < cells) ++bits;
    return (bits + 7) / 8;
}

// cnt[0] += edges with an end outside the usable cells, cnt[1] += edges from a
// cell to itself; both are skipped.
hipError_t launch_pc_init(const PcShape& s, uint32_t* parent, hipStream_t st);
hipError_t launch_pc_union(const PcShape& s, const uint64_t* edges, uint64_t n_edges, uint32_t* parent,
                           unsigned long long* cnt, hipStream_t st);
hipError_t launch_pc_flatten(const PcShape& s, uint32_t* parent, hipStream_t st);
// flag: cells bytes, zero before the call.
hipError_t launch_pc_flag(const PcShape& s, const uint32_t* parent, uint8_t* flag, hipStream_t st);
// bsum[t] = the members before tile t (pc_tiles(cells) entries), *total = all.
hipError_t launch_pc_member_scan(const PcShape& s, const uint32_t* parent, const uint8_t* flag, uint64_t* bsum,
                                 unsigned long long* total, hipStream_t st);
// key / val: the m = *total pairs.
hipError_t launch_pc_compact(const PcShape& s, const uint32_t* parent, const uint8_t* flag, const uint64_t* bsum,
                             uint64_t m, uint32_t* key, uint32_t* val, hipStream_t st);
// One pass of the sort by the digit at `shift`: (key, val) to (key2, val2).
// hist: 256 x pc_sort_blocks(m) words, bsum: pc_tiles of those.
hipError_t launch_pc_sort_pass(const uint32_t* key, const uint32_t* val, uint64_t m, uint32_t shift, uint32_t* hist,
                               uint64_t* bsum, uint32_t* key2, uint32_t* val2, hipStream_t st);
// cnt[0] += classes, cnt[1] = max(cnt[1], the largest class).
hipError_t launch_pc_link(const PcShape& s, const uint32_t* key, const uint32_t* val, uint64_t m, uint64_t* mapping,
                          unsigned long long* cnt, hipStream_t st);
hipError_t launch_pc_identity(const PcShape& s, const uint32_t* parent, const uint8_t* flag, uint64_t* mapping,
                              hipStream_t st);

// ---- the checker. hit: cells words, zero before the call; nm: cells (next, min)
// pairs. cnt[0] += entries out of range, cnt[1] += non-identity entries of rows
// >= usable.
hipError_t launch_pm_hits(const PcShape& s, const uint64_t* mapping, uint32_t* hit, uint2* nm, unsigned long long* cnt,
                          hipStream_t st);
hipError_t launch_pm_double(const PcShape& s, const uint2* in, uint2* out, hipStream_t st);
// desc: cells words, zero before the call: desc[min of i's cycle] += 1 where
// mapping[i] < i; cnt[0] += cells not hit exactly once.
hipError_t launch_pm_descents(const PcShape& s, const uint64_t* mapping, const uint32_t* hit, const uint2* nm,
                              uint32_t* desc, unsigned long long* cnt, hipStream_t st);
// cnt[0] += cycles of two or more cells, cnt[1] += those whose descents are not 1.
hipError_t launch_pm_cycles(const PcShape& s, const uint64_t* mapping, const uint2* nm, const uint32_t* desc,
                            unsigned long long* cnt, hipStream_t st);
// cnt[0] += edges with both ends usable cells, cnt[1] += those whose ends differ in their cycle's minimum.
hipError_t launch_pm_edges(const PcShape& s, const uint64_t* edges, uint64_t n_edges, const uint2* nm,
                           unsigned long long* cnt, hipStream_t st);

// ---- the witness's edge list (svdw_permutation_edges). The argument's columns:
// base[phase] = the first advice column of the phase, ext_col the external one.
struct PcColumns {
    uint32_t k, base[2], ext_col;
};
// The copy records of one phase in physical coordinates (k_eq_phys; nc pairs of
// source with its phase in the top two bits, destination) as edges of cells:
// those with source phase 2 to ext (the external column at the source's row),
// the others to copy, each list in record order. bsum: pc_tiles(nc) words.
// ncopy + next = nc are the lists' lengths as the host counted them: a record
// beyond them is not written and sets *err |= 2.
hipError_t launch_pcw_split(const uint64_t* recs, uint64_t nc, const PcColumns& w, uint32_t phase, uint64_t* bsum,
                            uint64_t* copy, uint64_t ncopy, uint64_t* ext, uint64_t next, unsigned* err,
                            hipStream_t st);
// The constant records of one phase (nk of 5 words: cell, value) against the
// table of distinct values (ntab x 4 words, ascending as numbers): out[2 i] = the
// cell, out[2 i + 1] = the value's place in the table, first[place] = the
// smallest g0 + i over its records; *err |= 1 for a value that is not there.
hipError_t launch_pcw_consts(const uint64_t* recs, uint64_t nk, const uint64_t* table, uint32_t ntab, uint64_t g0,
                             const PcColumns& w, uint32_t phase, unsigned long long* first, uint64_t* out,
                             unsigned* err, hipStream_t st);
// out[2 i + 1] (a place in the table) becomes the fixed cell of constant rank[place]:
// column fixed_col + rank % nfixed, row rank / nfixed.
hipError_t launch_pcw_place(uint64_t* out, uint64_t n, const uint32_t* rank, uint32_t ntab, uint32_t fixed_col,
                            uint32_t nfixed, hipStream_t st);

}  // namespace svdw
