// sweep_plan.hpp -- WHAT the plan of the L2 sweep holds (rt_plans.inc build_plans builds it on the device): how many column panels a part gets, which
// rows are cut into segments, which rows leave the sweep for the segment kernels, the locality rank of the rows and, per panel, the list of work
// items the sweep's workgroups walk.  Every group the LDS-staged kernel does not take runs on this plan, and so do correction parts, the sparse
// half of a density split and every SpMV.
//
// Everything here is a pure function of plain numbers and host arrays: the part's sizes, its row pointers, the panel pointers of every row (the
// device cuts them by binary search; for one panel they are the row pointers), a copy of the ten tunables the rules read (SweepKnobs, filled in one
// place: rt_plans.inc sweep_knobs) and what the runtime had to ask the device, as values: whether the columns are stored in order, and which rows
// are alike (sim_kind, sim_order).  One rule is written once here and asked twice: panels PAY when a (row, panel) pair holds panel_min_seg
// entries on average (panels_pay; rt_launch.inc want_panel asks it again per product).  tests/native/sweep_plan_main.cpp asks all of it on a CPU.
// What needs the device stays with the runtime: the copies, the sortedness and panel-pointer kernels, find_similarity, the uploads, the 16-bit ids.
//
// Host-only C++17: no device header, no runtime state.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace pygim {

// exactly the tunables the rules read (rt_state.inc Tunables, same names and meanings)
struct SweepKnobs {
    int64_t panel_mode = 0, panel_bytes = 4 << 20, panel_min_seg = 8, panel_coop = 512, panel_locality = 1, panel_col16 = 1;
    int64_t vec_lds = 1, vec_kernel = 1, long_row_threshold = 4096, long_segment = 512;
};

// ---- long rows ----------------------------------------------------------------------------------------------------------------------------------------
inline uint32_t long_row_base_threshold(const SweepKnobs &k) { return (uint32_t)std::min<int64_t>(0x7FFFFFFF, std::max<int64_t>(64, k.long_row_threshold)); }
inline uint32_t long_row_segment(uint32_t thresh, const SweepKnobs &k) { return (uint32_t)std::min<int64_t>(thresh, std::max<int64_t>(64, k.long_segment)); }

// Long-row plan from a host copy of rowptr: a row is long when it has more than `thresh` entries, or -- when flags are given -- when flagged.
// Long rows are cut into segments of `seg` entries: tasks (row, first entry, end) x n, desc (row, first task, tasks) per long row.
inline void plan_long_rows(const uint32_t *rowptr, int64_t nrows, uint32_t thresh, uint32_t seg, const std::vector<char> *flags, std::vector<uint32_t> &tasks,
                           std::vector<uint32_t> &desc) {
    for (int64_t r = 0; r < nrows; r++) {
        const uint32_t s = rowptr[r], e = rowptr[r + 1];
        const bool is_long = flags ? (*flags)[(size_t)r] != 0 : (e - s > thresh);
        if (!is_long || e == s) continue;
        const uint32_t first = (uint32_t)(tasks.size() / 3);
        uint32_t n = 0;
        for (uint32_t a = s; a < e; a += seg, n++) {
            tasks.push_back((uint32_t)r);
            tasks.push_back(a);
            tasks.push_back(std::min(e, a + seg));
        }
        desc.push_back((uint32_t)r);
        desc.push_back(first);
        desc.push_back(n);
    }
}

// ---- the panel count ----------------------------------------------------------------------------------------------------------------------------------
// L2 blocking: the columns are cut into panels whose 128-byte feature slice fits the L2 budget.  It pays when a (row, panel) pair holds enough
// entries; the plan's builder and every product (want_panel) ask this one function.
inline bool panels_pay(int64_t nnz, int64_t nrows, uint32_t npanels, int64_t panel_min_seg) {
    return npanels == 1 || (double)nnz / ((double)nrows * npanels) >= (double)panel_min_seg;
}

struct SweepPanels {
    bool plan = false;        // a sweep plan is built at all
    uint32_t npan = 0;        // the wanted panel count ...
    bool ask_sorted = false;  // ... which holds only if every row stores its column ids in order: ask, and take sweep_panels_given's answer
};
inline SweepPanels sweep_panel_count(int64_t nrows, int64_t ncols, int64_t nnz, size_t es, int64_t h_hint, const SweepKnobs &k) {
    SweepPanels w;
    if (k.panel_mode == 2 || nrows <= 0 || nnz <= 0) return w;
    w.plan = true;
    int64_t budget_rows = std::max<int64_t>(1, k.panel_bytes / 128);
    // groups whose rows of X hold at most 4 elements never take the wide sweep: their panels are sized for the LDS-staged SpMV kernel instead
    // (a panel of X, h elements per column, inside 128 KiB of a workgroup's LDS; the rest parks results)
    if (h_hint >= 1 && h_hint <= 4 && k.vec_lds && k.vec_kernel)
        budget_rows = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(budget_rows, 65536),  // (16-bit panel-local ids)
                                                             (int64_t)((128 * 1024 - 64) / ((size_t)h_hint * es))));
    const uint32_t npan = (uint32_t)std::max<int64_t>(1, (ncols + budget_rows - 1) / budget_rows);
    // too few entries per (row, panel) for L2 blocking: ONE panel, never no plan.  The sweep's other half -- length-sorted items, 32-id column
    // chunks, line-sized gathers from the slice-major copy, wave-cooperative long rows -- still beats whole-row gathers (products-shaped,
    // X = 2.5 GB: 23.8 ms against 28.6 ms for k_csr_wide)
    const bool worth = k.panel_mode == 1 || panels_pay(nnz, nrows, npan, k.panel_min_seg);
    w.npan = worth ? npan : 1;
    // column panels are cut by binary search inside each row: the rows must hold sorted column ids (torch_sparse / coalesce() deliver them sorted)
    w.ask_sorted = w.npan > 1;
    return w;
}
// the panel count once the device has answered (unsorted means nothing where it was not asked)
inline uint32_t sweep_panels_given(const SweepPanels &w, bool unsorted) { return w.ask_sorted && unsorted ? 1 : w.npan; }
inline uint32_t sweep_panel_cols(int64_t ncols, uint32_t npan) { return (uint32_t)((ncols + npan - 1) / npan); }

// Panel pointers: pp[q * nrows + r] is the first entry of row r in panel q, pp[npan * nrows + r] its end.  One panel: the row pointers.
inline std::vector<uint32_t> one_panel_pointers(const uint32_t *rowptr, size_t nrows) {
    std::vector<uint32_t> pp(2 * nrows);
    std::copy(rowptr, rowptr + nrows, pp.begin());
    std::copy(rowptr + 1, rowptr + nrows + 1, pp.begin() + nrows);
    return pp;
}

// ---- heavy rows ---------------------------------------------------------------------------------------------------------------------------------------
// rows whose share of ONE panel is enormous (16x the long-row threshold) leave the sweep for the segment kernels; merely long items stay and
// are walked by a whole wave (panel_coop)
inline std::vector<char> sweep_heavy_rows(const uint32_t *pp, size_t nrows, uint32_t npan, uint32_t base_thresh) {
    std::vector<char> heavy(nrows, 0);
    for (uint32_t q = 0; q < npan; q++) {
        const uint32_t *lo = pp + (size_t)q * nrows, *hi = lo + nrows;
        for (size_t r = 0; r < nrows; r++)
            if ((uint64_t)(hi[r] - lo[r]) > (uint64_t)base_thresh * 16) heavy[r] = 1;
    }
    return heavy;
}

// ---- the locality rank --------------------------------------------------------------------------------------------------------------------------------
// Is the question "which rows are alike" asked for the sweep's items?  The SpMV end keeps its length classes; a part that only adds into C (a
// correction part) is not asked about, unless it brings its parent's order along (the sparse half of a density split: sim_kind == 2).
inline bool sweep_wants_similarity(const SweepKnobs &k, int64_t h_hint, bool is_extra, int sim_kind) {
    return k.panel_locality && !(h_hint >= 1 && h_hint <= 4) && (!is_extra || sim_kind == 2);
}
// rank of every row in the locality order (empty = items by length alone).  kind 1: the stored ids are local already; kind 2: sim_order holds
// the rows ordered by (label, id), one entry per row
inline std::vector<uint32_t> sweep_locality_rank(int sim_kind, const std::vector<uint32_t> &sim_order, size_t nrows) {
    std::vector<uint32_t> rank;
    if (sim_kind == 1) {
        rank.resize(nrows);
        for (size_t r = 0; r < nrows; r++) rank[r] = (uint32_t)r;
    } else if (sim_kind == 2 && sim_order.size() >= nrows) {
        rank.resize(nrows);
        for (size_t k = 0; k < nrows; k++) rank[sim_order[k]] = (uint32_t)k;
    }
    return rank;
}

// ---- the items ----------------------------------------------------------------------------------------------------------------------------------------
constexpr uint32_t SWEEP_ITEM_FIRST = 0x80000000u;   // the item starts at its row's first entry (no entries in earlier panels): it writes, not adds
constexpr uint32_t SWEEP_ITEM_LAST = 0x40000000u;    // it ends at the row's last (none in later panels)

struct SweepItems {
    std::vector<uint32_t> rows, beg, lens;   // per item: its row, its first entry, length | FIRST | LAST
    std::vector<size_t> panel_off;           // npan + 1 offsets into the item arrays
    std::vector<uint32_t> panel_coop;        // per panel: leading items longer than coop_cap (walked by a whole wave)
    std::vector<uint32_t> panel_long128;     // per panel: leading items with more than 256 / 128 / 64 / 32 entries, 4 counts each
    std::vector<uint64_t> panel_nnz;         // per panel: entries of its items
};

// Per panel the rows with entries in it, longest first (stable); heavy rows in none.  rank empty: by length alone.
inline SweepItems sweep_items(const uint32_t *rowptr, const uint32_t *pp, size_t nrows, uint32_t npan, const std::vector<char> &heavy,
                              const std::vector<uint32_t> &rank, bool is_extra, uint32_t coop_cap) {
    SweepItems it;
    it.panel_off.assign(1, 0);
    std::vector<uint32_t> order;
    for (uint32_t q = 0; q < npan; q++) {
        const uint32_t *lo = pp + (size_t)q * nrows, *hi = lo + nrows;
        order.clear();
        for (size_t r = 0; r < nrows; r++) {
            if (heavy[r]) continue;   // segment kernels
            // (empty rows are items of panel 0: they zero their row of C; a correction part only ever adds, so it has none)
            if (hi[r] > lo[r] || (q == 0 && rowptr[r + 1] == rowptr[r] && !is_extra)) order.push_back((uint32_t)r);
        }
        {   // stable counting sort by item length, longest first (O(items + longest))
            uint32_t longest = 0;
            for (uint32_t r : order) longest = std::max(longest, hi[r] - lo[r]);
            std::vector<size_t> start((size_t)longest + 2, 0);
            for (uint32_t r : order) start[(size_t)(longest - (hi[r] - lo[r])) + 1]++;
            for (size_t k = 1; k < start.size(); k++) start[k] += start[k - 1];
            std::vector<uint32_t> sorted(order.size());
            for (uint32_t r : order) sorted[start[(size_t)(longest - (hi[r] - lo[r]))]++] = r;
            order.swap(sorted);
        }
        uint32_t nco = 0;
        for (uint32_t r : order) nco += (hi[r] - lo[r] > coop_cap) ? 1u : 0u;   // sorted: a prefix
        if (!rank.empty() && order.size() > nco) {
            // LOCALITY order behind the wave-cooperative prefix: blocks of 2048 rows of the similarity (or id) order, longest first inside a block
            // (a stable counting sort by block of the length-sorted list).  Workgroups that run side by side on an XCD then gather the same
            // community's rows of X out of its L2 instead of 8 x 32 unrelated ones
            const uint32_t nblk = (uint32_t)((nrows + 2047) / 2048);
            std::vector<size_t> bstart((size_t)nblk + 1, 0);
            for (size_t k = nco; k < order.size(); k++) bstart[(size_t)(rank[order[k]] >> 11) + 1]++;
            for (size_t k = 1; k < bstart.size(); k++) bstart[k] += bstart[k - 1];
            std::vector<uint32_t> byblk(order.size() - nco);
            for (size_t k = nco; k < order.size(); k++) byblk[bstart[rank[order[k]] >> 11]++] = order[k];
            std::copy(byblk.begin(), byblk.end(), order.begin() + nco);
        }
        it.panel_coop.push_back(nco);
        uint32_t n256 = 0, n128 = 0, n64 = 0, n32 = 0;
        uint64_t pn = 0;
        for (uint32_t r : order) {
            const uint32_t l = hi[r] - lo[r];
            n256 += l > 256u ? 1u : 0u;   // sorted: prefixes
            n128 += l > 128u ? 1u : 0u;
            n64 += l > 64u ? 1u : 0u;
            n32 += l > 32u ? 1u : 0u;
            pn += l;
        }
        for (uint32_t n : {n256, n128, n64, n32}) it.panel_long128.push_back(n);
        it.panel_nnz.push_back(pn);
        for (uint32_t r : order) {
            it.rows.push_back(r);
            it.beg.push_back(lo[r]);
            it.lens.push_back((hi[r] - lo[r]) | (lo[r] == rowptr[r] ? SWEEP_ITEM_FIRST : 0u) | (hi[r] == rowptr[r + 1] ? SWEEP_ITEM_LAST : 0u));
        }
        it.panel_off.push_back(it.rows.size());
    }
    return it;
}
inline uint32_t sweep_coop_cap(const SweepKnobs &k) { return (uint32_t)std::max<int64_t>(64, k.panel_coop); }

// ---- 16-bit panel-local column ids (2 bytes per entry more, half the index bytes per sweep) -------------------------------------------------------------
inline bool sweep_wants_col16(const SweepKnobs &k, uint32_t panel_cols, int64_t nnz, size_t n_items) {
    return k.panel_col16 && panel_cols <= 65536 && nnz > 0 && n_items > 0;
}
// (+ 64 bytes: the LDS-staged SpMV kernel fetches ids four at a time and may read past the last entry)
inline size_t sweep_col16_bytes(int64_t nnz) { return (size_t)nnz * 2 + 64; }

}  // namespace pygim
