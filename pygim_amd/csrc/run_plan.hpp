// run_plan.hpp -- WHAT one call of a group product does (rt_run.inc run_group_common does it): the geometry of the caller's dense windows, whether host
// operands run as a pipeline of feature windows and which, and the ordered block products with where each finds its X.
//
// Everything run_group_common decides is a pure function of plain numbers: element size, the group's sizes, the parts' column counts and dense
// splits, the caller's window addresses as integers and their strides, a copy of the four tunables the rules read (RunKnobs, filled in one
// place: rt_run.inc run_knobs) and the facts the runtime had to ask the device for, as values (HostFacts).  Where the rules ask "is this window's
// product ONE pass of the LDS-staged kernel" (rt_launch.inc lds_writes_c_once) they take a callable writes_once(w, c_address).
// One rule is written once here: dense windows that do not already sit side by side in one row-major matrix are laid side by side in
// Group::xcat with a row stride rounded up to 16 bytes (place_runs).  tests/native/run_plan_main.cpp asks all of it on a CPU.
// What needs the device stays with the runtime: the pointer queries, every allocation, the copies, the launches, the streams and events of the
// pipeline, the timers.
//
// Host-only C++17: no device header, no runtime state.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace pygim {

// exactly the tunables the rules read (rt_state.inc Tunables, same names and meanings)
struct RunKnobs {
    int64_t host_windows = 0, host_direct = 1, fuse_windows = 1, merge_parts = 1;
};

struct RunPart {   // a sparse part, as far as a call's plan goes
    int64_t ncols = 0;
    const int64_t *dense_cols = nullptr;   // widths of its dense windows
    size_t nd = 0;
};
struct RunShape {
    size_t es = 4;           // bytes of an element
    bool is_float = false;   // FLT32 / DBL64
    int64_t h = 0, total_rows = 0, total_cols = 0;
    const RunPart *parts = nullptr;
    size_t nparts = 0;
    bool per_part = false;   // grande layout: windows flattened over the parts, each holding only the rows of its own part; else every part reads
                             // its row range of the SAME windows
};
struct RunWindow {
    int64_t rows = 0, ld = 0, width = 0;   // ld: row stride, elements
};

inline size_t run_window_count(const RunShape &s) {
    if (!s.per_part) return s.parts[0].nd;
    size_t n = 0;
    for (size_t i = 0; i < s.nparts; i++) n += s.parts[i].nd;
    return n;
}

// the windows' geometry for both conventions (ld == nullptr: every window is as wide as its stride); the refusal's text, or nullptr
inline const char *run_windows(const RunShape &s, const int64_t *ld, std::vector<RunWindow> &win) {
    win.resize(run_window_count(s));
    size_t k = 0;
    if (s.per_part) {
        for (size_t i = 0; i < s.nparts; i++)
            for (size_t j = 0; j < s.parts[i].nd; j++, k++) {
                win[k] = {s.parts[i].ncols, ld ? ld[k] : s.parts[i].dense_cols[j], s.parts[i].dense_cols[j]};
                if (win[k].ld < win[k].width) return "window stride smaller than its width";
            }
    } else {
        for (; k < win.size(); k++) win[k] = {s.total_cols, ld ? ld[k] : s.parts[0].dense_cols[k], s.parts[0].dense_cols[k]};
    }
    return nullptr;
}

// ---- the one layout rule ---------------------------------------------------------------------------------------------------------------------------
// Windows that sit side by side in one row-major matrix (equal strides, each starting where its left neighbour's columns end) are read in place.
// Others are laid side by side in Group::xcat, one 2-D copy each: window j's columns start where the widths before it end, and the row stride is
// the full width rounded up to 16 bytes, so that the sweep's 16-byte pieces stay available.
inline int64_t xcat_row_stride(int64_t width, size_t es) { return (int64_t)((((size_t)width * es + 15) & ~(size_t)15) / es); }

struct RunCopy {      // rows x width elements of window `win`, from byte src_off of it at the window's own stride, to byte dst_off of xcat at the stride of
    size_t dst_off;   // the product (or pipeline window) that reads them; one per window, so some are empty (no columns, or no rows): nothing to issue
    size_t win, src_off;
    int64_t width, rows;
};
struct WindowRun {    // windows [k0, k0 + n) from their row src_row on, `rows` rows; the runs of one placement lie one below the other in xcat
    size_t k0, n;
    int64_t src_row, rows;
};
struct XSource {
    bool in_place = true;
    uintptr_t base = 0;        // in place: the address of the first element; else the rows start at xcat
    int64_t ldx = 0;           // row stride, elements
    size_t xcat_bytes = 0;     // what xcat must hold (0 in place)
};

inline bool side_by_side(const RunWindow *win, const uintptr_t *addr, size_t k0, size_t n, size_t es) {
    for (size_t j = 1; j < n; j++)
        if (win[k0 + j].ld != win[k0].ld || addr[k0 + j] != addr[k0 + j - 1] + (size_t)win[k0 + j - 1].width * es) return false;
    return true;
}

// `width`: the columns the reader takes (the row of xcat is that wide).  In place when allowed, every run is side by side, and the runs are one
// row range after the other of the same windows.  Otherwise the copies are appended to `copies` (addr may be nullptr when in place is not allowed).
inline XSource place_runs(const RunWindow *win, const uintptr_t *addr, const WindowRun *runs, size_t nruns, int64_t width, size_t es, bool may_stay,
                          std::vector<RunCopy> &copies) {
    XSource x;
    int64_t next_row = nruns ? runs[0].src_row : 0;
    for (size_t r = 0; r < nruns && may_stay; r++) {
        may_stay = runs[r].k0 == runs[0].k0 && runs[r].n == runs[0].n && runs[r].src_row == next_row && (r > 0 || side_by_side(win, addr, runs[0].k0, runs[0].n, es));
        next_row += runs[r].rows;
    }
    if (may_stay && nruns && runs[0].n) {
        x.base = addr[runs[0].k0] + (size_t)runs[0].src_row * (size_t)win[runs[0].k0].ld * es;
        x.ldx = win[runs[0].k0].ld;
        return x;
    }
    x.in_place = false;
    x.ldx = xcat_row_stride(width, es);
    int64_t drow = 0;
    for (size_t r = 0; r < nruns; r++) {
        int64_t a = 0;
        for (size_t k = runs[r].k0; k < runs[r].k0 + runs[r].n; k++) {
            copies.push_back({((size_t)drow * x.ldx + (size_t)a) * es, k, (size_t)runs[r].src_row * (size_t)win[k].ld * es, win[k].width, runs[r].rows});
            a += win[k].width;
        }
        drow += runs[r].rows;
    }
    x.xcat_bytes = std::max<size_t>((size_t)drow * x.ldx * es, 256);
    return x;
}

// ---- the block products of a call: sum over sparse parts, concatenate over dense windows -------------------------------------------------------------
struct RunProduct {
    int part = 0;            // index of the sparse part; -1: the merged matrix (Group::merged)
    XSource x;               // not in place: copies [copy0, copy1) of the plan go first, then the product reads xcat
    uint32_t copy0 = 0, copy1 = 0;
    int64_t ccol = 0, width = 0;   // columns [ccol, ccol + width) of C
    bool accumulate = false;
};
struct ProductPlan {
    std::vector<RunProduct> products;
    std::vector<RunCopy> copies;
    size_t xcat_bytes = 0;   // the largest any product needs (0: none reads xcat)
};

// addr: the windows on the device.  Three shapes: ONE product with the merged matrix; per part ONE product of its windows' full width (fuse_windows:
// a window is an artefact of the reference's DPU layout, and narrow windows -- 32 int8 = 32 bytes -- would waste the 128-byte gather); one product
// per window.
inline void plan_products(const RunShape &s, const RunWindow *win, const uintptr_t *addr, const RunKnobs &t, bool has_merged, ProductPlan &plan) {
    plan.products.clear();
    plan.copies.clear();
    plan.xcat_bytes = 0;
    auto place = [&](int part, const WindowRun *runs, size_t nruns, int64_t width, bool accumulate) {
        RunProduct q;
        q.part = part;
        q.copy0 = (uint32_t)plan.copies.size();
        q.x = place_runs(win, addr, runs, nruns, width, s.es, true, plan.copies);
        q.copy1 = (uint32_t)plan.copies.size();
        q.width = width;
        q.accumulate = accumulate;
        plan.xcat_bytes = std::max(plan.xcat_bytes, q.x.xcat_bytes);
        plan.products.push_back(q);
    };
    int64_t brow = 0;
    size_t kbase = 0;
    if (has_merged && t.merge_parts && s.nparts > 1) {
        // (per-part windows: the parts' row ranges one below the other)
        std::vector<WindowRun> runs(s.nparts);
        for (size_t i = 0; i < s.nparts; i++) {
            runs[i] = {s.per_part ? kbase : 0, s.parts[i].nd, s.per_part ? 0 : brow, s.parts[i].ncols};
            brow += s.parts[i].ncols;
            kbase += s.parts[i].nd;
        }
        place(-1, runs.data(), runs.size(), s.h, false);
        return;
    }
    for (size_t i = 0; i < s.nparts; i++) {
        const size_t nd = s.parts[i].nd, k0 = s.per_part ? kbase : 0;
        const int64_t src_row = s.per_part ? 0 : brow;
        if (nd > 1 && t.fuse_windows) {
            int64_t wsum = 0;
            for (size_t j = 0; j < nd; j++) wsum += win[k0 + j].width;
            const WindowRun run{k0, nd, src_row, s.parts[i].ncols};
            place((int)i, &run, 1, wsum, i > 0);
        } else {
            int64_t acol = 0;
            for (size_t j = 0; j < nd; j++) {
                RunProduct q;
                q.part = (int)i;
                q.x.base = addr[k0 + j] + (size_t)src_row * (size_t)win[k0 + j].ld * s.es;
                q.x.ldx = win[k0 + j].ld;
                q.ccol = acol;
                q.width = win[k0 + j].width;
                q.accumulate = i > 0;
                plan.products.push_back(q);
                acol += q.width;
            }
        }
        brow += s.parts[i].ncols;
        kbase += nd;
    }
}

// ---- host operands as a pipeline of feature windows (rt_run.inc run_group_windows; the measurements are told there) ---------------------------------
struct HostPiece {       // one of the caller's narrow feature blocks inside a window (grande's per-unit windows, ds_parts blocks of a few bytes per row)
    uintptr_t src;        // host: [rows x pitch_el], contiguous
    int64_t pitch_el, w;  // its row stride and true width, elements
    size_t dev_off;       // where the block lands in stage_in (as it is: one 1-D copy)
    int64_t acol;         // its first column in C (and in the assembled X)
};
struct HostWindow {
    uintptr_t src;        // host
    int64_t pitch_el;     // host and device row stride of this window's block, elements
    size_t dev_off;       // byte offset of the window's first element in stage_in
    int64_t acol, w;      // columns [acol, acol + w) of C
    // a window ASSEMBLED from several of the caller's blocks: each goes up as it is and is laid into its columns of Group::xcat (row stride xcat_ld elements)
    // on the device -- the copies of place_runs with an upload in front; the product then reads xcat
    std::vector<HostPiece> pieces;
    int64_t xcat_ld = 0;
};
struct HostFacts {             // what the runtime asked the device (host_facts_needed says which of the first two a call needs; the others cost nothing)
    bool out_pinned = false;   // the result is page-locked host memory
    uintptr_t out_alias = 0;   // ... as the kernels see it; 0: pageable, or not mapped for this device
    bool copies_slow = false;  // Group::host_copies_slow
    bool has_merged = false;
    uintptr_t stage_out = 0;   // the staged result (a window's product is asked about at its columns of it)
};
struct HostPlan {
    std::vector<HostWindow> windows;   // empty: the serial path
    bool direct = false;               // the products store straight into the result's device alias
    size_t xcat_bytes = 0;             // what xcat must hold (0: not touched) -- asked for even where the windows are dropped afterwards
};

// where window k lands in stage_in (each on a 256-byte boundary); the bytes of stage_in
inline size_t host_stage_layout(const RunWindow *win, size_t nwin, size_t es, std::vector<size_t> &off) {
    size_t total = 0;
    off.resize(nwin);
    for (size_t k = 0; k < nwin; k++) {
        off[k] = total;
        total += (((size_t)win[k].rows * win[k].ld * es) + 255) & ~(size_t)255;
    }
    return std::max<size_t>(total, 256);
}

// the pipeline serves one sparse operand (a single part, or the merged matrix) and windows that are column ranges of C (per-part windows of ONE part: grande)
inline bool host_pipeline_eligible(const RunShape &s, const RunKnobs &t, bool has_merged) {
    return t.host_windows != 1 && s.h > 0 && (s.nparts == 1 || (!s.per_part && has_merged && t.merge_parts));
}
inline bool host_operands_large(const RunShape &s) {   // both ways at least 32 MB: below that the serial call is as fast
    return (size_t)s.total_cols * s.h * s.es >= ((size_t)32 << 20) && (size_t)s.total_rows * s.h * s.es >= ((size_t)32 << 20);
}
struct HostFactsNeeded {
    bool out_pinned, out_alias;
};
inline HostFactsNeeded host_facts_needed(const RunShape &s, const RunKnobs &t, bool has_merged, bool copies_slow) {
    const bool e = host_pipeline_eligible(s, t, has_merged);
    return {e && t.host_windows == 0 && host_operands_large(s), e && (t.host_direct == 2 || (t.host_direct == 1 && copies_slow))};
}

// the last window's download, alone on the link, ran below 40 GB/s (bytes per ms = MB/s x 1e-3): later calls of the group store directly (host_direct = 1)
inline bool host_download_was_slow(int64_t w, size_t es, int64_t rows, double ms) {
    if (w <= 0 || rows <= 0) return false;
    const double mb = (double)w * (double)es * (double)rows * 1e-6;
    return mb >= 16 && ms > 0 && mb / ms < 40.0;
}

// addr: the windows in HOST memory; off: host_stage_layout.  writes_once(w, c_address): the product of width w into C at that address (row stride h) is
// one pass of the LDS-staged kernel that writes every element once and reads none.
template <typename WritesOnce>
inline HostPlan plan_host_pipeline(const RunShape &s, const RunWindow *win, const uintptr_t *addr, const size_t *off, const RunKnobs &t, const HostFacts &f,
                                   WritesOnce &&writes_once) {
    HostPlan plan;
    if (!host_pipeline_eligible(s, t, f.has_merged)) return plan;
    const size_t es = s.es, nwin = run_window_count(s);
    const int64_t h = s.h;
    // automatic: large operands and a page-locked result (a pitched copy into pageable memory is slower than the serial call)
    const bool automatic = host_operands_large(s) && (t.host_windows != 0 || f.out_pinned);
    // DIRECT mode (tunable host_direct): the products store straight into the caller's page-locked tensor -- decided on the full width here, checked
    // window by window below.  1 = adaptive: the copies first (8.2 ms per call when the DMA engines move the result's windows at the link rate); a call
    // whose last download ran below 40 GB/s -- the runtime's pitched copies to the host run at 55, 34 or 21 GB/s depending on what the process allocated
    // and freed before (its DMA-engine bookkeeping; the rect_lottery micro-benchmark under scripts/micro:the same buffers, the same stream, 34 -> 21 GB/s after the device heap
    // was churned): the same call then takes 11.8 ms -- turns this group to the direct mode (8.9 ms, whatever the engines do) for its later calls.  2 = always.
    uintptr_t out_dev = (t.host_direct == 2 || (t.host_direct == 1 && f.copies_slow)) ? f.out_alias : 0;
    if (out_dev && ((out_dev & 255) || (((size_t)h * es) & 15) || !writes_once(h, out_dev))) out_dev = 0;
    const int64_t slice_el = std::max<int64_t>(1, 256 / (int64_t)es);
    std::vector<HostWindow> &pw = plan.windows;
    // the windows: once for the direct mode, again for the copies if a window's product turns out not to be the one-pass LDS-staged kernel
    for (int attempt = out_dev ? 0 : 1; attempt < 2; attempt++) {
        pw.clear();
        if (attempt == 1) out_dev = 0;
        if (nwin == 1 && win[0].ld >= win[0].width && win[0].width == h) {
            // one row-major X: cut into windows of whole 256-byte slices (64 lanes of the LDS-staged product), the wider ones first.  Automatic: 512 bytes
            // of a row per window (the DMA engines move such pieces at the 1-D rate; four windows of 256 bytes: 8.8 ms with the copies, 10.2 direct)
            const int64_t S = (h + slice_el - 1) / slice_el;
            const int64_t auto_bytes = 512;
            int64_t n = t.host_windows > 1 ? t.host_windows : (automatic ? (h * (int64_t)es + auto_bytes - 1) / auto_bytes : 1);
            n = std::min<int64_t>(std::min<int64_t>(n, 16), S);
            if (n > 1) {
                int64_t a = 0;
                for (int64_t k = 0; k < n && a < h; k++) {
                    const int64_t w = std::min<int64_t>((S / n + (k < S % n ? 1 : 0)) * slice_el, h - a);
                    pw.push_back({addr[0] + (size_t)a * es, win[0].ld, (size_t)a * es, a, w, {}, 0});
                    a += w;
                }
            }
        } else if (nwin > 1 && (t.host_windows > 1 || automatic)) {
            // the caller's own feature blocks (ds_parts; grande's per-unit windows, grande.py:12-23: blocks of `pad` columns of which the first
            // width count): blocks of 512 bytes of a row and more are windows as they are; narrower ones (eight units: 32 floats each) are gathered
            // into windows of that size -- each block goes up in one piece and is laid into its columns of xcat on the device
            int64_t hsum = 0;
            bool narrow = false;
            for (size_t k = 0; k < nwin; k++) {
                hsum += win[k].width;
                narrow = narrow || (size_t)win[k].width * es < 512 || win[k].ld != win[k].width;
            }
            if (hsum == h && !narrow && nwin <= 16) {
                int64_t a = 0;
                for (size_t k = 0; k < nwin; k++) {
                    pw.push_back({addr[k], win[k].ld, off[k], a, win[k].width, {}, 0});
                    a += win[k].width;
                }
            } else if (hsum == h) {
                std::vector<RunCopy> copies;
                const WindowRun all{0, nwin, 0, s.total_cols};
                const XSource x = place_runs(win, nullptr, &all, 1, h, es, /*may_stay=*/false, copies);
                plan.xcat_bytes = x.xcat_bytes;
                const int64_t target = t.host_windows > 1 ? (h + t.host_windows - 1) / t.host_windows : std::max<int64_t>(1, 512 / (int64_t)es);
                HostWindow cur{0, 0, 0, 0, 0, {}, x.ldx};
                for (size_t k = 0; k < nwin; k++) {   // (copies[k] places window k)
                    const int64_t acol = (int64_t)(copies[k].dst_off / es);
                    cur.pieces.push_back({addr[k], win[k].ld, copies[k].width, off[k], acol});
                    cur.w += copies[k].width;
                    if (cur.w >= target || k + 1 == nwin) {
                        pw.push_back(cur);
                        cur = HostWindow{0, 0, 0, acol + copies[k].width, 0, {}, x.ldx};
                    }
                }
                if (pw.size() > 16) pw.clear();
            }
        }
        bool direct_ok = out_dev != 0;
        for (const HostWindow &q : pw)
            if (direct_ok && ((((size_t)q.acol * es) & 15) || !writes_once(q.w, out_dev + (size_t)q.acol * es))) direct_ok = false;
        if (direct_ok || attempt == 1) break;
    }
    // FLOAT sums on the L2 sweep depend on the product's width (how many lanes share a long row's entries): a window's product would be inside the norm-wise
    // contract but not the serial call's bits.  Left to itself the library pipelines a float product only where every window is the LDS-staged kernel's
    // (stored-order sums, or the plan's fixed column ranges: the same bits at any width); host_windows > 1 asks for the windows whatever the kernels.
    if (t.host_windows == 0 && s.is_float)
        for (const HostWindow &q : pw)
            if (!writes_once(q.w, f.stage_out + (size_t)q.acol * es)) {
                pw.clear();
                break;
            }
    if (pw.size() <= 1) pw.clear();   // (one window is the serial call)
    plan.direct = !pw.empty() && out_dev != 0;
    return plan;
}

}  // namespace pygim
