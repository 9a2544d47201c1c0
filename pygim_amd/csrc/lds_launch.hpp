// lds_launch.hpp -- HOW a product runs on a part's LDS-staged plan (lds_form.hpp chose the plan's form; rt_launch.inc launch_lds does the device work).
//
// Everything launch_lds decides before it touches the device is a pure function of plain numbers: the geometry of the staged copy of X
// (lds_staged), how the workgroups lie over the XCDs (lds_xcd_layout), whether a product takes the LDS-staged kernel at all (lds_takes) and
// the launch itself (lds_plan_launch: kernel, grid, the scalar arguments, the scratch layout, the reduce and tail steps that follow, or a
// refusal).  Each is written once here and asked on a CPU by tests/native/lds_launch_main.cpp.
// What needs the device stays with the launcher: finding or making the staged copy, the pointers of the arguments, the kernel table, the
// dynamic-LDS attribute and the launches.
//
// Host-only C++17: no device header, no runtime state.
#pragma once
#include "lds_form.hpp"

namespace pygim {

// rows of a slice of the staged copy: whole chunks of the part's ring (the DMA of a tile's last chunk reads KC rows whatever the
// matrix's width; 320-column chunks of the token kernels when the part names none), 64-row aligned
inline uint64_t lds_rows_pad(uint64_t ncols, uint32_t kc) {
    const uint64_t k = kc ? kc : 320;
    return ((ncols + k - 1) / k * k + 63) / 64 * 64;
}

// exactly the tunables the launch rules read (rt_state.inc Tunables, same names and meanings)
struct LdsLaunchKnobs {
    int64_t lds_xcd_slices = 0, lds_touch_share = 1, lds_code = 1, lds_ablate = 0, lds_mode = 0, lds_min_width = 5, lds_min_width8 = 33;
    int64_t panel_mode = 0, csr_kernel = 0, force_vec_bytes = 0, lds_direct_x = 1;
};

// the plan fields of a Part that the rules read (rt_launch.inc lds_part_plan copies them, the only place)
struct LdsPartPlan {
    bool has_plan = false, is_code = false;       // lds_tiles != nullptr; lds_is_code
    bool valued = false, wdelta = false;          // vals != nullptr; lds_wdelta != 0
    bool contig_tiles = false, col_order = false, tail_tables = false;   // lds_contig_tiles; lds_col_order / both tail tables != nullptr
    uint32_t nw = 8, batch = 8, kc = 0, row_bytes = 256, col_splits = 1, half = 0, rows = 0, ntiles = 0, tail_nseg = 0;   // lds_nw .. lds_tail_nseg
    uint32_t code_gsize = 0, code_nsets = 0;
    uint64_t slots = 0;
    int64_t nrows = 0, ncols = 0;
};

inline size_t lds_el_bytes(int dtype) {
    return dtype == LDS_EL_INT8 ? 1 : dtype == LDS_EL_INT16 ? 2 : (dtype == LDS_EL_INT64 || dtype == LDS_EL_DBL64) ? 8 : 4;
}

// ---- the staged copy of X: slice-major, 256-byte rows (64 features of 4 bytes, 128 of 2; INT8 widened to 16 bits: 128) or 512-byte rows (64 features
// of 8 bytes), rows padded to whole chunks.  A half-split plan: ONE slice whose rows hold two columns' 32 lanes side by side, H = lds_half rows.
struct LdsStaged {
    uint32_t eps = 64, row_bytes = 256, nslices = 1;   // elements of a slice, bytes of a staged row, slices
    uint64_t rows_pad = 0, slice_stride = 0;           // rows of a slice, bytes between two slices
    size_t bytes = 0;                                  // of the whole copy
    int kind = 1;                                      // what a cached copy is labelled with: 1 = plain, 3 = widened INT8, 5 = half-split
};
inline LdsStaged lds_staged(size_t es, bool widen8, uint32_t w, uint64_t ncols, uint32_t lds_kc, uint32_t lds_half) {
    LdsStaged s;
    s.row_bytes = es == 8 ? 512 : 256;
    s.eps = widen8 ? 128 : s.row_bytes / (uint32_t)es;
    s.nslices = lds_half ? 1u : (w + s.eps - 1) / s.eps;
    s.rows_pad = lds_half ? (uint64_t)lds_half : lds_rows_pad(ncols, lds_kc);
    s.slice_stride = s.rows_pad * s.row_bytes;
    s.bytes = (size_t)s.slice_stride * s.nslices;
    s.kind = lds_half ? 5 : widen8 ? 3 : 1;
    return s;
}

// ---- How a launch of the LDS-staged kernel lays its workgroups over the XCDs: group = XCDs that share the tiles of one set of slices (0 = no
// XCD mapping: slice counts that do not divide 8), sx = slices per XCD, touch_share = the sx workgroups that run a tile's code streams side
// by side share the touches (LdsArgs.touch_share).  One rule for the launch and for what pygim_group_lds_geometry reports.
struct LdsXcdLayout {
    uint32_t group = 0, sx = 1, touch_share = 0;
};
inline LdsXcdLayout lds_xcd_layout(const LdsPartPlan &p, uint32_t nslices, bool el8, const LdsLaunchKnobs &t) {
    LdsXcdLayout l;
    // (slice counts that do not divide 8 interleave the slices over the XCDs; a slice-major order measured the same: 2.86 vs 2.80 ms at h = 192)
    l.group = (nslices == 1 || nslices == 2 || nslices == 4 || nslices == 8) ? 8 / nslices : 0;
    // round 5: sx slices per XCD -- the workgroups an XCD runs side by side are then the sx slices of ONE tile and
    // share its code stream in that XCD's L2 (fetched from the fabric nslices / sx times instead of nslices), at the price of sx
    // slices of X streamed through every L2 instead of one
    if (l.group && p.is_code && nslices > 1) {
        // 0 = automatic (profiles/r05_exp_xcd.txt): two slices per XCD -- fabric traffic 5.28 -> 4.19 GB on the bench workload --
        // and all (up to four) of them for plans whose tiles skip most chunks (little of X to un-share): 5.57 -> 3.72 GB, 1.05 -> 0.98 ms
        uint32_t sx = (uint32_t)std::max<int64_t>(0, t.lds_xcd_slices);
        if (sx == 0) {
            const uint64_t nchunks = ((uint64_t)p.ncols + p.kc - 1) / std::max(1u, p.kc);
            const double fill = p.ntiles && nchunks ? (double)p.slots / ((double)p.ntiles * (double)nchunks) : 1.0;
            sx = fill < 0.3 ? std::min(nslices, 4u) : (el8 ? 1u : 2u);   // (8-byte rows: one slice per XCD measured 1 % ahead, 7.05-7.13 against 7.17-7.18 ms)
            // (plans that stream every chunk, with the touches shared -- profiles/exp_touch_share.txt, bench workload: two slices 2.04 -> 1.97 ms, four 2.10 -> 1.99:
            // the pair stays the fastest arrangement, the second pair's slices of X cost more than its touches save)
        }
        if (sx > 1 && sx <= nslices && nslices % sx == 0) {
            l.sx = sx;
            l.group *= sx;
        }
    }
    // the partners of a toucher ask for one dword per touch instead of eight lines (L1 -> L2 read requests of the bench workload 271.5 M -> 257.0 M per product,
    // 2.04 -> 1.97 ms): only the 8-wave shells set the touch register per workgroup, and only plans whose x registers leave it free touch through it
    // (lds_plan.hpp lds_code_regs)
    if (l.sx > 1 && t.lds_touch_share && p.is_code && p.nw == 8 && lds_code_touch_shareable(lds_code_regs(8, p.code_gsize, p.code_nsets, p.row_bytes == 512)))
        l.touch_share = 1;
    return l;
}

// ---- Whether launch_block hands a product of w elements a row, written to C (row stride ldc elements, address c_addr), to the LDS-staged kernel.
// busy: the group is inside a fused call that owns the product (deq_out or pre_xs set)
inline bool lds_takes(int dtype, const LdsPartPlan &p, uint32_t w, int64_t ldc, uintptr_t c_addr, bool accumulate, bool busy, const LdsLaunchKnobs &t) {
    const size_t es = lds_el_bytes(dtype);
    if (es == 8) {  // INT64 / DBL64: the 8-wave code stream on 512-byte rows (unit weights; round 5: valued too -- a valued part has a code plan only when its values allow it)
        if (!p.is_code || p.nw != 8 || p.row_bytes != 512 || p.col_splits > 1) return false;
    } else if (p.row_bytes == 512) return false;
    if (es == 1) {  // INT8 rides the 8-wave INT16 code stream (features widened to 16 bits in the staged copy); it adds into C only on a column-split plan
                    // (round 5: valued too -- the values are part of the stream; round 6: column-split plans -- k_lds_reduce16 makes the bytes, and adds into C when asked)
        if (!p.is_code || p.nw != 8 || (accumulate && p.col_splits <= 1)) return false;
        if ((int64_t)(w / 2) < t.lds_min_width) return false;
    }
    if (es == 2) {  // two features to a lane: whole lanes, dword-aligned rows of C, the 16-wave plan
        if ((w & 1) || (ldc & 1) || (c_addr & 3) || (p.nw != 16 && !p.is_code)) return false;
    }
    if (!p.has_plan || t.lds_mode == 2 || (!p.is_code && p.valued != p.wdelta) || busy) return false;
    if (p.half && (es != 4 || w > 32)) return false;   // (a half-split plan: plain products of at most 32 lanes)
    if (p.is_code && (!t.lds_code || t.lds_ablate)) return false;   // (a code-stream plan serves no token kernel: the sweep instead)
    if (t.lds_mode == 0 && (t.panel_mode == 1 || t.csr_kernel != 0 || t.force_vec_bytes != 0)) return false;  // another kernel was asked for by name
    if (es > 1 && (int64_t)(es == 8 ? (size_t)w : (size_t)w * es / 4) < (es == 8 ? t.lds_min_width8 : t.lds_min_width)) return false;   // (lanes: 4-byte units of a row; 8-byte: features)
    if ((uint64_t)ldc * es >= (1ull << 32)) return false;
    return true;
}

// ---- the launch
// which kernel: the shell, the element of its stream, the dequantising store, the measurement and timing-experiment builds (rt_launch.inc holds the table)
enum : uint32_t { LDS_SH_W16 = 0, LDS_SH_W16B = 1, LDS_SH_W16_VAL = 2, LDS_SH_W8 = 3, LDS_SH_CODE16 = 4, LDS_SH_CODE8 = 5 };
struct LdsKernelId {
    uint32_t shell = LDS_SH_W16;
    int el = LDS_EL_FLT32;      // (INT8 names the INT8 stores of the INT16 stream; its column-split plans run the INT16 kernel itself)
    bool deq = false, stamp = false;
    uint32_t ablate = 0;        // the ablation build's variant (0 = the kernel itself)
    constexpr uint32_t key() const { return shell | (uint32_t)el << 4 | (deq ? 1u : 0u) << 8 | (stamp ? 1u : 0u) << 9 | ablate << 16; }
};
constexpr uint32_t lds_kernel_key(uint32_t shell, int el, bool deq = false, bool stamp = false, uint32_t ablate = 0) {
    return LdsKernelId{shell, el, deq, stamp, ablate}.key();
}

enum : int { LDS_RED_NONE = 0, LDS_RED_16_PLAIN, LDS_RED_16_DEQ8, LDS_RED_16_DEQ16, LDS_RED_V4, LDS_RED_DEQ, LDS_RED_PLAIN };   // k_lds_reduce16<0|1|2>, _v4, _deq, k_lds_reduce

struct LdsLaunchInput {
    int dtype = LDS_EL_FLT32;
    LdsPartPlan p;
    uint32_t w = 0;
    int64_t ldx = 0, ldc = 0;
    bool x_aligned256 = false;   // X's address is a multiple of 256
    bool accumulate = false;
    bool prestaged = false;      // X came slice-major from the caller (the fused quantiser)
    bool amax = false;           // the result is dequantised: C holds floats
    bool c_aligned16 = false;    // C's address is a multiple of 16
    bool stamp = false;          // a stamp buffer is set (lds_stamp)
    bool ablate_build = false;   // the library holds the timing-experiment variants
    uint32_t l16_batch = 16;     // LDS_L16_BATCH of the generated header
};

struct LdsLaunch {
    const char *refusal = nullptr;   // != nullptr: no launch, this text
    LdsStaged xs;
    bool x_in_place = false;         // the caller's matrix IS the staged form (if its allocation also covers the padded rows: the launcher looks)
    uint32_t w_lanes = 0;
    bool split16 = false;            // a column-split plan of the 16-bit streams whose result is not the packed sum: k_lds_reduce16 makes it
    bool deq_at_reduce = false;      // the dequantisation happens where the ranges' partial sums meet
    bool kernel_amax = false;        // amax (and the per-column epilogue) rides the kernel's own store
    bool to_scratch = false;         // the kernel writes partial sums to the group's scratch block
    uint32_t ldc_bytes = 0, accumulate = 0;   // ... of the kernel's store (LdsArgs)
    uint32_t ntiles = 0, xcd_group = 0, xcd_sx = 1, touch_share = 0, half_split = 0, xcd_contig = 0;
    uint32_t grid = 0, block = 0;
    LdsKernelId kernel;
    // the scratch block: [col_splits][lds_rows][ldp] partial sums of part_es bytes, then, 256-byte aligned, what the tail kernels park
    uint32_t col_splits = 1;
    uint64_t lds_rows = 0, ldp = 0;
    size_t part_es = 0, split_bytes = 0, park_bytes = 0, scratch_bytes = 0;   // scratch_bytes: 0 = the launch needs none
    int reduce = LDS_RED_NONE;
    uint64_t reduce_total = 0;       // threads of the reduce step
    bool tail = false;               // k_lds_tail_seg / _fin take the rows behind lds_rows
    uint32_t ntail = 0;
    int64_t tail_ldc_bytes = 0;      // bytes of a row of C as the tail's store sees it (4-byte results either way)
};

inline LdsLaunch lds_plan_launch(const LdsLaunchInput &in, const LdsLaunchKnobs &t) {
    LdsLaunch L;
    const LdsPartPlan &p = in.p;
    const size_t es = lds_el_bytes(in.dtype);
    const bool wide8 = es == 1, el8 = es == 8;   // INT8: staged as INT16, summed by the INT16 stream; INT64 / DBL64: 512-byte rows, a register pair per value
    const uint32_t w = in.w, S = p.col_splits;
    auto refuse = [&](const char *why) { L.refusal = why; return L; };
    // round 6: column-split plans of the 16-bit streams whose result is not the packed 16-bit sum itself (INT8 results, dequantised INT8 / INT16): the INT16 stream's
    // plain kernel writes the ranges' packed partial sums, k_lds_reduce16 makes the result where they meet
    L.split16 = S > 1 && (wide8 || (es == 2 && in.amax));
    // (INT8, and the dequantising INT16 store: the kernel masks features one by one; 8-byte: a lane = a feature)
    L.w_lanes = L.split16 ? (uint32_t)(((size_t)w * 2 + 3) / 4) : (wide8 || el8 || (es == 2 && in.amax)) ? w : (uint32_t)(((size_t)w * es + 3) / 4);
    if (p.half && (es != 4 || w > 32 || in.prestaged || in.amax)) return refuse("internal: a half-split LDS plan serves plain 4-byte products of at most 32 lanes");
    L.xs = lds_staged(es, wide8, w, (uint64_t)p.ncols, p.kc, p.half);
    const uint32_t nslices = L.xs.nslices;
    // A product of ONE slice whose rows of X are exactly the staged row (64 FLT32 / INT32 features at a stride of 64; 128 INT16; 64 of an 8-byte type) needs no copy
    // (all rows x 64 FLT32 features: 0.61 -> 0.59 ms)
    L.x_in_place = !in.prestaged && t.lds_direct_x && L.xs.kind == 1 && nslices == 1 && !p.col_order && (size_t)in.ldx * es == L.xs.row_bytes &&
                   (size_t)w * es == L.xs.row_bytes && in.x_aligned256;
    L.ldc_bytes = (uint32_t)((size_t)in.ldc * (((wide8 || es == 2) && in.amax) ? 4 : es));   // (the dequantising store writes floats)
    L.ntiles = p.ntiles;
    L.accumulate = in.accumulate ? 1 : 0;
    // column-split plans: the tiles write the partial sums of column range c to row r + c * nrows of a scratch block (compact rows of
    // w_lanes dwords); the reduce step adds the S blocks in range order into C afterwards
    L.col_splits = S;
    L.ldp = L.split16 ? (uint64_t)L.w_lanes * 2 : (uint64_t)L.w_lanes * 4 / es;   // elements of a partial row (split16: 16-bit numbers)
    L.part_es = L.split16 ? 2 : es;
    L.lds_rows = p.rows ? p.rows : (uint64_t)p.nrows;   // rows the plan's tiles cover (the rest: the tail step)
    // round 6: the dequantising product on a column-split plan -- the plain kernel writes the ranges' partial sums, the reduce step dequantises where they meet
    L.deq_at_reduce = S > 1 && in.amax;
    L.kernel_amax = in.amax && !L.deq_at_reduce && !L.split16;
    L.tail = L.lds_rows < (uint64_t)p.nrows && w > 0;   // the share's last rows, from the same staged copy
    if (S > 1) {
        L.to_scratch = true;
        L.ldc_bytes = (uint32_t)(L.ldp * L.part_es);
        L.accumulate = 0;
        L.split_bytes = ((size_t)S * (size_t)L.lds_rows * L.ldp * L.part_es + 255) & ~(size_t)255;
    }
    // (what the tail kernels park lies behind the ranges' partial sums: ONE allocation, made before anything is launched into it)
    if (S > 1 || L.tail) {
        L.park_bytes = (size_t)p.tail_nseg * nslices * 64 * 8;   // 64 accumulators per (segment, slice), 8 bytes kept for each (the 4-byte types' are 4)
        L.scratch_bytes = std::max<size_t>(L.split_bytes + L.park_bytes, 256);
    }
    const LdsXcdLayout lay = lds_xcd_layout(p, nslices, el8, t);
    L.xcd_group = lay.group;
    L.xcd_sx = lay.sx;
    L.touch_share = lay.touch_share;
    L.half_split = p.half ? 1u : 0u;
    L.xcd_contig = (L.xcd_group && p.contig_tiles) ? (p.ntiles + L.xcd_group - 1) / L.xcd_group : 0;
    L.grid = L.xcd_group ? 8 * ((p.ntiles + L.xcd_group - 1) / L.xcd_group) * L.xcd_sx : p.ntiles * nslices;
    L.block = p.nw * 64;
    // ---- which kernel
    const bool long16 = p.nw == 16 && p.batch == in.l16_batch;   // the 16-token-batch geometry (no values)
    const bool w8 = p.nw == 8, deq = L.kernel_amax;
    LdsKernelId &k = L.kernel;
    k.el = in.dtype;
    k.deq = deq;
    if (p.is_code) {   // the schedule compiled into machine code: 16 waves x 96 accumulators, or 8 x 228
        if (!t.lds_code || t.lds_ablate) return refuse("this group's LDS plan is a code stream: lds_code was switched off (or lds_ablate on) after it was created");
        k.shell = w8 ? LDS_SH_CODE8 : LDS_SH_CODE16;
        if (el8) {
            if (!w8 || deq || S > 1 || p.row_bytes != 512) return refuse("internal: 8-byte LDS-staged product on an unsupported plan");
        } else if (es == 1) {
            if (!w8 || (in.accumulate && S <= 1)) return refuse("internal: INT8 LDS-staged product on an unsupported plan");
            if (L.split16) k.el = LDS_EL_INT16;   // (widened to 16 bits in the staged copy: the INT16 stream)
        } else if (es == 2) {
            if ((deq || L.split16) && !w8) return refuse("internal: dequantising LDS-staged product on an unsupported plan");   // (two features to a lane: v_pk_add_u16)
        }
        // measurement build (scripts/exp_stamps.py): the caller's buffer gets four clock stamps per wave of every workgroup
        k.stamp = in.stamp && w8 && in.dtype == LDS_EL_FLT32 && !deq;
    } else if (es == 1 || es == 8) {
        return refuse("internal: the INT8 / INT64 / DBL64 LDS-staged product exists in the code-stream form only");
    } else if (deq) {
        if (p.nw != 16 || p.wdelta || es != 4) return refuse("internal: dequantising LDS-staged product on an unsupported plan");
        k.shell = long16 ? LDS_SH_W16B : LDS_SH_W16;
    } else if (es == 2) {
        if (p.nw != 16) return refuse("internal: INT16 LDS-staged product needs the 16-wave plan");
        k.shell = long16 ? LDS_SH_W16B : p.wdelta ? LDS_SH_W16_VAL : LDS_SH_W16;
    } else {
        k.shell = long16 ? LDS_SH_W16B : p.nw != 16 ? LDS_SH_W8 : p.wdelta ? LDS_SH_W16_VAL : LDS_SH_W16;
        if (in.dtype == LDS_EL_FLT32 && !long16) {
            // timing experiments (wrong results, scripts/gen_lds_kernel.py; make ablate): variants of the plain 16-wave kernel
            if (in.ablate_build) k.ablate = k.shell == LDS_SH_W16 ? (uint32_t)std::max<int64_t>(0, t.lds_ablate) : 0;
            else if (t.lds_ablate) return refuse("lds_ablate needs the ablation build (make -C pygim_amd/csrc ablate)");
        }
    }
    if (deq && t.lds_ablate) return refuse("lds_ablate is a timing experiment of the plain kernel");
    // ---- what follows the kernel
    if (S > 1 && L.lds_rows > 0 && w > 0) {
        if (L.split16) {
            L.reduce = !in.amax ? LDS_RED_16_PLAIN : wide8 ? LDS_RED_16_DEQ8 : LDS_RED_16_DEQ16;
            L.reduce_total = L.lds_rows * w;
        } else if (es == 4 && (w & 3) == 0 && (L.ldp & 3) == 0 && (in.ldc & 3) == 0 && in.c_aligned16) {
            // four features to a thread (16-byte loads and stores): a 1/8 row share's reduce 32 -> 21 us
            L.reduce = LDS_RED_V4;
            L.reduce_total = L.lds_rows * (w >> 2);
        } else {
            L.reduce = L.deq_at_reduce ? LDS_RED_DEQ : LDS_RED_PLAIN;
            L.reduce_total = L.lds_rows * w;
        }
    }
    if (L.tail) {
        if (es != 4) return refuse("internal: an LDS plan that leaves rows to the tail kernels exists for 4-byte element types only");
        if (!p.tail_tables) return refuse("internal: an LDS plan that leaves rows out has no segment table for them");
        L.ntail = (uint32_t)((uint64_t)p.nrows - L.lds_rows);
        L.tail_ldc_bytes = in.ldc * 4;
    }
    return L;
}

}  // namespace pygim
