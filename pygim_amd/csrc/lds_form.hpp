// lds_form.hpp -- WHICH LDS-staged form a sparse part gets (lds_plan.hpp builds it; rt_plans.inc build_lds_plan_form does the device work).
//
// lds_choose_form is a pure function of a handful of integers: the part's sizes and flags, the width of the group's products, the
// device's compute units, the kernel constants of the generated header and a copy of the tunables the decision reads.  It touches no
// device, no global and no file, so every rule below can be asked on a CPU in microseconds (tests/native/lds_form_main.cpp).
// What needs the device or the built schedule stays with the builder: whether the columns are sorted, the similarity order, whether the
// long-slots geometry is taken (it depends on the schedule's slot count), the forced failures of lds_fail and everything that allocates.
//
// Host-only C++17: no device header, no runtime state.
#pragma once
#include "lds_plan.hpp"

namespace pygim {

// element type codes (the C ABI's PYGIM_INT8 .. PYGIM_DBL64; rt_plans.inc asserts that they agree)
enum : int { LDS_EL_INT8 = 0, LDS_EL_INT16 = 1, LDS_EL_INT32 = 2, LDS_EL_INT64 = 3, LDS_EL_FLT32 = 4, LDS_EL_DBL64 = 5 };

// the constants of the generated kernels (lds_kernel_gen.hpp), handed in so that this header needs none of it
struct LdsKernelConsts {
    uint32_t kc = 320, lds_bytes = 163840;     // LDS_KC, LDS_BYTES
    uint32_t ka8 = 0, batch8 = 0;              // lds_ka(8), lds_batch(8)
    uint32_t ka16 = 0, batch16 = 0;            // lds_ka(16), lds_batch(16)
    uint32_t l16_ka = 0, l16_batch = 0;        // LDS_L16_KA, LDS_L16_BATCH
};

struct LdsFormInput {
    int dtype = -1;                 // element type code
    size_t val_es = 0;              // bytes of a stored value (and of an element of X)
    int64_t nrows = 0, ncols = 0, nnz = 0;
    bool valued = false;            // the part carries values (else unit weights)
    bool is_extra = false, lds_forced = false, lds_contig_tiles = false;
    int64_t h_hint = 0;             // width of the group's products (0 = unknown)
    int cu_count = 0;
    bool allow_code = true;         // false: the second rung of build_lds_plan's ladder (the token form of the same product)
    LdsKernelConsts k;
};

// exactly the tunables the decision reads (rt_state.inc Tunables, same names and meanings)
struct LdsFormKnobs {
    int64_t lds_mode = 0, lds_min_reuse_x100 = 75, lds_min_width = 5, lds_min_width8 = 33, lds_min_reuse_narrow_x100 = 75;
    int64_t lds_waves = 16, lds_long_slots = 128, lds_code = 1;
    int64_t lds_col_split = 0, lds_col_split_f32 = 1, lds_row_tail = 3, lds_half_split = 1, lds_split_order = 1, lds_fill_tiles = 1;
    int64_t lds_code_nbuf = 0, lds_code_waves = 0, lds_code_kc = 0, lds_code_boundary = 0, lds_code_exp = 0;
    int64_t lds_round_tiles = 1, lds_tile_order = 2, lds_codegen = 1, lds_fail = 0;
};

struct LdsForm {
    bool plan = false;              // false: no LDS-staged plan for this part (rule, type or width) -- nothing else below is meaningful
    LdsGeometry geo;                // complete: ring, hand-off, tile height, column ranges, half-split
    bool want_code = false;         // the code-stream form (else the token form)
    size_t es = 0;                  // element size the plan is made for (INT8 rides the INT16 stream: 2)
    uint32_t rows_lds = 0;          // rows the plan's tiles cover (fewer than nrows: the others take the tail kernels)
    uint32_t half_H = 0;            // > 0: half-split plan, rows of its staged copy
    uint32_t code_op = 0;           // the accumulate of a code stream (lds_code_from_plan's opcode_add)
    double min_reuse_x100 = 0;      // the reuse threshold that was applied (x 100)
    bool want_similarity = false;   // similarity tiles are asked for ...
    bool similarity_forced = false; // ... whatever the ids' locality says
    bool device_codegen = false;    // the device code generator may write the stream; else, for a code stream, codegen_why says why not
    const char *codegen_why = "";
    bool long_candidate = false;    // token form: the builder re-plans in long_geo when the schedule has lds_long_slots tokens per (wave, slot)
    LdsGeometry long_geo;           // (whether it does depends on the schedule's slot count, which only the builder knows)
};

// The ring of a code-stream plan: buffers and columns per chunk (from the tunables; whole 1 KiB pieces per wave, inside the LDS).
inline void lds_code_ring(uint32_t NW, uint32_t row_bytes, const LdsFormKnobs &t, uint32_t lds_bytes, uint32_t &NBUF, uint32_t &KC) {
    int64_t nbuf = t.lds_code_nbuf;
    if (nbuf == 0) nbuf = NW == 8 ? LDS_CODE8_AUTO_NBUF : 2;
    nbuf = std::min<int64_t>(std::max<int64_t>(nbuf, 2), 10);
    static const uint32_t kc_of[11] = {0, 0, 320, 192, 160, 128, 96, 64, 64, 64, 64};
    uint32_t kc = t.lds_code_kc > 0 ? (uint32_t)t.lds_code_kc : kc_of[nbuf] * 256 / row_bytes;
    const uint32_t kq = 1024 * NW / row_bytes;                          // columns of one 1 KiB piece per wave
    kc = std::max(kq, kc / kq * kq);                                    // whole pieces per wave
    while ((uint64_t)kc * row_bytes * (uint64_t)nbuf > lds_bytes || kc * (uint32_t)nbuf > 640) kc -= kq;   // (the LDS; 10-bit LDS rows in a token)
    KC = kc;
    NBUF = (uint32_t)nbuf;
}

inline uint32_t lds_code_op(int dtype) {
    return dtype == LDS_EL_FLT32 ? 0x02000000u : dtype == LDS_EL_INT32 ? 0x68000000u : dtype == LDS_EL_DBL64 ? LDS_CODE_ADD_F64 :
           dtype == LDS_EL_INT64 ? LDS_CODE_ADD_U64 : LDS_CODE_PK_ADD_U16;
}

inline LdsForm lds_choose_form(const LdsFormInput &in, const LdsFormKnobs &t) {
    LdsForm f;
    size_t es = in.val_es;
    const bool code_knobs = in.allow_code && t.lds_code && t.lds_waves == 16 && t.lds_code_waves != 16;
    const bool int8_code = es == 1 && in.dtype == LDS_EL_INT8 && code_knobs;
    if (es == 1) {   // INT8: the 8-wave INT16 code stream on features widened to 16 bits (no token form, no 16-wave form)
        if (!int8_code) return f;
        es = 2;
    }
    // INT64 / DBL64, unit weights: the 8-wave code stream on rows of 512 bytes (a register pair per value; no token form)
    // (round 5: valued DBL64 too -- the value through an SGPR pair)
    // valued INT64: the 64-bit product from 32-bit pieces (v_mul_lo_u32 + v_mad_u64_u32; values of any size, the encoders pick the form)
    const bool el8_code = es == 8 && (in.dtype == LDS_EL_INT64 || in.dtype == LDS_EL_DBL64) && code_knobs;
    if (es == 8 && !el8_code) return f;
    if (t.lds_mode == 2 || (es != 4 && es != 2 && es != 8) || in.is_extra || in.nnz == 0 || in.nrows == 0 || in.ncols == 0) return f;
    if ((in.valued || es == 2) && t.lds_waves != 16) return f;  // the valued and the INT16 kernels exist for the 16-wave geometry
    // no product of this group is wide enough (lds_launch.hpp lds_takes; INT8 rides the INT16 stream: lanes of two features): no plan, no code
    if (in.h_hint > 0 && (es == 8 ? in.h_hint : (in.h_hint * (int64_t)std::max<size_t>(es, 2)) / 4) < (es == 8 ? t.lds_min_width8 : t.lds_min_width)) return f;
    if ((uint64_t)in.ncols * (es == 8 ? 512ull : 256ull) >= (1ull << 32) - (1ull << 20) || (uint64_t)in.nnz >= (1ull << 31)) return f;
    const uint32_t nrows = (uint32_t)in.nrows, ncols = (uint32_t)in.ncols;
    const uint32_t cus = (uint32_t)std::max(in.cu_count, 1);
    LdsGeometry geo;
    geo.NW = t.lds_waves == 16 ? 16 : 8;
    geo.KA = geo.NW == 16 ? in.k.ka16 : in.k.ka8;
    geo.KC = in.k.kc;
    geo.BATCH = geo.NW == 16 ? in.k.batch16 : in.k.batch8;
    geo.keep_tile_order = in.lds_contig_tiles ? 1u : 0u;
    // FLT32 / INT32 with unit weights: the code-stream form (the schedule compiled into machine code); its plan is built in the
    // geometry of its kernels and serves no token kernel
    // (valued matrices: FLT32 -- the value is the literal of a v_mul_f32 in the stream -- and, round 5, INT32: v_mul_lo_u32 is VOP3 and takes no
    // literal on gfx9, so the value rides as an inline constant when every value of the matrix lies in [-16, 64], else through an SGPR)
    const bool want_code = in.allow_code && t.lds_code && geo.NW == 16 &&
                           ((es == 4 && in.dtype == LDS_EL_FLT32) || (es == 4 && in.dtype == LDS_EL_INT32) ||
                            (es == 2 && in.dtype == LDS_EL_INT16) || int8_code || el8_code);
    const int64_t slice_b = es == 8 ? 512 : 256;   // bytes of a row of a slice
    const int64_t nsl_hint = in.h_hint > 0 ? (in.h_hint * (int64_t)es + slice_b - 1) / slice_b : 4;
    if (want_code) {
        // 8 waves x 228 accumulators (2 waves per SIMD): tiles of 1 824 rows -- Reddit h = 256 is two rounds of workgroups on 256 CUs
        // instead of three, a third less of X staged -- or round 3's 16 waves x 96
        const int64_t cw = t.lds_code_waves;
        const bool eight = cw == 8 || (cw != 16 && LDS_CODE_AUTO_WAVES == 8) || int8_code || el8_code;
        if (eight) {
            geo.NW = 8;
            geo.KA = el8_code ? LDS_CODE8_KA64 : LDS_CODE8_KA;
            geo.BATCH = 8;
        }
        if (el8_code) geo.row_bytes = 512;
    }
    // tiles sized so that one product of the group's width runs as whole rounds of workgroups (lds_plan.hpp)
    if (t.lds_round_tiles && in.h_hint > 0) geo.rows_per_tile = lds_rows_per_tile(nrows, geo.NW * geo.KA, (uint32_t)nsl_hint, cus);
    // a row share too short to fill the device with workgroups that each stream a whole slice of X (a rank's share on N GPUs: 24 tiles x
    // 4 slices on 256 CUs): full-height row tiles, each split into S column ranges -- S x as many workgroups, each landing 1/S of X;
    // partial sums per range, reduced in range order (launch_lds).  Integers stay exact; FLT32 only when asked (lds_col_split_f32)
    // Round 6: FLT32 too by default, for parts of a million entries and more (a rank's share of a large graph: 0.93 -> 0.45 ms for a 1/8 row share of the
    // Reddit-shaped graph) -- a row's sum is then the sum of its column ranges' sums, inside the path's 1e-5 of |A|.|x| but no longer the CPU loop's bits;
    // lds_col_split_f32 = 0 keeps the stored-order form, and the group's note says which one it got
    const bool f32_split_ok = t.lds_col_split_f32 == 1 ? in.nnz >= (1 << 20) : t.lds_col_split_f32 != 0;
    uint32_t rows_lds = nrows;   // rows the plan's tiles will cover (fewer: see below)
    if (t.lds_col_split != 1 && (geo.NW == 16 || want_code) && !el8_code && (in.dtype != LDS_EL_FLT32 || f32_split_ok) && !in.valued) {   // (round 6: INT8 too)
        const uint64_t nsl = in.h_hint > 0 ? (uint64_t)nsl_hint : 1;
        const uint64_t tall = ((uint64_t)in.nrows + geo.NW * geo.KA - 1) / (geo.NW * geo.KA), wgs = tall * nsl;
        uint32_t S = 1;
        if (t.lds_col_split > 1) S = (uint32_t)std::min<int64_t>(t.lds_col_split, 16);
        else if (wgs * 2 <= cus) S = (uint32_t)std::min<uint64_t>(8, cus / wgs);
        // Round 6: a share whose rows ALL BUT fit tall' x slices x S' = one workgroup per compute unit for a larger S' (29 471 rows: 16 full tiles x 4 slices x 4
        // ranges = 256 workgroups hold 29 184 of them, against 17 x 4 x 3 = 204 for all) keeps its last few rows out of the plan: k_lds_tail takes them from the
        // same staged copy (launch_lds).  4-byte element types, unit weights, plans written by the device or the host encoder alike (they see fewer rows).
        if (t.lds_col_split == 0 && t.lds_row_tail > 0 && want_code && es == 4 && !in.lds_forced && (uint64_t)in.nrows * 8 < (1ull << 31)) {
            const uint64_t full = (uint64_t)geo.NW * geo.KA;
            for (uint32_t S2 = 8; S2 > S; S2--) {
                const uint64_t tall2 = cus / (nsl * S2);
                if (!tall2) continue;
                const uint64_t covered = tall2 * full;
                if (covered >= (uint64_t)in.nrows) break;   // (S itself would be at least S2)
                if (((uint64_t)in.nrows - covered) * 100 <= (uint64_t)in.nrows * (uint64_t)t.lds_row_tail && tall2 * nsl * S2 * 10 >= (uint64_t)cus * 9) {
                    S = S2;
                    rows_lds = (uint32_t)covered;
                    break;
                }
            }
        }
        if (S > 1 && (uint64_t)in.nrows * S < (1ull << 31)) {
            geo.col_splits = S;
            geo.rows_per_tile = 0;   // full-height tiles: the column ranges fill the device
            // one round of workgroups: nothing to gain from heaviest-first, and in their natural order (row tile x S + range) the launch's XCD interleave
            // (tile t on XCD set t mod G, G = 4 or 8) hands an XCD the tiles of ONE column range when S is 2, 4 or 8 -- its L2 then streams one range per
            // slice for 16 row tiles instead of every range for four (0.64 -> 0.57 us per chunk on a 1/8 share, profiles/r06_stamps.txt)
            if (t.lds_split_order && (((uint64_t)rows_lds + geo.NW * geo.KA - 1) / (geo.NW * geo.KA)) * nsl * S <= cus) geo.keep_tile_order = 1;
            // ... and when tall x slices x S still leaves compute units without a workgroup (17 tall tiles x 4 slices x 3 ranges = 204 of 256), MORE,
            // lighter row tiles for the same S: every workgroup streams the same N / S columns either way, with fewer entries per chunk
            // (the stamps of profiles/r06_stamps.txt: 26 % of the CU-time of that launch was idle; one round only -- workgroups of a later round
            // would stream their chunks out of step with the others and miss them in the L2)
            if (t.lds_col_split == 0 && t.lds_fill_tiles && rows_lds == nrows) {
                const uint64_t tall2 = cus / (nsl * S);
                if (tall2 > tall && tall2 <= 2 * tall) geo.rows_per_tile = (uint32_t)std::max<uint64_t>(16, ((uint64_t)in.nrows + tall2 - 1) / tall2);
            }
        }
    }
    if (want_code) {
        // the ring.  Two buffers of 320 columns: the workgroup meets at every slot boundary (round 3).  Three or more (round 4): one
        // barrier in the middle of a slot, NBUF - 2 chunks in flight beside the one being read, no drain at the boundary -- the DMA
        // requests of a CU never dry up (the fill-rate micro-benchmark of scripts/micro: 81 GB/s per CU with 2 x 80 KiB, 113 GB/s with 3 x 48 or 4 x 40 KiB)
        lds_code_ring(geo.NW, geo.row_bytes, t, in.k.lds_bytes, geo.NBUF, geo.KC);
        // measured (profiles/r04_lds_kernel.md): with five buffers the boundary form -- four chunks in flight -- is 1-2 % ahead of the mid-slot form on
        // every shape tried (2.02-2.04 against 2.06 ms on the bench workload, DBL64 7.03 against 7.12): the default
        geo.boundary = t.lds_code_boundary == 2 ? 0u : 1u;
    }
    // Round 6: HALF-SPLIT plans for products of 17..32 lanes (all rows x 32 FLT32 features: a feature-split rank).  A 64-lane slice would be half empty and every tile
    // would still stage all of X in 256-byte rows; instead a staged row holds TWO columns' 32 lanes side by side ([X[c] | X[c + H]]: half the rows, half the
    // staged bytes), the plan is made of the virtual columns c mod H with each entry's half in its value slot, the stream adds under the lower / upper half of
    // EXEC and the store adds the two halves (lds_plan.hpp LdsGeometry::half_split, scripts/gen_lds_kernel.py).  A row's sum becomes (sum over the lower range)
    // + (sum over the upper range): integers exact, FLT32 under the same rule as column-split tiles.
    const int64_t lanes_hint = in.h_hint > 0 ? (in.h_hint * (int64_t)es + 3) / 4 : 0;
    const bool half = want_code && t.lds_half_split && es == 4 && geo.NW == 8 && !in.valued && !in.lds_forced && lanes_hint > 0 && lanes_hint <= 32 &&
                      (in.dtype == LDS_EL_INT32 || (in.dtype == LDS_EL_FLT32 && f32_split_ok)) && rows_lds == nrows && (uint64_t)in.ncols >= 4ull * geo.KC &&
                      !t.lds_code_exp && !(t.lds_fail & 7);
    uint32_t half_H = 0;
    if (half) {
        half_H = (uint32_t)(((((uint64_t)in.ncols + 1) / 2 + geo.KC - 1) / geo.KC) * geo.KC);
        geo.half_split = 1;
    }
    // (products of at most 32 lanes gather fewer bytes per entry on the sweep: their plans must serve more entries per staged column to pay -- rt_state.inc)
    const bool narrow_hint = es != 8 && lanes_hint > 0 && lanes_hint <= 32;
    f.min_reuse_x100 = !narrow_hint ? (double)t.lds_min_reuse_x100
                                    : std::max((double)t.lds_min_reuse_x100, (double)t.lds_min_reuse_narrow_x100 * (half ? 1.6 : 1.0));
    if (t.lds_mode == 0 && !in.lds_forced && lds_plan_uniform_reuse((uint64_t)in.nnz, nrows, half ? half_H : ncols, geo) * 100.0 < f.min_reuse_x100) return f;
    f.plan = true;
    f.geo = geo;
    f.want_code = want_code;
    f.es = es;
    f.rows_lds = rows_lds;
    f.half_H = half_H;
    f.code_op = lds_code_op(in.dtype);
    // Round 5: similarity tiles (lds_reorder_dev.hpp) -- rows with similar neighbourhoods share a tile: shared LDS reads, skipped chunks.
    // The result does not depend on the order (each row is summed by one wave in stored order whichever tile holds it).
    f.want_similarity = want_code && in.nrows == in.ncols && rows_lds == nrows && !half &&
                        (t.lds_tile_order == 1 || in.lds_forced || (t.lds_tile_order == 2 && in.nnz >= (1 << 20)));
    f.similarity_forced = t.lds_tile_order == 1 || in.lds_forced;
    // Round 5: the code stream GENERATED ON THE DEVICE (lds_codegen_dev.hpp) -- not with a forced failure or a timing experiment
    f.device_codegen = want_code && t.lds_codegen && !(t.lds_fail & 7) && !t.lds_code_exp;
    if (want_code && !f.device_codegen) f.codegen_why = !t.lds_codegen ? "lds_codegen = 0" : (t.lds_fail & 7) ? "lds_fail set" : "timing experiment";
    // long slots (a community-structured graph: a tile streams few chunks, a wave gets hundreds of tokens per chunk): the per-batch
    // bookkeeping is what is left to save -- the 16-token-batch geometry, when the tiles fit its 80 accumulators per wave
    if (geo.NW == 16 && !in.valued && !want_code && t.lds_long_slots) {
        LdsGeometry gl = geo;
        gl.KA = in.k.l16_ka;
        gl.BATCH = in.k.l16_batch;
        gl.rows_per_tile = geo.col_splits > 1 ? 0 : t.lds_round_tiles && in.h_hint > 0 ? lds_rows_per_tile(nrows, gl.NW * gl.KA, (uint32_t)nsl_hint, cus) : 0;
        const uint32_t r_now = geo.rows_per_tile ? geo.rows_per_tile : geo.NW * geo.KA, r_new = gl.rows_per_tile ? gl.rows_per_tile : gl.NW * gl.KA;
        if (r_new >= r_now) {  // no more tiles than before
            f.long_candidate = true;
            f.long_geo = gl;
        }
    }
    return f;
}

}  // namespace pygim
