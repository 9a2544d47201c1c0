// Test infrastructure: the launch rules of the LDS-staged product (pygim_amd/csrc/lds_launch.hpp) asked from a command line, without a device.
//   g++ -std=c++17 -O1 -Wall tests/native/lds_launch_main.cpp -o lds_launch
//   lds_launch -        one case per line of standard input, "name=value ..." (names: the fields of LdsLaunchInput, of its LdsPartPlan and of
//                       LdsLaunchKnobs, plus c_addr and busy for lds_takes; anything not named keeps its default); one line of
//                       "name=value ..." per case on standard output: lds_staged, lds_xcd_layout, lds_takes and lds_plan_launch
//   lds_launch          the self-check: the shapes whose launches the documents quote, derived by hand, then every plan lds_choose_form hands
//                       out on a grid of shapes, widths, element types and tunables through the launch rules with their invariants checked
//                       -- the run to make under -fsanitize=address,undefined -fno-sanitize-recover=all
#include "../../pygim_amd/csrc/lds_launch.hpp"

#include <cinttypes>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

using namespace pygim;

// the geometries of the generated kernels (scripts/gen_lds_kernel.py GEOS, GEO_L16)
static LdsKernelConsts kernel_consts() {
    LdsKernelConsts k;
    k.kc = 320; k.lds_bytes = 163840;
    k.ka8 = 192; k.batch8 = 16;
    k.ka16 = 96; k.batch16 = 8;
    k.l16_ka = 80; k.l16_batch = 16;
    return k;
}

struct Case {
    LdsLaunchInput in;
    LdsLaunchKnobs t;
    uintptr_t c_addr = 0;
    bool busy = false;
};

static bool set_field(Case &c, const std::string &name, int64_t v) {
#define IN(f) if (name == #f) { c.in.f = (decltype(c.in.f))v; return true; }
    IN(dtype) IN(w) IN(ldx) IN(ldc) IN(x_aligned256) IN(accumulate) IN(prestaged) IN(amax) IN(c_aligned16) IN(stamp) IN(ablate_build) IN(l16_batch)
#undef IN
#define PL(f) if (name == #f) { c.in.p.f = (decltype(c.in.p.f))v; return true; }
    PL(has_plan) PL(is_code) PL(valued) PL(wdelta) PL(contig_tiles) PL(col_order) PL(tail_tables) PL(nw) PL(batch) PL(kc) PL(row_bytes) PL(col_splits) PL(half)
    PL(rows) PL(ntiles) PL(tail_nseg) PL(code_gsize) PL(code_nsets) PL(slots) PL(nrows) PL(ncols)
#undef PL
#define KN(f) if (name == #f) { c.t.f = v; return true; }
    KN(lds_xcd_slices) KN(lds_touch_share) KN(lds_code) KN(lds_ablate) KN(lds_mode) KN(lds_min_width) KN(lds_min_width8) KN(panel_mode) KN(csr_kernel)
    KN(force_vec_bytes) KN(lds_direct_x)
#undef KN
    if (name == "c_addr") { c.c_addr = (uintptr_t)v; return true; }
    if (name == "busy") { c.busy = v != 0; return true; }
    return false;
}

static void print_case(const Case &c) {
    const LdsLaunchInput &in = c.in;
    const size_t es = lds_el_bytes(in.dtype);
    const LdsStaged s = lds_staged(es, es == 1, in.w, (uint64_t)in.p.ncols, in.p.kc, in.p.half);
    const LdsXcdLayout lay = lds_xcd_layout(in.p, s.nslices, es == 8, c.t);
    const bool takes = lds_takes(in.dtype, in.p, in.w, in.ldc, c.c_addr, in.accumulate, c.busy, c.t);
    const LdsLaunch L = lds_plan_launch(in, c.t);
    printf("eps=%u row_bytes=%u nslices=%u rows_pad=%" PRIu64 " slice_stride=%" PRIu64 " bytes=%zu kind=%d xcd_group=%u xcd_sx=%u touch_share=%u takes=%d refusal=\"%s\" "
           "w_lanes=%u split16=%d deq_at_reduce=%d kernel_amax=%d to_scratch=%d ldc_bytes=%u accumulate=%u grid=%u block=%u xcd_contig=%u half_split=%u shell=%u el=%d deq=%d "
           "stamp=%d ablate=%u lds_rows=%" PRIu64 " ldp=%" PRIu64 " part_es=%zu split_bytes=%zu park_bytes=%zu scratch_bytes=%zu reduce=%d reduce_total=%" PRIu64
           " tail=%d ntail=%u x_in_place=%d\n",
           s.eps, s.row_bytes, s.nslices, s.rows_pad, s.slice_stride, s.bytes, s.kind, lay.group, lay.sx, lay.touch_share, takes ? 1 : 0, L.refusal ? L.refusal : "", L.w_lanes,
           L.split16 ? 1 : 0, L.deq_at_reduce ? 1 : 0, L.kernel_amax ? 1 : 0, L.to_scratch ? 1 : 0, L.ldc_bytes, L.accumulate, L.grid, L.block, L.xcd_contig, L.half_split,
           L.kernel.shell, L.kernel.el, L.kernel.deq ? 1 : 0, L.kernel.stamp ? 1 : 0, L.kernel.ablate, L.lds_rows, L.ldp, L.part_es, L.split_bytes, L.park_bytes, L.scratch_bytes,
           L.reduce, L.reduce_total, L.tail ? 1 : 0, L.ntail, L.x_in_place ? 1 : 0);
}

static int from_stdin() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        Case c;
        std::istringstream ss(line);
        std::string tok;
        while (ss >> tok) {
            const size_t eq = tok.find('=');
            if (eq == std::string::npos || !set_field(c, tok.substr(0, eq), strtoll(tok.c_str() + eq + 1, nullptr, 10))) {
                fprintf(stderr, "lds_launch: what is '%s'?\n", tok.c_str());
                return 2;
            }
        }
        print_case(c);
    }
    return 0;
}

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "lds_launch self-check, line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

// the Part fields adopt_lds_plan (rt_plans.inc) would write for a form of the chooser; the schedule's numbers (tiles, chunk fills) as the builder counts them
static LdsPartPlan plan_of(const LdsFormInput &in, const LdsForm &f, const LdsGeometry &g, bool every_chunk) {
    LdsPartPlan p;
    p.has_plan = true;
    p.is_code = f.want_code;
    p.valued = in.valued;
    p.wdelta = in.valued && !f.want_code;
    p.contig_tiles = in.lds_contig_tiles;
    p.nw = g.NW; p.batch = g.BATCH; p.kc = g.KC; p.row_bytes = g.row_bytes; p.col_splits = g.col_splits;
    p.half = f.half_H;
    p.rows = f.rows_lds < (uint32_t)in.nrows ? f.rows_lds : 0;
    const uint32_t rpt = g.rows_per_tile ? g.rows_per_tile : g.NW * g.KA;
    p.ntiles = (f.rows_lds + rpt - 1) / rpt * g.col_splits;
    const uint64_t nchunks = ((uint64_t)(f.half_H ? f.half_H : in.ncols) + g.KC - 1) / g.KC;
    p.slots = every_chunk ? (uint64_t)p.ntiles * nchunks : (uint64_t)p.ntiles * nchunks / 4;
    p.tail_tables = p.rows != 0;
    p.tail_nseg = p.rows ? (uint32_t)in.nrows - p.rows : 0;   // (a segment per row left out)
    p.nrows = in.nrows;
    p.ncols = in.ncols;
    return p;
}

// RESTATEMENT (test only) of what rt_run.inc lds_fusable_part asks of the plan and the tunables beyond its own conditions (unit weights, the serving
// part, fuse_windows, no values, no half-split, the tail for 4-byte types): the gate of the DEQUANTISING product, as lds_takes is the plain product's
static bool fusable_rest(int dtype, const LdsPartPlan &p, uint32_t h, const LdsLaunchKnobs &t) {
    const size_t es = lds_el_bytes(dtype);
    if (es == 8) return false;
    if (t.lds_mode == 2 || (int64_t)h / (es <= 2 ? 2 : 1) < t.lds_min_width) return false;
    if (t.lds_mode == 0 && (t.panel_mode != 0 || t.csr_kernel != 0 || t.force_vec_bytes != 0)) return false;
    if (!p.has_plan || p.wdelta || (p.nw != 16 && !p.is_code)) return false;
    if (p.is_code && (!t.lds_code || t.lds_ablate)) return false;
    if (es <= 2 && (!p.is_code || p.nw != 8)) return false;
    return true;
}

struct Tally {
    long plans = 0, launches = 0, taken = 0, fused = 0, ablate_refusals = 0;
    long takes_not_fusable = 0, fusable_not_takes = 0;   // rows where the two gates part (unit weights, no half-split, 1-, 2- and 4-byte types)
};

// what holds for every launch the rules hand out
static int launch_invariants(const LdsLaunchInput &in, const LdsLaunch &L) {
    const LdsPartPlan &p = in.p;
    const size_t es = lds_el_bytes(in.dtype);
    CHECK(L.grid > 0 && L.block > 0 && (uint64_t)L.grid * L.block > 0);
    CHECK(L.block == p.nw * 64);
    CHECK(L.xs.nslices >= 1 && L.xs.bytes == (size_t)L.xs.rows_pad * L.xs.row_bytes * L.xs.nslices && L.xs.slice_stride == L.xs.rows_pad * L.xs.row_bytes);
    CHECK(L.xs.rows_pad % 64 == 0 || p.half);
    CHECK((uint64_t)L.xs.nslices * L.xs.eps >= in.w || p.half);
    // every workgroup of the grid finds a (tile, slice), and every (tile, slice) a workgroup
    CHECK(L.xcd_group ? (uint64_t)L.grid * L.xcd_group / (8 * L.xcd_sx) >= p.ntiles && L.xs.nslices % L.xcd_sx == 0 : L.grid == p.ntiles * L.xs.nslices);
    CHECK(L.touch_share == 0 || (L.xcd_sx > 1 && p.is_code && p.nw == 8));
    // the scratch block as the parent's launch spelled it twice: before the main launch (partial sums of part_es bytes, then 8 bytes per parked sum) and before
    // the tail launch (partial sums of the element's bytes, then the tail's 4-byte accumulators) -- the two must name the same start of the parked block
    const size_t S = p.col_splits;
    const size_t main_split = S > 1 ? (((size_t)S * (size_t)L.lds_rows * L.ldp * L.part_es + 255) & ~(size_t)255) : 0;
    CHECK(L.split_bytes == main_split && L.split_bytes % 256 == 0);
    CHECK(L.to_scratch == (S > 1) && (!L.to_scratch || (L.accumulate == 0 && L.ldc_bytes == L.ldp * L.part_es)));
    if (S > 1) CHECK(L.scratch_bytes >= main_split + (size_t)p.tail_nseg * L.xs.nslices * 64 * 8 && L.scratch_bytes >= 256);
    if (L.tail) {
        CHECK(es == 4 && L.part_es == 4 && !L.split16);
        const size_t tail_split = S > 1 ? (((size_t)S * (size_t)L.lds_rows * L.ldp * es + 255) & ~(size_t)255) : 0;
        CHECK(tail_split == L.split_bytes);
        CHECK(L.scratch_bytes >= tail_split + (size_t)p.tail_nseg * L.xs.nslices * 64 * 4);
        CHECK(L.ntail == (uint64_t)p.nrows - L.lds_rows && L.ntail > 0 && L.tail_ldc_bytes == in.ldc * 4);
    }
    CHECK((L.reduce != LDS_RED_NONE) == (S > 1 && L.lds_rows > 0 && in.w > 0));
    CHECK(L.reduce != LDS_RED_V4 || (es == 4 && in.c_aligned16 && in.w % 4 == 0 && in.ldc % 4 == 0));
    CHECK(!L.kernel_amax || (in.amax && S == 1));
    CHECK(!L.deq_at_reduce || (L.reduce == LDS_RED_V4 || L.reduce == LDS_RED_DEQ || L.reduce == LDS_RED_16_DEQ8 || L.reduce == LDS_RED_16_DEQ16));
    CHECK(L.kernel.deq == L.kernel_amax);
    return 0;
}

static int quoted_shapes() {
    const LdsLaunchKnobs t;
    // the Reddit-shaped FLT32 product at h = 256 (lds_form_main.cpp: 128 tiles of 1 821 rows, 8 waves, 5 x 128 columns): 4 slices, every chunk streamed ->
    // two slices per XCD, groups of 8 / 4 * 2 = 4 XCDs, 8 * ceil(128 / 4) * 2 = 512 workgroups: two whole rounds of 256 compute units
    LdsLaunchInput in;
    in.dtype = LDS_EL_FLT32; in.w = 256; in.ldc = 256; in.c_aligned16 = true;
    in.p.has_plan = in.p.is_code = true; in.p.nw = 8; in.p.batch = 8; in.p.kc = 128; in.p.ntiles = 128; in.p.nrows = in.p.ncols = 232965;
    in.p.slots = 128ull * ((232965 + 127) / 128);
    LdsLaunch L = lds_plan_launch(in, t);
    CHECK(!L.refusal && L.xs.nslices == 4 && L.xs.eps == 64 && L.xs.kind == 1 && L.xcd_sx == 2 && L.xcd_group == 4 && L.touch_share == 1 && L.grid == 512 && L.grid == 2 * 256);
    CHECK(L.block == 512 && L.kernel.shell == LDS_SH_CODE8 && L.kernel.el == LDS_EL_FLT32 && !L.kernel.deq && L.reduce == LDS_RED_NONE && !L.tail && L.scratch_bytes == 0);
    CHECK(L.xs.rows_pad == 233088 && L.xs.slice_stride == 233088ull * 256 && L.w_lanes == 256 && L.ldc_bytes == 1024);
    // a 1/8 row share, INT32, h = 256: 16 full tiles x 4 column ranges = 64 tiles hold 29 184 of 29 384 rows, a quarter of the chunks filled (5 008 of 64 x 313) ->
    // all four slices on one XCD, groups of 8 XCDs, 8 * ceil(64 / 8) * 4 = 256 workgroups; the partial sums take 4 * 29184 * 256 * 4 bytes and the parked block starts there
    in = LdsLaunchInput();
    in.dtype = LDS_EL_INT32; in.w = 256; in.ldc = 256; in.c_aligned16 = true;
    in.p.has_plan = in.p.is_code = true; in.p.nw = 8; in.p.batch = 8; in.p.kc = 128; in.p.ntiles = 64; in.p.nrows = 29384; in.p.ncols = 40000; in.p.col_splits = 4; in.p.rows = 29184;
    in.p.slots = 5008; in.p.tail_tables = true; in.p.tail_nseg = 200;
    L = lds_plan_launch(in, t);
    CHECK(!L.refusal && L.xs.nslices == 4 && L.xcd_sx == 4 && L.xcd_group == 8 && L.grid == 256);
    CHECK(L.to_scratch && L.ldp == 256 && L.part_es == 4 && L.split_bytes == 119537664 && L.split_bytes == 4ull * 29184 * 256 * 4);
    CHECK(L.park_bytes == 200ull * 4 * 64 * 8 && L.scratch_bytes == L.split_bytes + L.park_bytes);
    CHECK(L.reduce == LDS_RED_V4 && L.reduce_total == 29184ull * 64 && L.tail && L.ntail == 200 && L.accumulate == 0 && L.ldc_bytes == 1024);
    in.c_aligned16 = false;
    CHECK(lds_plan_launch(in, t).reduce == LDS_RED_PLAIN && lds_plan_launch(in, t).reduce_total == 29184ull * 256);
    // INT8, h = 256: widened to 16 bits in the staged copy -- 2 slices of 128 elements, kind 3
    LdsStaged s = lds_staged(1, true, 256, 30000, 128, 0);
    CHECK(s.nslices == 2 && s.eps == 128 && s.row_bytes == 256 && s.kind == 3 && s.rows_pad == 30080 && s.bytes == 30080ull * 256 * 2);
    // DBL64, h = 64: one slice of 512-byte rows, one slice per XCD
    s = lds_staged(8, false, 64, 4096, 64, 0);
    CHECK(s.nslices == 1 && s.eps == 64 && s.row_bytes == 512 && s.kind == 1 && s.rows_pad == 4096 && s.slice_stride == 4096ull * 512);
    in = LdsLaunchInput();
    in.dtype = LDS_EL_DBL64; in.w = 64; in.ldc = 64;
    in.p.has_plan = in.p.is_code = true; in.p.nw = 8; in.p.kc = 64; in.p.row_bytes = 512; in.p.ntiles = 9; in.p.nrows = 8192; in.p.ncols = 4096; in.p.slots = 9 * 64;
    L = lds_plan_launch(in, t);
    CHECK(!L.refusal && L.xcd_sx == 1 && L.xcd_group == 8 && L.touch_share == 0 && L.grid == 8 * 2 && L.w_lanes == 64 && L.kernel.shell == LDS_SH_CODE8 && L.kernel.el == LDS_EL_DBL64);
    // ... whose 64 features at a stride of 64 from a 256-byte boundary ARE a staged row of 512 bytes: X in place; not at another stride, boundary, or lds_direct_x = 0
    in.ldx = 64; in.x_aligned256 = true;
    CHECK(lds_plan_launch(in, t).x_in_place);
    in.ldx = 72;
    CHECK(!lds_plan_launch(in, t).x_in_place);
    in.ldx = 64; in.x_aligned256 = false;
    CHECK(!lds_plan_launch(in, t).x_in_place);
    in.x_aligned256 = true; in.p.col_order = true;
    CHECK(!lds_plan_launch(in, t).x_in_place);
    in.p.col_order = false;
    LdsLaunchKnobs copy_always;
    copy_always.lds_direct_x = 0;
    CHECK(!lds_plan_launch(in, copy_always).x_in_place);
    // a half-split plan, h = 32: one slice whose H rows hold two columns side by side, kind 5
    s = lds_staged(4, false, 32, 20000, 128, 10112);
    CHECK(s.nslices == 1 && s.rows_pad == 10112 && s.kind == 5 && s.bytes == 10112ull * 256);
    // no chunk size named: whole 320-column chunks of the token kernels, 64-row aligned
    CHECK(lds_rows_pad(1000, 0) == 1280 && lds_rows_pad(1, 128) == 128 && lds_rows_pad(0, 128) == 0 && lds_rows_pad(40000, 128) == 40064);
    return 0;
}

static int sweep(Tally &n) {
    const struct { int dtype; size_t es; } types[] = {{LDS_EL_INT8, 1}, {LDS_EL_INT16, 2}, {LDS_EL_INT32, 4}, {LDS_EL_INT64, 8}, {LDS_EL_FLT32, 4}, {LDS_EL_DBL64, 8}};
    const int64_t rows[] = {1, 1825, 2500, 29384, 232965};
    const int64_t cols[] = {1, 511, 40000, 232965, 16777215};
    const int64_t hints[] = {0, 4, 16, 32, 64, 100, 256, 1000};
    // form tunables: {which, value} -- the geometries the launch must serve (token forms, 16-wave code, rings, forced column ranges, no half-split, no tail)
    const int64_t form_sets[][2] = {{-1, 0}, {0, 1}, {1, 0}, {2, 0}, {4, 8}, {5, 16}, {6, 2}, {10, 3}, {10, 16}, {11, 2}, {12, 0}, {14, 0}};
    // launch tunables: {lds_mode, lds_xcd_slices, lds_touch_share, lds_ablate}
    const int64_t launch_sets[][4] = {{0, 0, 1, 0}, {1, 0, 1, 0}, {0, 1, 1, 0}, {0, 2, 0, 0}, {0, 4, 1, 0}, {0, 3, 1, 0}, {0, 0, 1, 6}};
    for (const auto &fs : form_sets) {
        LdsFormKnobs ft;
        switch (fs[0]) {
            case 0: ft.lds_mode = fs[1]; break;
            case 1: ft.lds_code = 0; break;
            case 2: ft.lds_code = 0; ft.lds_long_slots = 0; break;
            case 4: ft.lds_waves = fs[1]; ft.lds_mode = 1; break;
            case 5: ft.lds_code_waves = fs[1]; break;
            case 6: ft.lds_code_nbuf = fs[1]; break;
            case 10: ft.lds_col_split = fs[1]; break;
            case 11: ft.lds_col_split_f32 = fs[1]; break;
            case 12: ft.lds_row_tail = 0; break;
            case 14: ft.lds_half_split = 0; break;
            default: break;
        }
        for (const auto &ty : types)
            for (int64_t nr : rows)
                for (int64_t nc : cols)
                    for (int64_t hh : hints)
                        for (int flags = 0; flags < 4; flags++) {
                            LdsFormInput fi;
                            fi.k = kernel_consts();
                            fi.dtype = ty.dtype; fi.val_es = ty.es; fi.nrows = nr; fi.ncols = nc; fi.h_hint = hh; fi.cu_count = 256;
                            fi.nnz = nr * 40;
                            fi.valued = flags & 1;
                            fi.lds_forced = fi.lds_contig_tiles = (flags & 2) != 0;
                            const LdsForm f = lds_choose_form(fi, ft);
                            if (!f.plan) continue;
                            for (int geo = 0; geo < (f.long_candidate ? 2 : 1); geo++)
                                for (int every = 0; every < 2; every++) {
                                    LdsLaunchInput in;
                                    in.dtype = ty.dtype;
                                    in.p = plan_of(fi, f, geo ? f.long_geo : f.geo, every != 0);
                                    in.l16_batch = fi.k.l16_batch;
                                    n.plans++;
                                    const uint32_t eps = lds_staged(ty.es, ty.es == 1, 1, 1, 0, 0).eps;
                                    const uint32_t widths[] = {1, 2, 31, 32, 33, eps - 1, eps, eps + 1, 3 * eps, 4 * eps, 4 * eps + 2, (uint32_t)std::max<int64_t>(hh, 1)};
                                    for (const auto &ls : launch_sets) {
                                        LdsLaunchKnobs t;
                                        t.lds_mode = ls[0]; t.lds_xcd_slices = ls[1]; t.lds_touch_share = ls[2]; t.lds_ablate = ls[3];
                                        for (uint32_t w : widths)
                                            for (int bits = 0; bits < 16; bits++) {
                                                in.w = w;
                                                in.ldc = w + ((bits & 8) ? 0 : 3);
                                                in.accumulate = bits & 1; in.amax = bits & 2; in.prestaged = bits & 4; in.c_aligned16 = bits & 8;
                                                const uintptr_t c_addr = (bits & 8) ? 0x7f0000001000ull : 0x7f0000001004ull;
                                                const LdsLaunch L = lds_plan_launch(in, t);
                                                n.launches++;
                                                if (!L.refusal)
                                                    if (int rc = launch_invariants(in, L)) return rc;
                                                const bool takes = lds_takes(in.dtype, in.p, w, in.ldc, c_addr, in.accumulate, false, t);
                                                // the plain product (launch_block): what lds_takes accepts, lds_plan_launch launches.  The one combination it does not:
                                                // lds_ablate set on a library without the timing-experiment kernels, FLT32, token form -- the refusal that tells the user so
                                                if (takes && !in.amax && !in.prestaged) {
                                                    n.taken++;
                                                    const bool ablate_case = t.lds_ablate && !in.p.is_code && in.dtype == LDS_EL_FLT32;
                                                    if (ablate_case) n.ablate_refusals += L.refusal != nullptr;
                                                    if (L.refusal && !(ablate_case && !strcmp(L.refusal, "lds_ablate needs the ablation build (make -C pygim_amd/csrc ablate)"))) {
                                                        fprintf(stderr, "lds_takes accepts, lds_plan_launch refuses: %s\n", L.refusal);
                                                        print_case(Case{in, t, c_addr, false});
                                                        return 1;
                                                    }
                                                }
                                                // the dequantising product of the group's width (quant_run_t / dequant_run_t behind lds_fusable_part): its own conditions
                                                // (unit weights, no half-split, the tail for 4-byte types) and the restated rest
                                                const bool own = !fi.valued && !in.p.half && (!in.p.rows || ty.es == 4) && !in.accumulate && w == (uint32_t)std::max<int64_t>(hh, 1) && in.ldc == (int64_t)w;
                                                if (own && in.amax) {
                                                    const bool fus = fusable_rest(in.dtype, in.p, w, t);
                                                    if (fus) {
                                                        n.fused++;
                                                        if (L.refusal && !(t.lds_ablate && !in.p.is_code && !strncmp(L.refusal, "lds_ablate ", 11))) {   // (either of lds_ablate's own two texts)
                                                            fprintf(stderr, "lds_fusable_part accepts, lds_plan_launch refuses: %s\n", L.refusal);
                                                            print_case(Case{in, t, c_addr, false});
                                                            return 1;
                                                        }
                                                    }
                                                    if (ty.es != 8 && !in.prestaged) {
                                                        const bool tk = lds_takes(in.dtype, in.p, w, in.ldc, c_addr, false, false, t);
                                                        n.takes_not_fusable += tk && !fus;
                                                        n.fusable_not_takes += fus && !tk;
                                                    }
                                                }
                                            }
                                    }
                                }
                        }
    }
    return 0;
}

static int self_check() {
    if (int rc = quoted_shapes()) return rc;
    Tally n;
    if (int rc = sweep(n)) return rc;
    printf("lds_launch: the quoted shapes hold; %ld plans of the chooser, %ld launches planned, all within the invariants; %ld accepted by lds_takes and %ld by "
           "lds_fusable_part, none refused (but %ld by lds_ablate on a build without its kernels); the two gates part on %ld + %ld rows\n",
           n.plans, n.launches, n.taken, n.fused, n.ablate_refusals, n.takes_not_fusable, n.fusable_not_takes);
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "-")) return from_stdin();
    return self_check();
}
