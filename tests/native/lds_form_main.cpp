// Test infrastructure: lds_choose_form (pygim_amd/csrc/lds_form.hpp) asked from a command line, without a device.
//   g++ -std=c++17 -O1 -Wall tests/native/lds_form_main.cpp -o lds_form
//   lds_form -          one case per line of standard input, "name=value ..." (names: the fields of LdsFormInput and LdsFormKnobs; anything
//                       not named keeps its default); one line of "name=value ..." per case on standard output
//   lds_form            the self-check: the two shapes whose forms the documents quote, then a sweep of shapes, widths, element types and
//                       tunables through the chooser with its invariants checked -- the run to make under
//                       -fsanitize=address,undefined -fno-sanitize-recover=all
#include "../../pygim_amd/csrc/lds_form.hpp"

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

static bool set_field(LdsFormInput &in, LdsFormKnobs &t, const std::string &name, int64_t v) {
#define IN(f) if (name == #f) { in.f = (decltype(in.f))v; return true; }
    IN(dtype) IN(val_es) IN(nrows) IN(ncols) IN(nnz) IN(valued) IN(is_extra) IN(lds_forced) IN(lds_contig_tiles) IN(h_hint) IN(cu_count) IN(allow_code)
#undef IN
#define KC(f) if (name == #f) { in.k.f = (uint32_t)v; return true; }
    KC(kc) KC(lds_bytes) KC(ka8) KC(batch8) KC(ka16) KC(batch16) KC(l16_ka) KC(l16_batch)
#undef KC
#define KN(f) if (name == #f) { t.f = v; return true; }
    KN(lds_mode) KN(lds_min_reuse_x100) KN(lds_min_width) KN(lds_min_width8) KN(lds_min_reuse_narrow_x100) KN(lds_waves) KN(lds_long_slots) KN(lds_code)
    KN(lds_col_split) KN(lds_col_split_f32) KN(lds_row_tail) KN(lds_half_split) KN(lds_split_order) KN(lds_fill_tiles)
    KN(lds_code_nbuf) KN(lds_code_waves) KN(lds_code_kc) KN(lds_code_boundary) KN(lds_code_exp)
    KN(lds_round_tiles) KN(lds_tile_order) KN(lds_codegen) KN(lds_fail)
#undef KN
    return false;
}

static void print_form(const LdsFormInput &in, const LdsForm &f) {
    const LdsGeometry &g = f.geo;
    printf("plan=%d waves=%u acc_per_wave=%u chunk_cols=%u buffers=%u col_splits=%u code=%d rows_lds=%u covered_rows=%u half_H=%u rows_per_tile=%u boundary=%u "
           "keep_tile_order=%u row_bytes=%u batch=%u es=%zu code_op=%u min_reuse_x100=%.6g similarity=%d similarity_forced=%d device_codegen=%d long_candidate=%d why=\"%s\"\n",
           f.plan ? 1 : 0, g.NW, g.KA, g.KC, g.NBUF, g.col_splits, f.want_code ? 1 : 0, f.rows_lds, f.plan && f.rows_lds < (uint32_t)in.nrows ? f.rows_lds : 0, f.half_H,
           g.rows_per_tile, g.boundary, g.keep_tile_order, g.row_bytes, g.BATCH, f.es, f.code_op, f.min_reuse_x100, f.want_similarity ? 1 : 0,
           f.similarity_forced ? 1 : 0, f.device_codegen ? 1 : 0, f.long_candidate ? 1 : 0, f.codegen_why);
}

static int from_stdin() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        LdsFormInput in;
        LdsFormKnobs t;
        in.k = kernel_consts();
        in.cu_count = 256;
        std::istringstream ss(line);
        std::string tok;
        while (ss >> tok) {
            const size_t eq = tok.find('=');
            if (eq == std::string::npos || !set_field(in, t, tok.substr(0, eq), strtoll(tok.c_str() + eq + 1, nullptr, 10))) {
                fprintf(stderr, "lds_form: what is '%s'?\n", tok.c_str());
                return 2;
            }
        }
        print_form(in, lds_choose_form(in, t));
    }
    return 0;
}

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "lds_form self-check, line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

// what holds for every form the chooser hands out, whatever it was asked
static int invariants(const LdsFormInput &in, const LdsFormKnobs &t, const LdsForm &f) {
    if (!f.plan) return 0;
    const LdsGeometry &g = f.geo;
    CHECK(g.NW == 8 || g.NW == 16);
    CHECK(g.KA >= 1 && g.KA * (g.row_bytes == 512 ? 2 : 1) <= 228);
    CHECK(g.row_bytes == 256 || g.row_bytes == 512);
    CHECK(g.KC >= 1 && g.NBUF >= 2 && (uint64_t)g.KC * g.row_bytes * g.NBUF <= in.k.lds_bytes && g.KC * g.NBUF <= 640);
    CHECK(g.col_splits >= 1 && g.col_splits <= 16);
    CHECK(f.rows_lds >= 1 && f.rows_lds <= (uint32_t)in.nrows);
    CHECK(g.rows_per_tile <= g.NW * g.KA);
    CHECK(f.rows_lds == (uint32_t)in.nrows || (g.col_splits > 1 && f.rows_lds % (g.NW * g.KA) == 0 && f.half_H == 0));   // a tail: whole tiles, no half-split
    CHECK((f.half_H != 0) == (g.half_split != 0));
    CHECK(!f.half_H || (f.half_H % g.KC == 0 && 2ull * f.half_H >= (uint64_t)in.ncols));
    CHECK(!f.want_code || (uint64_t)g.KC * g.row_bytes % (1024 * g.NW) == 0);                                    // whole 1 KiB pieces per wave
    CHECK(f.want_code || (!f.device_codegen && !f.want_similarity && !f.half_H && f.codegen_why[0] == 0));
    CHECK(!f.device_codegen || f.codegen_why[0] == 0);
    CHECK(!f.long_candidate || (!f.want_code && g.NW == 16 && f.long_geo.KA == in.k.l16_ka));
    CHECK(f.es == (in.val_es == 1 ? 2 : in.val_es));
    (void)t;
    return 0;
}

static int self_check() {
    LdsFormInput in;
    LdsFormKnobs t;
    in.k = kernel_consts();
    in.cu_count = 256;
    // a row share that all but fits one workgroup per compute unit: 16 full tiles x 4 slices x 4 ranges hold 29 184 of its 29 384 rows
    in.dtype = LDS_EL_INT32; in.val_es = 4; in.nrows = 16 * 1824 + 200; in.ncols = 40000; in.nnz = 1100000; in.h_hint = 256;
    LdsForm f = lds_choose_form(in, t);
    CHECK(f.plan && f.want_code && f.geo.col_splits == 4 && f.rows_lds == 29184);
    t.lds_row_tail = 0;
    f = lds_choose_form(in, t);
    CHECK(f.plan && f.geo.col_splits == 3 && f.rows_lds == 29384);
    // the Reddit-shaped FLT32 product at h = 256: 128 tiles x 4 slices = two whole rounds of 256 workgroups
    t = LdsFormKnobs();
    in.dtype = LDS_EL_FLT32; in.nrows = in.ncols = 232965; in.nnz = 114615892;
    f = lds_choose_form(in, t);
    CHECK(f.plan && f.want_code && f.geo.NW == 8 && f.geo.KA == 228 && f.geo.NBUF == 5 && f.geo.KC == 128 && f.geo.boundary == 1 && f.geo.col_splits == 1 &&
          f.geo.rows_per_tile == 1821 && f.rows_lds == 232965 && f.device_codegen && f.want_similarity && !f.similarity_forced);
    CHECK((232965 + 1820) / 1821 == 128);
    // the sweep: every combination goes through the chooser (under the sanitizers: no overflow, no division by zero) and keeps the invariants
    const struct { int dtype; size_t es; } types[] = {{LDS_EL_INT8, 1}, {LDS_EL_INT16, 2}, {LDS_EL_INT32, 4}, {LDS_EL_INT64, 8}, {LDS_EL_FLT32, 4}, {LDS_EL_DBL64, 8}, {-1, 3}};
    const int64_t rows[] = {0, 1, 15, 1823, 1824, 1825, 2500, 14560, 29384, 232965, 4000000000ll};
    const int64_t cols[] = {0, 1, 511, 512, 40000, 232965, 16777216, 4294967295ll};
    const int64_t widths[] = {0, 1, 4, 5, 16, 17, 32, 33, 64, 100, 128, 200, 256, 1000};
    const int64_t knob_sets[][2] = {{-1, 0}, {0, 1}, {0, 2}, {1, 0}, {2, 0}, {3, 0}, {4, 8}, {5, 16}, {6, 2}, {6, 3}, {6, 4}, {6, 10}, {7, 2}, {8, 1}, {8, 2}, {8, 4},
                                    {9, 0}, {9, 2}, {10, 1}, {10, 3}, {10, 16}, {11, 0}, {11, 2}, {12, 0}, {13, 0}, {14, 0}, {15, 1}, {16, 1}, {17, 0}, {18, 64}};
    long plans = 0, total = 0;
    for (const auto &ks : knob_sets) {
        t = LdsFormKnobs();
        switch (ks[0]) {
            case 0: t.lds_mode = ks[1]; break;
            case 1: t.lds_code = 0; break;
            case 2: t.lds_code = 0; t.lds_long_slots = 0; break;
            case 3: t.lds_code = 0; t.lds_round_tiles = 0; break;
            case 4: t.lds_waves = ks[1]; break;
            case 5: t.lds_code_waves = ks[1]; break;
            case 6: t.lds_code_nbuf = ks[1]; break;
            case 7: t.lds_code_boundary = ks[1]; break;
            case 8: t.lds_fail = ks[1]; break;
            case 9: t.lds_codegen = ks[1]; break;
            case 10: t.lds_col_split = ks[1]; break;
            case 11: t.lds_col_split_f32 = ks[1]; break;
            case 12: t.lds_row_tail = 0; break;
            case 13: t.lds_fill_tiles = 0; break;
            case 14: t.lds_half_split = 0; break;
            case 15: t.lds_tile_order = 1; break;
            case 16: t.lds_code_exp = 1; break;
            case 17: t.lds_split_order = 0; break;
            case 18: t.lds_code_kc = ks[1]; break;
            default: break;
        }
        for (const auto &ty : types)
            for (int64_t nr : rows)
                for (int64_t nc : cols)
                    for (int64_t h : widths)
                        for (int flags = 0; flags < 8; flags++)
                            for (int cus : {0, 256, 304}) {
                                in = LdsFormInput();
                                in.k = kernel_consts();
                                in.dtype = ty.dtype; in.val_es = ty.es; in.nrows = nr; in.ncols = nc; in.h_hint = h; in.cu_count = cus;
                                in.nnz = std::min<int64_t>((int64_t)1 << 31, nr * ((flags & 4) ? 40 : 1));
                                in.valued = flags & 1;
                                in.lds_forced = in.lds_contig_tiles = (flags & 2) != 0;
                                for (int allow = 0; allow < 2; allow++) {
                                    in.allow_code = allow != 0;
                                    f = lds_choose_form(in, t);
                                    if (int rc = invariants(in, t, f)) {
                                        print_form(in, f);
                                        return rc;
                                    }
                                    plans += f.plan;
                                    total++;
                                }
                            }
    }
    printf("lds_choose_form: the quoted shapes hold; %ld of %ld swept inputs get a plan, all within the invariants\n", plans, total);
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "-")) return from_stdin();
    return self_check();
}
