// Test infrastructure: the plan of one group-product call (pygim_amd/csrc/run_plan.hpp) asked from a command line, without a device.
//   g++ -std=c++17 -O1 -Wall tests/native/run_plan_main.cpp -o run_plan
//   run_plan -        one case per line of standard input, "name=value ...": es is_float h total_rows per_part, the knobs host_windows host_direct
//                     fuse_windows merge_parts, the facts out_pinned out_alias copies_slow has_merged stage_out; lists with commas: ncols (one per
//                     sparse part), dense (the dense split, every part's), ld and addr (one per window; default: stride = width, windows far apart);
//                     once=W:0,W:1,... with once_default: the writes_once table by width.  One line of "name=value ..." per case on standard output:
//                     the geometry or its refusal, the host pipeline's plan, the product plan (of the windows at addr, taken as device addresses)
//   run_plan          the self-check: a sweep over element sizes, widths, splits, strides, both conventions, the four tunables and random
//                     writes_once tables with the invariants of every plan checked -- the run to make under
//                     -fsanitize=address,undefined -fno-sanitize-recover=all
#include "../../pygim_amd/csrc/run_plan.hpp"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <map>
#include <sstream>
#include <string>

using namespace pygim;

struct Case {
    RunShape s;
    RunKnobs t;
    HostFacts facts;
    std::vector<int64_t> ncols{0}, dense{0}, ld;
    std::vector<uintptr_t> addr;
    std::map<int64_t, bool> once;
    bool once_default = true;
    std::vector<RunPart> parts;

    size_t finish() {   // the derived fields; the number of windows
        parts.clear();
        s.total_cols = 0;
        for (int64_t c : ncols) {
            parts.push_back({c, dense.data(), dense.size()});
            s.total_cols += c;
        }
        s.parts = parts.data();
        s.nparts = parts.size();
        return run_window_count(s);
    }
    bool writes_once(int64_t w) const {
        auto it = once.find(w);
        return it == once.end() ? once_default : it->second;
    }
};

static std::vector<int64_t> list_of(const std::string &v) {
    std::vector<int64_t> out;
    std::istringstream ss(v);
    std::string item;
    while (std::getline(ss, item, ',')) out.push_back(strtoll(item.c_str(), nullptr, 0));
    return out;
}

static bool set_field(Case &c, const std::string &name, const std::string &val) {
    const int64_t v = strtoll(val.c_str(), nullptr, 0);
#define SH(f) if (name == #f) { c.s.f = (decltype(c.s.f))v; return true; }
    SH(es) SH(is_float) SH(h) SH(total_rows) SH(per_part)
#undef SH
#define KN(f) if (name == #f) { c.t.f = v; return true; }
    KN(host_windows) KN(host_direct) KN(fuse_windows) KN(merge_parts)
#undef KN
#define FA(x) if (name == #x) { c.facts.x = (decltype(c.facts.x))v; return true; }
    FA(out_pinned) FA(out_alias) FA(copies_slow) FA(has_merged) FA(stage_out)
#undef FA
    if (name == "ncols") { c.ncols = list_of(val); return true; }
    if (name == "dense") { c.dense = list_of(val); return true; }
    if (name == "ld") { c.ld = list_of(val); return true; }
    if (name == "addr") { c.addr.clear(); for (int64_t a : list_of(val)) c.addr.push_back((uintptr_t)a); return true; }
    if (name == "once_default") { c.once_default = v != 0; return true; }
    if (name == "once") {
        std::istringstream ss(val);
        std::string item;
        while (std::getline(ss, item, ',')) {
            const size_t colon = item.find(':');
            if (colon == std::string::npos) return false;
            c.once[strtoll(item.c_str(), nullptr, 0)] = strtoll(item.c_str() + colon + 1, nullptr, 0) != 0;
        }
        return true;
    }
    return false;
}

struct Planned {
    const char *refusal = nullptr;
    std::vector<RunWindow> win;
    std::vector<uintptr_t> addr;
    std::vector<size_t> off;
    size_t stage_in_bytes = 0;
    HostFactsNeeded need{false, false};
    HostPlan host;
    ProductPlan prod;
};

static Planned plan_case(Case &c) {
    Planned p;
    const size_t nwin = c.finish();
    if (!c.ld.empty() && c.ld.size() != nwin) { p.refusal = "harness: ld needs one entry per window"; return p; }
    p.refusal = run_windows(c.s, c.ld.empty() ? nullptr : c.ld.data(), p.win);
    if (p.refusal) return p;
    p.addr = c.addr;
    if (p.addr.empty())
        for (size_t k = 0; k < nwin; k++) p.addr.push_back((uintptr_t)0x10000000u * (k + 1));
    if (p.addr.size() != nwin) { p.refusal = "harness: addr needs one entry per window"; return p; }
    p.stage_in_bytes = host_stage_layout(p.win.data(), nwin, c.s.es, p.off);
    p.need = host_facts_needed(c.s, c.t, c.facts.has_merged, c.facts.copies_slow);
    p.host = plan_host_pipeline(c.s, p.win.data(), p.addr.data(), p.off.data(), c.t, c.facts, [&](int64_t w, uintptr_t) { return c.writes_once(w); });
    plan_products(c.s, p.win.data(), p.addr.data(), c.t, c.facts.has_merged, p.prod);
    return p;
}

static void print_case(Case &c) {
    const Planned p = plan_case(c);
    if (p.refusal) {
        printf("refusal=\"%s\"\n", p.refusal);
        return;
    }
    std::ostringstream geo, hw, pr, cp;
    for (const RunWindow &w : p.win) geo << (geo.tellp() ? "|" : "") << w.rows << ":" << w.ld << ":" << w.width;
    for (const HostWindow &q : p.host.windows) {   // acol:w:pitch:dev_off:xcat_ld then /acol:w:pitch:dev_off per piece
        hw << (hw.tellp() ? "|" : "") << q.acol << ":" << q.w << ":" << q.pitch_el << ":" << q.dev_off << ":" << q.xcat_ld;
        for (const HostPiece &pc : q.pieces) hw << "/" << pc.acol << ":" << pc.w << ":" << pc.pitch_el << ":" << pc.dev_off;
    }
    for (const RunProduct &q : p.prod.products)   // part:in_place:base:ldx:ccol:width:accumulate:copy0:copy1
        pr << (pr.tellp() ? "|" : "") << q.part << ":" << q.x.in_place << ":" << q.x.base << ":" << q.x.ldx << ":" << q.ccol << ":" << q.width << ":" << q.accumulate << ":"
           << q.copy0 << ":" << q.copy1;
    for (const RunCopy &q : p.prod.copies)   // dst_off:window:src_off:width:rows
        cp << (cp.tellp() ? "|" : "") << q.dst_off << ":" << q.win << ":" << q.src_off << ":" << q.width << ":" << q.rows;
    printf("refusal=\"\" nwin=%zu geometry=\"%s\" stage_in_bytes=%zu need_pinned=%d need_alias=%d windows=%zu direct=%d host_xcat_bytes=%zu host=\"%s\" nproducts=%zu "
           "xcat_bytes=%zu products=\"%s\" copies=\"%s\"\n",
           p.win.size(), geo.str().c_str(), p.stage_in_bytes, p.need.out_pinned ? 1 : 0, p.need.out_alias ? 1 : 0, p.host.windows.size(), p.host.direct ? 1 : 0,
           p.host.xcat_bytes, hw.str().c_str(), p.prod.products.size(), p.prod.xcat_bytes, pr.str().c_str(), cp.str().c_str());
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
            if (eq == std::string::npos || !set_field(c, tok.substr(0, eq), tok.substr(eq + 1))) {
                fprintf(stderr, "run_plan: what is '%s'?\n", tok.c_str());
                return 2;
            }
        }
        print_case(c);
    }
    return 0;
}

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "run_plan self-check, line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

struct Tally {
    long cases = 0, refused = 0, pipelined = 0, direct = 0, gathered = 0, serial = 0, products = 0, in_place = 0, laid = 0, copies = 0;
};

// what holds for every host plan
static int host_invariants(const Case &c, const Planned &p, Tally &n) {
    const HostPlan &hp = p.host;
    const size_t es = c.s.es;
    const int64_t rows = c.s.total_cols;
    if (!host_pipeline_eligible(c.s, c.t, c.facts.has_merged)) CHECK(hp.windows.empty() && hp.xcat_bytes == 0 && !p.need.out_pinned && !p.need.out_alias);
    if (hp.windows.empty()) {
        CHECK(!hp.direct);
        n.serial++;
        return 0;
    }
    n.pipelined++;
    n.direct += hp.direct;
    CHECK(hp.windows.size() >= 2 && hp.windows.size() <= 16);
    int64_t a = 0;
    for (const HostWindow &q : hp.windows) {
        CHECK(q.acol == a && q.w >= 0);   // in order, disjoint, no gap
        a += q.w;
        if (q.pieces.empty()) {
            CHECK(q.pitch_el >= q.w);
            if (rows > 0 && q.w > 0) CHECK(q.dev_off + ((size_t)(rows - 1) * q.pitch_el + q.w) * es <= p.stage_in_bytes);
        } else {
            n.gathered++;
            CHECK(((size_t)q.xcat_ld * es) % 16 == 0 && q.xcat_ld >= c.s.h);
            int64_t pa = q.acol;
            for (const HostPiece &pc : q.pieces) {
                CHECK(pc.acol == pa && pc.pitch_el >= pc.w);   // the pieces tile the window's columns
                pa += pc.w;
                CHECK(pc.dev_off + (size_t)rows * pc.pitch_el * es <= p.stage_in_bytes);
                if (rows > 0 && pc.w > 0) CHECK(((size_t)(rows - 1) * q.xcat_ld + pc.acol + pc.w) * es <= hp.xcat_bytes);
            }
            CHECK(pa == q.acol + q.w);
        }
        if (hp.direct) CHECK(c.facts.out_alias && c.facts.out_alias % 256 == 0 && ((size_t)q.acol * es) % 16 == 0 && c.writes_once(q.w) && c.writes_once(c.s.h));
        if (c.t.host_windows == 0 && c.s.is_float) CHECK(c.writes_once(q.w));
    }
    CHECK(a == c.s.h);   // ... and cover [0, h)
    if (hp.direct) CHECK(c.t.host_direct == 2 || (c.t.host_direct == 1 && c.facts.copies_slow));
    return 0;
}

// what holds for every product plan
static int product_invariants(const Case &c, const Planned &p, Tally &n) {
    const size_t es = c.s.es;
    const bool merged = c.facts.has_merged && c.t.merge_parts && c.s.nparts > 1;
    int64_t wsum = 0;
    for (int64_t w : c.dense) wsum += w;
    std::vector<std::vector<int>> written(c.s.nparts, std::vector<int>((size_t)wsum, 0));
    size_t next_copy = 0;
    int last_part = merged ? -1 : 0;
    for (const RunProduct &q : p.prod.products) {
        n.products++;
        CHECK(merged ? q.part == -1 && p.prod.products.size() == 1 && q.width == c.s.h && q.ccol == 0 : q.part >= last_part && q.part < (int)c.s.nparts);   // part by part
        last_part = q.part;
        CHECK(q.accumulate == (q.part > 0));
        CHECK(q.copy0 == next_copy && q.copy1 >= q.copy0 && q.copy1 <= p.prod.copies.size());
        next_copy = q.copy1;
        if (!merged) {
            CHECK(q.ccol >= 0 && q.ccol + q.width <= wsum);
            for (int64_t j = q.ccol; j < q.ccol + q.width; j++) written[(size_t)q.part][(size_t)j]++;
        }
        if (q.x.in_place) {
            n.in_place++;
            CHECK(q.copy0 == q.copy1 && q.x.xcat_bytes == 0 && q.x.ldx >= 0);
        } else {
            n.laid++;
            CHECK(((size_t)q.x.ldx * es) % 16 == 0 && q.x.ldx >= q.width && q.x.xcat_bytes <= p.prod.xcat_bytes && p.prod.xcat_bytes >= 256);
            int64_t cols = 0;
            for (uint32_t k = q.copy0; k < q.copy1; k++) {
                const RunCopy &cp = p.prod.copies[k];
                n.copies++;
                CHECK(cp.win < p.win.size() && cp.width == p.win[cp.win].width);
                if (cp.rows > 0 && cp.width > 0) {
                    CHECK(cp.dst_off + ((size_t)(cp.rows - 1) * q.x.ldx + cp.width) * es <= p.prod.xcat_bytes);          // inside xcat
                    CHECK(cp.src_off + ((size_t)(cp.rows - 1) * p.win[cp.win].ld + cp.width) * es <= (size_t)p.win[cp.win].rows * p.win[cp.win].ld * es);   // inside its window
                }
                cols += cp.width;
            }
            CHECK(merged ? cols == wsum * (int64_t)c.s.nparts : cols == q.width);
        }
    }
    CHECK(next_copy == p.prod.copies.size());
    if (!merged)
        for (auto &part : written)
            for (int times : part) CHECK(times == 1);   // every column of C exactly once per part
    return 0;
}

static uint64_t rnd(uint64_t &s) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return s >> 33;
}

static int sweep(Tally &n) {
    uint64_t seed = 12345;
    const int64_t hs[] = {1, 2, 3, 7, 16, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129, 200, 255, 256, 257, 300, 320, 384};
    for (size_t es : {(size_t)1, (size_t)2, (size_t)4, (size_t)8})
        for (int64_t h : hs)
            for (int split = 0; split < 7; split++)
                for (int conv = 0; conv < 2; conv++)
                    for (int rep = 0; rep < 24; rep++) {
                        Case c;
                        c.s.es = es;
                        c.s.h = h;
                        c.s.is_float = es >= 4 && (rnd(seed) & 1);
                        c.s.per_part = conv != 0;
                        // the dense split: one window, equal parts, or random cuts (zero-width windows among them)
                        const int nd = split == 0 ? 1 : split < 4 ? std::min<int64_t>(h, split + 1) : 1 + (int)(rnd(seed) % 20);
                        c.dense.assign((size_t)nd, 0);
                        if (split < 4)
                            for (int j = 0; j < nd; j++) c.dense[(size_t)j] = h / nd + (j < h % nd ? 1 : 0);
                        else
                            for (int64_t j = 0; j < h; j++) c.dense[(size_t)(rnd(seed) % (uint64_t)nd)]++;
                        const int np = 1 + (int)(rnd(seed) % 3);
                        c.ncols.clear();
                        const bool large = rnd(seed) % 4 == 0;   // both operands above the automatic rule's 32 MB
                        for (int i = 0; i < np; i++) c.ncols.push_back(large ? (int64_t)(((size_t)40 << 20) / ((size_t)h * es) + 1 + rnd(seed) % 50) : (int64_t)(rnd(seed) % 400));
                        c.s.total_rows = large ? c.ncols[0] * np : (int64_t)(rnd(seed) % 500);
                        const size_t nwin = c.finish();
                        // strides: the width, padded, or (rarely) too small -- and windows that are views of one row-major matrix
                        const int stride = (int)(rnd(seed) % 4);
                        const bool views = !c.s.per_part && rnd(seed) % 3 == 0;
                        c.ld.clear();
                        c.addr.clear();
                        int64_t col = 0;
                        for (size_t k = 0; k < nwin; k++) {
                            const int64_t w = c.dense[k % c.dense.size()];
                            c.ld.push_back(views ? h + (stride == 1 ? 3 : 0) : stride == 0 ? w : stride == 1 ? w + 3 : stride == 2 ? (w + 7) / 8 * 8 : (c.s.per_part && rnd(seed) % 8 == 0 ? w - 1 : w));
                            c.addr.push_back(views ? (uintptr_t)0x40000000u + (size_t)col * es : (uintptr_t)0x10000000u * (k + 1));
                            col += w;
                        }
                        if (stride == 0 && rnd(seed) & 1) c.ld.clear();
                        c.t.host_windows = (int64_t)(rnd(seed) % 7);
                        c.t.host_direct = (int64_t)(rnd(seed) % 3);
                        c.t.fuse_windows = (int64_t)(rnd(seed) & 1);
                        c.t.merge_parts = (int64_t)(rnd(seed) & 1);
                        c.facts.out_pinned = rnd(seed) % 4 != 0;
                        c.facts.out_alias = c.facts.out_pinned ? (uintptr_t)0x7f0000000000ull + (rnd(seed) % 8 == 0 ? 64 : 0) : 0;
                        c.facts.copies_slow = rnd(seed) & 1;
                        c.facts.has_merged = np > 1 && (rnd(seed) % 4 != 0);
                        c.facts.stage_out = 0x20000000u;
                        c.once_default = rnd(seed) % 4 != 0;
                        for (int k = 0; k < 3; k++) c.once[(int64_t)(rnd(seed) % (uint64_t)(h + 1))] = rnd(seed) & 1;
                        if (rnd(seed) % 4 == 0) c.once[h] = true;
                        n.cases++;
                        const Planned p = plan_case(c);
                        if (p.refusal) {
                            CHECK(c.s.per_part && !strcmp(p.refusal, "window stride smaller than its width"));
                            n.refused++;
                            continue;
                        }
                        if (int rc = host_invariants(c, p, n)) return rc;
                        if (int rc = product_invariants(c, p, n)) return rc;
                    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "-")) return from_stdin();
    Tally n;
    if (int rc = sweep(n)) return rc;
    printf("run_plan: %ld calls planned (%ld refused for a stride below the width), all within the invariants: %ld pipelined (%ld direct, %ld gathered windows), %ld serial; "
           "%ld products, %ld in place, %ld laid side by side with %ld copies\n",
           n.cases, n.refused, n.pipelined, n.direct, n.gathered, n.serial, n.products, n.in_place, n.laid, n.copies);
    return n.pipelined && n.direct && n.gathered && n.serial && n.in_place && n.laid && n.refused ? 0 : 1;
}
