// Test infrastructure: the plan of the L2 sweep (pygim_amd/csrc/sweep_plan.hpp) and creation's argument checks (group_args.hpp) asked from a
// command line, without a device.
//   g++ -std=c++17 -O1 -Wall tests/native/sweep_plan_main.cpp -o sweep_plan
//   sweep_plan -      one case per line of standard input, "name=value ...", lists with commas.
//                     A sweep plan: nrows ncols es h_hint is_extra sim_kind, sim_order (kind 2: the rows in similarity order), the ten knobs by their
//                     names, rowptr and col (the CSR).  What the runtime asks the device is answered here the way its kernels answer: whether every
//                     row's columns are in order, and the panel pointers by a binary search per (row, panel).
//                     kind=args: format es n_parts h_size, nrows ncols nnz n_dense (one per part), dense (all parts' widths), null_idx / null_col (one
//                     flag per part), null_table null_out -- check_group_args.  kind=flags: format f0 f1 -- group_validation_error.
//                     One line of "name=value ..." per case on standard output.
//   sweep_plan        the self-check: random small matrices and knob settings with the invariants of every plan checked -- the run to make under
//                     -fsanitize=address,undefined -fno-sanitize-recover=all
#include "../../pygim_amd/csrc/group_args.hpp"
#include "../../pygim_amd/csrc/sweep_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <map>
#include <sstream>
#include <string>

using namespace pygim;

struct Case {
    int64_t nrows = 0, ncols = 0, h_hint = 0;
    size_t es = 4;
    bool is_extra = false;
    int sim_kind = 0;
    std::vector<uint32_t> sim_order, rowptr{0}, col;
    SweepKnobs k;
};

struct Planned {
    SweepPanels want;
    bool unsorted = false;
    uint32_t npan = 0, panel_cols = 0, base_thresh = 0;
    std::vector<uint32_t> pp, base_tasks, base_desc, heavy_tasks, heavy_desc, rank;
    std::vector<char> heavy;
    bool want_sim = false, col16 = false;
    SweepItems it;
};

// build_plans' steps (rt_plans.inc) with the device's answers computed on the host
static Planned plan_case(const Case &c) {
    Planned p;
    const size_t nr = (size_t)c.nrows;
    const int64_t nnz = (int64_t)c.col.size();
    p.base_thresh = long_row_base_threshold(c.k);
    plan_long_rows(c.rowptr.data(), c.nrows, p.base_thresh, long_row_segment(p.base_thresh, c.k), nullptr, p.base_tasks, p.base_desc);
    p.want = sweep_panel_count(c.nrows, c.ncols, nnz, c.es, c.h_hint, c.k);
    if (!p.want.plan) return p;
    for (size_t r = 0; r < nr; r++)   // k_check_sorted_cols
        for (uint32_t e = c.rowptr[r] + 1; e < c.rowptr[r + 1]; e++) p.unsorted = p.unsorted || c.col[e] < c.col[e - 1];
    p.npan = sweep_panels_given(p.want, p.unsorted);
    p.panel_cols = sweep_panel_cols(c.ncols, p.npan);
    if (p.npan == 1) {
        p.pp = one_panel_pointers(c.rowptr.data(), nr);
    } else {   // k_build_panel_ptr
        p.pp.resize((size_t)(p.npan + 1) * nr);
        for (uint32_t q = 0; q <= p.npan; q++)
            for (size_t r = 0; r < nr; r++)
                p.pp[(size_t)q * nr + r] = q == 0 ? c.rowptr[r] : q == p.npan ? c.rowptr[r + 1] :
                    (uint32_t)(std::lower_bound(c.col.begin() + c.rowptr[r], c.col.begin() + c.rowptr[r + 1], (uint64_t)q * p.panel_cols,
                                                [](uint32_t a, uint64_t b) { return (uint64_t)a < b; }) - c.col.begin());
    }
    p.heavy = sweep_heavy_rows(p.pp.data(), nr, p.npan, p.base_thresh);
    plan_long_rows(c.rowptr.data(), c.nrows, p.base_thresh, long_row_segment(p.base_thresh, c.k), &p.heavy, p.heavy_tasks, p.heavy_desc);
    p.want_sim = sweep_wants_similarity(c.k, c.h_hint, c.is_extra, c.sim_kind);
    if (p.want_sim) p.rank = sweep_locality_rank(c.sim_kind, c.sim_order, nr);
    p.it = sweep_items(c.rowptr.data(), p.pp.data(), nr, p.npan, p.heavy, p.rank, c.is_extra, sweep_coop_cap(c.k));
    p.col16 = sweep_wants_col16(c.k, p.panel_cols, nnz, p.it.rows.size());
    return p;
}

template <typename V> static std::string joined(const V &v) {
    std::ostringstream s;
    for (size_t i = 0; i < v.size(); i++) s << (i ? "," : "") << (unsigned long long)v[i];
    return s.str();
}

static void print_plan(const Case &c) {
    const Planned p = plan_case(c);
    std::vector<uint32_t> heavy_rows;
    for (size_t r = 0; r < p.heavy.size(); r++)
        if (p.heavy[r]) heavy_rows.push_back((uint32_t)r);
    printf("plan=%d want_npan=%u ask_sorted=%d unsorted=%d n_panels=%u panel_cols=%u base_thresh=%u seg=%u base_tasks=\"%s\" heavy=\"%s\" segment_tasks=\"%s\" "
           "want_sim=%d locality=%d n_items=%zu rows=\"%s\" beg=\"%s\" lens=\"%s\" panel_off=\"%s\" panel_coop=\"%s\" panel_long128=\"%s\" panel_nnz=\"%s\" col16=%d "
           "col16_bytes=%zu\n",
           p.want.plan ? 1 : 0, p.want.npan, p.want.ask_sorted ? 1 : 0, p.unsorted ? 1 : 0, p.npan, p.panel_cols, p.base_thresh, long_row_segment(p.base_thresh, c.k),
           joined(p.base_tasks).c_str(), joined(heavy_rows).c_str(), joined(p.heavy_tasks).c_str(), p.want_sim ? 1 : 0, p.rank.empty() ? 0 : 1, p.it.rows.size(),
           joined(p.it.rows).c_str(), joined(p.it.beg).c_str(), joined(p.it.lens).c_str(), joined(p.it.panel_off).c_str(), joined(p.it.panel_coop).c_str(),
           joined(p.it.panel_long128).c_str(), joined(p.it.panel_nnz).c_str(), p.col16 ? 1 : 0, sweep_col16_bytes((int64_t)c.col.size()));
}

static std::vector<int64_t> list_of(const std::string &v) {
    std::vector<int64_t> out;
    std::istringstream ss(v);
    std::string item;
    while (std::getline(ss, item, ',')) out.push_back(strtoll(item.c_str(), nullptr, 0));
    return out;
}

static bool set_field(Case &c, const std::string &name, const std::string &val) {
    const int64_t v = strtoll(val.c_str(), nullptr, 0);
#define FD(f) if (name == #f) { c.f = (decltype(c.f))v; return true; }
    FD(nrows) FD(ncols) FD(h_hint) FD(es) FD(is_extra) FD(sim_kind)
#undef FD
#define KN(f) if (name == #f) { c.k.f = v; return true; }
    KN(panel_mode) KN(panel_bytes) KN(panel_min_seg) KN(panel_coop) KN(panel_locality) KN(panel_col16) KN(vec_lds) KN(vec_kernel) KN(long_row_threshold) KN(long_segment)
#undef KN
    std::vector<uint32_t> *dst = name == "rowptr" ? &c.rowptr : name == "col" ? &c.col : name == "sim_order" ? &c.sim_order : nullptr;
    if (!dst) return false;
    dst->clear();
    for (int64_t x : list_of(val)) dst->push_back((uint32_t)x);
    return true;
}

// kind=args / kind=flags
static int print_refusal(const std::map<std::string, std::string> &f) {
    auto num = [&](const char *n, int64_t dflt) { auto it = f.find(n); return it == f.end() ? dflt : strtoll(it->second.c_str(), nullptr, 0); };
    auto list = [&](const char *n) { auto it = f.find(n); return it == f.end() ? std::vector<int64_t>() : list_of(it->second); };
    ArgError e;
    if (f.at("kind") == "flags") {
        const int flags[4] = {(int)num("f0", 0), (int)num("f1", 0), 0, 0};
        e = group_validation_error((int)num("format", 0), flags);
    } else {
        const int n_parts = (int)num("n_parts", 1);
        const size_t n = (size_t)std::max(n_parts, 1);
        std::vector<int64_t> nrows = list("nrows"), ncols = list("ncols"), nnz = list("nnz"), n_dense = list("n_dense"), dense = list("dense"), null_idx = list("null_idx"),
                             null_col = list("null_col");
        for (auto *v : {&nrows, &ncols, &nnz, &n_dense})
            if (v->size() < n) { fprintf(stderr, "sweep_plan: args need one entry per part\n"); return 2; }
        null_idx.resize(n, 0);
        null_col.resize(n, 0);
        static const int32_t some = 0;
        std::vector<const int32_t *> idx0(n), colind(n);
        for (size_t i = 0; i < n; i++) {
            idx0[i] = null_idx[i] ? nullptr : &some;
            colind[i] = null_col[i] ? nullptr : &some;
        }
        const int64_t handle = 0;
        e = check_group_args((int)num("format", 0), (size_t)num("es", 4), n_parts, num("null_table", 0) ? nullptr : idx0.data(), colind.data(), nrows.data(), ncols.data(), nnz.data(),
                             n_dense.data(), dense.data(), num("h_size", 0), num("null_out", 0) ? nullptr : &handle);
    }
    printf("code=%d text=\"%s\"\n", e.code, e.text ? e.text : "");
    return 0;
}

static int from_stdin() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::map<std::string, std::string> fields;
        std::istringstream ss(line);
        std::string tok;
        while (ss >> tok) {
            const size_t eq = tok.find('=');
            if (eq == std::string::npos) { fprintf(stderr, "sweep_plan: what is '%s'?\n", tok.c_str()); return 2; }
            fields[tok.substr(0, eq)] = tok.substr(eq + 1);
        }
        if (fields.count("kind")) {
            if (int rc = print_refusal(fields)) return rc;
            continue;
        }
        Case c;
        for (auto &kv : fields)
            if (!set_field(c, kv.first, kv.second)) { fprintf(stderr, "sweep_plan: what is '%s'?\n", kv.first.c_str()); return 2; }
        if (c.rowptr.size() != (size_t)c.nrows + 1 || c.rowptr.back() != c.col.size()) { fprintf(stderr, "sweep_plan: rowptr does not describe col\n"); return 2; }
        print_plan(c);
    }
    return 0;
}

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "sweep_plan self-check, line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

struct Tally {
    long cases = 0, no_plan = 0, one_panel = 0, several = 0, unsorted_one = 0, heavy = 0, segment_tasks = 0, items = 0, coop = 0, locality = 0, empty_items = 0, extra = 0,
         col16 = 0, spmv = 0;
};

// what holds for every plan
static int invariants(const Case &c, const Planned &p, Tally &n) {
    const size_t nr = (size_t)c.nrows;
    const uint32_t *rp = c.rowptr.data();
    const SweepItems &it = p.it;
    const uint32_t cap = sweep_coop_cap(c.k);
    CHECK(p.npan >= 1 && (uint64_t)p.npan * p.panel_cols >= (uint64_t)c.ncols && (p.npan == 1 || !p.unsorted));
    CHECK(it.panel_off.size() == (size_t)p.npan + 1 && it.panel_off[0] == 0 && it.panel_off.back() == it.rows.size());   // monotone, ending at n_items
    CHECK(it.beg.size() == it.rows.size() && it.lens.size() == it.rows.size());
    CHECK(it.panel_coop.size() == p.npan && it.panel_long128.size() == 4 * (size_t)p.npan && it.panel_nnz.size() == p.npan);
    std::vector<uint32_t> next(rp, rp + nr), firsts(nr, 0), lasts(nr, 0), nitems(nr, 0);
    uint64_t covered = 0, heavy_nnz = 0;
    for (uint32_t q = 0; q < p.npan; q++) {
        CHECK(it.panel_off[q] <= it.panel_off[q + 1]);
        const size_t a = it.panel_off[q], b = it.panel_off[q + 1];
        uint32_t over[5] = {0, 0, 0, 0, 0};   // longer than the cap / 256 / 128 / 64 / 32
        uint64_t pn = 0;
        for (size_t k = a; k < b; k++) {
            const uint32_t r = it.rows[k], len = it.lens[k] & 0x3FFFFFFFu;
            CHECK(r < nr && !p.heavy[r]);
            // the entries of a row are covered once, panel after panel, each inside its panel's columns
            CHECK(it.beg[k] == next[r] && it.beg[k] + len <= rp[r + 1]);
            for (uint32_t e = it.beg[k]; e < it.beg[k] + len && p.npan > 1; e++) CHECK(c.col[e] / p.panel_cols == q);
            CHECK(len > 0 || (q == 0 && rp[r] == rp[r + 1] && !c.is_extra));
            next[r] += len;
            nitems[r]++;
            firsts[r] += (it.lens[k] & SWEEP_ITEM_FIRST) ? 1 : 0;
            lasts[r] += (it.lens[k] & SWEEP_ITEM_LAST) ? 1 : 0;
            CHECK(((it.lens[k] & SWEEP_ITEM_FIRST) != 0) == (it.beg[k] == rp[r]) && ((it.lens[k] & SWEEP_ITEM_LAST) != 0) == (it.beg[k] + len == rp[r + 1]));
            const uint32_t bounds[5] = {cap, 256, 128, 64, 32};
            for (int j = 0; j < 5; j++) over[j] += len > bounds[j] ? 1 : 0;
            pn += len;
            n.empty_items += len == 0;
            // the order: the cooperative prefix, then by length -- or by locality block, and by length inside a block
            if (k > a) {
                const uint32_t prev = it.lens[k - 1] & 0x3FFFFFFFu;
                if (p.rank.empty() || len > cap || prev > cap) CHECK(prev >= len);
                else CHECK((p.rank[it.rows[k - 1]] >> 11) < (p.rank[r] >> 11) || ((p.rank[it.rows[k - 1]] >> 11) == (p.rank[r] >> 11) && prev >= len));
                if (prev == len && (p.rank.empty() || (p.rank[it.rows[k - 1]] >> 11) == (p.rank[r] >> 11))) CHECK(it.rows[k - 1] < r);   // stable
            }
        }
        CHECK(it.panel_coop[q] == over[0] && it.panel_nnz[q] == pn);
        for (int j = 0; j < 4; j++) CHECK(it.panel_long128[4 * q + j] == over[j + 1]);
        // true prefixes: the first `count` items are the ones above the bound (the four length classes: outside locality mode)
        for (size_t k = a; k < b; k++) {
            const uint32_t len = it.lens[k] & 0x3FFFFFFFu;
            CHECK((len > cap) == (k - a < over[0]));
            const uint32_t bounds[4] = {256, 128, 64, 32};
            for (int j = 0; j < 4 && p.rank.empty(); j++) CHECK((len > bounds[j]) == (k - a < over[j + 1]));
        }
        covered += pn;
        n.coop += over[0];
    }
    for (size_t r = 0; r < nr; r++) {
        if (p.heavy[r]) {
            CHECK(nitems[r] == 0);
            heavy_nnz += rp[r + 1] - rp[r];
            n.heavy++;
            continue;
        }
        CHECK(next[r] == rp[r + 1]);
        if (rp[r] == rp[r + 1]) CHECK(nitems[r] == (c.is_extra ? 0u : 1u));
        if (nitems[r]) CHECK(firsts[r] == 1 && lasts[r] == 1);
    }
    CHECK(covered + heavy_nnz == c.col.size());
    // the heavy rows' segments cover their entries once, in order
    uint64_t seg_nnz = 0;
    for (size_t t = 0; t < p.heavy_tasks.size(); t += 3) {
        CHECK(p.heavy[p.heavy_tasks[t]] && p.heavy_tasks[t + 1] < p.heavy_tasks[t + 2] && p.heavy_tasks[t + 2] - p.heavy_tasks[t + 1] <= long_row_segment(p.base_thresh, c.k));
        CHECK(p.heavy_tasks[t + 1] == (t && p.heavy_tasks[t - 3] == p.heavy_tasks[t] ? p.heavy_tasks[t - 1] : rp[p.heavy_tasks[t]]));
        seg_nnz += p.heavy_tasks[t + 2] - p.heavy_tasks[t + 1];
    }
    CHECK(seg_nnz == heavy_nnz);
    n.segment_tasks += (long)(p.heavy_tasks.size() / 3);
    n.items += (long)it.rows.size();
    n.locality += !p.rank.empty();
    n.col16 += p.col16;
    CHECK(!p.col16 || (p.panel_cols <= 65536 && c.k.panel_col16 && !it.rows.empty()));
    return 0;
}

static uint64_t rnd(uint64_t &s) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return s >> 33;
}

static int sweep(Tally &n) {
    uint64_t seed = 2468;
    for (int rep = 0; rep < 1500; rep++) {
        Case c;
        c.nrows = (int64_t)(rnd(seed) % 8 == 0 ? 2049 + rnd(seed) % 300 : rnd(seed) % 120);
        c.ncols = (int64_t)(1 + rnd(seed) % 700);
        c.es = (size_t)1 << (rnd(seed) % 4);
        c.h_hint = (int64_t)(rnd(seed) % 4 == 0 ? 1 + rnd(seed) % 5 : 64);
        c.is_extra = rnd(seed) % 4 == 0;
        c.k.panel_mode = (int64_t)(rnd(seed) % 8 == 0 ? 2 : rnd(seed) % 2);
        c.k.panel_bytes = (int64_t)(128 * (1 + rnd(seed) % 400));
        c.k.panel_min_seg = (int64_t)(rnd(seed) % 6);
        c.k.panel_coop = (int64_t)(rnd(seed) % 3 == 0 ? 1 << 20 : rnd(seed) % 200);
        c.k.panel_locality = (int64_t)(rnd(seed) % 3);
        c.k.panel_col16 = (int64_t)(rnd(seed) % 4 != 0);
        c.k.vec_lds = (int64_t)(rnd(seed) % 4 != 0);
        c.k.long_row_threshold = (int64_t)(rnd(seed) % 2 ? 4096 : rnd(seed) % 100);   // (clamped to 64: heavy from 1025 entries in a panel)
        c.k.long_segment = (int64_t)(rnd(seed) % 300);
        // rows: mostly short, some empty, a few of hundreds of entries (repeated columns: a multigraph's), now and then one stored out of order
        const bool shuffle = rnd(seed) % 6 == 0;
        for (int64_t r = 0; r < c.nrows; r++) {
            const uint64_t kind = rnd(seed) % 40;
            const size_t deg = kind < 6 ? 0 : kind == 6 ? 900 + rnd(seed) % 1500 : kind < 10 ? 30 + rnd(seed) % 300 : 1 + rnd(seed) % 12;
            const size_t at = c.col.size();
            for (size_t e = 0; e < deg; e++) c.col.push_back((uint32_t)(rnd(seed) % (uint64_t)c.ncols));
            std::sort(c.col.begin() + at, c.col.end());
            if (shuffle && deg > 1 && rnd(seed) % 8 == 0) std::swap(c.col[at], c.col[at + deg - 1]);
            c.rowptr.push_back((uint32_t)c.col.size());
        }
        c.sim_kind = (int)(rnd(seed) % 3);
        if (c.sim_kind == 2) {   // a random order of the rows
            for (int64_t r = 0; r < c.nrows; r++) c.sim_order.push_back((uint32_t)r);
            for (size_t i = c.sim_order.size(); i > 1; i--) std::swap(c.sim_order[i - 1], c.sim_order[rnd(seed) % i]);
        }
        n.cases++;
        const Planned p = plan_case(c);
        n.spmv += c.h_hint <= 4;
        n.extra += c.is_extra;
        if (!p.want.plan) {
            CHECK(c.k.panel_mode == 2 || c.nrows == 0 || c.col.empty());
            n.no_plan++;
            continue;
        }
        (p.npan == 1 ? n.one_panel : n.several)++;
        n.unsorted_one += p.want.ask_sorted && p.unsorted;
        CHECK(p.want_sim || p.rank.empty());
        if (int rc = invariants(c, p, n)) return rc;
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "-")) return from_stdin();
    Tally n;
    if (int rc = sweep(n)) return rc;
    printf("sweep_plan: %ld parts planned, all within the invariants: %ld without a plan, %ld of one panel (%ld for unsorted columns), %ld of several; %ld items, %ld cooperative, "
           "%ld of empty rows; %ld heavy rows in %ld segment tasks; %ld plans in locality order, %ld with 16-bit ids, %ld adding parts, %ld SpMV-sized\n",
           n.cases, n.no_plan, n.one_panel, n.unsorted_one, n.several, n.items, n.coop, n.empty_items, n.heavy, n.segment_tasks, n.locality, n.col16, n.extra, n.spmv);
    return n.no_plan && n.one_panel && n.unsorted_one && n.several && n.coop && n.empty_items && n.heavy && n.locality && n.col16 ? 0 : 1;
}
