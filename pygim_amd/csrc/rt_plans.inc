// rt_plans.inc -- part of pygim_hip.hip (inside its anonymous namespace): the one-time plans of a part -- long rows, the sweep's panels and work items
// (decided in sweep_plan.hpp, built here), which rows are alike (find_similarity), the LDS-staged plan and its code stream (generated on the device, lds_codegen_dev.hpp; the host
// encoder as checker and rung below).  The reference's counterpart: prepare_pim_csr / partition walks, spmm_default/spmm_mul_csr.c:118-330.
template <typename T> void launch_check_ones(const void *v, uint32_t n, int *flag, hipStream_t st) {
    hipLaunchKernelGGL((k_check_ones<T>), dim3((n + 255) / 256), dim3(256), 0, st, (const T *)v, n, flag);
}

int build_lds_plan(Part &p, size_t es, int *d_flag_sorted, hipStream_t st, const std::vector<uint32_t> &h_rowptr, int64_t h_hint);
double now_ms();
static thread_local int t_plan_dtype = -1;   // element type of the group being created (the plan builders see the element SIZE only)

// Which rows are alike: once per part (square parts of a million entries and more).  sim_kind 1: a row's columns span a small part of
// the id range -- the ids carry the locality themselves; 2: label propagation found communities (more than one label, none holding half
// of the rows); 0: neither.
static void find_similarity(Part &p, hipStream_t st, bool force_lp) {
    if (p.sim_kind >= 0 && !(force_lp && p.sim_kind != 2)) return;
    p.sim_kind = 0;
    p.sim_order.clear();
    p.sim_why.clear();
    if (p.nrows != p.ncols || p.nrows == 0 || (!force_lp && p.nnz < (1 << 20))) { p.sim_why = "not a square part of a million entries and more"; return; }
    if (p.cols_sorted == 0) { p.sim_why = "rows not stored in column order"; return; }
    const double t0 = now_ms();
    const double span = force_lp ? 1.0 : lds_mean_row_span(p.rowptr, p.colind, (uint32_t)p.nrows, (uint32_t)p.ncols, st);
    if (span < 0.5) {
        p.sim_kind = 1;
        p.sim_why = "the stored ids are local already (mean row span " + std::to_string(span) + " of the id range)";
    } else {
        uint64_t agree = 0;
        std::string why = lds_similarity_order(p.rowptr, p.colind, (uint32_t)p.nrows, (int)std::min<int64_t>(std::max<int64_t>(g_tune.lds_lp_rounds, 0), 64), st, p.sim_order,
                                               &p.sim_labels, &p.sim_largest, &agree);
        p.sim_agree = p.nnz ? (double)agree / (double)p.nnz : 0.0;
        // communities: more than one label, none holding half of the rows, and the labels MEAN something -- at least 30 % of the stored
        // entries join two rows of one label (a planted partition: its inside fraction; labels of a graph without structure: ~0, and
        // ordering by them only costs the sweep its balance: products-shaped uniform 19.8 -> 22.6 ms)
        if (why.empty() && !force_lp && (p.sim_labels < 2 || (uint64_t)p.sim_largest * 2 > (uint64_t)p.nrows || p.sim_agree < 0.3))
            why = "the propagation found no communities (" + std::to_string(p.sim_labels) + " labels, " + std::to_string(p.sim_agree) + " of the entries inside one)";
        if (!why.empty()) {
            p.sim_order.clear();
            p.sim_why = why;
            (void)hipGetLastError();
        } else {
            p.sim_kind = 2;
        }
    }
    if (getenv("PYGIM_PLAN_TIMING"))
        fprintf(stderr, "[pygim plan] similarity: kind %d, %u labels, the largest holds %u of %lld rows%s%s  (%.1f ms)\n", p.sim_kind, p.sim_labels, p.sim_largest,
                (long long)p.nrows, p.sim_why.empty() ? "" : " -- ", p.sim_why.c_str(), now_ms() - t0);
}

// The tunables the sweep's plan reads (sweep_plan.hpp), copied in this one place.
static SweepKnobs sweep_knobs() {
    SweepKnobs k;
#define PYGIM_KNOB(name) k.name = g_tune.name
    PYGIM_KNOB(panel_mode); PYGIM_KNOB(panel_bytes); PYGIM_KNOB(panel_min_seg); PYGIM_KNOB(panel_coop); PYGIM_KNOB(panel_locality); PYGIM_KNOB(panel_col16);
    PYGIM_KNOB(vec_lds); PYGIM_KNOB(vec_kernel); PYGIM_KNOB(long_row_threshold); PYGIM_KNOB(long_segment);
#undef PYGIM_KNOB
    return k;
}

// One long-row plan (sweep_plan.hpp plan_long_rows) and its two tables on the device.
static bool upload_long_plan(LongPlan &lp, const std::vector<uint32_t> &h_rowptr, uint32_t thresh, const std::vector<char> *flags, const SweepKnobs &k) {
    lp.thresh = thresh;
    std::vector<uint32_t> tasks, desc;
    plan_long_rows(h_rowptr.data(), (int64_t)h_rowptr.size() - 1, thresh, long_row_segment(thresh, k), flags, tasks, desc);
    lp.n_tasks = (uint32_t)(tasks.size() / 3);
    lp.n_long = (uint32_t)(desc.size() / 3);
    if (!lp.n_tasks) return true;
    return hipMalloc((void **)&lp.d_tasks, tasks.size() * 4) == hipSuccess &&
           hipMalloc((void **)&lp.d_desc, desc.size() * 4) == hipSuccess &&
           hipMemcpy(lp.d_tasks, tasks.data(), tasks.size() * 4, hipMemcpyHostToDevice) == hipSuccess &&
           hipMemcpy(lp.d_desc, desc.data(), desc.size() * 4, hipMemcpyHostToDevice) == hipSuccess;
}

// Does every row store its column ids in order?  The answer stays with the part (cols_sorted).
static int check_cols_sorted(Part &p, int *d_flag_sorted, hipStream_t st) {
    int unsorted = 0;
    if (hipMemsetAsync(d_flag_sorted, 0, sizeof(int), st) != hipSuccess) return fail(PYGIM_ERR_HIP, "flag reset");
    hipLaunchKernelGGL(k_check_sorted_cols, dim3((unsigned)((p.nrows + 255) / 256)), dim3(256), 0, st, p.rowptr, p.colind, (uint32_t)p.nrows, d_flag_sorted);
    if (hipMemcpy(&unsorted, d_flag_sorted, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return fail(PYGIM_ERR_HIP, "sortedness check");
    p.cols_sorted = unsorted ? 0 : 1;
    return 0;
}

// Panel pointers of every row: binary searches on the device for several panels, the row pointers for one.
static int panel_pointers(const Part &p, uint32_t npan, uint32_t panel_cols, const std::vector<uint32_t> &h_rowptr, hipStream_t st, std::vector<uint32_t> &pp) {
    if (npan == 1) {
        pp = one_panel_pointers(h_rowptr.data(), (size_t)p.nrows);
        return 0;
    }
    const size_t pp_elems = (size_t)(npan + 1) * (size_t)p.nrows;
    pp.resize(pp_elems);
    uint32_t *d_pp = nullptr;
    if (hipMalloc((void **)&d_pp, pp_elems * 4) != hipSuccess) return fail(PYGIM_ERR_HIP, "panel pointers");
    hipLaunchKernelGGL(k_build_panel_ptr, dim3((unsigned)((pp_elems + 255) / 256)), dim3(256), 0, st, (const uint32_t *)nullptr, p.rowptr, p.colind, (uint32_t)p.nrows, npan,
                       panel_cols, d_pp);
    const hipError_t ce = hipMemcpy(pp.data(), d_pp, pp_elems * 4, hipMemcpyDeviceToHost);
    (void)hipFree(d_pp);
    return ce == hipSuccess ? 0 : fail(PYGIM_ERR_HIP, "panel pointers D2H");
}

// The one place that writes a planned sweep into its part: the tables on the host, the three item arrays and the 16-bit column ids on the device.
static int adopt_sweep_plan(Part &p, uint32_t npan, uint32_t panel_cols, SweepItems &it, bool locality, const SweepKnobs &k, hipStream_t st) {
    p.npanels = npan;
    p.panel_cols = panel_cols;
    p.panel_locality_used = locality;
    p.n_items = it.rows.size();
    p.panel_off = std::move(it.panel_off);
    p.panel_coop = std::move(it.panel_coop);
    p.panel_long128 = std::move(it.panel_long128);
    p.panel_nnz = std::move(it.panel_nnz);
    if (!p.n_items) return 0;
    if (hipMalloc((void **)&p.d_items, 3 * p.n_items * 4) != hipSuccess ||
        hipMemcpy(p.d_items, it.rows.data(), p.n_items * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(p.d_items + p.n_items, it.beg.data(), p.n_items * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(p.d_items + 2 * p.n_items, it.lens.data(), p.n_items * 4, hipMemcpyHostToDevice) != hipSuccess)
        return fail(PYGIM_ERR_HIP, "panel plan upload");
    if (!sweep_wants_col16(k, panel_cols, p.nnz, p.n_items)) return 0;
    if (hipMalloc((void **)&p.col16, sweep_col16_bytes(p.nnz)) != hipSuccess) return fail(PYGIM_ERR_HIP, "col16 alloc");
    hipLaunchKernelGGL(k_make_col16, dim3((unsigned)((p.nnz + 255) / 256)), dim3(256), 0, st, p.colind, (uint64_t)p.nnz, panel_cols, p.col16);
    if (hipStreamSynchronize(st) != hipSuccess) return fail(PYGIM_ERR_HIP, "col16 build");
    return 0;
}

// One-time plans of a part: the long-row segment plans and the L2-blocked panel plan.  Replaces the reference's prepare_pim_csr / prepare_pim_coo
// balancing (spmm_mul_csr.c:118-259) -- same purpose, different machine.  What the plans hold is decided in sweep_plan.hpp, without a device; here is
// what needs one, in the order it always had: the row pointers down,
// the long-row plan up, the sortedness question, the panel pointers, the heavy rows' plan up, which rows are alike, the items up, the 16-bit ids.
int build_plans(Part &p, size_t es, int *d_flag_sorted, hipStream_t st, int64_t h_hint = 0, bool allow_lds = true) {
    std::vector<uint32_t> h_rowptr((size_t)p.nrows + 1);
    if (hipMemcpy(h_rowptr.data(), p.rowptr, h_rowptr.size() * 4, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(PYGIM_ERR_HIP, "rowptr D2H");
    const SweepKnobs k = sweep_knobs();
    const uint32_t base_thresh = long_row_base_threshold(k);
    if (!upload_long_plan(p.lp_base, h_rowptr, base_thresh, nullptr, k)) return fail(PYGIM_ERR_HIP, "long-row plan upload");
    const SweepPanels want = sweep_panel_count(p.nrows, p.ncols, p.nnz, es, h_hint, k);
    if (want.plan) {
        if (want.ask_sorted)
            if (int rc = check_cols_sorted(p, d_flag_sorted, st)) return rc;
        const uint32_t npan = sweep_panels_given(want, p.cols_sorted == 0), panel_cols = sweep_panel_cols(p.ncols, npan);
        const size_t nr = (size_t)p.nrows;
        std::vector<uint32_t> pp;
        if (int rc = panel_pointers(p, npan, panel_cols, h_rowptr, st, pp)) return rc;
        const std::vector<char> heavy = sweep_heavy_rows(pp.data(), nr, npan, base_thresh);
        if (!upload_long_plan(p.lp_panel, h_rowptr, base_thresh, &heavy, k)) return fail(PYGIM_ERR_HIP, "long-row plan upload");
        std::vector<uint32_t> rank;
        if (sweep_wants_similarity(k, h_hint, p.is_extra, p.sim_kind)) {
            find_similarity(p, st, k.panel_locality == 2);   // (2: propagation whatever the size -- tests)
            rank = sweep_locality_rank(p.sim_kind, p.sim_order, nr);
        }
        SweepItems items = sweep_items(h_rowptr.data(), pp.data(), nr, npan, heavy, rank, p.is_extra, sweep_coop_cap(k));
        if (int rc = adopt_sweep_plan(p, npan, panel_cols, items, !rank.empty(), k, st)) return rc;
    }
    // (the column blocks of a group that also has its merged matrix run through the merged plan: no second token stream for them)
    return allow_lds ? build_lds_plan(p, es, d_flag_sorted, st, h_rowptr, h_hint) : 0;
}

// One-time: the schedule of the LDS-staged product (lds_plan.hpp) for parts it pays for.  Built on the host from
// the row pointers and column ids (the reference balances its DPU row ranges on the host too, spmm_mul_csr.c:118-259).
// The ladder (VERDICT r03 item 3): the code-stream form; if its generation or its executable memory fails, the SAME product as a token
// plan (k_lds_spmm_*: the schedule as data, ~20 % slower) -- not the L2 sweep (2-3 x slower); if the schedule itself cannot be built
// (host memory), the sweep.  Whatever happened is kept as text with the part (pygim_group_lds_note).
static int build_lds_plan_form(Part &p, size_t es, int *d_flag_sorted, hipStream_t st, const std::vector<uint32_t> &h_rowptr, int64_t h_hint,
                               bool allow_code);
int build_lds_plan(Part &p, size_t es, int *d_flag_sorted, hipStream_t st, const std::vector<uint32_t> &h_rowptr, int64_t h_hint) {
    p.lds_note.clear();
    int rc = build_lds_plan_form(p, es, d_flag_sorted, st, h_rowptr, h_hint, true);
    if (rc == -1) {
        const std::string why = p.lds_note;
        rc = build_lds_plan_form(p, es, d_flag_sorted, st, h_rowptr, h_hint, false);
        p.lds_note = why + (p.lds_tiles ? "; products take the token form of the LDS-staged kernel (k_lds_spmm_*)" : "; no token plan either: the L2 sweep serves this group");
    }
    if (p.lds_note.empty())
        p.lds_note = p.lds_tiles ? (p.lds_is_code ? (p.lds_codegen_device || p.lds_codegen_why.empty() ? std::string("code-stream form")
                                                                                                         : "code-stream form (written by the host encoder: " + p.lds_codegen_why + ")")
                                                  : std::string("token form of the LDS-staged kernel")) : "no LDS-staged plan (rule, type or width): the L2 sweep serves this group";
    if (p.lds_tiles && p.lds_half)
        p.lds_note += "; half-split plan: two column ranges of " + std::to_string(p.lds_half) + " columns in the two halves of a wave (a row's sum = the sum of its ranges' sums)";
    if (p.lds_tiles && p.lds_rows)
        p.lds_note += "; the plan's tiles hold the first " + std::to_string(p.lds_rows) + " of " + std::to_string(p.nrows) + " rows (one workgroup per compute unit), k_lds_tail the others";
    if (p.lds_tiles && p.lds_col_splits > 1 && t_plan_dtype == PYGIM_FLT32)
        p.lds_note += "; " + std::to_string(p.lds_col_splits) + " column ranges per row tile: a row's FLT32 sum is the sum of its ranges' sums (inside 1e-5 of |A|.|x|, not the "
                      "CPU loop's bits; lds_col_split_f32 = 0 keeps the stored-order form)";
    // (why the device did not write the stream, when a lower rung's text does not say it already)
    if (!p.lds_codegen_device && !p.lds_codegen_why.empty() && p.lds_note.find(p.lds_codegen_why) == std::string::npos)
        p.lds_note += " [device code generation not used: " + p.lds_codegen_why + "]";
    return rc;
}

// The tunables the form decision reads (lds_form.hpp lds_choose_form), copied in this one place.
static_assert(LDS_EL_INT8 == PYGIM_INT8 && LDS_EL_INT16 == PYGIM_INT16 && LDS_EL_INT32 == PYGIM_INT32 && LDS_EL_INT64 == PYGIM_INT64 &&
              LDS_EL_FLT32 == PYGIM_FLT32 && LDS_EL_DBL64 == PYGIM_DBL64, "lds_form.hpp restates the element type codes");
static LdsFormKnobs lds_form_knobs() {
    LdsFormKnobs k;
#define PYGIM_KNOB(name) k.name = g_tune.name
    PYGIM_KNOB(lds_mode); PYGIM_KNOB(lds_min_reuse_x100); PYGIM_KNOB(lds_min_width); PYGIM_KNOB(lds_min_width8); PYGIM_KNOB(lds_min_reuse_narrow_x100);
    PYGIM_KNOB(lds_waves); PYGIM_KNOB(lds_long_slots); PYGIM_KNOB(lds_code);
    PYGIM_KNOB(lds_col_split); PYGIM_KNOB(lds_col_split_f32); PYGIM_KNOB(lds_row_tail); PYGIM_KNOB(lds_half_split); PYGIM_KNOB(lds_split_order); PYGIM_KNOB(lds_fill_tiles);
    PYGIM_KNOB(lds_code_nbuf); PYGIM_KNOB(lds_code_waves); PYGIM_KNOB(lds_code_kc); PYGIM_KNOB(lds_code_boundary); PYGIM_KNOB(lds_code_exp);
    PYGIM_KNOB(lds_round_tiles); PYGIM_KNOB(lds_tile_order); PYGIM_KNOB(lds_codegen); PYGIM_KNOB(lds_fail);
#undef PYGIM_KNOB
    return k;
}

// The rows an LDS plan leaves out (p.lds_rows .. nrows): their segment table for k_lds_tail_seg / _fin
static int build_tail_segments(Part &p, const std::vector<uint32_t> &h_rowptr) {
    if (!p.lds_rows || p.lds_rows >= (uint32_t)p.nrows) return 0;
    std::vector<uint32_t> rows, e0, e1, rowseg;
    for (uint32_t r = p.lds_rows; r < (uint32_t)p.nrows; r++) {
        rowseg.push_back((uint32_t)rows.size());
        for (uint32_t e = h_rowptr[r]; e < h_rowptr[r + 1]; e += LDS_TAIL_SEG) {
            rows.push_back(r);
            e0.push_back(e);
            e1.push_back(std::min<uint32_t>(e + LDS_TAIL_SEG, h_rowptr[r + 1]));
        }
    }
    rowseg.push_back((uint32_t)rows.size());
    p.lds_tail_nseg = (uint32_t)rows.size();
    std::vector<uint32_t> segs;
    segs.insert(segs.end(), rows.begin(), rows.end());
    segs.insert(segs.end(), e0.begin(), e0.end());
    segs.insert(segs.end(), e1.begin(), e1.end());
    if (hipMalloc((void **)&p.lds_tail_segs, std::max<size_t>(segs.size() * 4, 256)) != hipSuccess ||
        hipMalloc((void **)&p.lds_tail_rowseg, rowseg.size() * 4) != hipSuccess ||
        (!segs.empty() && hipMemcpy(p.lds_tail_segs, segs.data(), segs.size() * 4, hipMemcpyHostToDevice) != hipSuccess) ||
        hipMemcpy(p.lds_tail_rowseg, rowseg.data(), rowseg.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
        return fail(PYGIM_ERR_HIP, "segment table of the rows outside the LDS plan");
    return 0;
}

// One-time (round 5): the density split of a community-structured part whose ids carry no locality (lds_hybrid_dev.hpp) -- for parts the LDS-staged
// product does not take as a whole (too few entries per staged column) and in which label propagation found communities.  Never fatal: a part
// without a split keeps its plans.
int build_hybrid(Part &p, int dtype, size_t es, int *d_flag_sorted, hipStream_t st, int64_t h_hint) {
    static const bool plan_timing = getenv("PYGIM_PLAN_TIMING") != nullptr;
    p.hy_note.clear();
    if (!g_tune.lds_hybrid || p.is_extra || p.vals || p.lds_tiles || p.sim_kind != 2 || p.nrows != p.ncols || p.nnz < (1 << 20) || !p.rowptr) {
        if (plan_timing && g_tune.lds_hybrid && !p.is_extra)
            fprintf(stderr, "[pygim plan] density split not considered: vals %d, lds plan %d, similarity kind %d, %lld x %lld, nnz %lld, rowptr %d\n", p.vals ? 1 : 0, p.lds_tiles ? 1 : 0,
                    p.sim_kind, (long long)p.nrows, (long long)p.ncols, (long long)p.nnz, p.rowptr ? 1 : 0);
        return 0;
    }
    // (INT8 measured and left out: its sweep gathers 256-byte rows, the LDS-staged kernel stages them widened to 16 bits -- products-shaped SBM 2.92 against 3.08 ms)
    if (!(dtype == PYGIM_INT32 || dtype == PYGIM_INT16 || (dtype == PYGIM_INT8 && g_tune.lds_hybrid >= 3) || (dtype == PYGIM_FLT32 && g_tune.lds_hybrid >= 2))) return 0;   // (floats: the order of a row's sums changes)
    if (g_tune.lds_mode == 2 || !g_tune.lds_code || g_tune.lds_waves != 16 || g_tune.lds_code_waves == 16) return 0;
    if (h_hint > 0 && (h_hint * (int64_t)std::max<size_t>(es, 2)) / 4 < g_tune.lds_min_width) return 0;   // (INT8 rides the INT16 stream: lanes of two features)
    const double t0 = now_ms();
    HybridSplit hs;
    const uint32_t min_cell = (uint32_t)std::min<int64_t>(std::max<int64_t>(g_tune.lds_hybrid_min, 1), 1 << 20);
    // the cells are counted in the geometry the dense half's plan will have (build_lds_plan_form: the 8-wave code stream on 256-byte rows, tiles sized
    // for whole rounds of workgroups, the ring's chunk) -- the density test then describes cells the kernel really stages
    uint32_t cell_rows = LDS_CODE_AUTO_WAVES * LDS_CODE8_KA, cell_cols = 128, ring_nbuf = 0;
    if (g_tune.lds_round_tiles && h_hint > 0)
        cell_rows = lds_rows_per_tile((uint32_t)p.nrows, cell_rows, (uint32_t)((h_hint * (int64_t)std::max<size_t>(es, 2) + 255) / 256), (uint32_t)std::max(g_ctx.cu_count, 1));
    lds_code_ring(LDS_CODE_AUTO_WAVES, 256, lds_form_knobs(), LDS_BYTES, ring_nbuf, cell_cols);
    std::string why = hybrid_split_on_device(p.rowptr, p.colind, (uint32_t)p.nrows, (uint64_t)p.nnz, p.sim_order, cell_rows, cell_cols, min_cell, st, hs);
    // worth it when the dense cells hold a good share of the entries (the rest is gathered as before, plus one more pass over C)
    if (why.empty() && (double)hs.nnz_d < 0.3 * (double)p.nnz) {
        why = "hybrid: the dense cells hold " + std::to_string(hs.nnz_d) + " of " + std::to_string(p.nnz) + " entries only";
        hs.release();
    }
    if (!why.empty()) {
        p.hy_note = why;
        if (plan_timing) fprintf(stderr, "[pygim plan] density split not used: %s (%.1f ms)\n", why.c_str(), now_ms() - t0);
        return 0;
    }
    std::unique_ptr<Part> d(new Part), sp(new Part);
    for (Part *q : {d.get(), sp.get()}) {
        q->nrows = p.nrows;
        q->ncols = p.ncols;
        q->dense_cols = p.dense_cols;
        q->own_rowptr = q->own_colind = true;
    }
    d->rowptr = hs.d_rowptr_d; d->colind = hs.d_col_d; d->nnz = (int64_t)hs.nnz_d;
    d->lds_col_order = hs.d_order;
    d->cols_sorted = 1;
    d->lds_contig_tiles = g_tune.lds_hybrid_contig != 0;   // neighbouring tiles stage the same chunks: they meet in one XCD's L2
    d->sim_kind = 2;            // tiles of rows in the same order the cells were counted in
    d->sim_order = p.sim_order;
    d->sim_labels = p.sim_labels;
    d->sim_largest = p.sim_largest;
    sp->rowptr = hs.d_rowptr_s; sp->colind = hs.d_col_s; sp->nnz = (int64_t)hs.nnz_s;
    sp->is_extra = true;        // adds into C, zeroes nothing
    sp->timed = true;
    sp->no_pack = true;
    sp->cols_sorted = 1;
    auto give_up = [&](const std::string &w) {
        free_part(*d);
        free_part(*sp);
        p.hy_note = w;
        (void)hipGetLastError();
        if (plan_timing) fprintf(stderr, "[pygim plan] density split not used: %s\n", w.c_str());
        return 0;
    };
    std::vector<uint32_t> h_rp((size_t)p.nrows + 1);
    if (hipMemcpy(h_rp.data(), d->rowptr, h_rp.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return give_up("hybrid: row pointers D2H failed");
    // the dense half: the LDS-staged plan whatever the uniform-reuse rule says (its tiles skip the chunks they have no entry in)
    d->lds_forced = true;       // (no reuse rule, tiles in the order the part brings along)
    const int rc_d = build_lds_plan(*d, es, d_flag_sorted, st, h_rp, h_hint);
    if (rc_d || !d->lds_tiles || !d->lds_is_code) return give_up("hybrid: no code-stream plan for the dense cells (" + d->lds_note + ")");
    // the sparse half: the sweep's plan (its items in the same locality order)
    sp->sim_kind = 2;
    sp->sim_order = p.sim_order;
    if (int rc = build_plans(*sp, es, d_flag_sorted, st, h_hint, /*allow_lds=*/false)) {
        (void)rc;
        return give_up("hybrid: no sweep plan for the sparse cells");
    }
    char buf[200];
    snprintf(buf, sizeof buf, "density split: %lld entries in dense (tile, chunk) cells through the LDS-staged kernel, %lld through the sweep", (long long)hs.nnz_d, (long long)hs.nnz_s);
    p.hy_note = buf;
    if (plan_timing)
        fprintf(stderr, "[pygim plan] %s (%.1f ms); dense plan: %u tiles, %llu chunk fills (%.1f per tile), %llu entries, %llu served by another entry's read, %.1f MB of code\n", buf,
                now_ms() - t0, d->lds_ntiles, (unsigned long long)d->lds_slots, d->lds_ntiles ? (double)d->lds_slots / d->lds_ntiles : 0.0, (unsigned long long)d->lds_tokens,
                (unsigned long long)d->lds_code_shared, d->lds_code_bytes / 1e6);
    p.hy_dense = std::move(d);
    p.hy_sparse = std::move(sp);
    if (p.extra) p.extra->no_pack = true;   // (the sparse half makes no slice-major copy the correction part could share: it gathers row-major too)
    return 0;
}

// lds_codegen = 2: the device-generated code stream against the host encoder's, word for word (and the stream offsets, the row map, the
// chunk counts of the tiles and the statistics).  "" = identical.
// a half-split plan's VIRTUAL matrix as the host encoder wants it: column c -> (c mod H, half); every row's two sorted runs merged by virtual column (stable: the lower
// range first); h_col is replaced, h_half gets every entry's half
static void half_split_virtual_matrix(const std::vector<uint32_t> &h_rowptr, uint32_t nrows, uint32_t H, std::vector<uint32_t> &h_col, std::vector<uint32_t> &h_half) {
    h_half.assign(h_col.size(), 0u);
    std::vector<uint32_t> col2(h_col.size());
    const uint32_t blocks = (uint32_t)(((uint64_t)nrows + 4095) / 4096);
    lds_parallel_for(blocks, (unsigned)std::max<int64_t>(0, g_tune.lds_threads), [&](uint32_t b) {
        for (uint64_t r = (uint64_t)b * 4096; r < std::min<uint64_t>((uint64_t)nrows, (uint64_t)(b + 1) * 4096); r++) {
            const uint32_t e0 = h_rowptr[r], e1 = h_rowptr[r + 1];
            uint32_t mid = (uint32_t)(std::lower_bound(h_col.begin() + e0, h_col.begin() + e1, H) - h_col.begin());
            uint32_t a = e0, c = mid, o = e0;
            while (a < mid || c < e1) {
                const bool take_low = c >= e1 || (a < mid && h_col[a] <= h_col[c] - H);
                if (take_low) { col2[o] = h_col[a++]; h_half[o++] = 0u; }
                else { col2[o] = h_col[c++] - H; h_half[o++] = 1u; }
            }
        }
    });
    h_col.swap(col2);
}

static std::string codegen_verify(const Part &p, const LdsGeometry &geo, uint32_t code_op, const std::vector<uint32_t> &h_rowptr, const uint32_t *rorder,
                                  const CgDeviceResult &dr, const uint32_t *d_vals32 = nullptr, uint32_t nrows_plan = 0, uint32_t half_H = 0) {
    if (!nrows_plan) nrows_plan = (uint32_t)p.nrows;   // d_vals32: INT8 / INT16 values widened to 4 bytes
    std::vector<uint32_t> h_col((size_t)p.nnz), h_val;
    std::vector<uint64_t> h_val64;
    if (hipMemcpy(h_col.data(), p.colind, h_col.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return "column ids D2H failed";
    if (p.vals && geo.row_bytes == 512) {   // DBL64: entry indices in the plan, the values beside it
        h_val.resize((size_t)p.nnz);
        h_val64.resize((size_t)p.nnz);
        for (size_t i = 0; i < h_val.size(); i++) h_val[i] = (uint32_t)i;
        if (hipMemcpy(h_val64.data(), p.vals, h_val64.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) return "values D2H failed";
    } else if (p.vals) {
        h_val.resize((size_t)p.nnz);
        if (hipMemcpy(h_val.data(), d_vals32 ? (const void *)d_vals32 : p.vals, h_val.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return "values D2H failed";
    }
    LdsPlanHost plan;
    LdsCodeHost ch;
    try {
        if (half_H) half_split_virtual_matrix(h_rowptr, nrows_plan, half_H, h_col, h_val);
        lds_plan_build(h_rowptr.data(), h_col.data(), nrows_plan, half_H ? half_H : (uint32_t)p.ncols, geo, plan, (unsigned)std::max<int64_t>(0, g_tune.lds_threads),
                       (p.vals || half_H) ? h_val.data() : nullptr, rorder);
        lds_code_from_plan(plan, code_op, ch, (unsigned)std::max<int64_t>(0, g_tune.lds_threads), (uint32_t)std::max<int64_t>(0, g_tune.lds_code_gsize),
                           (uint32_t)std::max<int64_t>(0, g_tune.lds_code_nsets), 0, h_val64.empty() ? nullptr : h_val64.data());
    } catch (const std::exception &e) {
        return std::string("the host encoder failed: ") + e.what();
    }
    if (ch.code.size() * 4 != dr.code_bytes) return "code size " + std::to_string(dr.code_bytes) + " against " + std::to_string(ch.code.size() * 4) + " bytes";
    if (plan.ntiles != dr.ntiles || plan.slots != dr.slots) return "tile / slot counts";
    std::vector<uint32_t> d_code(ch.code.size());
    void *stage = nullptr;   // (the executable allocation is read through a plain device buffer)
    if (hipMalloc(&stage, std::max<size_t>(dr.code_bytes, 256)) != hipSuccess) return "out of device memory for the comparison";
    const uint64_t n16 = dr.code_bytes / 16;
    hipLaunchKernelGGL(k_copy16, dim3((unsigned)((n16 + 255) / 256)), dim3(256), 0, 0, (const u32x4_t *)dr.code, (u32x4_t *)stage, n16);
    const bool got = hipMemcpy(d_code.data(), stage, dr.code_bytes, hipMemcpyDeviceToHost) == hipSuccess;
    (void)hipFree(stage);
    if (!got) return "code D2H failed";
    if (memcmp(d_code.data(), ch.code.data(), dr.code_bytes) != 0) {
        size_t at = 0;
        while (d_code[at] == ch.code[at]) at++;
        size_t s = 0;
        while (s + 1 < ch.start.size() && ch.start[s + 1] / 4 <= at) s++;
        char buf[160];
        snprintf(buf, sizeof buf, "first difference at dword %zu (stream %zu + %zu): %08x against the host's %08x", at, s, at - (size_t)(ch.start[s] / 4), d_code[at], ch.code[at]);
        return buf;
    }
    std::vector<uint64_t> d_start(ch.start.size());
    std::vector<uint32_t> d_rowmap(plan.rowmap.size());
    std::vector<LdsTile> d_tiles(plan.tiles.size());
    if (hipMemcpy(d_start.data(), dr.d_start, d_start.size() * 8, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(d_rowmap.data(), dr.d_rowmap, d_rowmap.size() * 4, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(d_tiles.data(), dr.d_tiles, d_tiles.size() * sizeof(LdsTile), hipMemcpyDeviceToHost) != hipSuccess)
        return "table D2H failed";
    if (d_start != ch.start) return "stream offsets";
    if (d_rowmap != plan.rowmap) return "row map";
    for (size_t t = 0; t < d_tiles.size(); t++)
        if (d_tiles[t].nch != plan.tiles[t].nch || d_tiles[t].row0 != plan.tiles[t].row0 || d_tiles[t].nnz != plan.tiles[t].nnz || d_tiles[t].chunk0 != plan.tiles[t].chunk0)
            return "tile table";
    if (dr.entries != ch.entries || dr.pairs != ch.pairs || dr.shared != ch.shared) return "statistics";
    return std::string();
}

// What a producer of an LDS-staged plan (the device code generator, the host encoder) hands over: device arrays and counts.
struct LdsBuilt {
    void *code = nullptr;                  // code stream in executable memory (nullptr: a token plan)
    uint64_t code_bytes = 0, pairs = 0, shared = 0;
    uint32_t gsize = 0, nsets = 0;
    uint64_t *d_start = nullptr;
    uint32_t *d_tok = nullptr, *d_rowmap = nullptr;
    LdsTile *d_tiles = nullptr;
    uint32_t ntiles = 0, wdelta = 0;
    uint64_t slots = 0, tokens = 0;
    bool device = false;                   // written by the device code generator
    void release() {
        if (code) (void)hsa_amd_memory_pool_free(code);
        for (void *q : {(void *)d_start, (void *)d_tok, (void *)d_rowmap, (void *)d_tiles})
            if (q) (void)hipFree(q);
    }
};

// The one place that writes a built plan into its part, whichever producer made it.
static int adopt_lds_plan(Part &p, const LdsForm &f, const LdsGeometry &geo, const LdsBuilt &b, const std::vector<uint32_t> &h_rowptr) {
    if (b.code) {
        p.lds_code = (char *)b.code;
        p.lds_code_bytes = b.code_bytes;
        p.lds_code_start = b.d_start;
        p.lds_code_pairs = b.pairs;
        p.lds_code_shared = b.shared;
        p.lds_is_code = true;
        p.lds_code_piece = geo.KC * geo.row_bytes / geo.NW;
        p.lds_code_gsize = b.gsize;
        p.lds_code_nsets = b.nsets;
        if (b.device) p.lds_codegen_device = true;
    } else {
        p.lds_tok = b.d_tok;
        p.lds_wdelta = b.wdelta;
    }
    p.lds_rowmap = b.d_rowmap;
    p.lds_tiles = b.d_tiles;
    p.lds_col_splits = geo.col_splits;
    p.lds_rows = f.rows_lds < (uint32_t)p.nrows ? f.rows_lds : 0;
    p.lds_half = f.half_H;
    p.lds_kc = geo.KC;
    p.lds_nbuf = geo.NBUF;
    p.lds_row_bytes = geo.row_bytes;
    p.lds_ka = geo.KA;
    p.lds_ntiles = b.ntiles;
    p.lds_nw = geo.NW;
    p.lds_batch = geo.BATCH;
    p.lds_slots = b.slots;
    p.lds_tokens = b.tokens;   // (a code stream has no padding: its entries)
    return build_tail_segments(p, h_rowptr);
}

// PYGIM_PLAN_TIMING=1: where the creation time of an LDS-staged plan goes (stderr; the reference prints its own prepare / load times)
struct PlanLap {
    const bool on = getenv("PYGIM_PLAN_TIMING") != nullptr;
    double t_mark = now_ms();
    void operator()(const char *what) {
        if (!on) return;
        const double t = now_ms();
        fprintf(stderr, "[pygim plan] %-34s %8.1f ms\n", what, t - t_mark);
        t_mark = t;
    }
};

// Round 5: the code stream GENERATED ON THE DEVICE (lds_codegen_dev.hpp) from the resident CSR -- the same bytes the host encoder
// would write (lds_codegen = 2 checks that, word for word) without the graph ever visiting the host.  A failure on the way is returned
// as text (the host encoder takes over); only a mismatch under lds_codegen = 2 is an error (rc).
static std::string lds_plan_on_device(const Part &p, const LdsForm &f, size_t val_es, hipStream_t st, const std::vector<uint32_t> &h_rowptr, const uint32_t *ro,
                                      PlanLap &lap, LdsBuilt &b, int &rc) {
    const size_t es = f.es;
    const uint32_t ncols_plan = f.half_H ? f.half_H : (uint32_t)p.ncols;
    CgDeviceResult dr;
    std::string exec_why;
    auto alloc_exec = [&](size_t bytes) -> void * { return exec_alloc(bytes, &exec_why); };
    auto free_exec = [&](void *q) { (void)hsa_amd_memory_pool_free(q); };
    // (round 5: valued INT16 / INT8 -- the values sign-extended to the 4-byte slot the encoders read: v_pk_mul_lo_u16 takes the low half)
    uint32_t *d_vals32 = nullptr;
    if (p.vals && val_es < 4) {
        if (hipMalloc((void **)&d_vals32, std::max<size_t>((size_t)p.nnz * 4, 256)) != hipSuccess) {
            (void)hipGetLastError();
            d_vals32 = nullptr;
        } else if (val_es == 1) hipLaunchKernelGGL((k_widen_vals<int8_t>), dim3((unsigned)(((uint64_t)p.nnz + 255) / 256)), dim3(256), 0, st, (const int8_t *)p.vals, (uint64_t)p.nnz, d_vals32);
        else hipLaunchKernelGGL((k_widen_vals<int16_t>), dim3((unsigned)(((uint64_t)p.nnz + 255) / 256)), dim3(256), 0, st, (const int16_t *)p.vals, (uint64_t)p.nnz, d_vals32);
    }
    struct FreeVals { uint32_t *q; ~FreeVals() { if (q) (void)hipFree(q); } } free_vals{d_vals32};
    g_cg_fail_big_alloc = (g_tune.lds_fail & 8) != 0;
    const std::string why = (p.vals && val_es < 4 && !d_vals32) ? std::string("out of device memory for the widened values") :
              cg_run_on_device(p.rowptr, p.colind, es == 8 ? nullptr : (p.vals && val_es < 4) ? d_vals32 : (const uint32_t *)p.vals, es == 8 ? (const uint64_t *)p.vals : nullptr, h_rowptr.data(), ro, f.rows_lds,
                               ncols_plan, f.geo, f.code_op,
                               (uint32_t)std::max<int64_t>(0, g_tune.lds_code_gsize), (uint32_t)std::max<int64_t>(0, g_tune.lds_code_nsets), st, alloc_exec,
                               free_exec, dr, [] { return now_ms(); }, f.half_H);
    if (!why.empty()) return why;
    if (lap.on)
        fprintf(stderr, "[pygim plan] device code generation: rows %.1f, chunk lists %.1f, keys + sort %.1f, columns %.1f, slots + groups %.1f, sizes %.1f, emission %.1f, "
                        "whole %.1f ms (%.1f MB of code)\n", dr.ms[0], dr.ms[1], dr.ms[2], dr.ms[3], dr.ms[4], dr.ms[5], dr.ms[6], dr.ms[7], dr.code_bytes / 1e6);
    b.code = dr.code;
    b.code_bytes = dr.code_bytes;
    b.d_start = dr.d_start;
    b.d_rowmap = dr.d_rowmap;
    b.d_tiles = dr.d_tiles;
    b.pairs = dr.pairs;
    b.shared = dr.shared;
    b.gsize = dr.regs.gsize;
    b.nsets = dr.regs.nsets;
    b.ntiles = dr.ntiles;
    b.slots = dr.slots;
    b.tokens = dr.entries;
    b.device = true;
    if (g_tune.lds_codegen == 2) {   // the checker: the host encoder's blob against what the device wrote
        const std::string diff = codegen_verify(p, f.geo, f.code_op, h_rowptr, ro, dr, d_vals32, f.rows_lds, f.half_H);
        if (!diff.empty()) {
            b.release();
            b = LdsBuilt();
            rc = fail(PYGIM_ERR_INVALID, ("lds_codegen = 2: the device-generated code stream differs from the host encoder's: " + diff).c_str());
        }
    }
    return std::string();
}

// The host encoder: column ids (and values) to the host, the schedule (lds_plan_build), for a code stream its machine code into executable
// memory, the tables to the device.  0 with b.d_tiles == nullptr: no plan (p.lds_note may say why); -1: the next rung of build_lds_plan's ladder.
static int lds_plan_on_host(Part &p, const LdsForm &f, LdsGeometry &geo, size_t val_es, const std::vector<uint32_t> &h_rowptr, const uint32_t *ro, PlanLap &lap, LdsBuilt &b) {
    const size_t es = f.es;
    const bool want_code = f.want_code, half = f.half_H != 0;
    const unsigned threads = (unsigned)std::max<int64_t>(0, g_tune.lds_threads);
    std::vector<uint32_t> h_col((size_t)p.nnz);
    if (hipMemcpy(h_col.data(), p.colind, h_col.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return fail(PYGIM_ERR_HIP, "colind D2H");
    lap("sortedness check + column ids D2H");
    std::vector<uint32_t> h_val;
    std::vector<uint64_t> h_val64;
    if (p.vals) {
        h_val.resize((size_t)p.nnz);
        if (es == 4) {
            if (hipMemcpy(h_val.data(), p.vals, h_val.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return fail(PYGIM_ERR_HIP, "values D2H");
        } else if (es == 8) {  // DBL64: the plan's value slot carries the entry index, the values travel beside it
            h_val64.resize((size_t)p.nnz);
            if (hipMemcpy(h_val64.data(), p.vals, h_val64.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) return fail(PYGIM_ERR_HIP, "values D2H");
            for (size_t i = 0; i < h_val.size(); i++) h_val[i] = (uint32_t)i;
        } else if (val_es == 1) {  // INT8 (code stream on the widened features): sign-extended
            std::vector<int8_t> v8((size_t)p.nnz);
            if (hipMemcpy(v8.data(), p.vals, v8.size(), hipMemcpyDeviceToHost) != hipSuccess) return fail(PYGIM_ERR_HIP, "values D2H");
            for (size_t i = 0; i < v8.size(); i++) h_val[i] = (uint32_t)(int32_t)v8[i];
        } else {  // INT16: sign-extended for the code stream (v_pk_mul_lo_u16 takes the low half for both features); the token kernel wants the
                  // value in both halves of its dword (its packed multiply reads the SGPR as it is)
            std::vector<uint16_t> v16((size_t)p.nnz);
            if (hipMemcpy(v16.data(), p.vals, v16.size() * 2, hipMemcpyDeviceToHost) != hipSuccess) return fail(PYGIM_ERR_HIP, "values D2H");
            for (size_t i = 0; i < v16.size(); i++) h_val[i] = want_code ? (uint32_t)(int32_t)(int16_t)v16[i] : (uint32_t)v16[i] * 0x10001u;
        }
    }
    LdsPlanHost plan;
    try {
        if (g_tune.lds_fail & 4) throw std::runtime_error("lds_fail: forced failure of the schedule build");
        if (half) half_split_virtual_matrix(h_rowptr, (uint32_t)p.nrows, f.half_H, h_col, h_val);
        lds_plan_build(h_rowptr.data(), h_col.data(), f.rows_lds, half ? f.half_H : (uint32_t)p.ncols, geo, plan, threads, (p.vals || half) ? h_val.data() : nullptr, ro);
        lap("schedule (tiles, tokens)");
        // long slots (lds_form.hpp): the 16-token-batch geometry for a schedule whose waves get this many tokens per slot
        if (f.long_candidate && plan.slots > 0 && (double)plan.ntokens / ((double)plan.slots * geo.NW) >= (double)g_tune.lds_long_slots) {
            lds_plan_build(h_rowptr.data(), h_col.data(), (uint32_t)p.nrows, (uint32_t)p.ncols, f.long_geo, plan, threads, nullptr);
            geo = f.long_geo;
        }
    } catch (const std::exception &e) {   // host memory, threads: no LDS-staged plan, the sweep serves the group
        p.lds_note = std::string("the schedule of the LDS-staged product could not be built (") + e.what() + "): the L2 sweep serves this group";
        return 0;
    }
    std::vector<uint32_t>().swap(h_col);
    std::vector<uint32_t>().swap(h_val);
    if (p.vals && !want_code) {
        // one buffer: the token stream, then the value stream at the same positions (the kernel adds a 32-bit byte offset)
        if ((uint64_t)plan.tok.size() * 8 >= (1ull << 32)) return 0;
        b.wdelta = (uint32_t)(plan.tok.size() * 4);
        plan.tok.insert(plan.tok.end(), plan.wts.begin(), plan.wts.end());
        std::vector<uint32_t>().swap(plan.wts);
    }
    auto up = [&](auto **dst, const auto &v) {
        using E = typename std::remove_reference<decltype(v[0])>::type;
        const size_t bytes = std::max<size_t>(v.size() * sizeof(E), 64);
        if (hipMalloc((void **)dst, bytes) != hipSuccess) return false;
        return v.empty() || hipMemcpy(*dst, v.data(), v.size() * sizeof(E), hipMemcpyHostToDevice) == hipSuccess;
    };
    if (plan.header_overflow) {  // a slot header field would not fit its 14 bits (a wave with > 16 383 batches in one chunk, > 5 M columns)
        p.lds_note = "the LDS-staged schedule does not fit its slot headers (more than 16 383 batches of one wave in one chunk, or more than 5 M columns): the L2 sweep serves this group";
        return 0;
    }
    b.ntiles = plan.ntiles;
    b.slots = plan.slots;
    b.tokens = plan.ntokens;
    if (!want_code) {
        if (up(&b.d_tok, plan.tok) && up(&b.d_rowmap, plan.rowmap) && up(&b.d_tiles, plan.tiles)) return 0;
        b.release();
        b = LdsBuilt();
        return fail(PYGIM_ERR_HIP, "LDS plan upload");
    }
    // the schedule as machine code (1.5 instructions per stored entry instead of 4 + bookkeeping) in EXECUTABLE memory; the token
    // stream itself stays on the host (the kernel needs the tile table and the row map only)
    LdsCodeHost ch;
    try {
        if (g_tune.lds_fail & 1) throw std::runtime_error("lds_fail: forced failure of the code generation");
        lds_code_from_plan(plan, f.code_op, ch, threads, (uint32_t)std::max<int64_t>(0, g_tune.lds_code_gsize), (uint32_t)std::max<int64_t>(0, g_tune.lds_code_nsets),
                           (uint32_t)std::max<int64_t>(0, g_tune.lds_code_exp), h_val64.empty() ? nullptr : h_val64.data());
    } catch (const std::exception &e) {   // out of host memory or threads: the same schedule as a token plan (build_lds_plan)
        p.lds_note = std::string("code-stream form not available: generating the instruction streams failed (") + e.what() + ")";
        return -1;
    }
    lap("code generation");
    std::vector<uint32_t>().swap(plan.tok);
    std::string why_exec;
    b.code = (g_tune.lds_fail & 2) ? nullptr : exec_alloc_upload(ch.code.data(), ch.code.size() * 4, &why_exec);
    if (!b.code) {                     // no executable pool on this runtime, or out of device memory: the token plan
        p.lds_note = "code-stream form not available: " + (why_exec.empty() ? std::string("lds_fail: forced failure of the executable allocation") : why_exec) +
                     " (" + std::to_string(ch.code.size() * 4) + " bytes of code)";
        return -1;
    }
    if (!up(&b.d_start, ch.start) || !up(&b.d_rowmap, plan.rowmap) || !up(&b.d_tiles, plan.tiles)) {
        b.release();
        b = LdsBuilt();
        return fail(PYGIM_ERR_HIP, "code-stream plan upload");
    }
    lap("code + tables upload");
    b.code_bytes = ch.code.size() * 4;
    b.pairs = ch.pairs;
    b.shared = ch.shared;
    b.gsize = ch.regs.gsize;
    b.nsets = ch.regs.nsets;
    return 0;
}

// One form of the LDS-staged plan of a part: choose it (lds_form.hpp: a pure function), ask the device what the choice cannot know,
// let the device generator or the host encoder build it, adopt what they made.  0 without p.lds_tiles: no plan; -1: the next rung.
static int build_lds_plan_form(Part &p, size_t val_es, int *d_flag_sorted, hipStream_t st, const std::vector<uint32_t> &h_rowptr, int64_t h_hint,
                               bool allow_code) {
    PlanLap lap;
    LdsFormInput in;
    in.dtype = t_plan_dtype;
    in.val_es = val_es;
    in.nrows = p.nrows;
    in.ncols = p.ncols;
    in.nnz = p.nnz;
    in.valued = p.vals != nullptr;
    in.is_extra = p.is_extra;
    in.lds_forced = p.lds_forced;
    in.lds_contig_tiles = p.lds_contig_tiles;
    in.h_hint = h_hint;
    in.cu_count = g_ctx.cu_count;
    in.allow_code = allow_code;
    in.k.kc = LDS_KC;
    in.k.lds_bytes = LDS_BYTES;
    in.k.ka8 = lds_ka(8);
    in.k.batch8 = lds_batch(8);
    in.k.ka16 = lds_ka(16);
    in.k.batch16 = lds_batch(16);
    in.k.l16_ka = LDS_L16_KA;
    in.k.l16_batch = LDS_L16_BATCH;
    const LdsForm f = lds_choose_form(in, lds_form_knobs());
    if (!f.plan) return 0;
    if (p.cols_sorted < 0)   // (the panel plan may have asked already)
        if (int rc = check_cols_sorted(p, d_flag_sorted, st)) return rc;
    if (!p.cols_sorted) return 0;  // stored order inside a row must be column order for the chunk walk
    std::vector<uint32_t> rorder;
    if (f.want_similarity) {
        // automatic: ids that are local already (a row's columns span a small part of the id range: tiles of consecutive rows skip most
        // chunks as they are) keep consecutive tiles; otherwise the propagation decides -- it must have found communities (more than
        // one label, none holding half of the rows), else its order is the consecutive one anyway (profiles/r05_structured.txt)
        find_similarity(p, st, f.similarity_forced);
        if (p.sim_kind == 2) {
            rorder = p.sim_order;
            p.lds_tile_labels = p.sim_labels;
            p.lds_tile_largest = p.sim_largest;
        }
        lap("similarity order (label propagation)");
    }
    const uint32_t *ro = rorder.empty() ? nullptr : rorder.data();
    LdsBuilt b;
    LdsGeometry geo = f.geo;   // (the host encoder may take the long-slots geometry instead)
    if (f.device_codegen) {    // plans the device generator does not cover, or a failure on the way, take the host encoder
        int rc = 0;
        const std::string dev_why = lds_plan_on_device(p, f, val_es, st, h_rowptr, ro, lap, b, rc);
        if (rc) return rc;
        if (dev_why.empty()) {
            lap("code stream generated on the device");
            return adopt_lds_plan(p, f, geo, b, h_rowptr);
        }
        (void)hipGetLastError();
        if (lap.on) fprintf(stderr, "[pygim plan] device code generation not used: %s\n", dev_why.c_str());
        p.lds_codegen_why = dev_why;
    } else if (f.want_code) {
        p.lds_codegen_why = f.codegen_why;
    }
    if (int rc = lds_plan_on_host(p, f, geo, val_es, h_rowptr, ro, lap, b)) return rc;
    return b.d_tiles ? adopt_lds_plan(p, f, geo, b, h_rowptr) : 0;
}

double now_ms() {
    using namespace std::chrono;
    return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}

int need_init() {
    if (!g_ctx.inited) return fail(PYGIM_ERR_NO_DEVICE, "backend not initialised: call dpu_init_ranks / pygim_init_ranks first");
    return 0;
}
