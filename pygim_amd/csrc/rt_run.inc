// rt_run.inc -- part of pygim_hip.hip (file scope): group assembly helpers (pattern + correction split, narrow values, merged parts), the shared body of the
// run_group entry points (run_group_common: it does what run_plan.hpp planned), the conv layers' quantiser around the product.
template <typename T>
static void launch_pack(const void *const *d_ptrs, uint32_t gcount, uint64_t n, void *out, hipStream_t st) {
    const uint64_t total = n * gcount;
    if (total == 0) return;
    hipLaunchKernelGGL((k_pack_vectors<T>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st,
                       (const T *const *)d_ptrs, gcount, n, (T *)out);
}

// Integer weights that are 1 except for a few entries (at most nnz / 32; nnz / 64 until the density split, which takes patterns only: a products-shaped
// community graph coalesces to 2 % of weights above 1): keep the unit-weight pattern in `p` and move
// the exceptions, as (weight - 1), into p.extra (CSR by rows, entries in stored order).  One-time, at group creation.
template <typename T>
int split_unit_pattern_t(Part &p, size_t es, int *d_flag_sorted, uint32_t *d_counter, hipStream_t st) {
    const uint32_t n = (uint32_t)p.nnz;
    if (hipMemsetAsync(d_counter, 0, sizeof(uint32_t), st) != hipSuccess) return fail(PYGIM_ERR_HIP, "counter reset");
    hipLaunchKernelGGL((k_count_non_ones<T>), dim3((n + 255) / 256), dim3(256), 0, st, (const T *)p.vals, n, d_counter);
    uint32_t cnt = 0;
    if (hipMemcpy(&cnt, d_counter, sizeof(cnt), hipMemcpyDeviceToHost) != hipSuccess) return fail(PYGIM_ERR_HIP, "non-one count");
    if (cnt == 0 || (uint64_t)cnt * 32 > (uint64_t)n) return 0;  // all ones is handled by the caller; many weights (more than nnz / 32): keep them
    uint32_t *d_e = nullptr, *d_c = nullptr;
    T *d_v = nullptr;
    auto drop = [&]() {
        if (d_e) (void)hipFree(d_e);
        if (d_c) (void)hipFree(d_c);
        if (d_v) (void)hipFree(d_v);
    };
    if (hipMalloc((void **)&d_e, (size_t)cnt * 4) != hipSuccess || hipMalloc((void **)&d_c, (size_t)cnt * 4) != hipSuccess ||
        hipMalloc((void **)&d_v, (size_t)cnt * sizeof(T)) != hipSuccess) {
        drop();
        return fail(PYGIM_ERR_HIP, "extra part scratch");
    }
    (void)hipMemsetAsync(d_counter, 0, sizeof(uint32_t), st);
    hipLaunchKernelGGL((k_extract_non_ones<T>), dim3((n + 255) / 256), dim3(256), 0, st, (const T *)p.vals, p.colind, n, cnt,
                       d_counter, d_e, d_c, d_v);
    std::vector<uint32_t> e(cnt), c(cnt), rp((size_t)p.nrows + 1);
    std::vector<T> v(cnt);
    const bool ok = hipMemcpy(e.data(), d_e, (size_t)cnt * 4, hipMemcpyDeviceToHost) == hipSuccess &&
                    hipMemcpy(c.data(), d_c, (size_t)cnt * 4, hipMemcpyDeviceToHost) == hipSuccess &&
                    hipMemcpy(v.data(), d_v, (size_t)cnt * sizeof(T), hipMemcpyDeviceToHost) == hipSuccess &&
                    hipMemcpy(rp.data(), p.rowptr, rp.size() * 4, hipMemcpyDeviceToHost) == hipSuccess;
    drop();
    if (!ok) return fail(PYGIM_ERR_HIP, "extra part D2H");
    // stored order (the append order on the device is arbitrary)
    std::vector<uint32_t> order(cnt);
    for (uint32_t k = 0; k < cnt; k++) order[k] = k;
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return e[a] < e[b]; });
    std::vector<uint32_t> xrp((size_t)p.nrows + 1, 0), xc(cnt);
    std::vector<T> xv(cnt);
    for (uint32_t k = 0; k < cnt; k++) {
        const uint32_t src = order[k];
        const uint32_t row = (uint32_t)(std::upper_bound(rp.begin(), rp.end(), e[src]) - rp.begin()) - 1;
        xrp[(size_t)row + 1]++;
        xc[k] = c[src];
        xv[k] = v[src];
    }
    for (int64_t r = 0; r < p.nrows; r++) xrp[(size_t)r + 1] += xrp[(size_t)r];
    std::unique_ptr<Part> x(new Part);
    x->is_extra = true;
    x->nrows = p.nrows;
    x->ncols = p.ncols;
    x->nnz = cnt;
    x->dense_cols = p.dense_cols;
    x->own_rowptr = x->own_colind = x->own_vals = true;
    if (hipMalloc((void **)&x->rowptr, xrp.size() * 4) != hipSuccess || hipMalloc((void **)&x->colind, (size_t)cnt * 4) != hipSuccess ||
        hipMalloc(&x->vals, (size_t)cnt * sizeof(T)) != hipSuccess ||
        hipMemcpy(x->rowptr, xrp.data(), xrp.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(x->colind, xc.data(), (size_t)cnt * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(x->vals, xv.data(), (size_t)cnt * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) {
        free_part(*x);
        return fail(PYGIM_ERR_HIP, "extra part upload");
    }
    if (int rc = build_plans(*x, es, d_flag_sorted, st)) {
        free_part(*x);
        return rc;
    }
    p.extra = std::move(x);
    if (p.own_vals) (void)hipFree(p.vals);
    p.vals = nullptr;
    p.own_vals = false;
    return 0;
}

// One-time: a 4-byte copy of the values of an 8-byte element type for the sweep (kernels.hpp SweepVal), when every value
// survives the round trip bit for bit.  The weights of a normalised adjacency are float32 numbers widened by the caller's
// DBL64 choice, integer weights are small counts: both halve the value bytes every 128-byte slice re-reads.
template <typename T> int narrow_values_t(Part &p, int *d_flag, hipStream_t st) {
    using NT = typename NarrowOf<T>::type;
    void *buf = nullptr;
    if (hipMalloc(&buf, (size_t)p.nnz * sizeof(NT)) != hipSuccess) {
        (void)hipGetLastError();
        return 0;  // (an optimisation only)
    }
    int bad = 0;
    if (hipMemsetAsync(d_flag, 0, sizeof(int), st) != hipSuccess) { (void)hipFree(buf); return fail(PYGIM_ERR_HIP, "flag reset"); }
    hipLaunchKernelGGL((k_narrow_vals<T>), dim3((unsigned)(((uint64_t)p.nnz + 255) / 256)), dim3(256), 0, st, (const T *)p.vals, (uint64_t)p.nnz,
                       (NT *)buf, d_flag);
    if (hipMemcpyAsync(&bad, d_flag, sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
        (void)hipFree(buf);
        return fail(PYGIM_ERR_HIP, "narrow values");
    }
    if (bad) (void)hipFree(buf);
    else p.vals_narrow = buf;
    return 0;
}
int narrow_values(Part &p, int dtype, int *d_flag, hipStream_t st) {
    if (!g_tune.narrow_vals || !p.vals || p.nnz == 0 || p.is_extra || !p.d_items) return 0;  // (d_items: the part has a sweep plan)
    if (dtype == PYGIM_INT64) return narrow_values_t<int64_t>(p, d_flag, st);
    if (dtype == PYGIM_DBL64) return narrow_values_t<double>(p, d_flag, st);
    return 0;
}

int split_unit_pattern(Part &p, int dtype, size_t es, int *d_flag_sorted, uint32_t *d_counter, hipStream_t st) {
    if (!p.vals || p.nnz == 0 || !g_tune.split_unit_pattern) return 0;
    switch (dtype) {
        case PYGIM_INT8: return split_unit_pattern_t<int8_t>(p, es, d_flag_sorted, d_counter, st);
        case PYGIM_INT16: return split_unit_pattern_t<int16_t>(p, es, d_flag_sorted, d_counter, st);
        case PYGIM_INT32: return split_unit_pattern_t<int32_t>(p, es, d_flag_sorted, d_counter, st);
        case PYGIM_INT64: return split_unit_pattern_t<int64_t>(p, es, d_flag_sorted, d_counter, st);
        default: return 0;  // floats keep their weights in the loop (stored-order sums)
    }
}

// One-time: the group's sparse parts as one matrix (see Group::merged).
template <typename T>
int build_merged_t(Group *g, size_t es, hipStream_t st) {
    const int64_t nrows = g->total_rows;
    uint64_t nnz = 0, ncols = 0;
    bool any_vals = false;
    for (auto &p : g->parts) {
        nnz += (uint64_t)p.nnz;
        ncols += (uint64_t)p.ncols;
        any_vals = any_vals || p.vals != nullptr;
    }
    any_vals = any_vals && !g->all_ones;
    if (nnz == 0 || nnz > 0xFFFFFFFFull || ncols > 0xFFFFFFFFull) return 0;  // nothing to gain / would not fit 32-bit ids
    std::unique_ptr<Part> m(new Part);
    m->nrows = nrows;
    m->ncols = (int64_t)ncols;
    m->nnz = (int64_t)nnz;
    m->dense_cols = g->parts[0].dense_cols;
    m->own_rowptr = m->own_colind = true;
    uint32_t *cursor = nullptr;
    auto fail_free = [&](const char *what) {
        if (cursor) (void)hipFree(cursor);
        free_part(*m);
        return fail(PYGIM_ERR_HIP, what);
    };
    const size_t rp_bytes = (size_t)(nrows + 1) * 4;
    if (hipMalloc((void **)&m->rowptr, rp_bytes) != hipSuccess || hipMalloc((void **)&m->colind, (size_t)nnz * 4) != hipSuccess ||
        hipMalloc((void **)&cursor, rp_bytes) != hipSuccess)
        return fail_free("merged matrix alloc");
    if (any_vals) {
        if (hipMalloc(&m->vals, (size_t)nnz * es) != hipSuccess) return fail_free("merged values alloc");
        m->own_vals = true;
    }
    if (hipMemsetAsync(m->rowptr, 0, rp_bytes, st) != hipSuccess) return fail_free("merged rowptr reset");
    const unsigned rgrid = (unsigned)((nrows + 1 + 255) / 256);
    for (auto &p : g->parts) hipLaunchKernelGGL(k_merge_count, dim3(rgrid), dim3(256), 0, st, p.rowptr, (uint32_t)nrows, m->rowptr);
    if (hipMemcpyAsync(cursor, m->rowptr, rp_bytes, hipMemcpyDeviceToDevice, st) != hipSuccess) return fail_free("cursor copy");
    uint32_t coff = 0;
    for (auto &p : g->parts) {
        if (p.nnz > 0)
            hipLaunchKernelGGL((k_merge_scatter<T>), dim3((unsigned)((p.nnz + 255) / 256)), dim3(256), 0, st, p.rowptr, p.rowind,
                               p.colind, (const T *)p.vals, (uint32_t)nrows, (uint32_t)p.nnz, coff, cursor, m->colind, (T *)m->vals);
        hipLaunchKernelGGL(k_merge_advance, dim3(rgrid), dim3(256), 0, st, p.rowptr, (uint32_t)nrows, cursor);
        coff += (uint32_t)p.ncols;
    }
    if (hipStreamSynchronize(st) != hipSuccess || hipGetLastError() != hipSuccess) return fail_free("merged matrix build");
    (void)hipFree(cursor);
    cursor = nullptr;
    int rc = 0;
    if (!g->all_ones) rc = split_unit_pattern(*m, g->dtype, es, g->d_flags + 4, (uint32_t *)(g->d_flags + 5), st);
    if (!rc) rc = build_plans(*m, es, g->d_flags + 4, st, g->h);
    if (!rc) rc = narrow_values(*m, g->dtype, g->d_flags + 6, st);
    if (rc) {
        free_part(*m);
        return rc;
    }
    g->merged = std::move(m);
    return 0;
}

int build_merged(Group *g, size_t es, hipStream_t st) {
    switch (g->dtype) {
        case PYGIM_INT8: return build_merged_t<int8_t>(g, es, st);
        case PYGIM_INT16: return build_merged_t<int16_t>(g, es, st);
        case PYGIM_INT32: return build_merged_t<int32_t>(g, es, st);
        case PYGIM_INT64: return build_merged_t<int64_t>(g, es, st);
        case PYGIM_FLT32: return build_merged_t<float>(g, es, st);
        case PYGIM_DBL64: return build_merged_t<double>(g, es, st);
    }
    return 0;
}

// ---- host operands as a pipeline of feature windows (round 6, VERDICT r05 item 6) -------------------------------------------------------------------
// The reference driver's default call hands CPU tensors in and takes a CPU tensor back (spmm_test.py:29-35, spmm_default/pytorch_api.cpp:269-271): for the
// Reddit shape that is 238.6 MB up, a 2 ms product and 238.6 MB down -- 10.7 ms one after the other, 8.4 of them the two copies.  PCIe is full duplex
// and a product over a WINDOW of the features (columns [a, a + w) of X -> the same columns of C) needs nothing of the other windows and keeps every
// row's stored order of sums (FLT32 stays bit-identical to the one-piece product): window k + 1 goes up while window k is multiplied and window k - 1
// comes down.  Both ways are the DMA engines' 2-D copies (512-byte pieces at the row pitch: 55 GB/s up, as fast as a 1-D copy; from pageable memory the
// call blocks the host while the product and the download of the earlier windows run).  Two windows of 128 features: 10.5 -> 8.2 ms per call (7.7 with a
// page-locked X); four windows of 64: 8.9 (256-byte pieces move at 43 GB/s).  A copy KERNEL writing the result into the page-locked tensor (53 GB/s alone
// against the engines' 21-38 in the micro-benchmark) was built and lost: 9.0 ms -- its workgroups queue behind the product's, which own every compute unit.
// The result tensor must be page-locked (the wrappers allocate it so, pim_ops._new_out): a 2-D copy into pageable memory runs at 10 GB/s and blocks the
// host (12.9 ms), so such a call keeps the serial path.  scripts/micro/pcie_windows.hip, scripts/exp_host_call.py, profiles/r06_pcie_windows.txt.
// WHICH windows a call moves (HostWindow, HostPiece) and whether their products store directly is decided in run_plan.hpp (plan_host_pipeline), without a
// device; run_group_windows below only moves and multiplies them.

// the caller's page-locked result as the kernels see it (nullptr: pageable memory, or not mapped for this device)
static char *host_result_on_device(void *out) {
    hipPointerAttribute_t attr;
    void *dp = nullptr;
    const bool ok = hipPointerGetAttributes(&attr, out) == hipSuccess && attr.type == hipMemoryTypeHost && hipHostGetDevicePointer(&dp, out, 0) == hipSuccess;
    (void)hipGetLastError();
    return ok ? (char *)dp : nullptr;
}

// `out_dev` != nullptr: DIRECT mode -- every window's product is one pass of the LDS-staged kernel (lds_writes_c_once) and stores its rows straight into the
// caller's page-locked tensor: no staged C, no copy down; a window's stores drain over PCIe while the next window goes up (the kernel is over when they have
// landed).  Two compute streams taking the windows in turn were measured too (a second product beside the first one's draining stores): 9.1 against 8.9 ms.
static int run_group_windows(Group *g, Part &m, const std::vector<HostWindow> &pw, int64_t xrows, void *out, char *out_dev, size_t es, hipStream_t st,
                             double timers[3]) {
    const size_t npw = pw.size();
    // The two copy streams belong to the PROCESS (one pair per device, made at the first pipelined call and kept).  They get the two ends of the priority
    // range: hardware queues are pooled per priority class, so neither shares one with the caller's stream.  (Neither the pair's age nor its priorities
    // decide how fast the pitched downloads run -- profiles/r06_exp_host_call.txt; see host_direct in run_plan.hpp plan_host_pipeline.)
    {
        int dev = 0;
        HIP_TRY(hipGetDevice(&dev));
        std::lock_guard<std::mutex> lk(g_ctx.mu);
        auto &ps = g_ctx.pipe_streams[dev];
        if (!ps.first || !ps.second) {
            int least = 0, greatest = 0;
            HIP_TRY(hipDeviceGetStreamPriorityRange(&least, &greatest));
            if (!ps.first) HIP_TRY(hipStreamCreateWithPriority(&ps.first, hipStreamNonBlocking, greatest));
            if (!ps.second) HIP_TRY(hipStreamCreateWithPriority(&ps.second, hipStreamNonBlocking, least));
        }
        g->pipe_up = ps.first;
        g->pipe_down = ps.second;
    }
    while (g->pipe_ev.size() < 2 * npw) {
        hipEvent_t e = nullptr;
        HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        g->pipe_ev.push_back(e);
    }
    const double t0 = now_ms();
    const size_t cpitch = (size_t)g->h * es;
    const int64_t crows = g->total_rows;
    auto body = [&]() -> int {
        for (size_t k = 0; k < npw; k++) {
            const HostWindow &q = pw[k];
            char *dx = (char *)g->stage_in + q.dev_off;
            int64_t ldx = q.pitch_el;
            const size_t wb = (size_t)q.w * es, pitch = (size_t)q.pitch_el * es;
            if (!q.pieces.empty()) {
                dx = (char *)g->xcat + (size_t)q.acol * es;
                ldx = q.xcat_ld;
                for (const HostPiece &pc : q.pieces) {
                    if (xrows <= 0 || pc.w <= 0) continue;
                    char *blk = (char *)g->stage_in + pc.dev_off;
                    HIP_TRY(hipMemcpyAsync(blk, (const void *)pc.src, (size_t)xrows * (size_t)pc.pitch_el * es, hipMemcpyHostToDevice, g->pipe_up));
                    HIP_TRY(hipMemcpy2DAsync((char *)g->xcat + (size_t)pc.acol * es, (size_t)q.xcat_ld * es, blk, (size_t)pc.pitch_el * es, (size_t)pc.w * es, (size_t)xrows,
                                             hipMemcpyDeviceToDevice, g->pipe_up));
                }
            } else if (xrows > 0 && wb > 0) {
                if (wb == pitch) HIP_TRY(hipMemcpyAsync(dx, (const void *)q.src, wb * (size_t)xrows, hipMemcpyHostToDevice, g->pipe_up));
                else HIP_TRY(hipMemcpy2DAsync(dx, pitch, (const void *)q.src, pitch, wb, (size_t)xrows, hipMemcpyHostToDevice, g->pipe_up));
            }
            HIP_TRY(hipEventRecord(g->pipe_ev[2 * k], g->pipe_up));
            HIP_TRY(hipStreamWaitEvent(st, g->pipe_ev[2 * k], 0));
            char *dc = (out_dev ? out_dev : (char *)g->stage_out) + (size_t)q.acol * es;
            if (int rc = launch_block_any(g, m, dx, ldx, dc, g->h, q.w, /*accumulate=*/false, st)) return rc;
            HIP_TRY(hipEventRecord(g->pipe_ev[2 * k + 1], st));
            if (!out_dev) {
                HIP_TRY(hipStreamWaitEvent(g->pipe_down, g->pipe_ev[2 * k + 1], 0));
                if (crows > 0 && wb > 0)
                    HIP_TRY(hipMemcpy2DAsync((char *)out + (size_t)q.acol * es, cpitch, dc, cpitch, wb, (size_t)crows, hipMemcpyDeviceToHost, g->pipe_down));
            }
        }
        HIP_TRY(hipEventSynchronize(g->pipe_ev[2 * (npw - 1)]));
        timers[0] = now_ms() - t0;
        HIP_TRY(hipEventSynchronize(g->pipe_ev[2 * (npw - 1) + 1]));   // (direct mode: the last product's end is the end of its stores)
        timers[1] = now_ms() - t0 - timers[0];
        if (!out_dev) HIP_TRY(hipStreamSynchronize(g->pipe_down));
        timers[2] = now_ms() - t0 - timers[0] - timers[1];
        HIP_TRY(hipGetLastError());
        return 0;
    };
    const int rc = body();
    if (rc) {   // nothing of this call stays in flight behind an error
        (void)hipStreamSynchronize(g->pipe_up);
        (void)hipStreamSynchronize(st);
        (void)hipStreamSynchronize(g->pipe_down);
    }
    return rc;
}

// The tunables a call's plan reads (run_plan.hpp), copied in this one place.
static RunKnobs run_knobs() {
    RunKnobs k;
    k.host_windows = g_tune.host_windows; k.host_direct = g_tune.host_direct; k.fuse_windows = g_tune.fuse_windows; k.merge_parts = g_tune.merge_parts;
    return k;
}

// the dense operands of a call: none null, all in host or all in device memory, the output on the same side (each entry point has its own texts)
struct OperandTexts {
    const char *null_call, *null_one, *mixed, *sides;
};
static int check_dense_operands(const void *const *ops, size_t n, const void *out, const OperandTexts &t, bool *on_device) {
    if (!ops || !out) return fail(PYGIM_ERR_INVALID, t.null_call);
    for (size_t k = 0; k < n; k++)
        if (!ops[k]) return fail(PYGIM_ERR_INVALID, t.null_one);
    *on_device = is_device_ptr(ops[0]);
    for (size_t k = 1; k < n; k++)
        if (is_device_ptr(ops[k]) != *on_device) return fail(PYGIM_ERR_INVALID, t.mixed);
    if (*on_device != is_device_ptr(out)) return fail(PYGIM_ERR_INVALID, t.sides);
    return 0;
}

// Host operands as a pipeline of feature windows, where plan_host_pipeline finds one: asks the device what the plan needs to know, makes room for the
// gathered windows, runs the pipeline and hands its counts and times to the group.  *done: the call is over (else: the serial path).
static int run_host_pipeline(Group *g, const RunShape &s, const RunKnobs &knobs, const std::vector<RunWindow> &win, const std::vector<uintptr_t> &addr,
                             const std::vector<size_t> &off, void *out, hipStream_t st, bool *done) {
    *done = false;
    HostFacts f;
    f.has_merged = g->merged != nullptr;
    f.copies_slow = g->host_copies_slow;
    f.stage_out = (uintptr_t)g->stage_out;
    if (!host_pipeline_eligible(s, knobs, f.has_merged)) return 0;
    const HostFactsNeeded need = host_facts_needed(s, knobs, f.has_merged, f.copies_slow);
    if (need.out_pinned) {
        hipPointerAttribute_t attr;
        f.out_pinned = hipPointerGetAttributes(&attr, out) == hipSuccess && attr.type == hipMemoryTypeHost;
        (void)hipGetLastError();
    }
    if (need.out_alias) f.out_alias = (uintptr_t)host_result_on_device(out);
    Part &m = g->parts.size() == 1 ? g->parts[0] : *g->merged;
    const HostPlan plan = plan_host_pipeline(s, win.data(), addr.data(), off.data(), knobs, f,
                                             [&](int64_t w, uintptr_t c) { return lds_writes_c_once(g, m, (uint32_t)w, g->h, (const void *)c); });
    if (plan.xcat_bytes)
        if (int rc = ensure(&g->xcat, &g->xcat_bytes, plan.xcat_bytes)) return rc;
    if (plan.windows.empty()) return 0;
    double tm[3] = {0, 0, 0};
    if (int rc = run_group_windows(g, m, plan.windows, g->total_cols, out, plan.direct ? (char *)f.out_alias : nullptr, s.es, st, tm)) return rc;
    g->host_windows_used = (int64_t)plan.windows.size();
    g->host_direct_used = plan.direct ? 1 : 0;
    if (!plan.direct && host_download_was_slow(plan.windows.back().w, s.es, g->total_rows, tm[2])) g->host_copies_slow = true;
    g->timers[0] = tm[0];
    g->timers[1] = tm[1];
    g->timers[2] = tm[2];
    g->timers[3] = 0;
    *done = true;
    return 0;
}

// shared body of the three run_group flavours: what it does is planned in run_plan.hpp, without a device; here it is done.
//   windows[k]   : dense operand k (flattened over parts when per_part)
//   ld[k]        : its row stride in elements
//   per_part     : grande layout (each window holds only the rows of its own sparse part)
static int run_group_common(Group *g, const void *const *windows, const int64_t *ld, bool per_part, void *out, hipStream_t st) {
    // 1. checks and geometry
    std::vector<RunPart> parts(g->parts.size());
    for (size_t i = 0; i < parts.size(); i++) parts[i] = {g->parts[i].ncols, g->parts[i].dense_cols.data(), g->parts[i].dense_cols.size()};
    RunShape s;
    s.es = dtype_size(g->dtype);
    s.is_float = g->dtype == PYGIM_FLT32 || g->dtype == PYGIM_DBL64;
    s.h = g->h; s.total_rows = g->total_rows; s.total_cols = g->total_cols;
    s.parts = parts.data(); s.nparts = parts.size(); s.per_part = per_part;
    const size_t es = s.es, nwin = run_window_count(s);
    static const OperandTexts texts{"null dense operand or output", "null dense part", "dense parts mix host and device memory",
                                    "dense parts and output must both be host or both be device memory"};
    bool dev_in = false;
    if (int rc = check_dense_operands(windows, nwin, out, texts, &dev_in)) return rc;
    std::vector<RunWindow> win;
    if (const char *why = run_windows(s, ld, win)) return fail(PYGIM_ERR_INVALID, why);
    std::vector<uintptr_t> addr(nwin);
    for (size_t k = 0; k < nwin; k++) addr[k] = (uintptr_t)windows[k];
    const RunKnobs knobs = run_knobs();
    void *dout = out;
    double t_in = 0;
    // 2. host operands: the pipeline of feature windows where the plan finds one, else one copy up per window
    if (!dev_in) {
        const double t0 = now_ms();
        std::vector<size_t> off;
        if (int rc = ensure(&g->stage_in, &g->stage_in_bytes, host_stage_layout(win.data(), nwin, es, off))) return rc;
        if (int rc = ensure(&g->stage_out, &g->stage_out_bytes, std::max<size_t>((size_t)g->total_rows * g->h * es, 256))) return rc;
        g->host_windows_used = 1;
        g->host_direct_used = 0;
        bool done = false;
        if (int rc = run_host_pipeline(g, s, knobs, win, addr, off, out, st, &done)) return rc;
        if (done) return 0;
        for (size_t k = 0; k < nwin; k++) {
            addr[k] = (uintptr_t)g->stage_in + off[k];
            const size_t bytes = (size_t)win[k].rows * win[k].ld * es;
            if (bytes) HIP_TRY(hipMemcpyAsync((void *)addr[k], windows[k], bytes, hipMemcpyHostToDevice, st));
        }
        dout = g->stage_out;
        HIP_TRY(hipStreamSynchronize(st));
        t_in = now_ms() - t0;
    }
    const double t1 = now_ms();
    // 3. the block products: windows that are not side by side go into xcat first (the copies of a product, then the product)
    ProductPlan plan;
    plan_products(s, win.data(), addr.data(), knobs, g->merged != nullptr, plan);
    if (plan.xcat_bytes)
        if (int rc = ensure(&g->xcat, &g->xcat_bytes, plan.xcat_bytes)) return rc;
    for (const RunProduct &q : plan.products) {
        for (uint32_t c = q.copy0; c < q.copy1; c++) {
            const RunCopy &cp = plan.copies[c];
            if (cp.width > 0 && cp.rows > 0)
                HIP_TRY(hipMemcpy2DAsync((char *)g->xcat + cp.dst_off, (size_t)q.x.ldx * es, (const char *)addr[cp.win] + cp.src_off, (size_t)win[cp.win].ld * es,
                                         (size_t)cp.width * es, (size_t)cp.rows, hipMemcpyDeviceToDevice, st));
        }
        Part &p = q.part < 0 ? *g->merged : g->parts[(size_t)q.part];
        const void *x = q.x.in_place ? (const void *)q.x.base : g->xcat;
        if (int rc = launch_block_any(g, p, x, q.x.ldx, (char *)dout + (size_t)q.ccol * es, g->h, q.width, q.accumulate, st)) return rc;
    }
    // 4. host operands: the result comes down; the three phases' times
    if (!dev_in) {
        HIP_TRY(hipStreamSynchronize(st));
        const double t_k = now_ms() - t1, t2 = now_ms();
        const size_t bytes = (size_t)g->total_rows * g->h * es;
        if (bytes) HIP_TRY(hipMemcpyAsync(out, dout, bytes, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        g->timers[0] = t_in;
        g->timers[1] = t_k;
        g->timers[2] = now_ms() - t2;
        g->timers[3] = 0;
    }
    return 0;
}

// ---- the conv layers' quantiser (models/quantize.py:20-42) in three launches -------------------------
static bool flat4(const void *a, int64_t ld, uint64_t rows, uint32_t w, const void *b = nullptr) {
    return ld == (int64_t)w && (rows * w) % 4 == 0 && ((uintptr_t)a % 16) == 0 && ((uintptr_t)b % 16) == 0;
}
static int launch_absmax(const float *X, int64_t ldx, uint64_t rows, uint32_t w, uint32_t *amax, hipStream_t st) {
    const uint64_t total = rows * w;
    if (!total) return 0;
    const bool flat = flat4(X, ldx, rows, w);
    const uint64_t work = flat ? total / 4 : total;
    const unsigned grid = (unsigned)std::min<uint64_t>((work + 255) / 256, 2048);  // 8 blocks per CU, grid-stride loop
    if (flat) hipLaunchKernelGGL(k_absmax_bits<true>, dim3(grid), dim3(256), 0, st, X, ldx, rows, w, amax);
    else hipLaunchKernelGGL(k_absmax_bits<false>, dim3(grid), dim3(256), 0, st, X, ldx, rows, w, amax);
    HIP_TRY(hipGetLastError());
    return 0;
}
template <typename T>
static int launch_quantize(const float *X, int64_t ldx, uint64_t rows, uint32_t w, const uint32_t *amax, int log2_range, T *xq,
                           float *scale_out, hipStream_t st) {
    const uint64_t total = rows * w;
    if (!total) return 0;
    if (flat4(X, ldx, rows, w, xq))
        hipLaunchKernelGGL((k_quantize<T, true>), dim3((unsigned)((total / 4 + 255) / 256)), dim3(256), 0, st, X, ldx, rows, w, amax,
                           log2_range, xq, scale_out);
    else
        hipLaunchKernelGGL((k_quantize<T, false>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, X, ldx, rows, w, amax,
                           log2_range, xq, scale_out);
    HIP_TRY(hipGetLastError());
    return 0;
}
template <typename T>
static int launch_dequantize(const T *q, uint64_t n, const uint32_t *amax, int log2_range, float *out, hipStream_t st) {
    if (!n) return 0;
    if (n % 4 == 0 && ((uintptr_t)q % 16) == 0 && ((uintptr_t)out % 16) == 0)
        hipLaunchKernelGGL((k_dequantize<T, true>), dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, st, q, n, amax, log2_range, out);
    else
        hipLaunchKernelGGL((k_dequantize<T, false>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, q, n, amax, log2_range, out);
    HIP_TRY(hipGetLastError());
    return 0;
}
static int quant_log2_range(int dtype) {  // ranges of models/quantize.py:22-30
    switch (dtype) {
        case PYGIM_INT8: return 5;
        case PYGIM_INT16: return 10;
        case PYGIM_INT32: return 20;
        case PYGIM_FLT32: return 20;
        default: return -1;
    }
}

// Can the group's product run as ONE sweep that reads a caller-made slice-major copy and dequantises in its last
// store?  (unit weights, one matrix -- a single part or the merged one --, a panel plan without segment-kernel rows)
template <typename T>
static Part *fusable_part(Group *g) {
    if (!g->all_ones || !g_tune.fuse_windows || g_tune.panel_mode == 2 || g->h <= 4) return nullptr;
    Part *p = nullptr;
    if (g->parts.size() == 1) p = &g->parts[0];
    else if (g->merged && g_tune.merge_parts) p = g->merged.get();
    if (!p || p->vals || p->extra || !p->d_items || p->lp_panel.n_tasks > 0 || p->nrows == 0 || p->ncols == 0) return nullptr;
    if (!want_panel<T>(*p, (uint32_t)g->h, g->h)) return nullptr;
    constexpr uint32_t F = 128 / sizeof(T);
    const uint64_t nslices = ((uint64_t)g->h + F - 1) / F;
    if (((uint64_t)p->ncols * 128ull + 128ull) >= (1ull << 32)) return nullptr;  // the fused store rides the 32-bit gather modes
    if ((uint64_t)p->ncols * nslices * 128ull > (8ull << 30)) return nullptr;
    return p;
}

// the part whose LDS-staged plan can carry the conv layers' quantised aggregation with the dequantisation in its store
// (INT32 / FLT32 adjacency types; the per-column epilogue, if any, is applied in the same store)
// Its conditions on the plan and the tunables are RESTATED in tests/native/lds_launch_main.cpp (fusable_rest), where a sweep checks that what this gate
// accepts lds_plan_launch launches: change the two together.
template <typename T>
static Part *lds_fusable_part(Group *g) {
    if constexpr (!(std::is_same<T, float>::value || std::is_same<T, int32_t>::value || std::is_same<T, int8_t>::value || std::is_same<T, int16_t>::value)) return nullptr;
    if (!g->all_ones || g_tune.lds_mode == 2 || (int64_t)g->h / (sizeof(T) <= 2 ? 2 : 1) < g_tune.lds_min_width) return nullptr;
    if (g_tune.lds_mode == 0 && (g_tune.panel_mode != 0 || g_tune.csr_kernel != 0 || g_tune.force_vec_bytes != 0 || !g_tune.fuse_windows)) return nullptr;
    Part *p = nullptr;
    if (g->parts.size() == 1) p = &g->parts[0];
    else if (g->merged && g_tune.merge_parts) p = g->merged.get();
    if (!p || p->vals || p->extra || !p->lds_tiles || p->lds_wdelta || (p->lds_nw != 16 && !p->lds_is_code) || p->nrows == 0 || p->ncols == 0) return nullptr;
    if (p->lds_is_code && (!g_tune.lds_code || g_tune.lds_ablate)) return nullptr;
    // (column-split plans -- a rank's row share: the dequantisation happens where the ranges' partial sums meet, k_lds_reduce_deq / k_lds_reduce16, round 6)
    if (p->lds_half) return nullptr;   // (a half-split plan serves plain narrow products; the quantised aggregation of such a group keeps the sweep's fused path)
    if (p->lds_rows && sizeof(T) != 4) return nullptr;   // (the tail kernels are the 4-byte types'; never planned for the others)
    if (sizeof(T) <= 2 && (!p->lds_is_code || p->lds_nw != 8)) return nullptr;   // (INT8 / INT16: the 8-wave code stream's dequantising stores)
    return p;
}

static int launch_post(Group *g, float *out, hipStream_t st) {
    if (!g->post_mul) return 0;
    const uint64_t total = (uint64_t)g->total_rows * (uint64_t)g->h;
    if (total)
        hipLaunchKernelGGL(k_post_affine, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, out, (uint64_t)g->total_rows,
                           (uint32_t)g->h, g->post_mul, g->post_add, g->post_relu);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <typename T>
static int quant_run_t(Group *g, const float *X, int64_t ldx, float *out, float *scale_out, int log2_range, hipStream_t st) {
    const uint64_t rows = (uint64_t)g->total_cols, orows = (uint64_t)g->total_rows;
    const uint32_t h = (uint32_t)g->h;
    uint32_t *amax = (uint32_t *)(g->d_flags + 3);
    hipLaunchKernelGGL(k_zero_word, dim3(1), dim3(1), 0, st, amax);
    if (int rc = launch_absmax(X, ldx, rows, h, amax, st)) return rc;
    if (rows * h == 0 && scale_out) hipLaunchKernelGGL(k_zero_word, dim3(1), dim3(1), 0, st, (uint32_t *)scale_out);
    if constexpr (sizeof(T) == 4 || sizeof(T) <= 2) {
        if (Part *p = lds_fusable_part<T>(g)) {
            // FUSED on the LDS-staged kernel: the 256-byte-slice copy is written quantised from the float features, the kernel's
            // store dequantises (no quantised matrix, no integer result).  INT8 (the conv layers' own type, models/quantize.py:22-23):
            // the quantised values are staged as 16-bit numbers, 128 features to a slice, and summed by the INT16 stream
            using S = typename std::conditional<sizeof(T) == 1, int16_t, T>::type;
            const LdsStaged sg = lds_staged(sizeof(T), sizeof(T) == 1, h, (uint64_t)p->ncols, p->lds_kc, p->lds_half);   // (the copy launch_lds will read)
            const uint32_t nslices = sg.nslices;
            const uint64_t rows_pad = sg.rows_pad;
            void *xs = nullptr;
            {
                std::lock_guard<std::mutex> lk(g_ctx.mu);
                Context::XsBuf *b = nullptr;
                if (int rc = xs_buffer_locked(st, std::max<size_t>(sg.bytes, 256), &b)) return rc;
                b->src = nullptr;  // quantised values of a float matrix: never matched by x_unchanged
                xs = b->ptr;
            }
            XsPin pin;
            pin.hold(xs);
            const uint64_t threads = (uint64_t)p->ncols * nslices * 16;
            hipLaunchKernelGGL((k_slice_pack_quant<S, 16 / (int)sizeof(S), 4>), dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, X, ldx,
                               (uint32_t)p->ncols, h, nslices, amax, log2_range, (S *)xs, scale_out, (uint32_t)rows_pad);
            HIP_TRY(hipGetLastError());
            return launch_lds<T>(g, *p, (const T *)nullptr, (int64_t)h, (T *)out, (int64_t)h, h, false, st, xs, amax, log2_range);
        }
    }
    if (Part *p = fusable_part<T>(g)) {
        // FUSED: |max| reduction, then the slice-major copy is written quantised straight from the float features,
        // and every row's last panel item stores float(sum) * scale (no row-major quantised matrix, no integer result,
        // no separate quantise / dequantise passes)
        constexpr int VEC = 16 / (int)sizeof(T), LOG_LPR = 3;
        constexpr uint32_t F = VEC << LOG_LPR;
        const uint32_t nslices = (h + F - 1) / F;
        const size_t need = (size_t)p->ncols * nslices * F * sizeof(T);
        void *xs = nullptr;
        {
            std::lock_guard<std::mutex> lk(g_ctx.mu);
            Context::XsBuf *b = nullptr;
            if (int rc = xs_buffer_locked(st, std::max<size_t>(need, 256), &b)) return rc;
            b->src = nullptr;  // holds quantised values of a float matrix: never matched by x_unchanged
            xs = b->ptr;
        }
        XsPin pin;
        pin.hold(xs);
        const uint64_t threads = (uint64_t)p->ncols * nslices * (1u << LOG_LPR);
        hipLaunchKernelGGL((k_slice_pack_quant<T, VEC, LOG_LPR>), dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, X, ldx,
                           (uint32_t)p->ncols, h, nslices, amax, log2_range, (T *)xs, scale_out, (uint32_t)p->ncols);
        HIP_TRY(hipGetLastError());
        // running sums between panels (rows whose entries span several panels) live in the group's integer buffer
        if (int rc = ensure(&g->oq, &g->oq_bytes, std::max<size_t>(orows * h * sizeof(T), 256))) return rc;
        g->pre_xs = xs;
        g->deq_out = out;
        g->deq_ld = (int64_t)h;
        g->deq_amax = amax;
        g->deq_log2 = log2_range;
        g->packed_buf = nullptr;
        const int rc = launch_block_main(g, *p, xs /* unused: pre_xs */, (int64_t)h, g->oq, (int64_t)h, (int64_t)h, false, st);
        g->pre_xs = nullptr;
        g->deq_out = nullptr;
        return rc;
    }
    // unfused: quantise -> product -> dequantise as three steps
    if (int rc = ensure(&g->xq, &g->xq_bytes, std::max<size_t>(rows * h * sizeof(T), 256))) return rc;
    if (int rc = ensure(&g->oq, &g->oq_bytes, std::max<size_t>(orows * h * sizeof(T), 256))) return rc;
    if (int rc = launch_quantize<T>(X, ldx, rows, h, amax, log2_range, (T *)g->xq, scale_out, st)) return rc;
    // the group's own dense split, as windows into the row-major quantised matrix
    const size_t nd = g->parts[0].dense_cols.size();
    std::vector<const void *> win(nd);
    std::vector<int64_t> lds(nd, (int64_t)h);
    int64_t off = 0;
    for (size_t j = 0; j < nd; j++) {
        win[j] = (const char *)g->xq + (size_t)off * sizeof(T);
        off += g->parts[0].dense_cols[j];
    }
    if (int rc = run_group_common(g, win.data(), lds.data(), false, g->oq, st)) return rc;
    if (int rc = launch_dequantize<T>((const T *)g->oq, orows * h, amax, log2_range, out, st)) return rc;
    return launch_post(g, out, st);
}

// A . Xq on ALREADY quantised features with the dequantisation in the sweep's last store (row-sharded multi-GPU
// aggregation: the quantised blocks were exchanged between the ranks, pygim_amd/dist.py RowShardAdj)
template <typename T>
static int dequant_run_t(Group *g, const void *Xq, int64_t ldx, float *out, const uint32_t *amax, int log2_range, hipStream_t st) {
    const uint64_t orows = (uint64_t)g->total_rows;
    const uint32_t h = (uint32_t)g->h;
    if constexpr (sizeof(T) == 4 || sizeof(T) <= 2) {
        if (Part *pl = lds_fusable_part<T>(g))  // the LDS-staged kernel packs the quantised rows itself and dequantises in its store
            return launch_lds<T>(g, *pl, (const T *)Xq, ldx, (T *)out, (int64_t)h, h, false, st, nullptr, amax, log2_range);
    }
    if (int rc = ensure(&g->oq, &g->oq_bytes, std::max<size_t>(orows * h * sizeof(T), 256))) return rc;
    Part *p = fusable_part<T>(g);
    // the dequantising store rides the sweep's slice-major gather modes: whole 16-byte pieces (so that the copy is made from
    // rows that are never over-read) and not the narrow-row shortcut that gathers from the caller's row-major matrix
    constexpr uint32_t V = 16 / sizeof(T), F = V * 8;
    const bool narrow_rowmajor = (h + F - 1) / F == 1 && (size_t)ldx * sizeof(T) < 128;
    if (p && h % V == 0 && g_tune.panel_pack && !narrow_rowmajor) {
        g->deq_out = out;
        g->deq_ld = (int64_t)h;
        g->deq_amax = amax;
        g->deq_log2 = log2_range;
        const int rc = launch_block_any(g, *p, Xq, ldx, g->oq, (int64_t)h, (int64_t)h, false, st);
        g->deq_out = nullptr;
        return rc;
    }
    const size_t nd = g->parts[0].dense_cols.size();
    std::vector<const void *> win(nd);
    std::vector<int64_t> lds(nd, ldx);
    int64_t off = 0;
    for (size_t j = 0; j < nd; j++) {
        win[j] = (const char *)Xq + (size_t)off * sizeof(T);
        off += g->parts[0].dense_cols[j];
    }
    if (int rc = run_group_common(g, win.data(), lds.data(), false, g->oq, st)) return rc;
    return launch_dequantize<T>((const T *)g->oq, orows * h, amax, log2_range, out, st);
}
