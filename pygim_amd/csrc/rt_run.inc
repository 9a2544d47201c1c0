// rt_run.inc -- part of pygim_hip.hip (file scope): group assembly helpers (pattern + correction split, narrow values, merged parts), the shared body of the
// run_group entry points, the conv layers' quantiser around the product.
template <typename T>
static void launch_pack(const void *const *d_ptrs, uint32_t gcount, uint64_t n, void *out, hipStream_t st) {
    const uint64_t total = n * gcount;
    if (total == 0) return;
    hipLaunchKernelGGL((k_pack_vectors<T>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st,
                       (const T *const *)d_ptrs, gcount, n, (T *)out);
}


// shared body of the three run_group flavours.
//   windows[k]   : dense operand k (flattened over parts when per_part)
//   ld[k]        : its row stride in elements
//   per_part     : grande layout (each window holds only the rows of its own sparse part)
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
struct HostPiece {       // one of the caller's narrow feature blocks inside a window (grande's per-unit windows, ds_parts blocks of a few bytes per row)
    const char *src;      // host: [rows x pitch_el], contiguous
    int64_t pitch_el, w;  // its row stride and true width, elements
    size_t dev_off;       // where the block lands in stage_in (as it is: one 1-D copy)
    int64_t acol;         // its first column in C (and in the assembled X)
};
struct HostWindow {
    const char *src;      // host
    int64_t pitch_el;     // host and device row stride of this window's block, elements
    size_t dev_off;       // byte offset of the window's first element in stage_in
    int64_t acol, w;      // columns [acol, acol + w) of C
    // a window ASSEMBLED from several of the caller's blocks: each goes up as it is and is laid into its columns of Group::xcat (row stride xcat_ld elements)
    // on the device; the product then reads xcat
    std::vector<HostPiece> pieces;
    int64_t xcat_ld = 0;
};

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
    // decide how fast the pitched downloads run -- profiles/r06_exp_host_call.txt; see host_direct in run_group_common.)
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
                    HIP_TRY(hipMemcpyAsync(blk, pc.src, (size_t)xrows * (size_t)pc.pitch_el * es, hipMemcpyHostToDevice, g->pipe_up));
                    HIP_TRY(hipMemcpy2DAsync((char *)g->xcat + (size_t)pc.acol * es, (size_t)q.xcat_ld * es, blk, (size_t)pc.pitch_el * es, (size_t)pc.w * es, (size_t)xrows,
                                             hipMemcpyDeviceToDevice, g->pipe_up));
                }
            } else if (xrows > 0 && wb > 0) {
                if (wb == pitch) HIP_TRY(hipMemcpyAsync(dx, q.src, wb * (size_t)xrows, hipMemcpyHostToDevice, g->pipe_up));
                else HIP_TRY(hipMemcpy2DAsync(dx, pitch, q.src, pitch, wb, (size_t)xrows, hipMemcpyHostToDevice, g->pipe_up));
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

static int run_group_common(Group *g, const void *const *windows, const int64_t *ld, bool per_part, void *out,
                            hipStream_t st) {
    const size_t es = dtype_size(g->dtype);
    size_t nwin = 0;
    if (per_part)
        for (auto &p : g->parts) nwin += p.dense_cols.size();
    else
        nwin = g->parts[0].dense_cols.size();
    if (!windows || !out) return fail(PYGIM_ERR_INVALID, "null dense operand or output");
    for (size_t k = 0; k < nwin; k++)
        if (!windows[k]) return fail(PYGIM_ERR_INVALID, "null dense part");
    const bool dev_out = is_device_ptr(out);
    bool dev_in = is_device_ptr(windows[0]);
    for (size_t k = 1; k < nwin; k++)
        if (is_device_ptr(windows[k]) != dev_in) return fail(PYGIM_ERR_INVALID, "dense parts mix host and device memory");
    if (dev_in != dev_out) return fail(PYGIM_ERR_INVALID, "dense parts and output must both be host or both be device memory");

    // window geometry
    std::vector<int64_t> rows(nwin), lds(nwin), widths(nwin);
    {
        size_t k = 0;
        if (per_part) {
            for (auto &p : g->parts)
                for (size_t j = 0; j < p.dense_cols.size(); j++, k++) {
                    rows[k] = p.ncols;
                    widths[k] = p.dense_cols[j];
                    lds[k] = ld ? ld[k] : p.dense_cols[j];
                    if (lds[k] < widths[k]) return fail(PYGIM_ERR_INVALID, "window stride smaller than its width");
                }
        } else {
            for (size_t j = 0; j < nwin; j++) {
                rows[j] = g->total_cols;
                widths[j] = g->parts[0].dense_cols[j];
                lds[j] = ld ? ld[j] : widths[j];
            }
        }
    }
    std::vector<const void *> dwin(nwin);
    void *dout = out;
    double t_in = 0, t_k = 0, t_out = 0;
    if (!dev_in) {
        const double t0 = now_ms();
        size_t total = 0;
        std::vector<size_t> off(nwin);
        for (size_t k = 0; k < nwin; k++) {
            off[k] = total;
            total += (((size_t)rows[k] * lds[k] * es) + 255) & ~(size_t)255;
        }
        if (int rc = ensure(&g->stage_in, &g->stage_in_bytes, std::max<size_t>(total, 256))) return rc;
        if (int rc = ensure(&g->stage_out, &g->stage_out_bytes, std::max<size_t>((size_t)g->total_rows * g->h * es, 256))) return rc;
        // the pipeline of feature windows (above): one sparse operand (a single part, or the merged matrix), windows that are column ranges of C
        g->host_windows_used = 1;
        g->host_direct_used = 0;
        if (g_tune.host_windows != 1 && g->h > 0 && (g->parts.size() == 1 || (!per_part && g->merged && g_tune.merge_parts))) {   // (per-part windows of ONE part: grande)
            Part &m = g->parts.size() == 1 ? g->parts[0] : *g->merged;
            std::vector<HostWindow> pw;
            const size_t xbytes = (size_t)g->total_cols * g->h * es, cbytes = (size_t)g->total_rows * g->h * es;
            bool automatic = xbytes >= ((size_t)32 << 20) && cbytes >= ((size_t)32 << 20);
            if (automatic && g_tune.host_windows == 0) {   // (a pitched copy into pageable memory is slower than the serial call)
                hipPointerAttribute_t attr;
                automatic = hipPointerGetAttributes(&attr, out) == hipSuccess && attr.type == hipMemoryTypeHost;
                (void)hipGetLastError();
            }
            // DIRECT mode (tunable host_direct): the products store straight into the caller's page-locked tensor -- decided on the full width here, checked
            // window by window below.  1 = adaptive: the copies first (8.2 ms per call when the DMA engines move the result's windows at the link rate); a call
            // whose last download ran below 40 GB/s -- the runtime's pitched copies to the host run at 55, 34 or 21 GB/s depending on what the process allocated
            // and freed before (its DMA-engine bookkeeping; scripts/micro/rect_lottery.hip: the same buffers, the same stream, 34 -> 21 GB/s after the device heap
            // was churned): the same call then takes 11.8 ms -- turns this group to the direct mode (8.9 ms, whatever the engines do) for its later calls.  2 = always.
            const int64_t slice_el = std::max<int64_t>(1, 256 / (int64_t)es);
            char *out_dev = (g_tune.host_direct == 2 || (g_tune.host_direct == 1 && g->host_copies_slow)) ? host_result_on_device(out) : nullptr;
            if (out_dev && ((((uintptr_t)out_dev) & 255) || (((size_t)g->h * es) & 15) ||
                            !lds_writes_c_once(g, m, (uint32_t)g->h, g->h, out_dev)))
                out_dev = nullptr;
            // the windows: once for the direct mode, again for the copies if a window's product turns out not to be the one-pass LDS-staged kernel
            for (int attempt = out_dev ? 0 : 1; attempt < 2; attempt++) {
                pw.clear();
                if (attempt == 1) out_dev = nullptr;
                if (nwin == 1 && lds[0] >= widths[0] && widths[0] == g->h) {
                    // one row-major X: cut into windows of whole 256-byte slices (64 lanes of the LDS-staged product), the wider ones first.  Automatic: 512 bytes
                    // of a row per window (the DMA engines move such pieces at the 1-D rate; four windows of 256 bytes: 8.8 ms with the copies, 10.2 direct)
                    const int64_t S = (g->h + slice_el - 1) / slice_el;
                    const int64_t auto_bytes = 512;
                    int64_t n = g_tune.host_windows > 1 ? g_tune.host_windows : (automatic ? ((int64_t)g->h * (int64_t)es + auto_bytes - 1) / auto_bytes : 1);
                    n = std::min<int64_t>(std::min<int64_t>(n, 16), S);
                    if (n > 1) {
                        int64_t a = 0;
                        for (int64_t k = 0; k < n && a < g->h; k++) {
                            const int64_t w = std::min<int64_t>((S / n + (k < S % n ? 1 : 0)) * slice_el, g->h - a);
                            pw.push_back({(const char *)windows[0] + (size_t)a * es, lds[0], (size_t)a * es, a, w, {}, 0});
                            a += w;
                        }
                    }
                } else if (nwin > 1 && (g_tune.host_windows > 1 || automatic)) {
                    // the caller's own feature blocks (ds_parts; grande's per-unit windows, grande.py:12-23: blocks of `pad` columns of which the first
                    // widths[k] count): blocks of 512 bytes of a row and more are windows as they are; narrower ones (eight units: 32 floats each) are gathered
                    // into windows of that size -- each block goes up in one piece and is laid into its columns of xcat on the device
                    int64_t hsum = 0;
                    bool narrow = false;
                    for (size_t k = 0; k < nwin; k++) {
                        hsum += widths[k];
                        narrow = narrow || (size_t)widths[k] * es < 512 || lds[k] != widths[k];
                    }
                    if (hsum == g->h && !narrow && nwin <= 16) {
                        int64_t a = 0;
                        for (size_t k = 0; k < nwin; k++) {
                            pw.push_back({(const char *)windows[k], lds[k], off[k], a, widths[k], {}, 0});
                            a += widths[k];
                        }
                    } else if (hsum == g->h) {
                        const int64_t ldc_el = (int64_t)((((size_t)g->h * es + 15) & ~(size_t)15) / es);
                        if (int rc = ensure(&g->xcat, &g->xcat_bytes, std::max<size_t>((size_t)g->total_cols * ldc_el * es, 256))) return rc;
                        const int64_t target = g_tune.host_windows > 1 ? (g->h + g_tune.host_windows - 1) / g_tune.host_windows : std::max<int64_t>(1, 512 / (int64_t)es);
                        int64_t a = 0;
                        HostWindow cur{nullptr, 0, 0, 0, 0, {}, ldc_el};
                        for (size_t k = 0; k < nwin; k++) {
                            cur.pieces.push_back({(const char *)windows[k], lds[k], widths[k], off[k], a});
                            cur.w += widths[k];
                            a += widths[k];
                            if (cur.w >= target || k + 1 == nwin) {
                                pw.push_back(cur);
                                cur = HostWindow{nullptr, 0, 0, a, 0, {}, ldc_el};
                            }
                        }
                        if (pw.size() > 16) pw.clear();
                    }
                }
                bool direct_ok = out_dev != nullptr;
                for (const HostWindow &q : pw)
                    if (direct_ok && ((((size_t)q.acol * es) & 15) || !lds_writes_c_once(g, m, (uint32_t)q.w, g->h, out_dev + (size_t)q.acol * es))) direct_ok = false;
                if (direct_ok || attempt == 1) break;
            }
            // FLOAT sums on the L2 sweep depend on the product's width (how many lanes share a long row's entries): a window's product would be inside the norm-wise
            // contract but not the serial call's bits.  Left to itself the library pipelines a float product only where every window is the LDS-staged kernel's
            // (stored-order sums, or the plan's fixed column ranges: the same bits at any width); host_windows > 1 asks for the windows whatever the kernels.
            if (g_tune.host_windows == 0 && (g->dtype == PYGIM_FLT32 || g->dtype == PYGIM_DBL64))
                for (const HostWindow &q : pw)
                    if (!lds_writes_c_once(g, m, (uint32_t)q.w, g->h, (char *)g->stage_out + (size_t)q.acol * es)) {
                        pw.clear();
                        break;
                    }
            if (pw.size() > 1) {
                double tm[3] = {0, 0, 0};
                if (int rc = run_group_windows(g, m, pw, g->total_cols, out, out_dev, es, st, tm)) return rc;
                g->host_windows_used = (int64_t)pw.size();
                g->host_direct_used = out_dev ? 1 : 0;
                if (!out_dev && pw.back().w > 0 && g->total_rows > 0) {   // (the last window's download, alone on the link: bytes per ms = MB/s x 1e-3)
                    const double mb = (double)pw.back().w * (double)es * (double)g->total_rows * 1e-6;
                    if (mb >= 16 && tm[2] > 0 && mb / tm[2] < 40.0) g->host_copies_slow = true;
                }
                g->timers[0] = tm[0];
                g->timers[1] = tm[1];
                g->timers[2] = tm[2];
                g->timers[3] = 0;
                return 0;
            }
        }
        for (size_t k = 0; k < nwin; k++) {
            dwin[k] = (char *)g->stage_in + off[k];
            const size_t bytes = (size_t)rows[k] * lds[k] * es;
            if (bytes) HIP_TRY(hipMemcpyAsync((void *)dwin[k], windows[k], bytes, hipMemcpyHostToDevice, st));
        }
        dout = g->stage_out;
        HIP_TRY(hipStreamSynchronize(st));
        t_in = now_ms() - t0;
    } else {
        for (size_t k = 0; k < nwin; k++) dwin[k] = windows[k];
    }
    const double t1 = now_ms();
    // block products: sum over sparse parts, concatenate over dense parts
    if (g->merged && g_tune.merge_parts && g->parts.size() > 1) {
        // ... as ONE product with the merged matrix (Group::merged)
        Part &m = *g->merged;
        const size_t nd0 = g->parts[0].dense_cols.size();
        bool in_place = !per_part;  // one window, or windows that sit side by side in one row-major matrix
        for (size_t j = 1; in_place && j < nd0; j++)
            in_place = lds[j] == lds[0] && (const char *)dwin[j] == (const char *)dwin[j - 1] + (size_t)widths[j - 1] * es;
        const char *x = nullptr;
        int64_t ldx = 0;
        if (in_place) {
            x = (const char *)dwin[0];
            ldx = lds[0];
        } else {
            // lay the windows side by side (and, for per-part windows, the parts' row ranges one below the other)
            const int64_t ldc_el = (int64_t)((((size_t)g->h * es + 15) & ~(size_t)15) / es);
            const size_t need = (size_t)g->total_cols * ldc_el * es;
            if (int rc = ensure(&g->xcat, &g->xcat_bytes, std::max<size_t>(need, 256))) return rc;
            int64_t brow = 0;
            size_t kbase = 0;
            for (size_t i = 0; i < g->parts.size(); i++) {
                Part &p = g->parts[i];
                int64_t a = 0;
                for (size_t j = 0; j < p.dense_cols.size(); j++) {
                    const size_t k = per_part ? kbase + j : j;
                    const char *src = (const char *)dwin[k] + (per_part ? 0 : (size_t)brow * lds[k] * es);
                    if (widths[k] > 0 && p.ncols > 0)
                        HIP_TRY(hipMemcpy2DAsync((char *)g->xcat + ((size_t)brow * ldc_el + (size_t)a) * es, (size_t)ldc_el * es, src,
                                                 (size_t)lds[k] * es, (size_t)widths[k] * es, (size_t)p.ncols,
                                                 hipMemcpyDeviceToDevice, st));
                    a += widths[k];
                }
                brow += p.ncols;
                kbase += p.dense_cols.size();
            }
            x = (const char *)g->xcat;
            ldx = ldc_el;
        }
        if (int rc = launch_block_any(g, m, x, ldx, dout, g->h, g->h, /*accumulate=*/false, st)) return rc;
    } else {
    int64_t brow = 0;
    size_t kbase = 0;
    for (size_t i = 0; i < g->parts.size(); i++) {
        Part &p = g->parts[i];
        int64_t acol = 0;
        const size_t nd = p.dense_cols.size();
        // Several dense windows (ds_parts chunks, grande's per-unit feature windows) are one product of the
        // full width here: a window is an artefact of the reference's DPU layout, and narrow windows
        // (32 int8 = 32 bytes) would waste the 128-byte gather.  Windows that already sit side by side in
        // one row-major matrix are used in place; others are laid side by side first (one 2-D copy each).
        if (nd > 1 && g_tune.fuse_windows) {
            const size_t k0 = per_part ? kbase : 0;
            int64_t wsum = 0;
            bool adjacent = true;
            for (size_t j = 0; j < nd; j++) {
                if (j > 0 && (lds[k0 + j] != lds[k0] ||
                              (const char *)dwin[k0 + j] != (const char *)dwin[k0 + j - 1] + (size_t)widths[k0 + j - 1] * es))
                    adjacent = false;
                wsum += widths[k0 + j];
            }
            const char *x = nullptr;
            int64_t ldx = 0;
            if (adjacent) {
                x = (const char *)dwin[k0] + (per_part ? 0 : (size_t)brow * lds[k0] * es);
                ldx = lds[k0];
            } else {
                // row stride rounded up to 16 bytes so that the sweep's 16-byte pieces stay available
                const int64_t ldc_el = (int64_t)((((size_t)wsum * es + 15) & ~(size_t)15) / es);
                const size_t need = (size_t)p.ncols * ldc_el * es;
                if (int rc = ensure(&g->xcat, &g->xcat_bytes, std::max<size_t>(need, 256))) return rc;
                int64_t a = 0;
                for (size_t j = 0; j < nd; j++) {
                    const size_t k = k0 + j;
                    const char *src = (const char *)dwin[k] + (per_part ? 0 : (size_t)brow * lds[k] * es);
                    if (widths[k] > 0 && p.ncols > 0)
                        HIP_TRY(hipMemcpy2DAsync((char *)g->xcat + (size_t)a * es, (size_t)ldc_el * es, src, (size_t)lds[k] * es,
                                                 (size_t)widths[k] * es, (size_t)p.ncols, hipMemcpyDeviceToDevice, st));
                    a += widths[k];
                }
                x = (const char *)g->xcat;
                ldx = ldc_el;
            }
            if (int rc = launch_block_any(g, p, x, ldx, dout, g->h, wsum, /*accumulate=*/i > 0, st)) return rc;
        } else
        for (size_t j = 0; j < nd; j++) {
            const size_t k = per_part ? kbase + j : j;
            const int64_t w = widths[k];
            const char *x = (const char *)dwin[k] + (per_part ? 0 : (size_t)brow * lds[k] * es);
            char *c = (char *)dout + (size_t)acol * es;
            if (int rc = launch_block_any(g, p, x, lds[k], c, g->h, w, /*accumulate=*/i > 0, st)) return rc;
            acol += w;
        }
        brow += p.ncols;
        kbase += p.dense_cols.size();
    }
    }
    if (!dev_in) {
        HIP_TRY(hipStreamSynchronize(st));
        t_k = now_ms() - t1;
        const double t2 = now_ms();
        const size_t bytes = (size_t)g->total_rows * g->h * es;
        if (bytes) HIP_TRY(hipMemcpyAsync(out, dout, bytes, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        t_out = now_ms() - t2;
        g->timers[0] = t_in;
        g->timers[1] = t_k;
        g->timers[2] = t_out;
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
