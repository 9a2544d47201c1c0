// rt_launch.inc -- part of pygim_hip.hip (inside its anonymous namespace): one block product -> kernels.  The sweep (launch_block_t), the LDS-staged
// product in its token and code-stream forms (launch_lds, want_lds), the dispatch by element type.
// ---------------------------------------------------------------------------
// launch plan for one block product
// ---------------------------------------------------------------------------
int pick_vec_bytes(size_t es, const void *X, int64_t ldx, const void *C, int64_t ldc) {
    // widest of {16, 8, element} bytes that every row start of X and C is aligned to
    auto ok = [&](size_t vb) {
        return ((uintptr_t)X % vb == 0) && ((uintptr_t)C % vb == 0) && ((size_t)ldx * es % vb == 0) &&
               ((size_t)ldc * es % vb == 0);
    };
    size_t cap = g_tune.force_vec_bytes > 0 ? (size_t)g_tune.force_vec_bytes : 16;
    for (size_t vb : {(size_t)16, (size_t)8})
        if (vb <= cap && vb > es && ok(vb)) return (int)vb;
    return (int)es;
}

struct KernelTimer {
    Group *g;
    hipStream_t st;
    hipEvent_t a = nullptr, b = nullptr;
    KernelTimer(Group *g_, hipStream_t st_, bool on = true) : g(g_), st(st_) {
        if (on && (g_tune.kernel_events || g->kernel_events) && hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess)
            (void)hipEventRecord(a, st);
        else
            a = b = nullptr;
    }
    void stop() {
        if (!a) return;
        (void)hipEventRecord(b, st);
        g->ev_pending.emplace_back(a, b);
        a = b = nullptr;
    }
};

// Does this block product take the panel sweep?  (16-byte pieces at any alignment and any width; narrow or ragged rows
// whose tail piece would reach past the row stride gather from the padded slice-major copy, which is skipped when
// that copy would be enormous.)
template <typename T>
bool want_panel(const Part &p, uint32_t w, int64_t ldx) {
    if (p.d_items == nullptr || g_tune.panel_mode == 2 || p.nrows == 0 || w == 0) return false;
    if (g_tune.panel_mode == 0 && !(p.npanels == 1 || (double)p.nnz / ((double)p.nrows * p.npanels) >= (double)g_tune.panel_min_seg))
        return false;
    constexpr uint32_t V = 16 / sizeof(T), F = V * 8;
    const uint32_t nslices = (w + F - 1) / F;
    const bool tail_inside = (w % V) == 0;  // no partial 16-byte piece: nothing is read past a row's width
    (void)ldx;
    if (!tail_inside && (uint64_t)p.ncols * nslices * 128ull > (8ull << 30)) return false;
    return true;
}

// element types of the conv layers' quantiser (models/quantize.py:22-30): the fused store exists for these
template <typename T> struct DeqType { static constexpr bool ok = false; };
template <> struct DeqType<int8_t> { static constexpr bool ok = true; };
template <> struct DeqType<int16_t> { static constexpr bool ok = true; };
template <> struct DeqType<int32_t> { static constexpr bool ok = true; };
template <> struct DeqType<float> { static constexpr bool ok = true; };

template <typename T, int VEC>
int launch_block_t(Group *g, Part &p, const T *X, int64_t ldx, T *C, int64_t ldc, uint32_t w, bool accumulate,
                   hipStream_t st) {
    const T *vals = (const T *)p.vals;
    const uint32_t nrows = (uint32_t)p.nrows;
    const uint32_t lanes_needed = (w + VEC - 1) / VEC;
    // L2-blocked panel sweep or row-per-wave kernels?
    bool use_panel = false;
    if constexpr (VEC * sizeof(T) == 16) use_panel = want_panel<T>(p, w, ldx);
    // COO groups: the panel sweep (through the row pointers derived at create time) when it pays,
    // else the native equal-nnz kernel
    const bool coo_native = (g->format == PYGIM_COO) && p.rowind != nullptr && !use_panel && !g_tune.coo_via_rowptr && lanes_needed > 16;
    if (coo_native) {
        // nnz-split kernel + carry fix-up
        if (!accumulate && (uint64_t)nrows * w > 0)
            hipLaunchKernelGGL((k_zero_rows<T>), dim3((unsigned)(((uint64_t)nrows * w + 255) / 256)), dim3(256), 0, st, C, ldc,
                               (uint64_t)nrows, w);
        if (p.nnz == 0) return 0;
        const uint32_t chunk = (uint32_t)g_tune.coo_chunk;
        const uint32_t nchunks = (uint32_t)((p.nnz + chunk - 1) / chunk);
        const size_t need = (size_t)nchunks * 2 * w * sizeof(T);
        if (int rc = ensure(&g->scratch, &g->scratch_bytes, need)) return rc;
        dim3 grid((nchunks + 3) / 4, (lanes_needed + 63) / 64);
        KernelTimer kt(g, st, !p.is_extra || p.timed);
        hipLaunchKernelGGL((k_coo_wide<T, VEC>), grid, dim3(256), 0, st, p.rowind, p.colind, vals,
                           (uint32_t)p.nnz, chunk, X, ldx, C, ldc, w, (T *)g->scratch, accumulate ? 1 : 0);
        kt.stop();
        hipLaunchKernelGGL((k_coo_fixup<T>), dim3((nchunks + 3) / 4), dim3(256), 0, st, p.rowind,
                           (uint32_t)p.nnz, chunk, nchunks, (const T *)g->scratch, C, ldc, w, accumulate ? 1 : 0);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    const LongPlan &lp = use_panel ? p.lp_panel : p.lp_base;
    // long rows: fixed-size segments on a forked stream, so that their few, long-running waves
    // overlap the main sweep instead of trailing it
    bool forked = false;
    if (lp.n_tasks > 0) {
        const size_t need = (size_t)lp.n_tasks * w * sizeof(T);
        if (int rc = ensure(&g->scratch, &g->scratch_bytes, need)) return rc;
        HIP_TRY(hipEventRecord(g->ev_fork, st));
        HIP_TRY(hipStreamWaitEvent(g->side, g->ev_fork, 0));
        dim3 grid((lp.n_tasks + 3) / 4, (lanes_needed + 63) / 64);
        hipLaunchKernelGGL((k_long_segments<T, VEC>), grid, dim3(256), 0, g->side, lp.d_tasks, lp.n_tasks, p.colind,
                           vals, X, ldx, (T *)g->scratch, w);
        hipLaunchKernelGGL((k_long_reduce<T>), dim3((w + 255) / 256, lp.n_long), dim3(256), 0, g->side, lp.d_desc,
                           lp.n_long, (const T *)g->scratch, C, ldc, w, accumulate ? 1 : 0);
        HIP_TRY(hipEventRecord(g->ev_join, g->side));
        forked = true;
    }
    auto join = [&]() -> int {
        if (forked) HIP_TRY(hipStreamWaitEvent(st, g->ev_join, 0));
        HIP_TRY(hipGetLastError());
        return 0;
    };
    // L2-blocked panel sweep (fast path for wide feature rows; see k_csr_panel)
    if constexpr (VEC * sizeof(T) == 16) {
        if (use_panel) {
            constexpr int LOG_LPR = 3;
            constexpr uint32_t F = VEC << LOG_LPR;            // elements per 128-byte slice
            const uint32_t nslices = (w + F - 1) / F;
            const uint32_t bthreads = (g_tune.panel_block == 64 || g_tune.panel_block == 128) ? (uint32_t)g_tune.panel_block : 256u;
            const uint32_t bwaves = bthreads >> 6;
            const uint32_t rows_per_block = bwaves * (64 >> LOG_LPR);
            // gather source: slice-major copy (default) or the caller's row-major X
            const T *Xg = X;
            int64_t ldg = ldx, slice_stride = F;
            KernelTimer kt(g, st, !p.is_extra || p.timed);
            XsPin pin;
            // (rows of one slice that are already contiguous lines need no copy -- as long as no 16-byte piece is
            // partial: X may be a window that ends at the end of an allocation (pygim_block_run on x + f0), so a
            // piece over a ragged tail must never be read from the caller's matrix; those go to the padded copy)
            const bool tail_inside = (w % VEC) == 0;
            if (g->pre_xs) {
                // the caller packed (and quantised) the features slice-major on this stream already
                Xg = (const T *)g->pre_xs;
                ldg = F;
                slice_stride = (int64_t)p.ncols * F;
            } else if (((g_tune.panel_pack && !p.no_pack) || !tail_inside) && !(nslices == 1 && (size_t)ldx * sizeof(T) <= 128 && tail_inside)) {
                const size_t need = (size_t)p.ncols * nslices * F * sizeof(T);
                void *xs_use = nullptr;
                if (p.is_extra && g->packed_buf && g->packed_src == (const void *)X && g->packed_ld == ldx &&
                    g->packed_w == (int64_t)w) {
                    xs_use = g->packed_buf;  // the pattern product of this very call packed it on this stream
                } else {
                    std::lock_guard<std::mutex> lk(g_ctx.mu);
                    if (g->x_unchanged) {
                        // the most recent copy of exactly this operand on this device, whichever stream made it
                        int dev = 0;
                        (void)hipGetDevice(&dev);
                        Context::XsBuf *hit = nullptr;
                        for (auto &kv : g_ctx.xs_bufs) {
                            Context::XsBuf &b = kv.second;
                            if (kv.first.first == dev && b.ptr && b.src == (const void *)X && b.ld == ldx && b.rows == p.ncols &&
                                b.w == (int64_t)w && b.es == sizeof(T) && b.kind == 0 && (!hit || b.stamp > hit->stamp))
                                hit = &b;
                        }
                        if (hit) {
                            hit->stamp = ++g_ctx.xs_clock;
                            hit->in_use++;
                            xs_use = hit->ptr;
                            pin.hold(xs_use);
                        }
                    }
                    if (!xs_use) {
                        Context::XsBuf *b = nullptr;
                        if (int rc = xs_buffer_locked(st, std::max<size_t>(need, 256), &b)) return rc;
                        xs_use = b->ptr;
                        pin.hold(xs_use);
                        b->src = X;
                        b->ld = ldx;
                        b->rows = p.ncols;
                        b->w = (int64_t)w;
                        b->es = sizeof(T);
                        b->kind = 0;
                        b->order = nullptr;
                        const uint64_t threads = (uint64_t)p.ncols * nslices * (1u << LOG_LPR);
                        if (threads > 0)
                            hipLaunchKernelGGL((k_slice_pack<T, VEC, LOG_LPR>), dim3((unsigned)((threads + 255) / 256)),
                                               dim3(256), 0, st, X, ldx, (uint32_t)p.ncols, w, nslices, (T *)xs_use, (uint32_t)p.ncols);
                    }
                }
                g->packed_src = X;
                g->packed_buf = xs_use;
                g->packed_ld = ldx;
                g->packed_w = (int64_t)w;
                Xg = (const T *)xs_use;
                ldg = F;
                slice_stride = (int64_t)p.ncols * F;
            }
            // 32-bit gather offsets when every gathered byte of a slice sits below 4 GiB of its base
            const bool off32 = ((uint64_t)p.ncols * (uint64_t)ldg + F) * sizeof(T) < (1ull << 32);
            // X far beyond the Infinity Cache (256 MiB): sweep a few slices per launch, every XCD on the same
            // slice(s), so that the gather footprint of a launch is ncols * 128 B * group instead of all of X
            uint32_t sgroup = nslices;
            if (g_tune.slice_group_bytes > 0) {
                const uint64_t per_slice = (uint64_t)p.ncols * F * sizeof(T);
                if (per_slice * nslices > (uint64_t)g_tune.slice_group_bytes)
                    sgroup = (uint32_t)std::max<uint64_t>(1, (uint64_t)g_tune.slice_group_bytes / std::max<uint64_t>(per_slice, 1));
                sgroup = std::min(sgroup, nslices);
            }
            for (uint32_t s0 = 0; s0 < nslices; s0 += sgroup) {
            const uint32_t ns = std::min(sgroup, nslices - s0);
            const T *Xs0 = Xg + (int64_t)s0 * slice_stride;
            T *Cs0 = C + (size_t)s0 * F;
            const uint32_t ws = std::min<uint32_t>(w - s0 * F, ns * F);
            for (uint32_t q = 0; q < p.npanels; q++) {
                const size_t o = p.panel_off[q];
                const uint32_t cnt = (uint32_t)(p.panel_off[q + 1] - o);
                if (cnt == 0) continue;
                const uint32_t ncoop = p.panel_coop[q], nnorm = cnt - ncoop;
                const uint32_t row_blocks = (nnorm + rows_per_block - 1) / rows_per_block;
                const uint32_t coop_blocks = (ncoop + bwaves - 1) / bwaves;  // one wave per long item
                const uint32_t coop_grid = ncoop ? 8u * ns * ((coop_blocks + 7) / 8) : 0u;
                const uint32_t norm_grid = nnorm ? 8u * ns * ((row_blocks + 7) / 8) : 0u;
                const uint32_t *ir = p.d_items + o, *ib = p.d_items + p.n_items + o, *il = p.d_items + 2 * p.n_items + o;
#define PYGIM_LAUNCH_PANEL_D(AM, HV, DQ)                                                                    \
    hipLaunchKernelGGL((k_csr_panel<T, VEC, LOG_LPR, AM, HV, DQ>), dim3(coop_grid + norm_grid), dim3(bthreads), (size_t)g_tune.panel_lds_pad, st,   \
                       ir + ncoop, ib + ncoop, il + ncoop, nnorm, ir, ib, il, ncoop, coop_grid,                           \
                       (AM == 3 ? (const uint32_t *)p.col16 : p.colind), vals, Xs0, ldg,                                  \
                       slice_stride, Cs0, ldc, ws, ns, (accumulate ? 1 : 0) | (p.panel_locality_used ? 2 : 0), q * p.panel_cols,   \
                       g->deq_out ? g->deq_out + (size_t)s0 * F : nullptr, g->deq_ld, g->deq_amax, g->deq_log2,                  \
                       g->post_mul ? g->post_mul + (size_t)s0 * F : nullptr, g->post_add ? g->post_add + (size_t)s0 * F : nullptr, \
                       g->post_relu)
#define PYGIM_LAUNCH_PANEL(AM, HV) PYGIM_LAUNCH_PANEL_D(AM, HV, false)
                // addressing mode of the gathers (kernels.hpp gather_raw): 128-byte rows of the slice-major copy
                // (with 16-bit panel-local column ids when the plan has them), any stride below 4 GiB, or 64-bit
                int amode = !off32 ? 0 : ((size_t)ldg * sizeof(T) == 128 ? 2 : 1);
                if (amode == 2 && p.col16 && g_tune.panel_col16) amode = 3;
                if constexpr (DeqType<T>::ok) {
                    if (g->deq_out && amode >= 2 && !vals) {
                        if (amode == 3) PYGIM_LAUNCH_PANEL_D(3, 0, true);
                        else PYGIM_LAUNCH_PANEL_D(2, 0, true);
                        continue;
                    }
                }
                if (g->deq_out) return fail(PYGIM_ERR_INVALID, "internal: fused dequantisation on an unsupported sweep");
                if constexpr (sizeof(T) == 8) {
                    if (vals && p.vals_narrow && g_tune.narrow_vals) {  // the 4-byte copy of the values (narrow_values)
                        const T *vals = (const T *)p.vals_narrow;       // (the kernel reads it as NarrowOf<T>)
                        if (amode == 3) PYGIM_LAUNCH_PANEL(3, 2);
                        else if (amode == 2) PYGIM_LAUNCH_PANEL(2, 2);
                        else if (amode == 1) PYGIM_LAUNCH_PANEL(1, 2);
                        else PYGIM_LAUNCH_PANEL(0, 2);
                        continue;
                    }
                }
                if (amode == 3 && vals) PYGIM_LAUNCH_PANEL(3, 1);
                else if (amode == 3) PYGIM_LAUNCH_PANEL(3, 0);
                else if (amode == 2 && vals) PYGIM_LAUNCH_PANEL(2, 1);
                else if (amode == 2) PYGIM_LAUNCH_PANEL(2, 0);
                else if (amode == 1 && vals) PYGIM_LAUNCH_PANEL(1, 1);
                else if (amode == 1) PYGIM_LAUNCH_PANEL(1, 0);
                else if (vals) PYGIM_LAUNCH_PANEL(0, 1);
                else PYGIM_LAUNCH_PANEL(0, 0);
#undef PYGIM_LAUNCH_PANEL
#undef PYGIM_LAUNCH_PANEL_D
            }
            }
            kt.stop();
            return join();
        }
    }
    // CSR kernels (native CSR, or COO through its derived rowptr)
    bool wide = lanes_needed > 32;
    if (g_tune.csr_kernel == 1) wide = true;
    if (g_tune.csr_kernel == 2 && lanes_needed <= 32) wide = false;
    if (nrows > 0) {
        KernelTimer kt(g, st, !p.is_extra || p.timed);
        if (wide) {
            dim3 grid((nrows + 3) / 4, (lanes_needed + 63) / 64);
            hipLaunchKernelGGL((k_csr_wide<T, VEC>), grid, dim3(256), 0, st, p.rowptr, p.colind, vals, X, ldx, C,
                               ldc, nrows, w, lp.thresh, accumulate ? 1 : 0);
        } else {
            int log_lpr = 0;
            while ((1u << log_lpr) < lanes_needed) log_lpr++;
            const uint32_t rows_per_wave = 64u >> log_lpr;
            const uint32_t waves = (nrows + rows_per_wave - 1) / rows_per_wave;
            hipLaunchKernelGGL((k_csr_sub<T, VEC>), dim3((waves + 3) / 4), dim3(256), 0, st, p.rowptr, p.colind,
                               vals, X, ldx, C, ldc, nrows, w, lp.thresh, accumulate ? 1 : 0, log_lpr);
        }
        kt.stop();
    }
    return join();
}

// How a launch of the LDS-staged kernel lays its workgroups over the XCDs: group = XCDs that share the tiles of one set of slices (0 = no
// XCD mapping: slice counts that do not divide 8), sx = slices per XCD, touch_share = the sx workgroups that run a tile's code streams side
// by side share the touches (LdsArgs.touch_share).  One rule for the launch and for what pygim_group_lds_geometry reports.
struct LdsXcdLayout {
    uint32_t group = 0, sx = 1, touch_share = 0;
};
static LdsXcdLayout lds_xcd_layout(const Part &p, uint32_t nslices, bool el8) {
    LdsXcdLayout l;
    // (slice counts that do not divide 8 interleave the slices over the XCDs; a slice-major order measured the same: 2.86 vs 2.80 ms at h = 192)
    l.group = (nslices == 1 || nslices == 2 || nslices == 4 || nslices == 8) ? 8 / nslices : 0;
    // round 5 (VERDICT r04 item 3): sx slices per XCD -- the workgroups an XCD runs side by side are then the sx slices of ONE tile and
    // share its code stream in that XCD's L2 (fetched from the fabric nslices / sx times instead of nslices), at the price of sx
    // slices of X streamed through every L2 instead of one
    if (l.group && p.lds_is_code && nslices > 1) {
        // 0 = automatic (profiles/r05_exp_xcd.txt): two slices per XCD -- fabric traffic 5.28 -> 4.19 GB on the bench workload --
        // and all (up to four) of them for plans whose tiles skip most chunks (little of X to un-share): 5.57 -> 3.72 GB, 1.05 -> 0.98 ms
        uint32_t sx = (uint32_t)std::max<int64_t>(0, g_tune.lds_xcd_slices);
        if (sx == 0) {
            const uint64_t nchunks = ((uint64_t)p.ncols + p.lds_kc - 1) / std::max(1u, p.lds_kc);
            const double fill = p.lds_ntiles && nchunks ? (double)p.lds_slots / ((double)p.lds_ntiles * (double)nchunks) : 1.0;
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
    if (l.sx > 1 && g_tune.lds_touch_share && p.lds_is_code && p.lds_nw == 8 &&
        lds_code_touch_shareable(lds_code_regs(8, p.lds_code_gsize, p.lds_code_nsets, p.lds_row_bytes == 512)))
        l.touch_share = 1;
    return l;
}

// LDS-staged product (lds_kernel_gen.hpp / lds_plan.hpp): X is copied slice-major in 256-byte slices (64 features, rows padded to
// whole 256-column chunks), then ONE launch: a 512-thread workgroup per (tile of rows, slice) streams the tile's chunks of X
// through a double-buffered 160 KiB LDS ring (two chunks of 320 columns) and keeps the tile's running sums in registers; C is written once.
// lds_xs: a slice-major copy the caller already made on this stream (the fused quantiser); deq_amax != nullptr: the store
// dequantises, C is then the FLOAT result (row stride ldc elements of 4 bytes)
template <typename T>
int launch_lds(Group *g, Part &p, const T *X, int64_t ldx, T *C, int64_t ldc, uint32_t w, bool accumulate, hipStream_t st,
               const void *lds_xs = nullptr, const uint32_t *deq_amax = nullptr, int deq_log2 = 0) {
    constexpr bool WIDE8 = sizeof(T) == 1;                 // INT8: staged as INT16 (k_slice_pack_widen8), summed by the INT16 stream
    constexpr bool EL8 = sizeof(T) == 8;                   // INT64 / DBL64: slices of 64 features = 512 bytes, a register pair per value
    constexpr uint32_t ROWB = EL8 ? 512 : 256;             // bytes of a staged row
    constexpr uint32_t EPS = WIDE8 ? 128 : ROWB / sizeof(T);   // elements of a slice
    constexpr int PVEC = WIDE8 ? 8 : 16 / (int)sizeof(T);
    // (INT8, and the dequantising INT16 store: the kernel masks features one by one; 8-byte: a lane = a feature)
    // round 6: column-split plans of the 16-bit streams whose result is not the packed 16-bit sum itself (INT8 results, dequantised INT8 / INT16): the INT16 stream's
    // plain kernel writes the ranges' packed partial sums, k_lds_reduce16 makes the result where they meet
    const bool split16 = p.lds_col_splits > 1 && (WIDE8 || (sizeof(T) == 2 && deq_amax != nullptr));
    const uint32_t w_lanes = split16 ? (uint32_t)(((size_t)w * 2 + 3) / 4)
                                     : (WIDE8 || EL8 || (sizeof(T) == 2 && deq_amax)) ? w : (uint32_t)(((size_t)w * sizeof(T) + 3) / 4);
    // half-split plans (round 6): ONE slice whose rows hold two columns' 32 lanes side by side, H = p.lds_half rows (a whole number of chunks)
    const bool HS = p.lds_half != 0;
    if (HS && (sizeof(T) != 4 || w > 32 || lds_xs || deq_amax)) return fail(PYGIM_ERR_INVALID, "internal: a half-split LDS plan serves plain 4-byte products of at most 32 lanes");
    const uint32_t nslices = HS ? 1u : (w + EPS - 1) / EPS;
    const uint64_t rows_pad = HS ? (uint64_t)p.lds_half : lds_rows_pad((uint64_t)p.ncols, p.lds_kc);
    const size_t need = (size_t)rows_pad * nslices * ROWB;
    KernelTimer kt(g, st, !p.is_extra || p.timed);
    XsPin pin;
    void *xs_use = const_cast<void *>(lds_xs);
    // A product of ONE slice whose rows of X are exactly the staged row (64 FLT32 / INT32 features at a stride of 64; 128 INT16; 64 of an 8-byte type) needs no copy:
    // the caller's matrix IS the slice-major form.  The last chunk's rows beyond the matrix are read too (never used): they must lie inside the caller's allocation.
    // (All rows x 64 FLT32 features: 0.61 -> 0.59 ms.)
    if (!xs_use && g_tune.lds_direct_x && nslices == 1 && !HS && !WIDE8 && !p.lds_col_order && (size_t)ldx * sizeof(T) == ROWB && (size_t)w * sizeof(T) == ROWB &&
        ((uintptr_t)X & 255) == 0) {
        void *base = nullptr;
        size_t size = 0;
        if (hipMemGetAddressRange((hipDeviceptr_t *)&base, &size, (hipDeviceptr_t)X) == hipSuccess && base && (const char *)X + (size_t)rows_pad * ROWB <= (const char *)base + size)
            xs_use = const_cast<void *>((const void *)X);
        else
            (void)hipGetLastError();
    }
    if (!xs_use) {
        std::lock_guard<std::mutex> lk(g_ctx.mu);
        if (g->x_unchanged) {
            int dev = 0;
            (void)hipGetDevice(&dev);
            Context::XsBuf *hit = nullptr;
            for (auto &kv : g_ctx.xs_bufs) {
                Context::XsBuf &b = kv.second;
                // (the padded row count depends on the part's chunk size: a copy made for another ring geometry has another slice stride)
                if (kv.first.first == dev && b.ptr && b.src == (const void *)X && b.ld == ldx && b.rows == p.ncols && b.w == (int64_t)w &&
                    b.es == sizeof(T) && b.kind == (HS ? 5 : WIDE8 ? 3 : 1) && b.rows_pad == rows_pad && b.order == (const void *)p.lds_col_order && b.bytes >= need &&
                    (!hit || b.stamp > hit->stamp))
                    hit = &b;
            }
            if (hit) {
                hit->stamp = ++g_ctx.xs_clock;
                hit->in_use++;
                xs_use = hit->ptr;
                pin.hold(xs_use);
            }
        }
        if (!xs_use) {
            Context::XsBuf *b = nullptr;
            if (int rc = xs_buffer_locked(st, std::max<size_t>(need, 256), &b)) return rc;
            xs_use = b->ptr;
            pin.hold(xs_use);
            b->src = X;
            b->ld = ldx;
            b->rows = p.ncols;
            b->w = (int64_t)w;
            b->es = sizeof(T);
            b->kind = HS ? 5 : WIDE8 ? 3 : 1;
            b->rows_pad = rows_pad;
            b->order = p.lds_col_order;
            const uint64_t threads = (uint64_t)p.ncols * nslices * 16;
            if (HS) {
                if constexpr (sizeof(T) == 4) {
                    const uint64_t th = rows_pad * 16;
                    hipLaunchKernelGGL((k_slice_pack_hs<T>), dim3((unsigned)((th + 255) / 256)), dim3(256), 0, st, X, ldx, (uint32_t)p.ncols, w, (uint32_t)rows_pad, (T *)xs_use);
                }
            } else if constexpr (WIDE8) {
                if (threads > 0)
                    hipLaunchKernelGGL(k_slice_pack_widen8, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, (const int8_t *)X, ldx,
                                       (uint32_t)p.ncols, w, nslices, (int16_t *)xs_use, (uint32_t)rows_pad, (const uint32_t *)p.lds_col_order);
            } else if constexpr (EL8) {
                const uint64_t th8 = (uint64_t)p.ncols * nslices * 32;   // 32 pieces of 16 bytes per 512-byte row
                if (th8 > 0)
                    hipLaunchKernelGGL((k_slice_pack<T, 2, 5>), dim3((unsigned)((th8 + 255) / 256)), dim3(256), 0, st, X, ldx,
                                       (uint32_t)p.ncols, w, nslices, (T *)xs_use, (uint32_t)rows_pad, (const uint32_t *)p.lds_col_order);
            } else if (threads > 0) {
                hipLaunchKernelGGL((k_slice_pack<T, PVEC, 4>), dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, X, ldx,
                                   (uint32_t)p.ncols, w, nslices, (T *)xs_use, (uint32_t)rows_pad, (const uint32_t *)p.lds_col_order);
            }
        }
    }
    LdsArgs a{};
    a.tok = p.lds_tok;
    a.tiles = p.lds_tiles;
    a.rowmap = p.lds_rowmap;
    a.xs = (const char *)xs_use;
    a.c = (char *)C;
    a.slice_stride = rows_pad * ROWB;
    a.ldc_bytes = (uint32_t)((size_t)ldc * (((WIDE8 || sizeof(T) == 2) && deq_amax) ? 4 : sizeof(T)));   // (the dequantising store writes floats)
    a.w = w_lanes;
    a.nslices = nslices;
    a.ntiles = p.lds_ntiles;
    a.accumulate = accumulate ? 1 : 0;
    // column-split plans: the tiles write the partial sums of column range c to row r + c * nrows of a scratch block (compact rows of
    // w_lanes dwords); k_lds_reduce adds the S blocks in range order into C afterwards
    const uint32_t S = p.lds_col_splits;
    const uint64_t ldp = split16 ? (uint64_t)w_lanes * 2 : (uint64_t)w_lanes * 4 / sizeof(T);   // elements of a partial row (split16: 16-bit numbers)
    const size_t part_es = split16 ? 2 : sizeof(T);
    const uint64_t lds_rows = p.lds_rows ? p.lds_rows : (uint64_t)p.nrows;   // rows the plan's tiles cover (the rest: k_lds_tail, below)
    // round 6: the dequantising product on a column-split plan -- the plain kernel writes the ranges' partial sums, k_lds_reduce_deq dequantises where they meet
    const bool deq_at_reduce = S > 1 && deq_amax != nullptr;
    if (S > 1) {
        // (+ what the tail kernels park behind the ranges' partial sums: ONE allocation, made before anything is launched into it)
        const size_t need = (((size_t)S * (size_t)lds_rows * ldp * part_es + 255) & ~(size_t)255) + (size_t)p.lds_tail_nseg * nslices * 64 * 8;
        if (int rc = ensure(&g->scratch, &g->scratch_bytes, std::max<size_t>(need, 256))) return rc;
        a.c = (char *)g->scratch;
        a.ldc_bytes = (uint32_t)(ldp * part_es);
        a.accumulate = 0;
    }
    const uint32_t *kernel_amax = (deq_at_reduce || split16) ? nullptr : deq_amax;
    a.wdelta = p.lds_wdelta;
    a.deq_amax = kernel_amax;
    a.deq_log2 = deq_log2;
    a.post_mul = kernel_amax ? g->post_mul : nullptr;   // (the per-column epilogue rides the dequantising store only)
    a.post_add = kernel_amax ? g->post_add : nullptr;
    a.post_relu = kernel_amax ? g->post_relu : 0;
    const LdsXcdLayout lay = lds_xcd_layout(p, nslices, EL8);
    a.xcd_group = lay.group;
    a.xcd_sx = lay.sx;
    a.touch_share = lay.touch_share;
    a.half_split = HS ? 1u : 0u;
    a.xcd_contig = (a.xcd_group && p.lds_contig_tiles) ? (p.lds_ntiles + a.xcd_group - 1) / a.xcd_group : 0;
    const uint32_t grid = a.xcd_group ? 8 * ((p.lds_ntiles + a.xcd_group - 1) / a.xcd_group) * a.xcd_sx : p.lds_ntiles * nslices;
    using KernelFn = void (*)(LdsArgs);
    KernelFn fn = nullptr;
    const bool long16 = p.lds_nw == 16 && p.lds_batch == LDS_L16_BATCH;   // the 16-token-batch geometry (no values)
    if (p.lds_is_code) {   // the schedule compiled into machine code: 16 waves x 96 accumulators, or 8 x 228 (k_lds_code8_*)
        if (!g_tune.lds_code || g_tune.lds_ablate) return fail(PYGIM_ERR_INVALID, "this group's LDS plan is a code stream: lds_code was switched off (or lds_ablate on) after it was created");
        const bool w8 = p.lds_nw == 8;
        if constexpr (EL8) {
            if (!w8 || kernel_amax || S > 1 || p.lds_row_bytes != 512) return fail(PYGIM_ERR_INVALID, "internal: 8-byte LDS-staged product on an unsupported plan");
            if constexpr (std::is_same<T, double>::value) fn = k_lds_code8_f64;
            else fn = k_lds_code8_i64;
        } else if constexpr (sizeof(T) == 1) {
            if (!w8 || (accumulate && S <= 1)) return fail(PYGIM_ERR_INVALID, "internal: INT8 LDS-staged product on an unsupported plan");
            fn = split16 ? k_lds_code8_i16 : kernel_amax ? k_lds_code8_i8_deq : k_lds_code8_i8;   // (widened to 16 bits in the staged copy: the INT16 stream)
        } else if constexpr (sizeof(T) == 2) {
            if ((kernel_amax || split16) && !w8) return fail(PYGIM_ERR_INVALID, "internal: dequantising LDS-staged product on an unsupported plan");
            fn = kernel_amax ? k_lds_code8_i16_deq : (w8 ? k_lds_code8_i16 : k_lds_code_i16);   // (two features to a lane: v_pk_add_u16)
        } else if constexpr (std::is_same<T, float>::value) {
            fn = kernel_amax ? (w8 ? k_lds_code8_f32_deq : k_lds_code_f32_deq) : (w8 ? k_lds_code8_f32 : k_lds_code_f32);
        } else {
            fn = kernel_amax ? (w8 ? k_lds_code8_i32_deq : k_lds_code_i32_deq) : (w8 ? k_lds_code8_i32 : k_lds_code_i32);
        }
        // measurement build (scripts/exp_stamps.py): the caller's buffer gets four clock stamps per wave of every workgroup
        if (g_tune.lds_stamp && fn == k_lds_code8_f32) {
            fn = k_lds_code8_f32_ts;
            a.stamps = (uint64_t *)(uintptr_t)g_tune.lds_stamp;
        }
        a.code = p.lds_code;
        a.code_start = p.lds_code_start;
        a.piece_bytes = p.lds_code_piece;
    } else if constexpr (sizeof(T) == 1 || sizeof(T) == 8) {
        return fail(PYGIM_ERR_INVALID, "internal: the INT8 / INT64 / DBL64 LDS-staged product exists in the code-stream form only");
    } else if (kernel_amax) {
        if (p.lds_nw != 16 || p.lds_wdelta || sizeof(T) != 4) return fail(PYGIM_ERR_INVALID, "internal: dequantising LDS-staged product on an unsupported plan");
        if constexpr (std::is_same<T, float>::value) fn = long16 ? k_lds_spmm_f32_w16b_deq : k_lds_spmm_f32_w16_deq;
        else if constexpr (std::is_same<T, int32_t>::value) fn = long16 ? k_lds_spmm_i32_w16b_deq : k_lds_spmm_i32_w16_deq;
    } else if constexpr (sizeof(T) == 2) {
        if (p.lds_nw != 16) return fail(PYGIM_ERR_INVALID, "internal: INT16 LDS-staged product needs the 16-wave plan");
        fn = long16 ? k_lds_spmm_i16_w16b : (p.lds_wdelta ? k_lds_spmm_i16_w16_val : k_lds_spmm_i16_w16);
    } else if (long16) {
        if constexpr (std::is_same<T, float>::value) fn = k_lds_spmm_f32_w16b;
        else fn = k_lds_spmm_i32_w16b;
    } else if constexpr (std::is_same<T, float>::value) {
        fn = p.lds_nw == 16 ? (p.lds_wdelta ? k_lds_spmm_f32_w16_val : k_lds_spmm_f32_w16) : k_lds_spmm_f32_w8;
#ifdef PYGIM_LDS_ABLATE
        if (p.lds_nw == 16 && !p.lds_wdelta && !long16) {  // timing experiments (wrong results, scripts/gen_lds_kernel.py; make ablate)
            switch (g_tune.lds_ablate) {
                case 6: fn = k_lds_spmm_f32_w16_ab6; break;
                case 7: fn = k_lds_spmm_f32_w16_ab7; break;
                case 10: fn = k_lds_spmm_f32_w16_ab10; break;
                case 11: fn = k_lds_spmm_f32_w16_ab11; break;
                case 12: fn = k_lds_spmm_f32_w16_ab12; break;
                case 15: fn = k_lds_spmm_f32_w16_ab15; break;
                case 16: fn = k_lds_spmm_f32_w16_ab16; break;
                case 17: fn = k_lds_spmm_f32_w16_ab17; break;
                case 18: fn = k_lds_spmm_f32_w16_ab18; break;
                case 19: fn = k_lds_spmm_f32_w16_ab19; break;
                default: break;
            }
        }
#else
        if (g_tune.lds_ablate) return fail(PYGIM_ERR_INVALID, "lds_ablate needs the ablation build (make -C pygim_amd/csrc ablate)");
#endif
    } else {
        fn = p.lds_nw == 16 ? (p.lds_wdelta ? k_lds_spmm_i32_w16_val : k_lds_spmm_i32_w16) : k_lds_spmm_i32_w8;
    }
    if (kernel_amax && g_tune.lds_ablate) return fail(PYGIM_ERR_INVALID, "lds_ablate is a timing experiment of the plain kernel");
    if (!fn) return fail(PYGIM_ERR_INVALID, "internal: no LDS-staged kernel for this plan");
    {
        static std::set<std::pair<int, KernelFn>> attr_done;   // (the attribute is per device)
        int dev = 0;
        HIP_TRY(hipGetDevice(&dev));
        std::lock_guard<std::mutex> lk(g_ctx.mu);
        if (!attr_done.count({dev, fn})) {
            HIP_TRY(hipFuncSetAttribute((const void *)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_BYTES));
            attr_done.insert({dev, fn});
        }
    }
    hipLaunchKernelGGL(fn, dim3(grid), dim3(p.lds_nw * 64), LDS_BYTES, st, a);
    g->lds_runs++;
    if (split16 && lds_rows > 0 && w > 0) {
        const uint64_t total = lds_rows * w;
        const dim3 rg((unsigned)((total + 255) / 256));
        if (!deq_amax)
            hipLaunchKernelGGL((k_lds_reduce16<0>), rg, dim3(256), 0, st, (const int16_t *)g->scratch, S, lds_rows, w, ldp, (void *)C, ldc, accumulate ? 1 : 0, nullptr, 0, nullptr, nullptr, 0);
        else if (WIDE8)
            hipLaunchKernelGGL((k_lds_reduce16<1>), rg, dim3(256), 0, st, (const int16_t *)g->scratch, S, lds_rows, w, ldp, (void *)C, ldc, 0, deq_amax, deq_log2, g->post_mul, g->post_add, g->post_relu);
        else
            hipLaunchKernelGGL((k_lds_reduce16<2>), rg, dim3(256), 0, st, (const int16_t *)g->scratch, S, lds_rows, w, ldp, (void *)C, ldc, 0, deq_amax, deq_log2, g->post_mul, g->post_add, g->post_relu);
    } else if (S > 1 && lds_rows > 0 && w > 0 && sizeof(T) == 4 && (w & 3) == 0 && (ldp & 3) == 0 && (ldc & 3) == 0 && ((uintptr_t)C & 15) == 0) {
        // four features to a thread (16-byte loads and stores): a 1/8 row share's reduce 32 -> 21 us
        if constexpr (sizeof(T) == 4) {
            const uint64_t total4 = lds_rows * (w >> 2);
            const dim3 rg((unsigned)((total4 + 255) / 256));
            if (deq_at_reduce)
                hipLaunchKernelGGL((k_lds_reduce_v4<T, true>), rg, dim3(256), 0, st, (const T *)g->scratch, S, lds_rows, w, ldp, (void *)C, ldc, 0, deq_amax, deq_log2, g->post_mul,
                                   g->post_add, g->post_relu);
            else
                hipLaunchKernelGGL((k_lds_reduce_v4<T, false>), rg, dim3(256), 0, st, (const T *)g->scratch, S, lds_rows, w, ldp, (void *)C, ldc, accumulate ? 1 : 0, nullptr, 0, nullptr,
                                   nullptr, 0);
        }
    } else if (S > 1 && lds_rows > 0 && w > 0) {
        const uint64_t total = lds_rows * w;
        if constexpr (sizeof(T) == 4) {
            if (deq_at_reduce)
                hipLaunchKernelGGL((k_lds_reduce_deq<T>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const T *)g->scratch, S, lds_rows, w, ldp, (float *)C, ldc,
                                   deq_amax, deq_log2, g->post_mul, g->post_add, g->post_relu);
        }
        if (!deq_at_reduce)
            hipLaunchKernelGGL((k_lds_reduce<T>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const T *)g->scratch, S, lds_rows, w, ldp, C,
                               ldc, accumulate ? 1 : 0);
    }
    if (lds_rows < (uint64_t)p.nrows && w > 0) {   // the share's last rows, from the same staged copy (k_lds_tail_seg / _fin)
        if constexpr (sizeof(T) == 4) {
            using A = typename AccOf<T>::type;
            if (!p.lds_tail_segs || !p.lds_tail_rowseg) return fail(PYGIM_ERR_INVALID, "internal: an LDS plan that leaves rows out has no segment table for them");
            const uint32_t ntail = (uint32_t)((uint64_t)p.nrows - lds_rows);
            const size_t split_bytes = S > 1 ? (((size_t)S * (size_t)lds_rows * ldp * sizeof(T) + 255) & ~(size_t)255) : 0;
            const size_t park_bytes = (size_t)p.lds_tail_nseg * nslices * 64 * sizeof(A);
            if (int rc = ensure(&g->scratch, &g->scratch_bytes, std::max<size_t>(split_bytes + park_bytes, 256))) return rc;   // (grows before the first product only)
            A *parked = (A *)((char *)g->scratch + split_bytes);
            if (p.lds_tail_nseg > 0)   // (rows without entries have no segment: k_lds_tail_fin still writes their zeros)
                hipLaunchKernelGGL((k_lds_tail_seg<T>), dim3(p.lds_tail_nseg, nslices), dim3(512), 0, st, p.lds_tail_segs, p.lds_tail_nseg, p.colind, (const char *)xs_use,
                                   (uint64_t)(rows_pad * ROWB), parked);
            const int64_t ldc_b = (int64_t)ldc * 4;
            if (deq_amax)
                hipLaunchKernelGGL((k_lds_tail_fin<T, true>), dim3(ntail, nslices), dim3(64), 0, st, p.lds_tail_rowseg, (uint32_t)lds_rows, parked, w, (void *)C, ldc_b, 0, deq_amax,
                                   deq_log2, g->post_mul, g->post_add, g->post_relu);
            else
                hipLaunchKernelGGL((k_lds_tail_fin<T, false>), dim3(ntail, nslices), dim3(64), 0, st, p.lds_tail_rowseg, (uint32_t)lds_rows, parked, w, (void *)C, ldc_b,
                                   accumulate ? 1 : 0, nullptr, 0, nullptr, nullptr, 0);
        } else {
            return fail(PYGIM_ERR_INVALID, "internal: an LDS plan that leaves rows to the tail kernels exists for 4-byte element types only");
        }
    }
    kt.stop();
    HIP_TRY(hipGetLastError());
    return 0;
}

template <typename T> bool want_lds(const Group *g, const Part &p, uint32_t w, int64_t ldc, const void *C, bool accumulate = false) {
    if constexpr (sizeof(T) == 8) {  // INT64 / DBL64: the 8-wave code stream on 512-byte rows (unit weights)
        if (!p.lds_is_code || p.lds_nw != 8 || p.lds_row_bytes != 512 || p.lds_col_splits > 1 || false) return false;   // (valued DBL64 / INT64: round 5 -- a valued part has a code plan only when its values allow it)
    } else if (p.lds_row_bytes == 512) return false;
    if constexpr (sizeof(T) == 1) {  // INT8 rides the 8-wave INT16 code stream (features widened to 16 bits in the staged copy); it neither accumulates
                                     // into C nor splits tiles into column ranges
        if (!p.lds_is_code || p.lds_nw != 8 || (accumulate && p.lds_col_splits <= 1)) return false;   // (round 5: valued too -- the values are part of the stream; round 6: column-split
                                                                                                     // plans -- k_lds_reduce16 makes the bytes, and adds into C when asked)
        if ((int64_t)(w / 2) < g_tune.lds_min_width) return false;
    }
    if constexpr (sizeof(T) == 2) {  // two features to a lane: whole lanes, dword-aligned rows of C, the 16-wave plan
        if ((w & 1) || (ldc & 1) || ((uintptr_t)C & 3) || (p.lds_nw != 16 && !p.lds_is_code)) return false;
    }
    if (!p.lds_tiles || g_tune.lds_mode == 2 || (!p.lds_is_code && (p.vals != nullptr) != (p.lds_wdelta != 0)) || g->deq_out || g->pre_xs) return false;
    if (p.lds_half && (sizeof(T) != 4 || w > 32)) return false;   // (a half-split plan: plain products of at most 32 lanes)
    if (p.lds_is_code && (!g_tune.lds_code || g_tune.lds_ablate)) return false;   // (a code-stream plan serves no token kernel: the sweep instead)
    if (g_tune.lds_mode == 0 && (g_tune.panel_mode == 1 || g_tune.csr_kernel != 0 || g_tune.force_vec_bytes != 0)) return false;  // another kernel was asked for by name
    if (sizeof(T) > 1 && (int64_t)(sizeof(T) == 8 ? (size_t)w : (size_t)w * sizeof(T) / 4) < (sizeof(T) == 8 ? g_tune.lds_min_width8 : g_tune.lds_min_width)) return false;   // (lanes: 4-byte units of a row; 8-byte: features)
    if ((uint64_t)ldc * sizeof(T) >= (1ull << 32)) return false;
    return true;
}

template <typename T>
int launch_block(Group *g, Part &p, const void *X, int64_t ldx, void *C, int64_t ldc, int64_t w, bool accumulate,
                 hipStream_t st) {
    const T *x = (const T *)X;
    T *c = (T *)C;
    const uint32_t ww = (uint32_t)w;
    if (want_lds<T>(g, p, ww, ldc, C, accumulate)) return launch_lds<T>(g, p, x, ldx, c, ldc, ww, accumulate, st);
    // SpMV end of the path: rows of X of at most 4 elements -> lanes over the ENTRIES of a row (k_csr_vec)
    if (ww <= 4 && g_tune.vec_kernel && g_tune.force_vec_bytes == 0 && g_tune.csr_kernel == 0 && p.rowptr && p.nrows > 0) {
        // LDS-staged form: the plan's column panels with 16-bit local ids, a panel of X (panel_cols x w elements) plus the
        // staging of results inside a workgroup's LDS; rows cut into segments (segment kernels) keep the plain form
        using A = typename AccOf<T>::type;
        constexpr size_t LDS_TOTAL = 160 * 1024 - 64;
        const size_t panel_lds = (((((size_t)p.panel_cols + 1) * ww * sizeof(T)) + 15) & ~(size_t)15) + 16;  // + zero row + alignment lead-in
        const size_t per_entry = 4 + (size_t)ww * sizeof(A);                                                 // a parked (row, sum)
        // (items in the sweep's locality order -- a group created for wide products and asked for a narrow one -- are not longest-first
        // inside a panel: the length classes below are prefixes of a length-sorted list, so such a part keeps k_csr_vec)
        const bool lds_rule = g_tune.vec_lds && g_tune.panel_mode != 2 && p.d_items && p.col16 && p.lp_panel.n_tasks == 0 && !p.panel_locality_used &&
                              p.npanels >= 1 && p.panel_long128.size() == 4 * (size_t)p.npanels && (uint64_t)p.nnz < (1ull << 31) &&
                              // every (row, panel) item costs one pipeline step whatever its length: against k_csr_vec it pays from about
                              // 14 entries per item (Reddit-shaped: w = 4, 17 entries per item, 0.46 against 0.73 ms)
                              (double)p.nnz >= (double)g_tune.vec_lds_min_seg * (double)p.nrows * (double)p.npanels;
        if (lds_rule && panel_lds + 64 * 12 * per_entry <= LDS_TOTAL) {
            // ONE launch over all panels (kernels.hpp, k_spmv_lds): a workgroup per (panel, slot) unit, the panels' sums parked
            // in part[panel][row] and added in panel order by k_spmv_reduce
            const size_t stage_budget = std::min<size_t>(32 * 1024, LDS_TOTAL - panel_lds);
            // parked pairs per 16-lane group: a multiple of 24 so that 4-lane groups get F16 / 4 (a multiple of the pipeline's 6), or
            // -- wide sums, little room -- a multiple of 12 and no 4-lane class
            uint32_t F16 = (uint32_t)(stage_budget / (64 * per_entry)) / 24 * 24;
            const int merge4 = F16 == 0 ? 1 : 0;
            if (merge4) F16 = (uint32_t)(stage_budget / (64 * per_entry)) / 12 * 12;
            const size_t shmem = panel_lds + 64 * (size_t)F16 * per_entry;
            const uint32_t cu = (uint32_t)std::max(g_ctx.cu_count, 1);
            if (!p.d_spmv_units) {
                std::vector<uint32_t> act;
                double wsum = 0;
                for (uint32_t q = 0; q < p.npanels; q++)
                    if (p.panel_off[q + 1] > p.panel_off[q]) {
                        act.push_back(q);
                        wsum += (double)std::max<uint64_t>(p.panel_nnz[q], p.panel_off[q + 1] - p.panel_off[q]);
                    }
                if (!act.empty()) {
                    // workgroups per panel in proportion to its entries (at least one); more panels than CUs: one each, taken in turn
                    std::vector<uint32_t> nb(act.size(), 1);
                    if (act.size() < cu) {
                        uint32_t left = cu - (uint32_t)act.size();
                        std::vector<std::pair<double, size_t>> rem;
                        uint32_t given = 0;
                        for (size_t k = 0; k < act.size(); k++) {
                            const uint32_t q = act[k];
                            const double share = (double)left * (double)std::max<uint64_t>(p.panel_nnz[q], p.panel_off[q + 1] - p.panel_off[q]) / wsum;
                            const uint32_t fl = (uint32_t)share;
                            nb[k] += fl;
                            given += fl;
                            rem.emplace_back(share - fl, k);
                        }
                        std::sort(rem.begin(), rem.end(), [](const std::pair<double, size_t> &x, const std::pair<double, size_t> &y) { return x.first > y.first; });
                        for (size_t k = 0; given < left && k < rem.size(); k++, given++) nb[rem[k].second]++;
                    }
                    // slot-major order: consecutive workgroups (dispatched round-robin over the XCDs) take different panels, so with
                    // 8 panels an XCD's L2 serves one panel of X to all its CUs
                    std::vector<SpmvUnit> units;
                    const uint32_t most = *std::max_element(nb.begin(), nb.end());
                    for (uint32_t slot = 0; slot < most; slot++)
                        for (size_t k = 0; k < act.size(); k++) {
                            if (slot >= nb[k]) continue;
                            const uint32_t q = act[k];
                            SpmvUnit u;
                            u.item_off = (uint32_t)p.panel_off[q];
                            u.n_items = (uint32_t)(p.panel_off[q + 1] - p.panel_off[q]);
                            u.n64 = p.panel_long128[4 * q];
                            u.n32 = p.panel_long128[4 * q + 1] - u.n64;
                            u.n16 = p.panel_long128[4 * q + 2] - u.n64 - u.n32;
                            u.n8 = p.panel_long128[4 * q + 3] - u.n64 - u.n32 - u.n16;
                            u.col_base = q * p.panel_cols;
                            u.pcols = (uint32_t)std::min<int64_t>(p.panel_cols, p.ncols - (int64_t)u.col_base);
                            u.slot = slot;
                            u.nslots = nb[k];
                            u.panel = q;
                            units.push_back(u);
                        }
                    HIP_TRY(hipMalloc((void **)&p.d_spmv_units, units.size() * sizeof(SpmvUnit)));
                    HIP_TRY(hipMemcpyAsync(p.d_spmv_units, units.data(), units.size() * sizeof(SpmvUnit), hipMemcpyHostToDevice, st));
                    HIP_TRY(hipStreamSynchronize(st));  // (units is a local; one-time)
                    p.n_spmv_units = (uint32_t)units.size();
                }
            }
            const size_t part_bytes = ((size_t)p.npanels * (size_t)p.nrows * ww * sizeof(A) + 15) & ~(size_t)15;
            if (int rc = ensure(&g->scratch, &g->scratch_bytes, part_bytes)) return rc;
            A *part = (A *)g->scratch;
            KernelTimer kt(g, st, !p.is_extra || p.timed);
            hipLaunchKernelGGL(k_zero16, dim3((unsigned)((part_bytes / 16 + 255) / 256)), dim3(256), 0, st, (u32x4_t *)part,
                               (uint64_t)(part_bytes / 16));
            if (p.n_spmv_units > 0) {
                const uint32_t *ir = p.d_items, *ib = p.d_items + p.n_items, *il = p.d_items + 2 * p.n_items;
                const uint32_t blocks = std::min(p.n_spmv_units, cu);
#define PYGIM_SPMV_LDS(W, HV)                                                                                                  \
    {                                                                                                                          \
        static std::atomic<uint64_t> attr_devs{0};   /* the attribute is per device: one bit per device ordinal */            \
        int dev_ = 0;                                                                                                          \
        HIP_TRY(hipGetDevice(&dev_));                                                                                          \
        const uint64_t bit_ = 1ull << (dev_ & 63);                                                                             \
        if (!(attr_devs.load(std::memory_order_acquire) & bit_)) {                                                             \
            HIP_TRY(hipFuncSetAttribute((const void *)k_spmv_lds<T, W, HV>, hipFuncAttributeMaxDynamicSharedMemorySize,        \
                                        (int)(LDS_TOTAL + 64)));                                                               \
            attr_devs.fetch_or(bit_, std::memory_order_release);                                                               \
        }                                                                                                                      \
        hipLaunchKernelGGL((k_spmv_lds<T, W, HV>), dim3(blocks), dim3(1024), shmem, st, p.d_spmv_units, p.n_spmv_units, ir, ib, \
                           il, p.col16, (const T *)p.vals, x, ldx, part, (uint32_t)p.nrows, (uint32_t)panel_lds, F16, merge4); \
    }
                if (p.vals) {
                    if (ww == 1) PYGIM_SPMV_LDS(1, true) else if (ww == 2) PYGIM_SPMV_LDS(2, true)
                    else if (ww == 3) PYGIM_SPMV_LDS(3, true) else PYGIM_SPMV_LDS(4, true)
                } else {
                    if (ww == 1) PYGIM_SPMV_LDS(1, false) else if (ww == 2) PYGIM_SPMV_LDS(2, false)
                    else if (ww == 3) PYGIM_SPMV_LDS(3, false) else PYGIM_SPMV_LDS(4, false)
                }
#undef PYGIM_SPMV_LDS
            }
            {
                const uint64_t total = (uint64_t)p.nrows * ww;
                const dim3 rgrid((unsigned)((total + 255) / 256));
                if (ww == 1) hipLaunchKernelGGL((k_spmv_reduce<T, 1>), rgrid, dim3(256), 0, st, part, p.npanels, (uint32_t)p.nrows, c, ldc, accumulate ? 1 : 0);
                else if (ww == 2) hipLaunchKernelGGL((k_spmv_reduce<T, 2>), rgrid, dim3(256), 0, st, part, p.npanels, (uint32_t)p.nrows, c, ldc, accumulate ? 1 : 0);
                else if (ww == 3) hipLaunchKernelGGL((k_spmv_reduce<T, 3>), rgrid, dim3(256), 0, st, part, p.npanels, (uint32_t)p.nrows, c, ldc, accumulate ? 1 : 0);
                else hipLaunchKernelGGL((k_spmv_reduce<T, 4>), rgrid, dim3(256), 0, st, part, p.npanels, (uint32_t)p.nrows, c, ldc, accumulate ? 1 : 0);
            }
            kt.stop();
            HIP_TRY(hipGetLastError());
            return 0;
        }
        const double avg = (double)p.nnz / (double)p.nrows;
        const int log_g = avg >= 96 ? 6 : avg >= 48 ? 5 : avg >= 24 ? 4 : avg >= 10 ? 3 : 2;
        const uint64_t waves = ((uint64_t)p.nrows + (64u >> log_g) - 1) / (64u >> log_g);
        KernelTimer kt(g, st, !p.is_extra || p.timed);
        const dim3 grid((unsigned)((waves + 3) / 4));
#define PYGIM_VEC(W)                                                                                                     \
    if (ww == W) {                                                                                                       \
        if (p.vals)                                                                                                      \
            hipLaunchKernelGGL((k_csr_vec<T, W, true>), grid, dim3(256), 0, st, p.rowptr, p.colind, (const T *)p.vals, x, ldx, c, \
                               ldc, (uint32_t)p.nrows, accumulate ? 1 : 0, log_g);                                      \
        else                                                                                                             \
            hipLaunchKernelGGL((k_csr_vec<T, W, false>), grid, dim3(256), 0, st, p.rowptr, p.colind, (const T *)nullptr, x, ldx, \
                               c, ldc, (uint32_t)p.nrows, accumulate ? 1 : 0, log_g);                                   \
    }
        PYGIM_VEC(1) PYGIM_VEC(2) PYGIM_VEC(3) PYGIM_VEC(4)
#undef PYGIM_VEC
        kt.stop();
        HIP_TRY(hipGetLastError());
        return 0;
    }
    const int vb = pick_vec_bytes(sizeof(T), X, ldx, C, ldc);
    int vec = vb / (int)sizeof(T);
    // The panel sweep moves 16-byte pieces with byte-aligned accesses (kernels.hpp u32x4_b), so it takes rows of
    // ANY alignment (h = 41 floats, 100 int8 ...); only its long-row side kernels want aligned rows, so parts that
    // have such rows keep the alignment-matched kernels.
    if (vb < 16 && g_tune.force_vec_bytes == 0 && p.lp_panel.n_tasks == 0 && want_panel<T>(p, ww, ldx))
        vec = 16 / (int)sizeof(T);
#define CASE(V)                                                               \
    if constexpr (V >= 1 && (size_t)V * sizeof(T) <= 16) {                    \
        if (vec == V) return launch_block_t<T, V>(g, p, x, ldx, c, ldc, ww, accumulate, st); \
    }
    CASE(16) CASE(8) CASE(4) CASE(2)
#undef CASE
    return launch_block_t<T, 1>(g, p, x, ldx, c, ldc, ww, accumulate, st);
}

int launch_block_main(Group *g, Part &p, const void *X, int64_t ldx, void *C, int64_t ldc, int64_t w, bool accumulate,
                      hipStream_t st);

static bool hybrid_takes(const Group *g, const Part &d, uint32_t w, int64_t ldc, const void *C) {
    switch (g->dtype) {
        case PYGIM_INT8: return want_lds<int8_t>(g, d, w, ldc, C, false);
        case PYGIM_INT16: return want_lds<int16_t>(g, d, w, ldc, C, false);
        case PYGIM_INT32: return want_lds<int32_t>(g, d, w, ldc, C, false);
        case PYGIM_FLT32: return want_lds<float>(g, d, w, ldc, C, false);
        default: return false;
    }
}

// true when launch_block_any(g, p, ..., C, ldc, w, accumulate = false) is ONE pass of the LDS-staged product that writes every element of C exactly once and
// reads none (no correction part, no density split adding on top): the call whose C may be the caller's page-locked host tensor (run_group_windows)
static bool lds_writes_c_once(const Group *g, const Part &p, uint32_t w, int64_t ldc, const void *C) {
    if (p.extra || p.hy_dense || p.hy_sparse || w == 0 || p.nrows == 0) return false;
    switch (g->dtype) {
        case PYGIM_INT8: return want_lds<int8_t>(g, p, w, ldc, C, false);
        case PYGIM_INT16: return want_lds<int16_t>(g, p, w, ldc, C, false);
        case PYGIM_INT32: return want_lds<int32_t>(g, p, w, ldc, C, false);
        case PYGIM_INT64: return want_lds<int64_t>(g, p, w, ldc, C, false);
        case PYGIM_FLT32: return want_lds<float>(g, p, w, ldc, C, false);
        case PYGIM_DBL64: return want_lds<double>(g, p, w, ldc, C, false);
    }
    return false;
}

int launch_block_any(Group *g, Part &p, const void *X, int64_t ldx, void *C, int64_t ldc, int64_t w,
                     bool accumulate, hipStream_t st) {
    if (w <= 0 || p.nrows == 0) return 0;  // nothing to write
    g->packed_buf = nullptr;
    // a density-split part (lds_hybrid_dev.hpp): the dense cells through the LDS-staged kernel, the rest added by the sweep -- when the LDS kernel takes
    // this call (width, alignment); otherwise the part's own plan as before
    if (p.hy_dense && p.hy_sparse && !accumulate && g_tune.lds_hybrid && hybrid_takes(g, *p.hy_dense, (uint32_t)w, ldc, C)) {
        if (int rc = launch_block_main(g, *p.hy_dense, X, ldx, C, ldc, w, false, st)) return rc;
        if (int rc = launch_block_main(g, *p.hy_sparse, X, ldx, C, ldc, w, true, st)) return rc;
    } else if (int rc = launch_block_main(g, p, X, ldx, C, ldc, w, accumulate, st)) return rc;
    // the few entries with a weight other than 1, as (weight - 1), added on top of the pattern product
    if (p.extra) return launch_block_main(g, *p.extra, X, ldx, C, ldc, w, true, st);
    return 0;
}

int launch_block_main(Group *g, Part &p, const void *X, int64_t ldx, void *C, int64_t ldc, int64_t w, bool accumulate,
                      hipStream_t st) {
    switch (g->dtype) {
        case PYGIM_INT8: return launch_block<int8_t>(g, p, X, ldx, C, ldc, w, accumulate, st);
        case PYGIM_INT16: return launch_block<int16_t>(g, p, X, ldx, C, ldc, w, accumulate, st);
        case PYGIM_INT32: return launch_block<int32_t>(g, p, X, ldx, C, ldc, w, accumulate, st);
        case PYGIM_INT64: return launch_block<int64_t>(g, p, X, ldx, C, ldc, w, accumulate, st);
        case PYGIM_FLT32: return launch_block<float>(g, p, X, ldx, C, ldc, w, accumulate, st);
        case PYGIM_DBL64: return launch_block<double>(g, p, X, ldx, C, ldc, w, accumulate, st);
    }
    return fail(PYGIM_ERR_INVALID, "unknown dtype");
}
