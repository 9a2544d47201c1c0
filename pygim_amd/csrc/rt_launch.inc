// rt_launch.inc -- part of pygim_hip.hip (inside its anonymous namespace): one block product -> kernels.  The sweep (launch_block_t), the LDS-staged
// product in its token and code-stream forms (launch_lds; its rules are lds_launch.hpp's), the dispatch by element type.
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
    if (g_tune.panel_mode == 0 && !panels_pay(p.nnz, p.nrows, p.npanels, g_tune.panel_min_seg)) return false;   // (sweep_plan.hpp: the builder's rule)
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

// The tunables the launch rules read (lds_launch.hpp) and the plan fields of a Part, each copied in this one place.
static LdsLaunchKnobs lds_launch_knobs() {
    LdsLaunchKnobs k;
#define PYGIM_KNOB(name) k.name = g_tune.name
    PYGIM_KNOB(lds_xcd_slices); PYGIM_KNOB(lds_touch_share); PYGIM_KNOB(lds_code); PYGIM_KNOB(lds_ablate); PYGIM_KNOB(lds_mode); PYGIM_KNOB(lds_min_width);
    PYGIM_KNOB(lds_min_width8); PYGIM_KNOB(panel_mode); PYGIM_KNOB(csr_kernel); PYGIM_KNOB(force_vec_bytes); PYGIM_KNOB(lds_direct_x);
#undef PYGIM_KNOB
    return k;
}
static LdsPartPlan lds_part_plan(const Part &p) {
    LdsPartPlan q;
    q.has_plan = p.lds_tiles != nullptr; q.is_code = p.lds_is_code; q.valued = p.vals != nullptr; q.wdelta = p.lds_wdelta != 0;
    q.contig_tiles = p.lds_contig_tiles; q.col_order = p.lds_col_order != nullptr; q.tail_tables = p.lds_tail_segs && p.lds_tail_rowseg;
    q.nw = p.lds_nw; q.batch = p.lds_batch; q.kc = p.lds_kc; q.row_bytes = p.lds_row_bytes; q.col_splits = p.lds_col_splits; q.half = p.lds_half;
    q.rows = p.lds_rows; q.ntiles = p.lds_ntiles; q.tail_nseg = p.lds_tail_nseg; q.code_gsize = p.lds_code_gsize; q.code_nsets = p.lds_code_nsets;
    q.slots = p.lds_slots; q.nrows = p.nrows; q.ncols = p.ncols;
    return q;
}

// does launch_block hand this product to the LDS-staged kernel (lds_launch.hpp lds_takes)
static bool lds_takes(const Group *g, const Part &p, uint32_t w, int64_t ldc, const void *C, bool accumulate = false) {
    return lds_takes(g->dtype, lds_part_plan(p), w, ldc, (uintptr_t)C, accumulate, g->deq_out || g->pre_xs, lds_launch_knobs());
}

// The staged copy of X that a launch reads (lds_launch.hpp lds_staged): the caller's matrix in place when it IS the slice-major form, else a
// copy of the same matrix made earlier when the caller says X is unchanged, else a fresh pack into the buffer of (device, stream).
template <typename T>
static int lds_stage_x(Group *g, const Part &p, const LdsStaged &xs, bool in_place, const T *X, int64_t ldx, uint32_t w, hipStream_t st, XsPin &pin, const void **out) {
    // in_place (lds_plan_launch): the caller's matrix IS the slice-major form.  The last chunk's rows beyond the matrix are read too (never used): they must lie
    // inside the caller's allocation.
    if (in_place) {
        void *base = nullptr;
        size_t size = 0;
        if (hipMemGetAddressRange((hipDeviceptr_t *)&base, &size, (hipDeviceptr_t)X) == hipSuccess && base && (const char *)X + xs.slice_stride <= (const char *)base + size) {
            *out = X;
            return 0;
        }
        (void)hipGetLastError();
    }
    Context::XsKey key;
    key.src = X; key.ld = ldx; key.rows = p.ncols; key.w = (int64_t)w; key.order = p.lds_col_order; key.rows_pad = xs.rows_pad; key.es = sizeof(T); key.kind = xs.kind;
    std::lock_guard<std::mutex> lk(g_ctx.mu);
    if (g->x_unchanged) {
        int dev = 0;
        (void)hipGetDevice(&dev);
        Context::XsBuf *hit = nullptr;
        for (auto &kv : g_ctx.xs_bufs) {
            Context::XsBuf &b = kv.second;
            // (the padded row count depends on the part's chunk size: a copy made for another ring geometry has another slice stride)
            if (kv.first.first == dev && b.ptr && (const Context::XsKey &)b == key && b.bytes >= xs.bytes && (!hit || b.stamp > hit->stamp)) hit = &b;
        }
        if (hit) {
            hit->stamp = ++g_ctx.xs_clock;
            hit->in_use++;
            pin.hold(hit->ptr);
            *out = hit->ptr;
            return 0;
        }
    }
    Context::XsBuf *b = nullptr;
    if (int rc = xs_buffer_locked(st, std::max<size_t>(xs.bytes, 256), &b)) return rc;
    pin.hold(b->ptr);
    *out = b->ptr;
    (Context::XsKey &)*b = key;
    const uint32_t ncols = (uint32_t)p.ncols, rows_pad = (uint32_t)xs.rows_pad;
    const uint32_t *order = (const uint32_t *)p.lds_col_order;
    // a thread per 16-byte piece of a staged row (half-split: of every padded row)
    const uint64_t threads = xs.kind == 5 ? xs.rows_pad * 16 : (uint64_t)p.ncols * xs.nslices * (xs.row_bytes / 16);
    const dim3 grid((unsigned)((threads + 255) / 256));
    if (xs.kind == 5) {
        if constexpr (sizeof(T) == 4) hipLaunchKernelGGL((k_slice_pack_hs<T>), grid, dim3(256), 0, st, X, ldx, ncols, w, rows_pad, (T *)b->ptr);
    } else if (threads > 0) {
        if constexpr (sizeof(T) == 1)
            hipLaunchKernelGGL(k_slice_pack_widen8, grid, dim3(256), 0, st, (const int8_t *)X, ldx, ncols, w, xs.nslices, (int16_t *)b->ptr, rows_pad, order);
        else if constexpr (sizeof(T) == 8)
            hipLaunchKernelGGL((k_slice_pack<T, 2, 5>), grid, dim3(256), 0, st, X, ldx, ncols, w, xs.nslices, (T *)b->ptr, rows_pad, order);   // 32 pieces per 512-byte row
        else
            hipLaunchKernelGGL((k_slice_pack<T, 16 / (int)sizeof(T), 4>), grid, dim3(256), 0, st, X, ldx, ncols, w, xs.nslices, (T *)b->ptr, rows_pad, order);
    }
    return 0;
}

// the kernels of the LDS-staged product by what lds_plan_launch asks for
using LdsKernelFn = void (*)(LdsArgs);
static LdsKernelFn lds_kernel_fn(const LdsKernelId &k) {
    static const struct { uint32_t key; LdsKernelFn fn; } table[] = {
        {lds_kernel_key(LDS_SH_CODE8, LDS_EL_DBL64), k_lds_code8_f64},
        {lds_kernel_key(LDS_SH_CODE8, LDS_EL_INT64), k_lds_code8_i64},
        {lds_kernel_key(LDS_SH_CODE8, LDS_EL_INT8), k_lds_code8_i8},
        {lds_kernel_key(LDS_SH_CODE8, LDS_EL_INT8, true), k_lds_code8_i8_deq},
        {lds_kernel_key(LDS_SH_CODE8, LDS_EL_INT16), k_lds_code8_i16},
        {lds_kernel_key(LDS_SH_CODE8, LDS_EL_INT16, true), k_lds_code8_i16_deq},
        {lds_kernel_key(LDS_SH_CODE8, LDS_EL_FLT32), k_lds_code8_f32},
        {lds_kernel_key(LDS_SH_CODE8, LDS_EL_FLT32, true), k_lds_code8_f32_deq},
        {lds_kernel_key(LDS_SH_CODE8, LDS_EL_FLT32, false, true), k_lds_code8_f32_ts},
        {lds_kernel_key(LDS_SH_CODE8, LDS_EL_INT32), k_lds_code8_i32},
        {lds_kernel_key(LDS_SH_CODE8, LDS_EL_INT32, true), k_lds_code8_i32_deq},
        {lds_kernel_key(LDS_SH_CODE16, LDS_EL_INT16), k_lds_code_i16},
        {lds_kernel_key(LDS_SH_CODE16, LDS_EL_FLT32), k_lds_code_f32},
        {lds_kernel_key(LDS_SH_CODE16, LDS_EL_FLT32, true), k_lds_code_f32_deq},
        {lds_kernel_key(LDS_SH_CODE16, LDS_EL_INT32), k_lds_code_i32},
        {lds_kernel_key(LDS_SH_CODE16, LDS_EL_INT32, true), k_lds_code_i32_deq},
        {lds_kernel_key(LDS_SH_W16, LDS_EL_INT16), k_lds_spmm_i16_w16},
        {lds_kernel_key(LDS_SH_W16B, LDS_EL_INT16), k_lds_spmm_i16_w16b},
        {lds_kernel_key(LDS_SH_W16_VAL, LDS_EL_INT16), k_lds_spmm_i16_w16_val},
        {lds_kernel_key(LDS_SH_W16, LDS_EL_FLT32), k_lds_spmm_f32_w16},
        {lds_kernel_key(LDS_SH_W16, LDS_EL_FLT32, true), k_lds_spmm_f32_w16_deq},
        {lds_kernel_key(LDS_SH_W16B, LDS_EL_FLT32), k_lds_spmm_f32_w16b},
        {lds_kernel_key(LDS_SH_W16B, LDS_EL_FLT32, true), k_lds_spmm_f32_w16b_deq},
        {lds_kernel_key(LDS_SH_W16_VAL, LDS_EL_FLT32), k_lds_spmm_f32_w16_val},
        {lds_kernel_key(LDS_SH_W8, LDS_EL_FLT32), k_lds_spmm_f32_w8},
        {lds_kernel_key(LDS_SH_W16, LDS_EL_INT32), k_lds_spmm_i32_w16},
        {lds_kernel_key(LDS_SH_W16, LDS_EL_INT32, true), k_lds_spmm_i32_w16_deq},
        {lds_kernel_key(LDS_SH_W16B, LDS_EL_INT32), k_lds_spmm_i32_w16b},
        {lds_kernel_key(LDS_SH_W16B, LDS_EL_INT32, true), k_lds_spmm_i32_w16b_deq},
        {lds_kernel_key(LDS_SH_W16_VAL, LDS_EL_INT32), k_lds_spmm_i32_w16_val},
        {lds_kernel_key(LDS_SH_W8, LDS_EL_INT32), k_lds_spmm_i32_w8},
#ifdef PYGIM_LDS_ABLATE
        // timing experiments (wrong results, scripts/gen_lds_kernel.py; make ablate); an lds_ablate without a variant runs the kernel itself
#define PYGIM_AB(n) {lds_kernel_key(LDS_SH_W16, LDS_EL_FLT32, false, false, n), k_lds_spmm_f32_w16_ab##n}
        PYGIM_AB(6), PYGIM_AB(7), PYGIM_AB(10), PYGIM_AB(11), PYGIM_AB(12), PYGIM_AB(15), PYGIM_AB(16), PYGIM_AB(17), PYGIM_AB(18), PYGIM_AB(19),
#undef PYGIM_AB
#endif
    };
    for (const uint32_t key : {k.key(), lds_kernel_key(k.shell, k.el, k.deq, k.stamp)})
        for (const auto &e : table)
            if (e.key == key) return e.fn;
    return nullptr;
}

// LDS-staged product (lds_kernel_gen.hpp / lds_plan.hpp): X is copied slice-major in 256-byte slices (64 features, rows padded to
// whole 256-column chunks), then ONE launch: a 512-thread workgroup per (tile of rows, slice) streams the tile's chunks of X
// through a double-buffered 160 KiB LDS ring (two chunks of 320 columns) and keeps the tile's running sums in registers; C is written once.
// lds_xs: a slice-major copy the caller already made on this stream (the fused quantiser); deq_amax != nullptr: the store
// dequantises, C is then the FLOAT result (row stride ldc elements of 4 bytes)
template <typename T>
int launch_lds(Group *g, Part &p, const T *X, int64_t ldx, T *C, int64_t ldc, uint32_t w, bool accumulate, hipStream_t st,
               const void *lds_xs = nullptr, const uint32_t *deq_amax = nullptr, int deq_log2 = 0) {
    // 1. the plan: everything that needs no device (lds_launch.hpp)
    LdsLaunchInput in;
    in.dtype = g->dtype; in.p = lds_part_plan(p); in.w = w; in.ldx = ldx; in.ldc = ldc; in.x_aligned256 = ((uintptr_t)X & 255) == 0; in.accumulate = accumulate; in.prestaged = lds_xs != nullptr; in.amax = deq_amax != nullptr;
    in.c_aligned16 = ((uintptr_t)C & 15) == 0; in.stamp = g_tune.lds_stamp != 0; in.l16_batch = LDS_L16_BATCH;
#ifdef PYGIM_LDS_ABLATE
    in.ablate_build = true;
#endif
    const LdsLaunch L = lds_plan_launch(in, lds_launch_knobs());
    if (L.refusal) return fail(PYGIM_ERR_INVALID, L.refusal);
    const LdsKernelFn fn = lds_kernel_fn(L.kernel);
    if (!fn) return fail(PYGIM_ERR_INVALID, "internal: no LDS-staged kernel for this plan");
    KernelTimer kt(g, st, !p.is_extra || p.timed);
    // 2. the staged copy of X, and the scratch block of partial and parked sums: ONE allocation, made before anything is launched into it
    XsPin pin;
    const void *xs = lds_xs;
    if (!xs)
        if (int rc = lds_stage_x<T>(g, p, L.xs, L.x_in_place, X, ldx, w, st, pin, &xs)) return rc;
    if (L.scratch_bytes)
        if (int rc = ensure(&g->scratch, &g->scratch_bytes, L.scratch_bytes)) return rc;   // (grows before the first product only)
    // 3. the arguments
    const uint32_t *kernel_amax = L.kernel_amax ? deq_amax : nullptr;
    LdsArgs a{};
    a.tok = p.lds_tok; a.tiles = p.lds_tiles; a.rowmap = p.lds_rowmap; a.xs = (const char *)xs; a.c = L.to_scratch ? (char *)g->scratch : (char *)C;
    a.slice_stride = L.xs.slice_stride; a.ldc_bytes = L.ldc_bytes; a.w = L.w_lanes; a.nslices = L.xs.nslices; a.ntiles = L.ntiles; a.accumulate = L.accumulate;
    a.wdelta = p.lds_wdelta; a.deq_amax = kernel_amax; a.deq_log2 = deq_log2;
    a.post_mul = kernel_amax ? g->post_mul : nullptr;   // (the per-column epilogue rides the dequantising store only)
    a.post_add = kernel_amax ? g->post_add : nullptr;
    a.post_relu = kernel_amax ? g->post_relu : 0;
    a.xcd_group = L.xcd_group; a.xcd_sx = L.xcd_sx; a.touch_share = L.touch_share; a.half_split = L.half_split; a.xcd_contig = L.xcd_contig;
    if (p.lds_is_code) {
        a.code = p.lds_code; a.code_start = p.lds_code_start; a.piece_bytes = p.lds_code_piece;
    }
    if (L.kernel.stamp) a.stamps = (uint64_t *)(uintptr_t)g_tune.lds_stamp;   // measurement build (scripts/exp_stamps.py)
    // 4. the dynamic-LDS attribute, once per device and kernel
    {
        static std::set<std::pair<int, LdsKernelFn>> attr_done;
        int dev = 0;
        HIP_TRY(hipGetDevice(&dev));
        std::lock_guard<std::mutex> lk(g_ctx.mu);
        if (!attr_done.count({dev, fn})) {
            HIP_TRY(hipFuncSetAttribute((const void *)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_BYTES));
            attr_done.insert({dev, fn});
        }
    }
    // 5. the launch, then the reduce of a column-split plan's partial sums, then the rows the plan leaves to the tail kernels
    hipLaunchKernelGGL(fn, dim3(L.grid), dim3(L.block), LDS_BYTES, st, a);
    g->lds_runs++;
    const dim3 rg((unsigned)((L.reduce_total + 255) / 256));
    const uint32_t S = L.col_splits;
    const int acc = accumulate ? 1 : 0;
    const int16_t *s16 = (const int16_t *)g->scratch;
    const T *sT = (const T *)g->scratch;
    switch (L.reduce) {
        case LDS_RED_16_PLAIN:
            hipLaunchKernelGGL((k_lds_reduce16<0>), rg, dim3(256), 0, st, s16, S, L.lds_rows, w, L.ldp, (void *)C, ldc, acc, nullptr, 0, nullptr, nullptr, 0);
            break;
        case LDS_RED_16_DEQ8:
            hipLaunchKernelGGL((k_lds_reduce16<1>), rg, dim3(256), 0, st, s16, S, L.lds_rows, w, L.ldp, (void *)C, ldc, 0, deq_amax, deq_log2, g->post_mul, g->post_add, g->post_relu);
            break;
        case LDS_RED_16_DEQ16:
            hipLaunchKernelGGL((k_lds_reduce16<2>), rg, dim3(256), 0, st, s16, S, L.lds_rows, w, L.ldp, (void *)C, ldc, 0, deq_amax, deq_log2, g->post_mul, g->post_add, g->post_relu);
            break;
        case LDS_RED_V4:
            if constexpr (sizeof(T) == 4) {
                if (L.deq_at_reduce)
                    hipLaunchKernelGGL((k_lds_reduce_v4<T, true>), rg, dim3(256), 0, st, sT, S, L.lds_rows, w, L.ldp, (void *)C, ldc, 0, deq_amax, deq_log2, g->post_mul, g->post_add, g->post_relu);
                else
                    hipLaunchKernelGGL((k_lds_reduce_v4<T, false>), rg, dim3(256), 0, st, sT, S, L.lds_rows, w, L.ldp, (void *)C, ldc, acc, nullptr, 0, nullptr, nullptr, 0);
            }
            break;
        case LDS_RED_DEQ:
            if constexpr (sizeof(T) == 4)
                hipLaunchKernelGGL((k_lds_reduce_deq<T>), rg, dim3(256), 0, st, sT, S, L.lds_rows, w, L.ldp, (float *)C, ldc, deq_amax, deq_log2, g->post_mul, g->post_add, g->post_relu);
            break;
        case LDS_RED_PLAIN: hipLaunchKernelGGL((k_lds_reduce<T>), rg, dim3(256), 0, st, sT, S, L.lds_rows, w, L.ldp, C, ldc, acc); break;
        default: break;
    }
    if constexpr (sizeof(T) == 4) {
        if (L.tail) {   // the share's last rows, from the same staged copy (k_lds_tail_seg / _fin)
            using A = typename AccOf<T>::type;
            A *parked = (A *)((char *)g->scratch + L.split_bytes);
            const dim3 fin(L.ntail, L.xs.nslices);
            if (p.lds_tail_nseg > 0)   // (rows without entries have no segment: k_lds_tail_fin still writes their zeros)
                hipLaunchKernelGGL((k_lds_tail_seg<T>), dim3(p.lds_tail_nseg, L.xs.nslices), dim3(512), 0, st, p.lds_tail_segs, p.lds_tail_nseg, p.colind, (const char *)xs,
                                   L.xs.slice_stride, parked);
            if (deq_amax)
                hipLaunchKernelGGL((k_lds_tail_fin<T, true>), fin, dim3(64), 0, st, p.lds_tail_rowseg, (uint32_t)L.lds_rows, parked, w, (void *)C, L.tail_ldc_bytes, 0, deq_amax, deq_log2,
                                   g->post_mul, g->post_add, g->post_relu);
            else
                hipLaunchKernelGGL((k_lds_tail_fin<T, false>), fin, dim3(64), 0, st, p.lds_tail_rowseg, (uint32_t)L.lds_rows, parked, w, (void *)C, L.tail_ldc_bytes, acc, nullptr, 0,
                                   nullptr, nullptr, 0);
        }
    }
    kt.stop();
    HIP_TRY(hipGetLastError());
    return 0;
}

template <typename T>
int launch_block(Group *g, Part &p, const void *X, int64_t ldx, void *C, int64_t ldc, int64_t w, bool accumulate,
                 hipStream_t st) {
    const T *x = (const T *)X;
    T *c = (T *)C;
    const uint32_t ww = (uint32_t)w;
    if (lds_takes(g, p, ww, ldc, C, accumulate)) return launch_lds<T>(g, p, x, ldx, c, ldc, ww, accumulate, st);
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
    return g->dtype != PYGIM_INT64 && g->dtype != PYGIM_DBL64 && lds_takes(g, d, w, ldc, C);   // (the density split serves the 1-, 2- and 4-byte types)
}

// true when launch_block_any(g, p, ..., C, ldc, w, accumulate = false) is ONE pass of the LDS-staged product that writes every element of C exactly once and
// reads none (no correction part, no density split adding on top): the call whose C may be the caller's page-locked host tensor (run_group_windows)
static bool lds_writes_c_once(const Group *g, const Part &p, uint32_t w, int64_t ldc, const void *C) {
    return !(p.extra || p.hy_dense || p.hy_sparse || w == 0 || p.nrows == 0) && lds_takes(g, p, w, ldc, C);
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
