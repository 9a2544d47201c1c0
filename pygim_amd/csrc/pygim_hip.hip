// pygim_hip.hip -- host runtime + C ABI (include/pygim_hip.h) of the MI355X
// aggregation backend.  Device code lives in kernels.hpp.
//
// Reference boundary this file replaces, function by function:
//   dpu_init_ranks / dpu_init_dpus / dpu_release   spmm_default/pytorch_api.cpp:154-164
//   spmm_{csr,coo}_to_device_group                 spmm_default/pytorch_api.cpp:204-243, 286-329
//     prepare_pim_{csr,coo} + copy_sparse_{csr,coo}  spmm_mul_csr.c:118-330, spmm_mul_coo.c:83-318
//   spmm_{csr,coo}_run_group                       spmm_default/pytorch_api.cpp:248-280, 332-367
//     spmm_pim_{csr,coo}                             spmm_mul_csr.c:335-561, spmm_mul_coo.c:323-592
//   grande / spmv twins                            spmm_grande/pytorch_api.cpp:221-321,
//                                                  spmv_sparseP/pytorch_api.cpp:184-266
// No CPU compute fallback exists in this file: without a HIP device every entry
// point fails with PYGIM_ERR_NO_DEVICE.
#include "../../include/pygim_hip.h"
#include "kernels.hpp"
#ifdef PYGIM_LDS_ABLATE
#include "lds_kernel_gen_ablate.hpp"   // (make ablate: the same kernels + round 3's timing-experiment variants; not committed)
#else
#include "lds_kernel_gen.hpp"
#endif
#include "lds_codegen_dev.hpp"
#include "lds_reorder_dev.hpp"
#include "lds_hybrid_dev.hpp"
#include "lds_form.hpp"
#include "lds_launch.hpp"
#include "run_plan.hpp"
#include "sweep_plan.hpp"
#include "group_args.hpp"
#include "transpose_dev.hpp"
#include "sddmm_dev.hpp"
#include "row_gather_dev.hpp"
#include "edge_softmax_dev.hpp"
#include "gat_aggregate_dev.hpp"
#include "sparse_attention_dev.hpp"
#include "gatv2_dev.hpp"
#include "spmm_reduce_dev.hpp"
#include "spmm_multi_dev.hpp"
#include "spmm_softmax_dev.hpp"
#include "spmm_edge_dev.hpp"
#include <hsa/hsa.h>
#include <hsa/hsa_ext_amd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <set>
#include <string>
#include <map>
#include <memory>
#include <vector>

using namespace pygim;

namespace {

#include "rt_state.inc"
#include "rt_launch.inc"
#include "rt_plans.inc"

}  // namespace

#include "rt_run.inc"

// the part whose plans the group's queries report: the merged matrix when it serves the products, else part 0
static const Part &serving_part(const Group *g) { return (g->merged && g_tune.merge_parts && g->parts.size() > 1) ? *g->merged : g->parts[0]; }

// ===========================================================================
// C ABI
// ===========================================================================
extern "C" {

const char *pygim_last_error(void) { return g_err.c_str(); }

int pygim_is_initialized(void) { return g_ctx.inited ? 1 : 0; }

int pygim_init_ranks(int64_t nr_ranks, int64_t *units_per_rank) {
    if (nr_ranks <= 0) return fail(PYGIM_ERR_INVALID, "nr_ranks must be positive");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        return fail(PYGIM_ERR_NO_DEVICE, "no HIP device visible (this backend has no CPU fallback)");
    }
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, dev));
    g_ctx.device = dev;
    g_ctx.cu_count = prop.multiProcessorCount;
    g_ctx.nr_ranks = nr_ranks;
    g_ctx.inited = true;
    if (units_per_rank)
        for (int64_t i = 0; i < nr_ranks; i++) units_per_rank[i] = 8;  // one feature window per XCD
    return 0;
}

int pygim_init_units(int64_t nr_units, int64_t *units_per_rank, int64_t *nr_ranks_out) {
    // the reference rounds a DPU count up to whole ranks of 64 (dpu_alloc); here a
    // "unit" is a feature window and a rank holds 8 of them (one per XCD)
    if (nr_units <= 0) return fail(PYGIM_ERR_INVALID, "nr_units must be positive");
    const int64_t ranks = (nr_units + 7) / 8;
    if (nr_ranks_out) *nr_ranks_out = ranks;
    return pygim_init_ranks(ranks, units_per_rank);
}

int pygim_release(void) {
    std::vector<Group *> gs;
    {
        std::lock_guard<std::mutex> lk(g_ctx.mu);
        gs.assign(g_ctx.groups.begin(), g_ctx.groups.end());
        g_ctx.groups.clear();
    }
    if (g_ctx.inited) (void)hipDeviceSynchronize();
    for (Group *g : gs) free_group(g);
    {
        std::lock_guard<std::mutex> lk(g_ctx.mu);
        free_xs_buffers_locked();
    }
    g_ctx.inited = false;
    g_ctx.generation++;
    return 0;
}

int64_t pygim_generation(void) { return g_ctx.generation; }

int pygim_device_info(char *name, int name_len, int *cu_count, int64_t *hbm_bytes) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(PYGIM_ERR_NO_DEVICE, "no HIP device visible");
    }
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, dev));
    if (name && name_len > 0) {
        std::snprintf(name, (size_t)name_len, "%s (%s)", prop.name, prop.gcnArchName);
    }
    if (cu_count) *cu_count = prop.multiProcessorCount;
    if (hbm_bytes) *hbm_bytes = (int64_t)prop.totalGlobalMem;
    return 0;
}

int64_t pygim_set_tunable(const char *name, int64_t value) {
    int64_t *slot = nullptr;
    std::string n = name ? name : "";
    if (n == "long_row_threshold") slot = &g_tune.long_row_threshold;
    else if (n == "long_segment") slot = &g_tune.long_segment;
    else if (n == "force_vec_bytes") slot = &g_tune.force_vec_bytes;
    else if (n == "csr_kernel") slot = &g_tune.csr_kernel;
    else if (n == "coo_chunk") slot = &g_tune.coo_chunk;
    else if (n == "coo_via_rowptr") slot = &g_tune.coo_via_rowptr;
    else if (n == "kernel_events") slot = &g_tune.kernel_events;
    else if (n == "host_windows") slot = &g_tune.host_windows;
    else if (n == "host_direct") slot = &g_tune.host_direct;
    else if (n == "panel_mode") slot = &g_tune.panel_mode;
    else if (n == "panel_bytes") slot = &g_tune.panel_bytes;
    else if (n == "panel_min_seg") slot = &g_tune.panel_min_seg;
    else if (n == "panel_pack") slot = &g_tune.panel_pack;
    else if (n == "panel_coop") slot = &g_tune.panel_coop;
    else if (n == "panel_block") slot = &g_tune.panel_block;
    else if (n == "slice_group_bytes") slot = &g_tune.slice_group_bytes;
    else if (n == "fuse_windows") slot = &g_tune.fuse_windows;
    else if (n == "panel_col16") slot = &g_tune.panel_col16;
    else if (n == "panel_locality") slot = &g_tune.panel_locality;
    else if (n == "split_unit_pattern") slot = &g_tune.split_unit_pattern;
    else if (n == "narrow_vals") slot = &g_tune.narrow_vals;
    else if (n == "merge_parts") slot = &g_tune.merge_parts;
    else if (n == "vec_kernel") slot = &g_tune.vec_kernel;
    else if (n == "vec_lds") slot = &g_tune.vec_lds;
    else if (n == "panel_lds_pad") slot = &g_tune.panel_lds_pad;
    else if (n == "vec_lds_min_seg") slot = &g_tune.vec_lds_min_seg;
    else if (n == "lds_mode") slot = &g_tune.lds_mode;
    else if (n == "lds_min_reuse_x100") slot = &g_tune.lds_min_reuse_x100;
    else if (n == "lds_min_width") slot = &g_tune.lds_min_width;
    else if (n == "lds_min_width8") slot = &g_tune.lds_min_width8;
    else if (n == "lds_min_reuse_narrow_x100") slot = &g_tune.lds_min_reuse_narrow_x100;
    else if (n == "lds_threads") slot = &g_tune.lds_threads;
    else if (n == "lds_waves") slot = &g_tune.lds_waves;
    else if (n == "lds_ablate") slot = &g_tune.lds_ablate;
    else if (n == "lds_round_tiles") slot = &g_tune.lds_round_tiles;
    else if (n == "lds_code") slot = &g_tune.lds_code;
    else if (n == "lds_code_nbuf") slot = &g_tune.lds_code_nbuf;
    else if (n == "lds_code_waves") slot = &g_tune.lds_code_waves;
    else if (n == "lds_fail") slot = &g_tune.lds_fail;
    else if (n == "lds_stamp") slot = &g_tune.lds_stamp;
    else if (n == "lds_code_exp") slot = &g_tune.lds_code_exp;
    else if (n == "lds_hybrid") slot = &g_tune.lds_hybrid;
    else if (n == "lds_hybrid_min") slot = &g_tune.lds_hybrid_min;
    else if (n == "lds_hybrid_contig") slot = &g_tune.lds_hybrid_contig;
    else if (n == "lds_code_boundary") slot = &g_tune.lds_code_boundary;
    else if (n == "lds_xcd_slices") slot = &g_tune.lds_xcd_slices;
    else if (n == "lds_touch_share") slot = &g_tune.lds_touch_share;
    else if (n == "lds_codegen") slot = &g_tune.lds_codegen;
    else if (n == "lds_tile_order") slot = &g_tune.lds_tile_order;
    else if (n == "lds_lp_rounds") slot = &g_tune.lds_lp_rounds;
    else if (n == "lds_code_kc") slot = &g_tune.lds_code_kc;
    else if (n == "lds_code_gsize") slot = &g_tune.lds_code_gsize;
    else if (n == "lds_code_nsets") slot = &g_tune.lds_code_nsets;
    else if (n == "lds_col_split") slot = &g_tune.lds_col_split;
    else if (n == "lds_col_split_f32") slot = &g_tune.lds_col_split_f32;
    else if (n == "lds_fill_tiles") slot = &g_tune.lds_fill_tiles;
    else if (n == "lds_row_tail") slot = &g_tune.lds_row_tail;
    else if (n == "lds_split_order") slot = &g_tune.lds_split_order;
    else if (n == "lds_half_split") slot = &g_tune.lds_half_split;
    else if (n == "lds_direct_x") slot = &g_tune.lds_direct_x;
    else if (n == "lds_long_slots") slot = &g_tune.lds_long_slots;
    if (!slot) {
        fail(PYGIM_ERR_INVALID, "unknown tunable: " + n);
        return -1;
    }
    const int64_t old = *slot;
    if (slot == &g_tune.panel_lds_pad) value = std::min<int64_t>(std::max<int64_t>(value, 0), 64 << 10);  // goes into a launch's dynamic LDS size
    *slot = value;
    return old;
}

}  // extern "C"

// The body of pygim_group_create.  adopt: the (device) arrays of the single part were allocated by the library for this group
// (pygim_group_create_transposed) -- the group owns them from creation on, and they are freed here when creation fails.
static int group_create(int format, int dtype, int n_parts, const int32_t *const *idx0, const int32_t *const *colind,
                        const void *const *values, const int64_t *nrows, const int64_t *ncols, const int64_t *nnz,
                        const int64_t *n_dense, const int64_t *dense_cols, int64_t h_size, int64_t *out_handle, bool adopt) {
    bool adopted = false;
    auto drop_adopted = [&]() {
        if (!adopt || adopted) return;
        adopted = true;
        (void)hipFree(const_cast<int32_t *>(idx0[0]));
        (void)hipFree(const_cast<int32_t *>(colind[0]));
        if (values && values[0]) (void)hipFree(const_cast<void *>(values[0]));
    };
    if (int rc = need_init()) return drop_adopted(), rc;
    const size_t es = dtype_size(dtype);
    const ArgError bad = check_group_args(format, es, n_parts, idx0, colind, nrows, ncols, nnz, n_dense, dense_cols, h_size, out_handle);   // (group_args.hpp)
    if (bad.code) return drop_adopted(), fail(bad.code, bad.text);
    const double t0 = now_ms();
    Group *g = new Group;
    g->format = format;
    g->dtype = dtype;
    t_plan_dtype = dtype;
    g->h = h_size;
    g->total_rows = nrows[0];
    g->parts.resize(n_parts);
    hipStream_t st = nullptr;
    int rc = 0;
    auto bail = [&](int code) {
        (void)hipDeviceSynchronize();
        drop_adopted();
        free_group(g);
        return code;
    };
    if (hipMalloc((void **)&g->d_flags, 8 * sizeof(int)) != hipSuccess) return bail(fail(PYGIM_ERR_HIP, "hipMalloc flags"));
    if (hipMemsetAsync(g->d_flags, 0, 8 * sizeof(int), st) != hipSuccess) return bail(fail(PYGIM_ERR_HIP, "memset flags"));
    if (hipStreamCreateWithFlags(&g->side, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&g->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&g->ev_join, hipEventDisableTiming) != hipSuccess)
        return bail(fail(PYGIM_ERR_HIP, "side stream / events"));
    size_t dpos = 0;
    for (int i = 0; i < n_parts; i++) {
        Part &p = g->parts[i];
        p.nrows = nrows[i];
        p.ncols = ncols[i];
        p.nnz = nnz[i];
        p.dense_cols.assign(dense_cols + dpos, dense_cols + dpos + (size_t)n_dense[i]);
        dpos += (size_t)n_dense[i];
        g->total_cols += p.ncols;
        if ((rc = to_device<uint32_t>(colind[i], (size_t)p.nnz * 4, &p.colind, &p.own_colind, st))) return bail(rc);
        const void *v = values ? values[i] : nullptr;
        if (v) {
            if ((rc = to_device<void>(v, (size_t)p.nnz * es, &p.vals, &p.own_vals, st))) return bail(rc);
        }
        if (format == PYGIM_CSR) {
            if ((rc = to_device<uint32_t>(idx0[i], (size_t)(p.nrows + 1) * 4, &p.rowptr, &p.own_rowptr, st))) return bail(rc);
            if (adopt) {
                p.own_rowptr = p.own_colind = true;
                if (p.vals) p.own_vals = true;
                adopted = true;
            }
            hipLaunchKernelGGL(k_check_csr, dim3((unsigned)((std::max(p.nrows + 1, p.nnz) + 255) / 256)), dim3(256), 0,
                               st, p.rowptr, p.colind, (uint32_t)p.nrows, (uint32_t)p.nnz, (uint32_t)p.ncols,
                               g->d_flags);
        } else {
            if ((rc = to_device<uint32_t>(idx0[i], (size_t)p.nnz * 4, &p.rowind, &p.own_rowind, st))) return bail(rc);
            if (p.nnz > 0)
                hipLaunchKernelGGL(k_check_coo, dim3((unsigned)((p.nnz + 255) / 256)), dim3(256), 0, st, p.rowind,
                                   p.colind, (uint32_t)p.nnz, (uint32_t)p.nrows, (uint32_t)p.ncols, g->d_flags);
            // derived rowptr: the reference also builds a per-row histogram of a COO part at
            // to_device time (spmm_default/pytorch_api.cpp:315-318)
            if (hipMalloc((void **)&p.rowptr, (size_t)(p.nrows + 1) * 4) != hipSuccess)
                return bail(fail(PYGIM_ERR_HIP, "hipMalloc rowptr"));
            p.own_rowptr = true;
            hipLaunchKernelGGL(k_coo_rowptr, dim3((unsigned)((p.nnz + 1 + 255) / 256)), dim3(256), 0, st, p.rowind,
                               (uint32_t)p.nnz, (uint32_t)p.nrows, p.rowptr);
        }
        if (p.vals && p.nnz > 0) {
            int *f = g->d_flags + 2;
            switch (dtype) {
                case PYGIM_INT8: launch_check_ones<int8_t>(p.vals, (uint32_t)p.nnz, f, st); break;
                case PYGIM_INT16: launch_check_ones<int16_t>(p.vals, (uint32_t)p.nnz, f, st); break;
                case PYGIM_INT32: launch_check_ones<int32_t>(p.vals, (uint32_t)p.nnz, f, st); break;
                case PYGIM_INT64: launch_check_ones<int64_t>(p.vals, (uint32_t)p.nnz, f, st); break;
                case PYGIM_FLT32: launch_check_ones<float>(p.vals, (uint32_t)p.nnz, f, st); break;
                case PYGIM_DBL64: launch_check_ones<double>(p.vals, (uint32_t)p.nnz, f, st); break;
            }
        }
    }
    int flags[4] = {0, 0, 0, 0};
    if (hipMemcpy(flags, g->d_flags, sizeof(flags), hipMemcpyDeviceToHost) != hipSuccess)
        return bail(fail(PYGIM_ERR_HIP, std::string("group validation: ") + hipGetErrorString(hipGetLastError())));
    if (const ArgError inv = group_validation_error(format, flags); inv.code) return bail(fail(inv.code, inv.text));
    g->all_ones = (flags[2] == 0);
    // several sparse parts: also one merged matrix (built from the parts as given, before values are dropped or split)
    if (n_parts > 1 && g_tune.merge_parts && (rc = build_merged(g, es, st))) return bail(rc);
    // long-row plan needs rowptr on the host
    for (int i = 0; i < n_parts; i++) {
        Part &p = g->parts[i];
        if (g->all_ones && p.vals) {
            // unit weights: drop the value array from the hot loop (legitimate: 1*x == x exactly)
            if (p.own_vals) (void)hipFree(p.vals);
            p.vals = nullptr;
            p.own_vals = false;
        }
        if (!g->all_ones && (rc = split_unit_pattern(p, dtype, es, g->d_flags + 4, (uint32_t *)(g->d_flags + 5), st))) return bail(rc);
        if ((rc = build_plans(p, es, g->d_flags + 4, st, g->h, /*allow_lds=*/!(g->merged && g_tune.merge_parts)))) return bail(rc);
        if (!(g->merged && g_tune.merge_parts) && (rc = narrow_values(p, dtype, g->d_flags + 6, st))) return bail(rc);
        if (!(g->merged && g_tune.merge_parts) && (rc = build_hybrid(p, dtype, es, g->d_flags + 4, st, g->h))) return bail(rc);
    }
    if (hipDeviceSynchronize() != hipSuccess) return bail(fail(PYGIM_ERR_HIP, "sync after create"));
    g->timers[4] = now_ms() - t0;
    {
        std::lock_guard<std::mutex> lk(g_ctx.mu);
        g->serial = ++g_ctx.group_serial;
        g_ctx.groups.insert(g);
    }
    *out_handle = (int64_t) reinterpret_cast<uintptr_t>(g);
    return 0;
}

extern "C" {

int pygim_group_create(int format, int dtype, int n_parts, const int32_t *const *idx0,
                       const int32_t *const *colind, const void *const *values, const int64_t *nrows,
                       const int64_t *ncols, const int64_t *nnz, const int64_t *n_dense,
                       const int64_t *dense_cols, int64_t h_size, int64_t *out_handle) {
    return group_create(format, dtype, n_parts, idx0, colind, values, nrows, ncols, nnz, n_dense, dense_cols, h_size,
                        out_handle, /*adopt=*/false);
}

int pygim_group_create_transposed(int format, int dtype, int n_parts, const int32_t *const *idx0,
                                  const int32_t *const *colind, const void *const *values, const int64_t *nrows,
                                  const int64_t *ncols, const int64_t *nnz, const int64_t *n_dense,
                                  const int64_t *dense_cols, int64_t h_size, int64_t *out_handle) {
    // the argument checks of pygim_group_create (group_args.hpp), then its validation kernels on the input as given
    if (int rc = need_init()) return rc;
    const size_t es = dtype_size(dtype);
    const ArgError bad = check_group_args(format, es, n_parts, idx0, colind, nrows, ncols, nnz, n_dense, dense_cols, h_size, out_handle);
    if (bad.code) return fail(bad.code, bad.text);
    uint64_t total_cols = 0, total_nnz = 0;
    for (int i = 0; i < n_parts; i++) {
        total_cols += (uint64_t)ncols[i];
        total_nnz += (uint64_t)nnz[i];
    }
    if (total_cols >= 0xFFFFFFFFull || total_nnz > 0xFFFFFFFFull)
        return fail(PYGIM_ERR_INVALID, "A^T must fit 32-bit indices: sum(ncols) rows, sum(nnz) entries");
    hipStream_t st = nullptr;
    // the input on the device: host arrays uploaded once, device arrays used in place
    struct Held { void *p = nullptr; bool own = false; };
    std::vector<Held> held;
    int *d_flags = nullptr;
    auto release_input = [&]() {
        (void)hipDeviceSynchronize();
        for (Held &x : held)
            if (x.own && x.p) (void)hipFree(x.p);
        held.clear();
        if (d_flags) (void)hipFree(d_flags);
        d_flags = nullptr;
    };
    auto bail = [&](int code) {
        release_input();
        return code;
    };
    if (hipMalloc((void **)&d_flags, 8 * sizeof(int)) != hipSuccess) return bail(fail(PYGIM_ERR_HIP, "hipMalloc flags"));
    if (hipMemsetAsync(d_flags, 0, 8 * sizeof(int), st) != hipSuccess) return bail(fail(PYGIM_ERR_HIP, "memset flags"));
    std::vector<TrPart> tp(n_parts);
    int rc = 0;
    for (int i = 0; i < n_parts; i++) {
        const uint32_t nr = (uint32_t)nrows[i], nc = (uint32_t)ncols[i], nz = (uint32_t)nnz[i];
        Held hc, hi, hv;
        uint32_t *d_col = nullptr, *d_idx = nullptr;
        void *d_val = nullptr;
        rc = to_device<uint32_t>(colind[i], (size_t)nz * 4, &d_col, &hc.own, st);
        hc.p = d_col;
        held.push_back(hc);
        if (rc) return bail(rc);
        const size_t idx_bytes = format == PYGIM_CSR ? (size_t)(nr + 1ull) * 4 : (size_t)nz * 4;
        rc = to_device<uint32_t>(idx0[i], idx_bytes, &d_idx, &hi.own, st);
        hi.p = d_idx;
        held.push_back(hi);
        if (rc) return bail(rc);
        const void *v = values ? values[i] : nullptr;
        if (v) {
            rc = to_device<void>(v, (size_t)nz * es, &d_val, &hv.own, st);
            hv.p = d_val;
            held.push_back(hv);
            if (rc) return bail(rc);
        }
        if (format == PYGIM_CSR) {
            hipLaunchKernelGGL(k_check_csr, dim3((unsigned)((std::max<uint64_t>(nr + 1ull, nz) + 255) / 256)), dim3(256), 0, st, d_idx, d_col, nr, nz,
                               nc, d_flags);
        } else if (nz > 0) {
            hipLaunchKernelGGL(k_check_coo, dim3((unsigned)((nz + 255) / 256)), dim3(256), 0, st, d_idx, d_col, nz, nr, nc, d_flags);
        }
        tp[i] = TrPart{d_idx, d_col, d_val, nr, nc, nz, format == PYGIM_CSR ? 1 : 0};
    }
    int flags[4] = {0, 0, 0, 0};
    if (hipMemcpy(flags, d_flags, sizeof(flags), hipMemcpyDeviceToHost) != hipSuccess)
        return bail(fail(PYGIM_ERR_HIP, std::string("group validation: ") + hipGetErrorString(hipGetLastError())));
    if (const ArgError inv = group_validation_error(format, flags); inv.code) return bail(fail(inv.code, inv.text));
    // the transpose (transpose_dev.hpp), then the creation path of any group: unit weights, plans, code streams and fallbacks as usual
    uint32_t *rowptrT = nullptr, *colT = nullptr;
    void *valsT = nullptr;
    uint64_t nT = 0, nnzT = 0;
    std::string err;
    switch (dtype) {
        case PYGIM_INT8: rc = tr_build_t<uint8_t>(tp, (uint8_t)1, &rowptrT, &colT, &valsT, &nT, &nnzT, st, &err); break;
        case PYGIM_INT16: rc = tr_build_t<uint16_t>(tp, (uint16_t)1, &rowptrT, &colT, &valsT, &nT, &nnzT, st, &err); break;
        case PYGIM_INT32: rc = tr_build_t<uint32_t>(tp, 1u, &rowptrT, &colT, &valsT, &nT, &nnzT, st, &err); break;
        case PYGIM_INT64: rc = tr_build_t<uint64_t>(tp, 1ull, &rowptrT, &colT, &valsT, &nT, &nnzT, st, &err); break;
        case PYGIM_FLT32: rc = tr_build_t<uint32_t>(tp, 0x3F800000u, &rowptrT, &colT, &valsT, &nT, &nnzT, st, &err); break;
        default: rc = tr_build_t<uint64_t>(tp, 0x3FF0000000000000ull, &rowptrT, &colT, &valsT, &nT, &nnzT, st, &err); break;
    }
    release_input();
    if (rc) return fail(rc, err);
    const int32_t *idx_t[1] = {(const int32_t *)rowptrT}, *col_t[1] = {(const int32_t *)colT};
    const void *val_t[1] = {valsT};
    const int64_t nrows_t[1] = {(int64_t)nT}, ncols_t[1] = {nrows[0]}, nnz_t[1] = {(int64_t)nnzT}, nd_t[1] = {1}, dc_t[1] = {h_size};
    return group_create(PYGIM_CSR, dtype, 1, idx_t, col_t, valsT ? val_t : nullptr, nrows_t, ncols_t, nnz_t, nd_t, dc_t, h_size, out_handle,
                        /*adopt=*/true);
}

int pygim_group_free(int64_t handle) {
    Group *g = lookup(handle);
    if (!g) return fail(PYGIM_ERR_INVALID, "unknown group handle");
    bool last = false;
    {
        std::lock_guard<std::mutex> lk(g_ctx.mu);
        g_ctx.groups.erase(g);
        last = g_ctx.groups.empty();
    }
    (void)hipDeviceSynchronize();
    free_group(g);
    if (last) {  // the slice-major copies belong to the products of live groups: none left, none kept
        std::lock_guard<std::mutex> lk(g_ctx.mu);
        free_xs_buffers_locked();
    }
    return 0;
}

int pygim_quant_spmm_run(int64_t handle, const float *X, int64_t ldx, float *out, float *scale_out, void *stream) {
    return pygim_quant_spmm_run_post(handle, X, ldx, out, scale_out, nullptr, nullptr, 0, stream);
}

int pygim_quant_spmm_run_post(int64_t handle, const float *X, int64_t ldx, float *out, float *scale_out, const float *col_mul,
                              const float *col_add, int relu, void *stream) {
    if (int rc = need_init()) return rc;
    Group *g = lookup(handle);
    if (!g) return fail(PYGIM_ERR_INVALID, "unknown group handle");
    if ((col_mul == nullptr) != (col_add == nullptr)) return fail(PYGIM_ERR_INVALID, "col_mul and col_add come together");
    if (col_mul && (!is_device_ptr(col_mul) || !is_device_ptr(col_add))) return fail(PYGIM_ERR_INVALID, "epilogue vectors must be device memory");
    struct PostGuard {
        Group *g;
        ~PostGuard() { g->post_mul = g->post_add = nullptr; g->post_relu = 0; }
    } guard{g};
    g->post_mul = col_mul;
    g->post_add = col_add;
    g->post_relu = col_mul ? relu : 0;
    if (!X || !out || ldx < g->h) return fail(PYGIM_ERR_INVALID, "bad X / out / ldx");
    if (!is_device_ptr(X) || !is_device_ptr(out) || (scale_out && !is_device_ptr(scale_out)))
        return fail(PYGIM_ERR_INVALID, "pygim_quant_spmm_run needs device pointers");
    for (auto &p : g->parts)
        if (p.dense_cols != g->parts[0].dense_cols) return fail(PYGIM_ERR_INVALID, "needs one dense split for all parts");
    hipStream_t st = (hipStream_t)stream;
    switch (g->dtype) {  // ranges of models/quantize.py:22-30
        case PYGIM_INT8: return quant_run_t<int8_t>(g, X, ldx, out, scale_out, 5, st);
        case PYGIM_INT16: return quant_run_t<int16_t>(g, X, ldx, out, scale_out, 10, st);
        case PYGIM_INT32: return quant_run_t<int32_t>(g, X, ldx, out, scale_out, 20, st);
        case PYGIM_FLT32: return quant_run_t<float>(g, X, ldx, out, scale_out, 20, st);
        default: return fail(PYGIM_ERR_INVALID, "quantised run: group type must be INT8/INT16/INT32/FLT32");
    }
}

int pygim_spmm_run_dequant(int64_t handle, const void *Xq, int64_t ldx, float *out, const uint32_t *absmax_bits, void *stream) {
    if (int rc = need_init()) return rc;
    Group *g = lookup(handle);
    if (!g) return fail(PYGIM_ERR_INVALID, "unknown group handle");
    if (!Xq || !out || !absmax_bits || ldx < g->h) return fail(PYGIM_ERR_INVALID, "bad Xq / out / absmax / ldx");
    if (!is_device_ptr(Xq) || !is_device_ptr(out) || !is_device_ptr(absmax_bits))
        return fail(PYGIM_ERR_INVALID, "pygim_spmm_run_dequant needs device pointers");
    for (auto &p : g->parts)
        if (p.dense_cols != g->parts[0].dense_cols) return fail(PYGIM_ERR_INVALID, "needs one dense split for all parts");
    const int k = quant_log2_range(g->dtype);
    hipStream_t st = (hipStream_t)stream;
    switch (g->dtype) {
        case PYGIM_INT8: return dequant_run_t<int8_t>(g, Xq, ldx, out, absmax_bits, k, st);
        case PYGIM_INT16: return dequant_run_t<int16_t>(g, Xq, ldx, out, absmax_bits, k, st);
        case PYGIM_INT32: return dequant_run_t<int32_t>(g, Xq, ldx, out, absmax_bits, k, st);
        case PYGIM_FLT32: return dequant_run_t<float>(g, Xq, ldx, out, absmax_bits, k, st);
        default: return fail(PYGIM_ERR_INVALID, "dequantising run: group type must be INT8/INT16/INT32/FLT32");
    }
}

int pygim_quant_absmax(const float *X, int64_t ldx, int64_t rows, int64_t width, uint32_t *absmax_bits, void *stream) {
    if (int rc = need_init()) return rc;
    if (rows < 0 || width < 0 || ldx < width || !absmax_bits) return fail(PYGIM_ERR_INVALID, "bad absmax arguments");
    if ((rows * width > 0 && (!X || !is_device_ptr(X))) || !is_device_ptr(absmax_bits))
        return fail(PYGIM_ERR_INVALID, "pygim_quant_absmax needs device pointers");
    return launch_absmax(X, ldx, (uint64_t)rows, (uint32_t)width, absmax_bits, (hipStream_t)stream);
}

int pygim_quantize(int dtype, const float *X, int64_t ldx, int64_t rows, int64_t width, const uint32_t *absmax_bits,
                   void *Xq, float *scale_out, void *stream) {
    if (int rc = need_init()) return rc;
    const int k = quant_log2_range(dtype);
    if (k < 0) return fail(PYGIM_ERR_INVALID, "quantise: type must be INT8/INT16/INT32/FLT32");
    if (rows < 0 || width < 0 || ldx < width || !absmax_bits) return fail(PYGIM_ERR_INVALID, "bad quantise arguments");
    if (rows * width > 0 && (!X || !Xq || !is_device_ptr(X) || !is_device_ptr(Xq)))
        return fail(PYGIM_ERR_INVALID, "pygim_quantize needs device pointers");
    hipStream_t st = (hipStream_t)stream;
    const uint64_t r = (uint64_t)rows;
    const uint32_t w = (uint32_t)width;
    switch (dtype) {
        case PYGIM_INT8: return launch_quantize<int8_t>(X, ldx, r, w, absmax_bits, k, (int8_t *)Xq, scale_out, st);
        case PYGIM_INT16: return launch_quantize<int16_t>(X, ldx, r, w, absmax_bits, k, (int16_t *)Xq, scale_out, st);
        case PYGIM_INT32: return launch_quantize<int32_t>(X, ldx, r, w, absmax_bits, k, (int32_t *)Xq, scale_out, st);
        default: return launch_quantize<float>(X, ldx, r, w, absmax_bits, k, (float *)Xq, scale_out, st);
    }
}

int pygim_dequantize(int dtype, const void *Q, int64_t n, const uint32_t *absmax_bits, float *out, void *stream) {
    if (int rc = need_init()) return rc;
    const int k = quant_log2_range(dtype);
    if (k < 0) return fail(PYGIM_ERR_INVALID, "dequantise: type must be INT8/INT16/INT32/FLT32");
    if (n < 0 || !absmax_bits) return fail(PYGIM_ERR_INVALID, "bad dequantise arguments");
    if (n > 0 && (!Q || !out || !is_device_ptr(Q) || !is_device_ptr(out)))
        return fail(PYGIM_ERR_INVALID, "pygim_dequantize needs device pointers");
    hipStream_t st = (hipStream_t)stream;
    switch (dtype) {
        case PYGIM_INT8: return launch_dequantize<int8_t>((const int8_t *)Q, (uint64_t)n, absmax_bits, k, out, st);
        case PYGIM_INT16: return launch_dequantize<int16_t>((const int16_t *)Q, (uint64_t)n, absmax_bits, k, out, st);
        case PYGIM_INT32: return launch_dequantize<int32_t>((const int32_t *)Q, (uint64_t)n, absmax_bits, k, out, st);
        default: return launch_dequantize<float>((const float *)Q, (uint64_t)n, absmax_bits, k, out, st);
    }
}

}  // extern "C"

// ---- functional entry points on a caller's CSR: sddmm, spmm_values, edge_softmax, gat_aggregate, spmm_reduce and its backward, spmm_multi_reduce, spmm_softmax and its backward, spmm_edge / spmm_edge_softmax and their backward ----
// f(T()) with T the element type of `dtype` (the caller has checked it); INTS = false: FLT32 / DBL64 only
template <bool INTS = false, typename F> static void with_elem_type(int dtype, F &&f) {
    if constexpr (INTS) {
        switch (dtype) {
            case PYGIM_INT8: return f(int8_t());
            case PYGIM_INT16: return f(int16_t());
            case PYGIM_INT32: return f(int32_t());
            case PYGIM_INT64: return f(int64_t());
        }
    }
    if (dtype == PYGIM_FLT32) f(float());
    else f(double());
}

static bool is_float_type(int dtype) { return dtype == PYGIM_FLT32 || dtype == PYGIM_DBL64; }

// The gather family (sddmm, spmm_values, gat_aggregate, spmm_reduce MEAN) also takes 16-bit features: X / G / out are stored as
// PYGIM_FLT16 or PYGIM_BF16 while values, a_dst, a_src, lse, the sddmm result and the workspace slots are float32.  dtype_size() stays 0 for
// the two codes (group creation and every other entry point reject them through it); these entry points ask here instead.
static bool is_half_type(int dtype) { return dtype == PYGIM_FLT16 || dtype == PYGIM_BF16; }
static bool is_gather_type(int dtype) { return is_float_type(dtype) || is_half_type(dtype); }
// bytes of an element of X / out, and of everything that is computed (values, partials, slots)
static size_t gather_storage_size(int dtype) { return is_half_type(dtype) ? 2 : dtype_size(dtype); }
static size_t gather_compute_size(int dtype) { return is_half_type(dtype) ? sizeof(float) : dtype_size(dtype); }
// f(T(), S()) with T the compute and S the storage type of `dtype` (is_gather_type: the caller has checked it)
template <typename F> static void with_gather_types(int dtype, F &&f) {
    switch (dtype) {
        case PYGIM_FLT16: return f(float(), _Float16());
        case PYGIM_BF16: return f(float(), __bf16());
        case PYGIM_FLT32: return f(float(), float());
        default: return f(double(), double());
    }
}

// a pointer argument: checked when the call will use it (`used`: rows > 0, nnz > 0, ...) -- not null unless `optional`, and device memory
struct PtrArg {
    const void *p;
    bool used, optional = false;
};

// the checks these entry points share, in their order; op names the entry point in the messages, `names` its pointers, ld0 / ld1 are
// the two row strides, need_ws what pygim_<op>_workspace returns (<= 0: no workspace)
static int check_csr_call(const char *op, const char *names, int64_t nrows, int64_t nnz, int64_t nnz_max, int64_t h, int64_t h_max, int64_t ld0, int64_t ld1,
                          std::initializer_list<PtrArg> ptrs, int64_t need_ws = 0, const void *workspace = nullptr, int64_t workspace_bytes = 0) {
    const std::string o(op);
    if (nrows < 0 || nrows >= 0xFFFFFFFFll || nnz < 0 || nnz > nnz_max || h < 1 || h > h_max || ld0 < h || ld1 < h)
        return fail(PYGIM_ERR_INVALID, "bad " + o + " sizes / strides");
    if (nnz > 0 && nrows == 0) return fail(PYGIM_ERR_INVALID, o + ": entries without rows");
    for (const PtrArg &a : ptrs)
        if (a.used && !a.optional && !a.p) return fail(PYGIM_ERR_INVALID, std::string("bad ") + names);
    for (const PtrArg &a : ptrs)
        if (a.used && a.p && !is_device_ptr(a.p)) return fail(PYGIM_ERR_INVALID, "pygim_" + o + " needs device pointers");
    if (need_ws > 0 && (!workspace || workspace_bytes < need_ws || (uintptr_t)workspace % 16 != 0 || !is_device_ptr(workspace)))
        return fail(PYGIM_ERR_INVALID, o + ": workspace too small, misaligned or not device memory (pygim_" + o + "_workspace)");
    return 0;
}

extern "C" {

int pygim_sddmm(int dtype, int64_t nrows, const int32_t *rowptr, const int32_t *colind, int64_t nnz, const void *G, int64_t ldg,
                const void *X, int64_t ldx, int64_t h, void *out, void *stream) {
    if (int rc = need_init()) return rc;
    if (!is_gather_type(dtype)) return fail(PYGIM_ERR_INVALID, "sddmm: type must be FLT32, DBL64, FLT16 or BF16");
    if (int rc = check_csr_call("sddmm", "rowptr / colind / G / X / out", nrows, nnz, 0xFFFFFFFFll - SD_EPW, h, 0xFFFFFFFFll, ldg, ldx,
                                {{rowptr, true}, {colind, nnz > 0}, {G, nnz > 0}, {X, nnz > 0}, {out, nnz > 0}}))
        return rc;
    if (nnz == 0) return 0;
    with_gather_types(dtype, [&](auto t, auto s) {
        using T = decltype(t);
        using S = decltype(s);
        launch_sddmm<T, S>((const uint32_t *)rowptr, (const uint32_t *)colind, (uint32_t)nrows, (uint32_t)nnz, (const S *)G, (uint64_t)ldg, (const S *)X,
                           (uint64_t)ldx, (uint32_t)h, (T *)out, (hipStream_t)stream);
    });
    HIP_TRY(hipGetLastError());
    return 0;
}

int64_t pygim_spmm_values_workspace(int dtype, int64_t nrows, int64_t nnz, int64_t h, int64_t heads) {
    (void)nrows;
    (void)heads;
    if (!is_gather_type(dtype) || nnz < 0 || h < 1 || h > (int64_t)RG_MAX_H) return -1;
    return (int64_t)row_gather_slot_bytes((uint64_t)nnz, (uint64_t)h, gather_compute_size(dtype));
}

int64_t pygim_edge_softmax_workspace(int dtype, int64_t nrows, int64_t nnz, int64_t heads) {
    (void)nrows;
    if (!is_float_type(dtype) || nnz < 0 || heads < 1) return -1;
    return (int64_t)edge_softmax_workspace_bytes((uint64_t)nnz, (uint64_t)heads, dtype_size(dtype));
}

int pygim_spmm_values(int dtype, int64_t nrows, const int32_t *rowptr, const int32_t *colind, int64_t nnz, const void *values, int64_t heads,
                      const void *X, int64_t ldx, int64_t h, void *out, int64_t ldo, void *workspace, int64_t workspace_bytes, void *stream) {
    if (int rc = need_init()) return rc;
    if (!is_gather_type(dtype)) return fail(PYGIM_ERR_INVALID, "spmm_values: type must be FLT32, DBL64, FLT16 or BF16");
    if (h >= 1 && (heads < 1 || h % heads != 0)) return fail(PYGIM_ERR_INVALID, "spmm_values: heads must divide h");
    if (int rc = check_csr_call("spmm_values", "rowptr / colind / values / X / out", nrows, nnz, 0x7FFFFFFFll, h, (int64_t)RG_MAX_H, ldx, ldo,
                                {{rowptr, true}, {out, nrows > 0}, {colind, nnz > 0}, {values, nnz > 0}, {X, nnz > 0}},
                                pygim_spmm_values_workspace(dtype, nrows, nnz, h, heads), workspace, workspace_bytes))
        return rc;
    with_gather_types(dtype, [&](auto t, auto s) {
        using T = decltype(t);
        using S = decltype(s);
        launch_row_gather<T, FoldSum<false>, S>((const uint32_t *)rowptr, (const uint32_t *)colind, (uint32_t)nrows, (uint32_t)nnz, (const T *)values,
                                                (uint32_t)heads, (const S *)X, (uint64_t)ldx, (uint32_t)h, (S *)out, (uint64_t)ldo, nullptr, workspace,
                                                (hipStream_t)stream);
    });
    HIP_TRY(hipGetLastError());
    return 0;
}

int64_t pygim_gat_aggregate_workspace(int dtype, int64_t nrows, int64_t nnz, int64_t h, int64_t heads) {
    (void)nrows;
    if (!is_gather_type(dtype) || nnz < 0 || h < 1 || h > (int64_t)RG_MAX_H || heads < 1 || h % heads != 0) return -1;
    return (int64_t)gat_workspace_bytes((uint64_t)nnz, (uint64_t)h, (uint64_t)heads, gather_compute_size(dtype));
}

// attention dropout: the rate of the *_dropout entry points (0 <= p < 1; NaN fails the first comparison)
static bool bad_dropout(double p) { return !(p >= 0.0 && p < 1.0); }

// p = 0 launches the instantiation without dropout: the base entry point and its bits.  edge: the call takes a per-entry term a_edge
// [nnz, heads] (pygim_gat_aggregate_edge) and launches the EDGE instantiations
static int gat_aggregate_call(int dtype, int64_t nrows, const int32_t *rowptr, const int32_t *colind, int64_t nnz, const void *a_dst, const void *a_src,
                              int64_t heads, double negative_slope, const void *X, int64_t ldx, int64_t h, void *out, int64_t ldo, void *lse,
                              void *workspace, int64_t workspace_bytes, void *stream, double p, uint64_t seed, bool edge = false,
                              const void *a_edge = nullptr) {
    if (bad_dropout(p)) return fail(PYGIM_ERR_INVALID, "gat_aggregate: the dropout rate must lie in [0, 1)");
    if (edge && nnz > 0 && !a_edge) return fail(PYGIM_ERR_INVALID, "gat_aggregate_edge: a_edge is NULL");
    if (int rc = need_init()) return rc;
    if (!is_gather_type(dtype)) return fail(PYGIM_ERR_INVALID, "gat_aggregate: type must be FLT32, DBL64, FLT16 or BF16");
    if (h >= 1 && (heads < 1 || h % heads != 0)) return fail(PYGIM_ERR_INVALID, "gat_aggregate: heads must divide h");
    if (int rc = check_csr_call("gat_aggregate", "rowptr / colind / a_dst / a_src / X / out", nrows, nnz, 0x7FFFFFFFll, h, (int64_t)RG_MAX_H, ldx, ldo,
                                {{rowptr, true}, {out, nrows > 0}, {lse, nrows > 0, true}, {colind, nnz > 0}, {a_dst, nnz > 0}, {a_src, nnz > 0}, {X, nnz > 0},
                                 {a_edge, edge && nnz > 0}},
                                pygim_gat_aggregate_workspace(dtype, nrows, nnz, h, heads), workspace, workspace_bytes))
        return rc;
    with_gather_types(dtype, [&](auto t, auto s) {
        using T = decltype(t);
        using S = decltype(s);
        if (edge && p > 0.0)
            launch_gat_aggregate<T, S, true, true>((const uint32_t *)rowptr, (const uint32_t *)colind, (uint32_t)nrows, (uint32_t)nnz, (const T *)a_dst,
                                                   (const T *)a_src, (uint32_t)heads, (T)negative_slope, (const S *)X, (uint64_t)ldx, (uint32_t)h, (S *)out,
                                                   (uint64_t)ldo, (T *)lse, workspace, (hipStream_t)stream, attn_dropout_args<T>(p, seed), (const T *)a_edge);
        else if (edge)
            launch_gat_aggregate<T, S, false, true>((const uint32_t *)rowptr, (const uint32_t *)colind, (uint32_t)nrows, (uint32_t)nnz, (const T *)a_dst,
                                                    (const T *)a_src, (uint32_t)heads, (T)negative_slope, (const S *)X, (uint64_t)ldx, (uint32_t)h, (S *)out,
                                                    (uint64_t)ldo, (T *)lse, workspace, (hipStream_t)stream, AttnDrop<T>(), (const T *)a_edge);
        else if (p > 0.0)
            launch_gat_aggregate<T, S, true>((const uint32_t *)rowptr, (const uint32_t *)colind, (uint32_t)nrows, (uint32_t)nnz, (const T *)a_dst,
                                             (const T *)a_src, (uint32_t)heads, (T)negative_slope, (const S *)X, (uint64_t)ldx, (uint32_t)h, (S *)out,
                                             (uint64_t)ldo, (T *)lse, workspace, (hipStream_t)stream, attn_dropout_args<T>(p, seed));
        else
            launch_gat_aggregate<T, S>((const uint32_t *)rowptr, (const uint32_t *)colind, (uint32_t)nrows, (uint32_t)nnz, (const T *)a_dst, (const T *)a_src,
                                       (uint32_t)heads, (T)negative_slope, (const S *)X, (uint64_t)ldx, (uint32_t)h, (S *)out, (uint64_t)ldo, (T *)lse, workspace,
                                       (hipStream_t)stream);
    });
    HIP_TRY(hipGetLastError());
    return 0;
}

int pygim_gat_aggregate(int dtype, int64_t nrows, const int32_t *rowptr, const int32_t *colind, int64_t nnz, const void *a_dst, const void *a_src,
                        int64_t heads, double negative_slope, const void *X, int64_t ldx, int64_t h, void *out, int64_t ldo, void *lse, void *workspace,
                        int64_t workspace_bytes, void *stream) {
    return gat_aggregate_call(dtype, nrows, rowptr, colind, nnz, a_dst, a_src, heads, negative_slope, X, ldx, h, out, ldo, lse, workspace, workspace_bytes,
                              stream, 0.0, 0);
}

int pygim_gat_aggregate_dropout(int dtype, int64_t nrows, const int32_t *rowptr, const int32_t *colind, int64_t nnz, const void *a_dst, const void *a_src,
                                int64_t heads, double negative_slope, const void *X, int64_t ldx, int64_t h, void *out, int64_t ldo, void *lse,
                                void *workspace, int64_t workspace_bytes, void *stream, double p, uint64_t seed) {
    return gat_aggregate_call(dtype, nrows, rowptr, colind, nnz, a_dst, a_src, heads, negative_slope, X, ldx, h, out, ldo, lse, workspace, workspace_bytes,
                              stream, p, seed);
}

int pygim_gat_aggregate_edge(int dtype, int64_t nrows, const int32_t *rowptr, const int32_t *colind, int64_t nnz, const void *a_dst, const void *a_src,
                             int64_t heads, double negative_slope, const void *X, int64_t ldx, int64_t h, void *out, int64_t ldo, void *lse,
                             void *workspace, int64_t workspace_bytes, void *stream, const void *a_edge, double p, uint64_t seed) {
    return gat_aggregate_call(dtype, nrows, rowptr, colind, nnz, a_dst, a_src, heads, negative_slope, X, ldx, h, out, ldo, lse, workspace, workspace_bytes,
                              stream, p, seed, true, a_edge);
}

int64_t pygim_sparse_attention_workspace(int dtype, int64_t nrows, int64_t nnz, int64_t h, int64_t heads) {
    (void)nrows;
    if (!is_gather_type(dtype) || nnz < 0 || h < 1 || heads < 1 || h % heads != 0 || h / heads > (int64_t)SA_MAX_HEAD) return -1;
    return (int64_t)gat_workspace_bytes((uint64_t)nnz, (uint64_t)h, (uint64_t)heads, gather_compute_size(dtype));
}

static int sparse_attention_call(int dtype, int64_t nrows, const int32_t *rowptr, const int32_t *colind, int64_t nnz, const void *Q, int64_t ldq,
                                 const void *K, int64_t ldk, const void *V, int64_t ldv, int64_t h, int64_t heads, double scale, void *out, int64_t ldo,
                                 void *lse, void *workspace, int64_t workspace_bytes, void *stream, double p, uint64_t seed, bool edge = false,
                                 const void *bias = nullptr) {
    if (bad_dropout(p)) return fail(PYGIM_ERR_INVALID, "sparse_attention: the dropout rate must lie in [0, 1)");
    if (edge && nnz > 0 && !bias) return fail(PYGIM_ERR_INVALID, "sparse_attention_bias: bias is NULL");
    if (int rc = need_init()) return rc;
    if (!is_gather_type(dtype)) return fail(PYGIM_ERR_INVALID, "sparse_attention: type must be FLT32, DBL64, FLT16 or BF16");
    if (h >= 1 && (heads < 1 || h % heads != 0)) return fail(PYGIM_ERR_INVALID, "sparse_attention: heads must divide h");
    if (h >= 1 && h / heads > (int64_t)SA_MAX_HEAD) return fail(PYGIM_ERR_INVALID, "sparse_attention: a head is at most 256 features wide");
    if (int rc = check_csr_call("sparse_attention", "rowptr / colind / Q / K / V / out", nrows, nnz, 0x7FFFFFFFll, h, 0x7FFFFFFFll, ldq < ldk ? ldq : ldk,
                                ldv < ldo ? ldv : ldo,
                                {{rowptr, true}, {out, nrows > 0}, {lse, nrows > 0, true}, {colind, nnz > 0}, {Q, nnz > 0}, {K, nnz > 0}, {V, nnz > 0},
                                 {bias, edge && nnz > 0}},
                                pygim_sparse_attention_workspace(dtype, nrows, nnz, h, heads), workspace, workspace_bytes))
        return rc;
    with_gather_types(dtype, [&](auto t, auto s) {
        using T = decltype(t);
        using S = decltype(s);
        if (edge && p > 0.0)
            launch_sparse_attention<T, S, true, true>((const uint32_t *)rowptr, (const uint32_t *)colind, (uint32_t)nrows, (uint32_t)nnz, (const S *)Q,
                                                      (uint64_t)ldq, (const S *)K, (uint64_t)ldk, (const S *)V, (uint64_t)ldv, (uint32_t)h, (uint32_t)heads,
                                                      (T)scale, (S *)out, (uint64_t)ldo, (T *)lse, workspace, (hipStream_t)stream,
                                                      attn_dropout_args<T>(p, seed), (const T *)bias);
        else if (edge)
            launch_sparse_attention<T, S, false, true>((const uint32_t *)rowptr, (const uint32_t *)colind, (uint32_t)nrows, (uint32_t)nnz, (const S *)Q,
                                                       (uint64_t)ldq, (const S *)K, (uint64_t)ldk, (const S *)V, (uint64_t)ldv, (uint32_t)h, (uint32_t)heads,
                                                       (T)scale, (S *)out, (uint64_t)ldo, (T *)lse, workspace, (hipStream_t)stream, AttnDrop<T>(),
                                                       (const T *)bias);
        else if (p > 0.0)
            launch_sparse_attention<T, S, true>((const uint32_t *)rowptr, (const uint32_t *)colind, (uint32_t)nrows, (uint32_t)nnz, (const S *)Q, (uint64_t)ldq,
                                                (const S *)K, (uint64_t)ldk, (const S *)V, (uint64_t)ldv, (uint32_t)h, (uint32_t)heads, (T)scale, (S *)out,
                                                (uint64_t)ldo, (T *)lse, workspace, (hipStream_t)stream, attn_dropout_args<T>(p, seed));
        else
            launch_sparse_attention<T, S>((const uint32_t *)rowptr, (const uint32_t *)colind, (uint32_t)nrows, (uint32_t)nnz, (const S *)Q, (uint64_t)ldq,
                                          (const S *)K, (uint64_t)ldk, (const S *)V, (uint64_t)ldv, (uint32_t)h, (uint32_t)heads, (T)scale, (S *)out,
                                          (uint64_t)ldo, (T *)lse, workspace, (hipStream_t)stream);
    });
    HIP_TRY(hipGetLastError());
    return 0;
}

int pygim_sparse_attention(int dtype, int64_t nrows, const int32_t *rowptr, const int32_t *colind, int64_t nnz, const void *Q, int64_t ldq, const void *K,
                           int64_t ldk, const void *V, int64_t ldv, int64_t h, int64_t heads, double scale, void *out, int64_t ldo, void *lse,
                           void *workspace, int64_t workspace_bytes, void *stream) {
    return sparse_attention_call(dtype, nrows, rowptr, colind, nnz, Q, ldq, K, ldk, V, ldv, h, heads, scale, out, ldo, lse, workspace, workspace_bytes, stream,
                                 0.0, 0);
}

int pygim_sparse_attention_dropout(int dtype, int64_t nrows, const int32_t *rowptr, const int32_t *colind, int64_t nnz, const void *Q, int64_t ldq,
                                   const void *K, int64_t ldk, const void *V, int64_t ldv, int64_t h, int64_t heads, double scale, void *out, int64_t ldo,
                                   void *lse, void *workspace, int64_t workspace_bytes, void *stream, double p, uint64_t seed) {
    return sparse_attention_call(dtype, nrows, rowptr, colind, nnz, Q, ldq, K, ldk, V, ldv, h, heads, scale, out, ldo, lse, workspace, workspace_bytes, stream,
                                 p, seed);
}

int pygim_sparse_attention_bias(int dtype, int64_t nrows, const int32_t *rowptr, const int32_t *colind, int64_t nnz, const void *Q, int64_t ldq,
                                const void *K, int64_t ldk, const void *V, int64_t ldv, int64_t h, int64_t heads, double scale, void *out, int64_t ldo,
                                void *lse, void *workspace, int64_t workspace_bytes, void *stream, const void *bias, double p, uint64_t seed) {
    return sparse_attention_call(dtype, nrows, rowptr, colind, nnz, Q, ldq, K, ldk, V, ldv, h, heads, scale, out, ldo, lse, workspace, workspace_bytes, stream,
                                 p, seed, true, bias);
}

int64_t pygim_gatv2_aggregate_workspace(int dtype, int64_t nrows, int64_t nnz, int64_t h, int64_t heads) {
    (void)nrows;
    if (!is_gather_type(dtype) || nnz < 0 || h < 1 || heads < 1 || h % heads != 0 || h / heads > (int64_t)GV2_MAX_HEAD) return -1;
    return (int64_t)gat_workspace_bytes((uint64_t)nnz, (uint64_t)h, (uint64_t)heads, gather_compute_size(dtype));
}

static int gatv2_aggregate_call(int dtype, int64_t nrows, const int32_t *rowptr, const int32_t *colind, int64_t nnz, const void *x_dst, int64_t ld_dst,
                                const void *x_src, int64_t ld_src, const void *att, int64_t h, int64_t heads, double negative_slope, void *out, int64_t ldo,
                                void *lse, void *workspace, int64_t workspace_bytes, void *stream, double p, uint64_t seed) {
    if (bad_dropout(p)) return fail(PYGIM_ERR_INVALID, "gatv2_aggregate: the dropout rate must lie in [0, 1)");
    if (int rc = need_init()) return rc;
    if (!is_gather_type(dtype)) return fail(PYGIM_ERR_INVALID, "gatv2_aggregate: type must be FLT32, DBL64, FLT16 or BF16");
    if (h >= 1 && (heads < 1 || h % heads != 0)) return fail(PYGIM_ERR_INVALID, "gatv2_aggregate: heads must divide h");
    if (h >= 1 && h / heads > (int64_t)GV2_MAX_HEAD) return fail(PYGIM_ERR_INVALID, "gatv2_aggregate: a head is at most 256 features wide");
    if (int rc = check_csr_call("gatv2_aggregate", "rowptr / colind / x_dst / x_src / att / out", nrows, nnz, 0x7FFFFFFFll, h, 0x7FFFFFFFll,
                                ld_dst < ld_src ? ld_dst : ld_src, ldo,
                                {{rowptr, true}, {out, nrows > 0}, {lse, nrows > 0, true}, {colind, nnz > 0}, {x_dst, nnz > 0}, {x_src, nnz > 0}, {att, nnz > 0}},
                                pygim_gatv2_aggregate_workspace(dtype, nrows, nnz, h, heads), workspace, workspace_bytes))
        return rc;
    with_gather_types(dtype, [&](auto t, auto s) {
        using T = decltype(t);
        using S = decltype(s);
        if (p > 0.0)
            launch_gatv2_aggregate<T, S, true>((const uint32_t *)rowptr, (const uint32_t *)colind, (uint32_t)nrows, (uint32_t)nnz, (const S *)x_dst,
                                               (uint64_t)ld_dst, (const S *)x_src, (uint64_t)ld_src, (const T *)att, (uint32_t)h, (uint32_t)heads,
                                               (T)negative_slope, (S *)out, (uint64_t)ldo, (T *)lse, workspace, (hipStream_t)stream,
                                               attn_dropout_args<T>(p, seed));
        else
            launch_gatv2_aggregate<T, S>((const uint32_t *)rowptr, (const uint32_t *)colind, (uint32_t)nrows, (uint32_t)nnz, (const S *)x_dst, (uint64_t)ld_dst,
                                         (const S *)x_src, (uint64_t)ld_src, (const T *)att, (uint32_t)h, (uint32_t)heads, (T)negative_slope, (S *)out,
                                         (uint64_t)ldo, (T *)lse, workspace, (hipStream_t)stream);
    });
    HIP_TRY(hipGetLastError());
    return 0;
}

int pygim_gatv2_aggregate(int dtype, int64_t nrows, const int32_t *rowptr, const int32_t *colind, int64_t nnz, const void *x_dst, int64_t ld_dst,
                          const void *x_src, int64_t ld_src, const void *att, int64_t h, int64_t heads, double negative_slope, void *out, int64_t ldo,
                          void *lse, void *workspace, int64_t workspace_bytes, void *stream) {
    return gatv2_aggregate_call(dtype, nrows, rowptr, colind, nnz, x_dst, ld_dst, x_src, ld_src, att, h, heads, negative_slope, out, ldo, lse, workspace,
                                workspace_bytes, stream, 0.0, 0);
}

int pygim_gatv2_aggregate_dropout(int dtype, int64_t nrows, const int32_t *rowptr, const int32_t *colind, int64_t nnz, const void *x_dst, int64_t ld_dst,
                                  const void *x_src, int64_t ld_src, const void *att, int64_t h, int64_t heads, double negative_slope, void *out,
                                  int64_t ldo, void *lse, void *workspace, int64_t workspace_bytes, void *stream, double p, uint64_t seed) {
    return gatv2_aggregate_call(dtype, nrows, rowptr, colind, nnz, x_dst, ld_dst, x_src, ld_src, att, h, heads, negative_slope, out, ldo, lse, workspace,
                                workspace_bytes, stream, p, seed);
}

int64_t pygim_gatv2_backward_workspace(int dtype, int64_t nrows, int64_t nnz, int64_t h, int64_t heads) {
    (void)nrows;
    if (!is_gather_type(dtype) || nnz < 0 || h < 1 || heads < 1 || h % heads != 0 || h / heads > (int64_t)GV2_MAX_HEAD) return -1;
    return (int64_t)gatv2_backward_workspace_bytes((uint64_t)nnz, (uint64_t)h, gather_compute_size(dtype));
}

static int gatv2_backward_call(int dtype, int transposed, int64_t nrows, const int32_t *rowptr, const int32_t *colind, int64_t nnz, const void *x_own,
                               int64_t ld_own, const void *x_oth, int64_t ld_oth, const void *att, int64_t h, int64_t heads, double negative_slope,
                               const void *G, int64_t ldg, const void *lse, const void *delta, void *d_own, int64_t ldd, void *datt, void *workspace,
                               int64_t workspace_bytes, void *stream, const int32_t *entry_ids, double p, uint64_t seed) {
    if (bad_dropout(p)) return fail(PYGIM_ERR_INVALID, "gatv2_backward: the dropout rate must lie in [0, 1)");
    if (int rc = need_init()) return rc;
    if (!is_gather_type(dtype)) return fail(PYGIM_ERR_INVALID, "gatv2_backward: type must be FLT32, DBL64, FLT16 or BF16");
    if (h >= 1 && (heads < 1 || h % heads != 0)) return fail(PYGIM_ERR_INVALID, "gatv2_backward: heads must divide h");
    if (h >= 1 && h / heads > (int64_t)GV2_MAX_HEAD) return fail(PYGIM_ERR_INVALID, "gatv2_backward: a head is at most 256 features wide");
    if (transposed && datt) return fail(PYGIM_ERR_INVALID, "gatv2_backward: datt belongs to the call on the CSR of A (transposed = 0)");
    if (int rc = check_csr_call("gatv2_backward", "rowptr / colind / x_own / x_oth / att / G / lse / delta / d_own", nrows, nnz, 0x7FFFFFFFll, h, 0x7FFFFFFFll,
                                ld_own < ld_oth ? ld_own : ld_oth, ldg < ldd ? ldg : ldd,
                                {{rowptr, true}, {d_own, nrows > 0}, {datt, true, true}, {colind, nnz > 0}, {x_own, nnz > 0}, {x_oth, nnz > 0},
                                 {att, nnz > 0}, {G, nnz > 0}, {lse, nnz > 0}, {delta, nnz > 0}, {entry_ids, nnz > 0 && p > 0.0, true}},
                                pygim_gatv2_backward_workspace(dtype, nrows, nnz, h, heads), workspace, workspace_bytes))
        return rc;
    with_gather_types(dtype, [&](auto t, auto s) {
        using T = decltype(t);
        using S = decltype(s);
        if (p > 0.0 && transposed)
            launch_gatv2_backward<T, S, true, true>((const uint32_t *)rowptr, (const uint32_t *)colind, (uint32_t)nrows, (uint32_t)nnz, (const S *)x_own,
                                                    (uint64_t)ld_own, (const S *)x_oth, (uint64_t)ld_oth, (const T *)att, (uint32_t)h, (uint32_t)heads,
                                                    (T)negative_slope, (const S *)G, (uint64_t)ldg, (const T *)lse, (const T *)delta, (S *)d_own,
                                                    (uint64_t)ldd, nullptr, workspace, (hipStream_t)stream, entry_ids, attn_dropout_args<T>(p, seed));
        else if (p > 0.0)
            launch_gatv2_backward<T, S, false, true>((const uint32_t *)rowptr, (const uint32_t *)colind, (uint32_t)nrows, (uint32_t)nnz, (const S *)x_own,
                                                     (uint64_t)ld_own, (const S *)x_oth, (uint64_t)ld_oth, (const T *)att, (uint32_t)h, (uint32_t)heads,
                                                     (T)negative_slope, (const S *)G, (uint64_t)ldg, (const T *)lse, (const T *)delta, (S *)d_own,
                                                     (uint64_t)ldd, (T *)datt, workspace, (hipStream_t)stream, entry_ids, attn_dropout_args<T>(p, seed));
        else if (transposed)
            launch_gatv2_backward<T, S, true>((const uint32_t *)rowptr, (const uint32_t *)colind, (uint32_t)nrows, (uint32_t)nnz, (const S *)x_own,
                                              (uint64_t)ld_own, (const S *)x_oth, (uint64_t)ld_oth, (const T *)att, (uint32_t)h, (uint32_t)heads,
                                              (T)negative_slope, (const S *)G, (uint64_t)ldg, (const T *)lse, (const T *)delta, (S *)d_own, (uint64_t)ldd,
                                              nullptr, workspace, (hipStream_t)stream);
        else
            launch_gatv2_backward<T, S, false>((const uint32_t *)rowptr, (const uint32_t *)colind, (uint32_t)nrows, (uint32_t)nnz, (const S *)x_own,
                                               (uint64_t)ld_own, (const S *)x_oth, (uint64_t)ld_oth, (const T *)att, (uint32_t)h, (uint32_t)heads,
                                               (T)negative_slope, (const S *)G, (uint64_t)ldg, (const T *)lse, (const T *)delta, (S *)d_own, (uint64_t)ldd,
                                               (T *)datt, workspace, (hipStream_t)stream);
    });
    HIP_TRY(hipGetLastError());
    return 0;
}

int pygim_gatv2_backward(int dtype, int transposed, int64_t nrows, const int32_t *rowptr, const int32_t *colind, int64_t nnz, const void *x_own,
                         int64_t ld_own, const void *x_oth, int64_t ld_oth, const void *att, int64_t h, int64_t heads, double negative_slope, const void *G,
                         int64_t ldg, const void *lse, const void *delta, void *d_own, int64_t ldd, void *datt, void *workspace, int64_t workspace_bytes,
                         void *stream) {
    return gatv2_backward_call(dtype, transposed, nrows, rowptr, colind, nnz, x_own, ld_own, x_oth, ld_oth, att, h, heads, negative_slope, G, ldg, lse, delta,
                               d_own, ldd, datt, workspace, workspace_bytes, stream, nullptr, 0.0, 0);
}

int pygim_gatv2_backward_dropout(int dtype, int transposed, int64_t nrows, const int32_t *rowptr, const int32_t *colind, int64_t nnz, const void *x_own,
                                 int64_t ld_own, const void *x_oth, int64_t ld_oth, const void *att, int64_t h, int64_t heads, double negative_slope,
                                 const void *G, int64_t ldg, const void *lse, const void *delta, void *d_own, int64_t ldd, void *datt, void *workspace,
                                 int64_t workspace_bytes, void *stream, const int32_t *entry_ids, double p, uint64_t seed) {
    return gatv2_backward_call(dtype, transposed, nrows, rowptr, colind, nnz, x_own, ld_own, x_oth, ld_oth, att, h, heads, negative_slope, G, ldg, lse, delta,
                               d_own, ldd, datt, workspace, workspace_bytes, stream, entry_ids, p, seed);
}

int pygim_attention_dropout_mask(int dtype, int64_t nnz, int64_t heads, const int32_t *entry_ids, double p, uint64_t seed, void *mask, void *stream) {
    if (bad_dropout(p)) return fail(PYGIM_ERR_INVALID, "attention_dropout_mask: the dropout rate must lie in [0, 1)");
    if (int rc = need_init()) return rc;
    if (!is_float_type(dtype)) return fail(PYGIM_ERR_INVALID, "attention_dropout_mask: type must be FLT32 or DBL64");
    if (nnz < 0 || nnz > 0x7FFFFFFFll || heads < 1 || heads > 0x7FFFFFFFll) return fail(PYGIM_ERR_INVALID, "bad attention_dropout_mask sizes");
    if (nnz == 0) return 0;
    if (!mask || !is_device_ptr(mask) || (entry_ids && !is_device_ptr(entry_ids)))
        return fail(PYGIM_ERR_INVALID, "pygim_attention_dropout_mask needs device pointers");
    const uint64_t total = (uint64_t)nnz * (uint64_t)heads;
    with_elem_type(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((k_attn_dropout_mask<T>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, total, (uint32_t)heads, entry_ids,
                           attn_dropout_args<T>(p, seed), (T *)mask);
    });
    HIP_TRY(hipGetLastError());
    return 0;
}

int pygim_attention_dropout_host(int64_t nnz, int64_t heads, int64_t e0, double p, uint64_t seed, uint8_t *keep) {
    if (bad_dropout(p)) return fail(PYGIM_ERR_INVALID, "attention_dropout_host: the dropout rate must lie in [0, 1)");
    if (nnz < 0 || heads < 1 || heads > 0x7FFFFFFFll || e0 < 0 || e0 + nnz > 0x100000000ll || (nnz > 0 && !keep))
        return fail(PYGIM_ERR_INVALID, "bad attention_dropout_host sizes");
    const uint32_t thr = attn_dropout_threshold(p);
    for (int64_t i = 0; i < nnz; i++)
        for (int64_t k = 0; k < heads; k++)
            keep[i * heads + k] = attn_dropout_keep((uint32_t)(e0 + i), (uint32_t)k, (uint32_t)(seed & 0xFFFFFFFFull), (uint32_t)(seed >> 32), thr) ? 1 : 0;
    return 0;
}

static int edge_softmax_call(int mode, int dtype, int64_t nrows, const int32_t *rowptr, int64_t nnz, const void *a, const void *b, int64_t heads, void *out,
                             void *workspace, int64_t workspace_bytes, void *stream) {
    if (int rc = need_init()) return rc;
    if (!is_float_type(dtype)) return fail(PYGIM_ERR_INVALID, "edge_softmax: type must be FLT32 or DBL64");
    if (nrows < 0 || nrows >= 0xFFFFFFFFll || nnz < 0 || nnz > 0x7FFFFFFFll || heads < 1 || heads > 0x7FFFFFFFll)
        return fail(PYGIM_ERR_INVALID, "bad edge_softmax sizes");
    if (nnz > 0 && nrows == 0) return fail(PYGIM_ERR_INVALID, "edge_softmax: entries without rows");
    const bool bwd = mode == ES_BACKWARD;
    if (!rowptr || (nnz > 0 && (!a || !out || (bwd && !b)))) return fail(PYGIM_ERR_INVALID, "bad rowptr / scores / out");
    if (!is_device_ptr(rowptr) || (nnz > 0 && (!is_device_ptr(a) || !is_device_ptr(out) || (bwd && !is_device_ptr(b)))))
        return fail(PYGIM_ERR_INVALID, "pygim_edge_softmax needs device pointers");
    if (nnz == 0) return 0;
    const int64_t need = pygim_edge_softmax_workspace(dtype, nrows, nnz, heads);
    if (!workspace || workspace_bytes < need || (uintptr_t)workspace % 16 != 0 || !is_device_ptr(workspace))
        return fail(PYGIM_ERR_INVALID, "edge_softmax: workspace too small, misaligned or not device memory (pygim_edge_softmax_workspace)");
    hipStream_t st = (hipStream_t)stream;
    const uint32_t *rp = (const uint32_t *)rowptr;
    with_elem_type(dtype, [&](auto t) {
        using T = decltype(t);
        if (bwd) launch_edge_softmax<T, ES_BACKWARD>(rp, (uint32_t)nrows, (uint32_t)nnz, (const T *)a, (const T *)b, (uint32_t)heads, (T *)out, workspace, st);
        else launch_edge_softmax<T, ES_FORWARD>(rp, (uint32_t)nrows, (uint32_t)nnz, (const T *)a, nullptr, (uint32_t)heads, (T *)out, workspace, st);
    });
    HIP_TRY(hipGetLastError());
    return 0;
}

int pygim_edge_softmax(int dtype, int64_t nrows, const int32_t *rowptr, int64_t nnz, const void *scores, int64_t heads, void *out, void *workspace,
                       int64_t workspace_bytes, void *stream) {
    return edge_softmax_call(ES_FORWARD, dtype, nrows, rowptr, nnz, scores, nullptr, heads, out, workspace, workspace_bytes, stream);
}

int pygim_edge_softmax_backward(int dtype, int64_t nrows, const int32_t *rowptr, int64_t nnz, const void *P, const void *dP, int64_t heads, void *out,
                                void *workspace, int64_t workspace_bytes, void *stream) {
    return edge_softmax_call(ES_BACKWARD, dtype, nrows, rowptr, nnz, P, dP, heads, out, workspace, workspace_bytes, stream);
}

int64_t pygim_spmm_reduce_workspace(int dtype, int op, int64_t nrows, int64_t nnz, int64_t h) {
    if (op != PYGIM_REDUCE_MEAN && op != PYGIM_REDUCE_MAX && op != PYGIM_REDUCE_MIN) return -1;
    if (op == PYGIM_REDUCE_MEAN ? !is_gather_type(dtype) : dtype_size(dtype) == 0) return -1;   // 16-bit features: the mean only
    if (nrows < 0 || nnz < 0 || nnz > 0x7FFFFFFFll || h < 1 || h > (int64_t)RG_MAX_H) return -1;
    return (int64_t)spmm_reduce_workspace_bytes(op, (uint64_t)nnz, (uint64_t)h, gather_compute_size(dtype));
}

int pygim_spmm_reduce(int dtype, int op, int64_t nrows, const int32_t *rowptr, const int32_t *colind, int64_t nnz, const void *values, const void *X,
                      int64_t ldx, int64_t h, void *out, int64_t ldo, int32_t *arg, void *workspace, int64_t workspace_bytes, void *stream) {
    if (int rc = need_init()) return rc;
    if (dtype_size(dtype) == 0 && !is_half_type(dtype)) return fail(PYGIM_ERR_INVALID, "spmm_reduce: unknown element type");
    if (op != PYGIM_REDUCE_MEAN && op != PYGIM_REDUCE_MAX && op != PYGIM_REDUCE_MIN)
        return fail(PYGIM_ERR_INVALID, "spmm_reduce: op must be PYGIM_REDUCE_MEAN, _MAX or _MIN (sums: pygim_spmm_values, pygim_spmm_run_group)");
    if (op == PYGIM_REDUCE_MEAN && !is_gather_type(dtype)) return fail(PYGIM_ERR_INVALID, "spmm_reduce: mean needs FLT32, DBL64, FLT16 or BF16");
    if (op != PYGIM_REDUCE_MEAN && is_half_type(dtype)) return fail(PYGIM_ERR_INVALID, "spmm_reduce: max / min take no 16-bit type (FLT16 / BF16: mean only)");
    if (op == PYGIM_REDUCE_MEAN && arg) return fail(PYGIM_ERR_INVALID, "spmm_reduce: mean has no arg output");
    if (arg && (uintptr_t)arg % 4 != 0) return fail(PYGIM_ERR_INVALID, "spmm_reduce: arg must be 4-byte aligned");
    if (int rc = check_csr_call("spmm_reduce", "rowptr / colind / X / out", nrows, nnz, 0x7FFFFFFFll, h, (int64_t)RG_MAX_H, ldx, ldo,
                                {{rowptr, true}, {out, nrows > 0}, {arg, nrows > 0, true}, {colind, nnz > 0}, {X, nnz > 0}, {values, nnz > 0, true}},
                                pygim_spmm_reduce_workspace(dtype, op, nrows, nnz, h), workspace, workspace_bytes))
        return rc;
    if (is_half_type(dtype)) {   // the mean alone: float32 values (or none), float32 sums and division, one rounding into out
        const uint32_t *rp = (const uint32_t *)rowptr, *ci = (const uint32_t *)colind;
        if (dtype == PYGIM_BF16)
            launch_spmm_mean16<__bf16>(rp, ci, (uint32_t)nrows, (uint32_t)nnz, (const float *)values, (const __bf16 *)X, (uint64_t)ldx, (uint32_t)h,
                                       (__bf16 *)out, (uint64_t)ldo, workspace, (hipStream_t)stream);
        else
            launch_spmm_mean16<_Float16>(rp, ci, (uint32_t)nrows, (uint32_t)nnz, (const float *)values, (const _Float16 *)X, (uint64_t)ldx, (uint32_t)h,
                                         (_Float16 *)out, (uint64_t)ldo, workspace, (hipStream_t)stream);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    with_elem_type<true>(dtype, [&](auto t) {
        using T = decltype(t);
        launch_spmm_reduce<T>(op, (const uint32_t *)rowptr, (const uint32_t *)colind, (uint32_t)nrows, (uint32_t)nnz, (const T *)values, (const T *)X,
                              (uint64_t)ldx, (uint32_t)h, (T *)out, (uint64_t)ldo, arg, workspace, (hipStream_t)stream);
    });
    HIP_TRY(hipGetLastError());
    return 0;
}

int pygim_spmm_reduce_backward(int dtype, int64_t ncols, const int32_t *rowptr_t, const int32_t *rows_t, const int32_t *perm, int64_t nnz,
                               const void *values, const void *G, int64_t ldg, const int32_t *arg, int64_t h, void *dX, int64_t ldd, void *stream) {
    if (int rc = need_init()) return rc;
    if (!is_float_type(dtype)) return fail(PYGIM_ERR_INVALID, "spmm_reduce_backward: type must be FLT32 or DBL64");
    if (int rc = check_csr_call("spmm_reduce_backward", "rowptr_t / rows_t / perm / G / arg / dX", ncols, nnz, 0x7FFFFFFFll, h, (int64_t)RG_MAX_H, ldg, ldd,
                                {{rowptr_t, true}, {dX, ncols > 0}, {rows_t, nnz > 0}, {perm, nnz > 0}, {G, nnz > 0}, {arg, nnz > 0}, {values, nnz > 0, true}}))
        return rc;
    if (nnz > 0 && (uintptr_t)arg % 4 != 0) return fail(PYGIM_ERR_INVALID, "spmm_reduce_backward: arg must be 4-byte aligned");
    with_elem_type(dtype, [&](auto t) {
        using T = decltype(t);
        launch_spmm_reduce_bwd<T>((const uint32_t *)rowptr_t, (const uint32_t *)rows_t, perm, (uint32_t)ncols, (const T *)values, (const T *)G, (uint64_t)ldg,
                                  arg, (uint32_t)h, (T *)dX, (uint64_t)ldd, (hipStream_t)stream);
    });
    HIP_TRY(hipGetLastError());
    return 0;
}

// the statistics list of pygim_spmm_multi_reduce: 1..6 distinct PYGIM_STAT_* codes; col[s] = the block of statistic s in a row of out, or -1
static bool parse_multi_stats(const int *stats, int nstats, int64_t h, int32_t col[MS_COUNT], bool &moments, bool &best) {
    static_assert(MS_SUM == PYGIM_STAT_SUM && MS_MEAN == PYGIM_STAT_MEAN && MS_MIN == PYGIM_STAT_MIN && MS_MAX == PYGIM_STAT_MAX &&
                      MS_VAR == PYGIM_STAT_VAR && MS_STD == PYGIM_STAT_STD,
                  "the codes of include/pygim_hip.h");
    for (int s = 0; s < MS_COUNT; s++) col[s] = -1;
    moments = best = false;
    if (!stats || nstats < 1 || nstats > MS_COUNT) return false;
    for (int j = 0; j < nstats; j++) {
        const int s = stats[j];
        if (s < 0 || s >= MS_COUNT || col[s] >= 0) return false;
        col[s] = (int32_t)(j * h);
        if (s == MS_MAX || s == MS_MIN) best = true;
        else moments = true;
    }
    return true;
}

int64_t pygim_spmm_multi_reduce_workspace(int dtype, const int *stats, int nstats, int64_t nrows, int64_t nnz, int64_t h) {
    int32_t col[MS_COUNT];
    bool moments, best;
    if (!is_gather_type(dtype) || nrows < 0 || nnz < 0 || nnz > 0x7FFFFFFFll || h < 1 || h > (int64_t)RG_MAX_H) return -1;
    if (!parse_multi_stats(stats, nstats, h, col, moments, best)) return -1;
    return (int64_t)multi_workspace_bytes(moments, best, (uint64_t)nnz, (uint64_t)h, gather_compute_size(dtype));
}

int pygim_spmm_multi_reduce(int dtype, const int *stats, int nstats, double eps, int64_t nrows, const int32_t *rowptr, const int32_t *colind, int64_t nnz,
                            const void *X, int64_t ldx, int64_t h, void *out, int64_t ldo, int32_t *arg_max, int32_t *arg_min, void *workspace,
                            int64_t workspace_bytes, void *stream) {
    if (int rc = need_init()) return rc;
    if (!is_gather_type(dtype)) return fail(PYGIM_ERR_INVALID, "spmm_multi_reduce: type must be FLT32, DBL64, FLT16 or BF16");
    int32_t col[MS_COUNT];
    bool moments, best;
    if (h < 1 || h > (int64_t)RG_MAX_H) return fail(PYGIM_ERR_INVALID, "bad spmm_multi_reduce sizes / strides");
    if (!parse_multi_stats(stats, nstats, h, col, moments, best))
        return fail(PYGIM_ERR_INVALID, "spmm_multi_reduce: stats must be 1 to 6 distinct PYGIM_STAT_* codes");
    if ((arg_max && col[MS_MAX] < 0) || (arg_min && col[MS_MIN] < 0))
        return fail(PYGIM_ERR_INVALID, "spmm_multi_reduce: arg_max / arg_min need PYGIM_STAT_MAX / _MIN in stats");
    if (col[MS_STD] >= 0 && !(eps > 0.0 && eps <= 1.7976931348623157e308))
        return fail(PYGIM_ERR_INVALID, "spmm_multi_reduce: PYGIM_STAT_STD needs a finite eps > 0");
    if ((arg_max && (uintptr_t)arg_max % 4 != 0) || (arg_min && (uintptr_t)arg_min % 4 != 0))
        return fail(PYGIM_ERR_INVALID, "spmm_multi_reduce: arg_max / arg_min must be 4-byte aligned");
    if (ldo < (int64_t)nstats * h) return fail(PYGIM_ERR_INVALID, "bad spmm_multi_reduce sizes / strides");
    if (int rc = check_csr_call("spmm_multi_reduce", "rowptr / colind / X / out", nrows, nnz, 0x7FFFFFFFll, h, (int64_t)RG_MAX_H, ldx, ldo,
                                {{rowptr, true}, {out, nrows > 0}, {arg_max, nrows > 0, true}, {arg_min, nrows > 0, true}, {colind, nnz > 0}, {X, nnz > 0}},
                                pygim_spmm_multi_reduce_workspace(dtype, stats, nstats, nrows, nnz, h), workspace, workspace_bytes))
        return rc;
    with_gather_types(dtype, [&](auto t, auto s) {
        using T = decltype(t);
        using S = decltype(s);
        MultiStats<T> st;
        for (int k = 0; k < MS_COUNT; k++) st.col[k] = col[k];
        st.eps = col[MS_STD] >= 0 ? (T)eps : T(0);
        launch_spmm_multi<T, S>((const uint32_t *)rowptr, (const uint32_t *)colind, (uint32_t)nrows, (uint32_t)nnz, (const S *)X, (uint64_t)ldx, (uint32_t)h,
                                (S *)out, (uint64_t)ldo, arg_max, arg_min, workspace, st, moments, best, (hipStream_t)stream);
    });
    HIP_TRY(hipGetLastError());
    return 0;
}

int64_t pygim_spmm_softmax_workspace(int dtype, int64_t nrows, int64_t nnz, int64_t h) {
    if (!is_gather_type(dtype) || nrows < 0 || nnz < 0 || nnz > 0x7FFFFFFFll || h < 1 || h > (int64_t)RG_MAX_H) return -1;
    return (int64_t)softmax_workspace_bytes((uint64_t)nnz, (uint64_t)h, gather_compute_size(dtype));
}

int pygim_spmm_softmax(int dtype, int64_t nrows, const int32_t *rowptr, const int32_t *colind, int64_t nnz, const void *X, int64_t ldx, const void *t,
                       int64_t h, void *out, int64_t ldo, void *lse, void *workspace, int64_t workspace_bytes, void *stream) {
    if (int rc = need_init()) return rc;
    if (!is_gather_type(dtype)) return fail(PYGIM_ERR_INVALID, "spmm_softmax: type must be FLT32, DBL64, FLT16 or BF16");
    if (int rc = check_csr_call("spmm_softmax", "rowptr / colind / X / t / out / lse", nrows, nnz, 0x7FFFFFFFll, h, (int64_t)RG_MAX_H, ldx, ldo,
                                {{rowptr, true}, {out, nrows > 0}, {lse, nrows > 0, true}, {colind, nnz > 0}, {X, nnz > 0}, {t, nnz > 0}},
                                pygim_spmm_softmax_workspace(dtype, nrows, nnz, h), workspace, workspace_bytes))
        return rc;
    if (lse && (uintptr_t)lse % gather_compute_size(dtype) != 0) return fail(PYGIM_ERR_INVALID, "spmm_softmax: lse must be aligned to its element");
    with_gather_types(dtype, [&](auto tt, auto s) {
        using T = decltype(tt);
        using S = decltype(s);
        launch_spmm_softmax<T, S>((const uint32_t *)rowptr, (const uint32_t *)colind, (uint32_t)nrows, (uint32_t)nnz, (const S *)X, (uint64_t)ldx, (const T *)t,
                                  (uint32_t)h, (S *)out, (uint64_t)ldo, (T *)lse, workspace, (hipStream_t)stream);
    });
    HIP_TRY(hipGetLastError());
    return 0;
}

int64_t pygim_spmm_softmax_backward_workspace(int dtype, int64_t ncols, int64_t nnz, int64_t h) {
    if (!is_gather_type(dtype) || ncols < 0 || nnz < 0 || nnz > 0x7FFFFFFFll || h < 1 || h > (int64_t)RG_MAX_H) return -1;
    return (int64_t)softmax_backward_workspace_bytes((uint64_t)nnz, (uint64_t)h, gather_compute_size(dtype));
}

int pygim_spmm_softmax_backward(int dtype, int64_t ncols, const int32_t *rowptr_t, const int32_t *rows_t, int64_t nnz, const void *X, int64_t ldx,
                                const void *t, int64_t h, const void *G, int64_t ldg, const void *out, int64_t ldo, const void *lse, void *dX, int64_t ldd,
                                void *dT, void *workspace, int64_t workspace_bytes, void *stream) {
    if (int rc = need_init()) return rc;
    if (!is_gather_type(dtype)) return fail(PYGIM_ERR_INVALID, "spmm_softmax_backward: type must be FLT32, DBL64, FLT16 or BF16");
    if (h >= 1 && (ldg < h || ldo < h)) return fail(PYGIM_ERR_INVALID, "bad spmm_softmax_backward sizes / strides");
    if (int rc = check_csr_call("spmm_softmax_backward", "rowptr_t / rows_t / X / t / G / out / lse / dX / dT", ncols, nnz, 0x7FFFFFFFll, h, (int64_t)RG_MAX_H,
                                ldx, ldd,
                                {{rowptr_t, true}, {dX, ncols > 0}, {dT, ncols > 0, true}, {rows_t, nnz > 0}, {X, nnz > 0}, {t, nnz > 0}, {G, nnz > 0},
                                 {out, nnz > 0}, {lse, nnz > 0}},
                                pygim_spmm_softmax_backward_workspace(dtype, ncols, nnz, h), workspace, workspace_bytes))
        return rc;
    if ((nnz > 0 && (uintptr_t)lse % gather_compute_size(dtype) != 0) || (dT && (uintptr_t)dT % gather_compute_size(dtype) != 0))
        return fail(PYGIM_ERR_INVALID, "spmm_softmax_backward: lse and dT must be aligned to their element");
    with_gather_types(dtype, [&](auto tt, auto s) {
        using T = decltype(tt);
        using S = decltype(s);
        launch_spmm_softmax_backward<T, S>((const uint32_t *)rowptr_t, (const uint32_t *)rows_t, (uint32_t)ncols, (uint32_t)nnz, (const S *)X, (uint64_t)ldx,
                                           (const T *)t, (uint32_t)h, (const S *)G, (uint64_t)ldg, (const S *)out, (uint64_t)ldo, (const T *)lse, (S *)dX,
                                           (uint64_t)ldd, (T *)dT, workspace, (hipStream_t)stream);
    });
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- messages with a feature-wide edge feature: act(X[col] + E) + eps, folded per row; the gradient of E in entry order ----
static bool edge_fold_op(int op) { return op == PYGIM_REDUCE_SUM || op == PYGIM_REDUCE_MEAN || op == PYGIM_REDUCE_MAX || op == PYGIM_REDUCE_MIN; }
static bool edge_best_op(int op) { return op == PYGIM_REDUCE_MAX || op == PYGIM_REDUCE_MIN; }
// the type an op takes: the four gather types, FLT32 / DBL64 alone for max / min
static bool edge_type_ok(int dtype, int op) { return edge_best_op(op) ? is_float_type(dtype) : is_gather_type(dtype); }
// op (softmax: whether the entry point has that fold), act, eps and the type, in the order the header lists them; 0 when all are fine
static int check_edge_message(const char *name, int dtype, int op, bool softmax_ok, int act, double eps) {
    const std::string o(name);
    if (!(edge_fold_op(op) || (softmax_ok && op == PYGIM_REDUCE_SOFTMAX)))
        return fail(PYGIM_ERR_INVALID, o + ": op must be PYGIM_REDUCE_SUM, _MEAN, _MAX or _MIN" + (softmax_ok ? " or _SOFTMAX" : ""));
    if (act != PYGIM_ACT_NONE && act != PYGIM_ACT_RELU) return fail(PYGIM_ERR_INVALID, o + ": act must be PYGIM_ACT_NONE or PYGIM_ACT_RELU");
    if (eps != eps) return fail(PYGIM_ERR_INVALID, o + ": eps is NaN");
    if (!edge_type_ok(dtype, op))
        return fail(PYGIM_ERR_INVALID, o + ": type must be FLT32, DBL64, FLT16 or BF16 (max / min: FLT32 or DBL64)");
    return 0;
}

int64_t pygim_spmm_edge_workspace(int dtype, int op, int64_t nrows, int64_t nnz, int64_t h) {
    static_assert(RD_SUM == PYGIM_REDUCE_SUM && RD_SOFTMAX == PYGIM_REDUCE_SOFTMAX && RD_MEAN == PYGIM_REDUCE_MEAN && RD_MAX == PYGIM_REDUCE_MAX &&
                      RD_MIN == PYGIM_REDUCE_MIN && EM_ACT_RELU == PYGIM_ACT_RELU,
                  "the codes of include/pygim_hip.h");
    if (!edge_fold_op(op) || !edge_type_ok(dtype, op)) return -1;
    if (nrows < 0 || nnz < 0 || nnz > 0x7FFFFFFFll || h < 1 || h > (int64_t)RG_MAX_H) return -1;
    return (int64_t)spmm_edge_workspace_bytes(op, (uint64_t)nnz, (uint64_t)h, gather_compute_size(dtype));
}

int pygim_spmm_edge(int dtype, int op, int act, double eps, int64_t nrows, const int32_t *rowptr, const int32_t *colind, int64_t nnz, const void *X,
                    int64_t ldx, const void *E, int64_t lde, int64_t h, void *out, int64_t ldo, int32_t *arg, void *workspace, int64_t workspace_bytes,
                    void *stream) {
    if (int rc = check_edge_message("spmm_edge", dtype, op, false, act, eps)) return rc;
    if (!edge_best_op(op) && arg) return fail(PYGIM_ERR_INVALID, "spmm_edge: sum and mean have no arg output");
    if (arg && (uintptr_t)arg % 4 != 0) return fail(PYGIM_ERR_INVALID, "spmm_edge: arg must be 4-byte aligned");
    if (h >= 1 && lde < h) return fail(PYGIM_ERR_INVALID, "bad spmm_edge sizes / strides");
    if (int rc = check_csr_call("spmm_edge", "rowptr / colind / X / E / out", nrows, nnz, 0x7FFFFFFFll, h, (int64_t)RG_MAX_H, ldx, ldo,
                                {{rowptr, true}, {out, nrows > 0}, {arg, nrows > 0, true}, {colind, nnz > 0}, {X, nnz > 0}, {E, nnz > 0}},
                                pygim_spmm_edge_workspace(dtype, op, nrows, nnz, h), workspace, workspace_bytes))
        return rc;
    if (int rc = need_init()) return rc;   // after the argument checks: they need no device
    with_gather_types(dtype, [&](auto t, auto s) {
        using T = decltype(t);
        using S = decltype(s);
        const EdgeMsg<T> msg = {(T)eps, act == PYGIM_ACT_RELU};
        launch_spmm_edge<T, S>(op, (const uint32_t *)rowptr, (const uint32_t *)colind, (uint32_t)nrows, (uint32_t)nnz, (const S *)X, (uint64_t)ldx, (const S *)E,
                               (uint64_t)lde, msg, (uint32_t)h, (S *)out, (uint64_t)ldo, arg, workspace, (hipStream_t)stream);
    });
    HIP_TRY(hipGetLastError());
    return 0;
}

int64_t pygim_spmm_edge_softmax_workspace(int dtype, int64_t nrows, int64_t nnz, int64_t h) { return pygim_spmm_softmax_workspace(dtype, nrows, nnz, h); }

int pygim_spmm_edge_softmax(int dtype, int act, double eps, int64_t nrows, const int32_t *rowptr, const int32_t *colind, int64_t nnz, const void *X, int64_t ldx,
                            const void *E, int64_t lde, const void *t, int64_t h, void *out, int64_t ldo, void *lse, void *workspace, int64_t workspace_bytes,
                            void *stream) {
    if (int rc = check_edge_message("spmm_edge_softmax", dtype, PYGIM_REDUCE_SOFTMAX, true, act, eps)) return rc;
    if (h >= 1 && lde < h) return fail(PYGIM_ERR_INVALID, "bad spmm_edge_softmax sizes / strides");
    if (int rc = check_csr_call("spmm_edge_softmax", "rowptr / colind / X / E / t / out / lse", nrows, nnz, 0x7FFFFFFFll, h, (int64_t)RG_MAX_H, ldx, ldo,
                                {{rowptr, true}, {out, nrows > 0}, {lse, nrows > 0, true}, {colind, nnz > 0}, {X, nnz > 0}, {E, nnz > 0}, {t, nnz > 0}},
                                pygim_spmm_edge_softmax_workspace(dtype, nrows, nnz, h), workspace, workspace_bytes))
        return rc;
    if (lse && (uintptr_t)lse % gather_compute_size(dtype) != 0) return fail(PYGIM_ERR_INVALID, "spmm_edge_softmax: lse must be aligned to its element");
    if (int rc = need_init()) return rc;   // after the argument checks: they need no device
    with_gather_types(dtype, [&](auto tt, auto s) {
        using T = decltype(tt);
        using S = decltype(s);
        const EdgeMsg<T> msg = {(T)eps, act == PYGIM_ACT_RELU};
        launch_spmm_edge_softmax<T, S>((const uint32_t *)rowptr, (const uint32_t *)colind, (uint32_t)nrows, (uint32_t)nnz, (const S *)X, (uint64_t)ldx,
                                       (const S *)E, (uint64_t)lde, msg, (const T *)t, (uint32_t)h, (S *)out, (uint64_t)ldo, (T *)lse, workspace,
                                       (hipStream_t)stream);
    });
    HIP_TRY(hipGetLastError());
    return 0;
}

// the rows of dT_part: one per run of RG_EPW entries
int64_t pygim_spmm_edge_backward_workspace(int dtype, int op, int64_t nrows, int64_t nnz, int64_t h) {
    if (!(edge_fold_op(op) || op == PYGIM_REDUCE_SOFTMAX) || !edge_type_ok(dtype, op)) return -1;
    if (nrows < 0 || nnz < 0 || nnz > 0x7FFFFFFFll || h < 1 || h > (int64_t)RG_MAX_H) return -1;
    return (int64_t)row_gather_runs((uint64_t)nnz);
}

int pygim_spmm_edge_backward(int dtype, int op, int act, double eps, int64_t nrows, const int32_t *rowptr, const int32_t *colind, int64_t nnz, const void *X,
                             int64_t ldx, const void *E, int64_t lde, const void *G, int64_t ldg, const int32_t *arg, const void *t, const void *out, int64_t ldo,
                             const void *lse, int64_t h, void *dE, int64_t ldde, void *dT_part, void *stream) {
    if (int rc = check_edge_message("spmm_edge_backward", dtype, op, true, act, eps)) return rc;
    const bool softmax = op == PYGIM_REDUCE_SOFTMAX, best = edge_best_op(op);
    if (h >= 1 && (lde < h || ldg < h || (softmax && ldo < h))) return fail(PYGIM_ERR_INVALID, "bad spmm_edge_backward sizes / strides");
    if (dT_part && !softmax) return fail(PYGIM_ERR_INVALID, "spmm_edge_backward: dT_part belongs to PYGIM_REDUCE_SOFTMAX");
    if (int rc = check_csr_call("spmm_edge_backward", "rowptr / colind / X / E / G / arg / t / out / lse / dE / dT_part", nrows, nnz, 0x7FFFFFFFll, h,
                                (int64_t)RG_MAX_H, ldx, ldde,
                                {{rowptr, true}, {colind, nnz > 0}, {X, nnz > 0}, {E, nnz > 0}, {G, nnz > 0}, {dE, nnz > 0}, {arg, nnz > 0 && best},
                                 {t, nnz > 0 && softmax}, {out, nnz > 0 && softmax}, {lse, nnz > 0 && softmax}, {dT_part, nnz > 0, true}}))
        return rc;
    if (nnz > 0 && best && (uintptr_t)arg % 4 != 0) return fail(PYGIM_ERR_INVALID, "spmm_edge_backward: arg must be 4-byte aligned");
    if (nnz > 0 && softmax && ((uintptr_t)lse % gather_compute_size(dtype) != 0 || (dT_part && (uintptr_t)dT_part % gather_compute_size(dtype) != 0)))
        return fail(PYGIM_ERR_INVALID, "spmm_edge_backward: lse and dT_part must be aligned to their element");
    if (int rc = need_init()) return rc;   // after the argument checks: they need no device
    with_gather_types(dtype, [&](auto tt, auto s) {
        using T = decltype(tt);
        using S = decltype(s);
        const EdgeMsg<T> msg = {(T)eps, act == PYGIM_ACT_RELU};
        launch_spmm_edge_backward<T, S>(op, (const uint32_t *)rowptr, (const uint32_t *)colind, (uint32_t)nrows, (uint32_t)nnz, (const S *)X, (uint64_t)ldx,
                                        (const S *)E, (uint64_t)lde, msg, (uint32_t)h, (const S *)G, (uint64_t)ldg, arg, (const T *)t, (const S *)out,
                                        (uint64_t)ldo, (const T *)lse, (S *)dE, (uint64_t)ldde, (T *)dT_part, (hipStream_t)stream);
    });
    HIP_TRY(hipGetLastError());
    return 0;
}

// the launch shape of a gather entry point, from the functions its launcher calls; no device, no launch (like the *_workspace functions)
int pygim_gather_launch_shape(int kind, int dtype, int64_t h, int64_t heads, int aligned, int64_t out[8]) {
    static_assert(LS_PART_PIECE == PYGIM_SHAPE_PART_PIECE && LS_PART_CHUNK == PYGIM_SHAPE_PART_CHUNK && LS_PART_HEADS == PYGIM_SHAPE_PART_HEADS &&
                      LS_SCALAR_SIZE == PYGIM_SHAPE_SCALAR_SIZE && LS_SCALAR_ALIGN == PYGIM_SHAPE_SCALAR_ALIGN,
                  "the flags of include/pygim_hip.h");
    if (!out) return PYGIM_ERR_INVALID;
    const bool head_wise = kind == PYGIM_SHAPE_SPARSE_ATTENTION || kind == PYGIM_SHAPE_GATV2_AGGREGATE || kind == PYGIM_SHAPE_GATV2_BACKWARD;
    const bool walker = kind == PYGIM_SHAPE_SPMM_VALUES || kind == PYGIM_SHAPE_SPMM_REDUCE || kind == PYGIM_SHAPE_GAT_AGGREGATE ||
                        kind == PYGIM_SHAPE_SPMM_REDUCE_BACKWARD || kind == PYGIM_SHAPE_SPMM_MULTI_REDUCE || kind == PYGIM_SHAPE_SPMM_SOFTMAX ||
                        kind == PYGIM_SHAPE_SPMM_SOFTMAX_BACKWARD || kind == PYGIM_SHAPE_SPMM_EDGE || kind == PYGIM_SHAPE_SPMM_EDGE_BACKWARD;
    bool type_ok;
    if (kind == PYGIM_SHAPE_SPMM_REDUCE) type_ok = dtype_size(dtype) != 0 || is_half_type(dtype);   // integers: max / min; 16-bit: the mean
    else if (kind == PYGIM_SHAPE_EDGE_SOFTMAX || kind == PYGIM_SHAPE_SPMM_REDUCE_BACKWARD) type_ok = is_float_type(dtype);
    else type_ok = is_gather_type(dtype);
    if (!(head_wise || walker || kind == PYGIM_SHAPE_SDDMM || kind == PYGIM_SHAPE_EDGE_SOFTMAX) || !type_ok) return PYGIM_ERR_INVALID;
    if (kind == PYGIM_SHAPE_SDDMM || kind == PYGIM_SHAPE_SPMM_REDUCE || kind == PYGIM_SHAPE_SPMM_REDUCE_BACKWARD) heads = 1;   // they have none
    if (kind == PYGIM_SHAPE_SPMM_MULTI_REDUCE && heads != 1) return PYGIM_ERR_INVALID;   // it has none either, and says so: heads must be 1
    if ((kind == PYGIM_SHAPE_SPMM_SOFTMAX || kind == PYGIM_SHAPE_SPMM_SOFTMAX_BACKWARD) && heads != 1) return PYGIM_ERR_INVALID;   // nor have these
    if ((kind == PYGIM_SHAPE_SPMM_EDGE || kind == PYGIM_SHAPE_SPMM_EDGE_BACKWARD) && heads != 1) return PYGIM_ERR_INVALID;         // nor these
    if (kind == PYGIM_SHAPE_EDGE_SOFTMAX) h = heads;                                                                           // it has no h
    if (h < 1 || heads < 1 || heads > 0x7FFFFFFFll || h % heads != 0 || h > (walker ? (int64_t)RG_MAX_H : 0xFFFFFFFFll)) return PYGIM_ERR_INVALID;
    if (head_wise && h / heads > (int64_t)SA_MAX_HEAD) return PYGIM_ERR_INVALID;
    const uint32_t V = (uint32_t)(16 / gather_storage_size(dtype));
    LaunchShape g;
    if (head_wise) g = head_gather_shape((uint32_t)h, (uint32_t)heads, V, aligned != 0);
    else if (kind == PYGIM_SHAPE_SDDMM) g = sddmm_shape((uint32_t)h, V, aligned != 0);
    else if (kind == PYGIM_SHAPE_EDGE_SOFTMAX) g = edge_softmax_shape((uint32_t)heads, V, aligned != 0);
    else if (kind == PYGIM_SHAPE_SPMM_REDUCE_BACKWARD) g = spmm_reduce_bwd_shape((uint32_t)h, V, aligned != 0);
    else if (kind == PYGIM_SHAPE_SPMM_MULTI_REDUCE) g = multi_gather_shape((uint32_t)h, V, aligned != 0);
    else if (kind == PYGIM_SHAPE_SPMM_SOFTMAX) g = softmax_gather_shape((uint32_t)h, V, aligned != 0);
    else if (kind == PYGIM_SHAPE_SPMM_SOFTMAX_BACKWARD) g = softmax_grad_shape((uint32_t)h, V, aligned != 0);
    else if (kind == PYGIM_SHAPE_SPMM_EDGE) g = edge_gather_shape((uint32_t)h, V, aligned != 0);
    else if (kind == PYGIM_SHAPE_SPMM_EDGE_BACKWARD) g = edge_grad_shape((uint32_t)h, V, aligned != 0);
    else g = row_gather_shape((uint32_t)h, (uint32_t)(h / heads), V, aligned != 0);
    const int64_t v[8] = {g.vec, g.npl, g.LH, g.L, g.per, g.chunks, g.launches, g.flags};
    for (int i = 0; i < 8; i++) out[i] = v[i];
    return 0;
}

int pygim_group_timers(int64_t handle, double out_ms[5]) {
    Group *g = lookup(handle);
    if (!g) return fail(PYGIM_ERR_INVALID, "unknown group handle");
    for (int i = 0; i < 5; i++) out_ms[i] = g->timers[i];
    return 0;
}

int pygim_group_kernel_ms(int64_t handle, double *sum_ms, int64_t *count, int reset) {
    Group *g = lookup(handle);
    if (!g) return fail(PYGIM_ERR_INVALID, "unknown group handle");
    for (auto &e : g->ev_pending) {
        float ms = 0;
        if (hipEventSynchronize(e.second) == hipSuccess && hipEventElapsedTime(&ms, e.first, e.second) == hipSuccess) {
            g->ev_ms += ms;
            g->ev_count++;
        }
        (void)hipEventDestroy(e.first);
        (void)hipEventDestroy(e.second);
    }
    g->ev_pending.clear();
    if (sum_ms) *sum_ms = g->ev_ms;
    if (count) *count = g->ev_count;
    if (reset) {
        g->ev_ms = 0;
        g->ev_count = 0;
    }
    return 0;
}

int pygim_group_kernel_events(int64_t handle, int on) {
    Group *g = lookup(handle);
    if (!g) return fail(PYGIM_ERR_INVALID, "unknown group handle");
    g->kernel_events = on != 0;
    return 0;
}

int pygim_group_plan(int64_t handle, int64_t out[8]) {
    Group *g = lookup(handle);
    if (!g) return fail(PYGIM_ERR_INVALID, "unknown group handle");
    const Part &p = serving_part(g);
    int64_t ncoop = 0;
    for (auto c : p.panel_coop) ncoop += c;
    out[0] = p.d_items ? (int64_t)p.npanels : 0;
    out[1] = p.panel_cols;
    out[2] = (int64_t)p.n_items;
    out[3] = p.col16 ? 1 : 0;
    out[4] = ncoop;
    out[5] = p.lp_panel.n_tasks;
    out[6] = (g->merged && g->parts.size() > 1) ? 1 : 0;
    out[7] = p.extra ? 1 : 0;
    return 0;
}

int pygim_group_lds_plan(int64_t handle, int64_t out[4]) {
    Group *g = lookup(handle);
    if (!g) return fail(PYGIM_ERR_INVALID, "unknown group handle");
    const Part &p = serving_part(g);
    out[0] = p.lds_tiles ? (int64_t)p.lds_ntiles : 0;
    out[1] = (int64_t)p.lds_slots;
    out[2] = (int64_t)p.lds_tokens;
    out[3] = p.nnz;
    return 0;
}

int pygim_group_lds_code(int64_t handle, int64_t out[4]) {
    Group *g = lookup(handle);
    if (!g) return fail(PYGIM_ERR_INVALID, "unknown group handle");
    const Part &p = serving_part(g);
    out[0] = p.lds_code ? (int64_t)p.lds_code_bytes : 0;
    out[1] = p.lds_code ? (int64_t)p.lds_code_pairs : 0;
    bool all_code = p.lds_is_code && g_tune.lds_code;
    if (!(g->merged && g_tune.merge_parts && g->parts.size() > 1))
        for (const Part &q : g->parts) all_code = all_code && q.lds_is_code;   // (1 only when EVERY part that serves products is a code stream)
    out[2] = all_code ? 1 : 0;
    out[3] = (p.lds_code && p.lds_codegen_device) ? 1 : 0;   // generated on the device (round 5), not by the host encoder
    return 0;
}

int pygim_group_lds_tiles(int64_t handle, int64_t out[4]) {
    Group *g = lookup(handle);
    if (!g) return fail(PYGIM_ERR_INVALID, "unknown group handle");
    const Part &p = serving_part(g);
    out[0] = p.lds_tile_labels ? 1 : 0;
    out[1] = p.lds_tile_labels;
    out[2] = p.lds_tile_largest;
    out[3] = p.panel_locality_used ? p.sim_kind : 0;   // the sweep's items in locality order: 1 = by id (local ids), 2 = by propagated label
    return 0;
}

int pygim_group_serial(int64_t handle, int64_t *out) {
    Group *g = lookup(handle);
    if (!g || !out) return fail(PYGIM_ERR_INVALID, "unknown group handle");
    *out = g->serial;
    return 0;
}

int pygim_group_lds_runs(int64_t handle, int64_t *out) {
    Group *g = lookup(handle);
    if (!g || !out) return fail(PYGIM_ERR_INVALID, "unknown group handle");
    *out = g->lds_runs;
    return 0;
}

int pygim_group_host_windows(int64_t handle, int64_t *windows, int64_t *direct) {
    Group *g = lookup(handle);
    if (!g || !windows) return fail(PYGIM_ERR_INVALID, "unknown group handle");
    *windows = g->host_windows_used;
    if (direct) *direct = g->host_direct_used;
    return 0;
}

int pygim_group_lds_geometry(int64_t handle, int64_t out[10]) {
    Group *g = lookup(handle);
    if (!g) return fail(PYGIM_ERR_INVALID, "unknown group handle");
    const Part &p = serving_part(g);
    for (int i = 0; i < 10; i++) out[i] = 0;
    if (!p.lds_tiles) return 0;
    out[0] = p.lds_nw;
    out[1] = p.lds_ka;
    out[2] = p.lds_kc;
    out[3] = p.lds_nbuf;
    out[4] = p.lds_is_code ? p.lds_code_gsize : 0;
    out[5] = p.lds_is_code ? p.lds_code_nsets : 0;
    out[6] = p.lds_is_code ? (int64_t)p.lds_code_shared : 0;
    out[7] = p.lds_col_splits;
    // a product of the group's full width, as launch_lds lays it over the XCDs under the tunables of this moment
    const size_t es = lds_el_bytes(g->dtype);
    const LdsStaged xs = lds_staged(es, es == 1, (uint32_t)std::max<int64_t>(g->h, 1), (uint64_t)p.ncols, p.lds_kc, p.lds_half);
    const LdsXcdLayout lay = lds_xcd_layout(lds_part_plan(p), xs.nslices, es == 8, lds_launch_knobs());
    out[8] = lay.sx;
    out[9] = lay.touch_share;
    return 0;
}

int pygim_group_lds_note(int64_t handle, char *out, int64_t cap) {
    Group *g = lookup(handle);
    if (!g) return fail(PYGIM_ERR_INVALID, "unknown group handle");
    if (!out || cap <= 0) return fail(PYGIM_ERR_INVALID, "no buffer");
    // the parts that serve the group's products: the merged matrix, or -- several parts run one by one -- every part: a later part that
    // took a lower rung of the ladder than part 0 is named too (nothing falls back silently)
    std::string text;
    if ((g->merged && g_tune.merge_parts && g->parts.size() > 1) || g->parts.size() == 1) {
        text = serving_part(g).lds_note;
    } else {
        text = g->parts[0].lds_note;
        for (size_t i = 1; i < g->parts.size(); i++)
            if (g->parts[i].lds_note != g->parts[0].lds_note) text += "; part " + std::to_string(i) + ": " + g->parts[i].lds_note;
    }
    for (size_t i = 0; i < g->parts.size(); i++)
        if (!g->parts[i].hy_note.empty()) text += "; part " + std::to_string(i) + ": " + g->parts[i].hy_note;   // (a split that was tried and dropped says why)
    const size_t n = std::min<size_t>(text.size(), (size_t)cap - 1);
    std::memcpy(out, text.data(), n);
    out[n] = 0;
    return 0;
}

int pygim_group_info(int64_t handle, int64_t out[8]) {
    Group *g = lookup(handle);
    if (!g) return fail(PYGIM_ERR_INVALID, "unknown group handle");
    out[0] = g->total_rows;
    out[1] = g->total_cols;
    out[2] = g->h;
    out[3] = (int64_t)g->parts.size();
    int64_t nl = 0;
    for (auto &p : g->parts) nl += p.lp_base.n_long;
    out[4] = nl;
    out[5] = g->all_ones ? 1 : 0;
    out[6] = g->parts[0].d_items ? (int64_t)g->parts[0].npanels : 0;
    out[7] = (int64_t)g->parts[0].n_items;
    return 0;
}

int pygim_block_run_x(int64_t handle, int part, const void *X, int64_t ldx, void *C, int64_t ldc, int64_t width,
                      int accumulate, int x_unchanged, void *stream) {
    if (int rc = need_init()) return rc;
    Group *g = lookup(handle);
    if (!g) return fail(PYGIM_ERR_INVALID, "unknown group handle");
    if (part < 0 || part >= (int)g->parts.size()) return fail(PYGIM_ERR_INVALID, "part index out of range");
    if (!X || !C || width <= 0 || ldx < width || ldc < width) return fail(PYGIM_ERR_INVALID, "bad X/C/width/stride");
    if (!is_device_ptr(X) || !is_device_ptr(C)) return fail(PYGIM_ERR_INVALID, "pygim_block_run needs device pointers");
    g->x_unchanged = x_unchanged != 0;
    const int rc = launch_block_any(g, g->parts[part], X, ldx, C, ldc, width, accumulate != 0, (hipStream_t)stream);
    g->x_unchanged = false;
    return rc;
}

int pygim_block_run(int64_t handle, int part, const void *X, int64_t ldx, void *C, int64_t ldc, int64_t width,
                    int accumulate, void *stream) {
    return pygim_block_run_x(handle, part, X, ldx, C, ldc, width, accumulate, 0, stream);
}

int pygim_spmm_run_group_x(int64_t handle, const void *const *B_parts, void *out, int x_unchanged, void *stream) {
    if (int rc = need_init()) return rc;
    Group *g = lookup(handle);
    if (!g) return fail(PYGIM_ERR_INVALID, "unknown group handle");
    for (auto &p : g->parts)
        if (p.dense_cols != g->parts[0].dense_cols)
            return fail(PYGIM_ERR_INVALID, "spmm_run_group needs the same dense split for every sparse part");
    g->x_unchanged = x_unchanged != 0;
    const int rc = run_group_common(g, B_parts, nullptr, false, out, (hipStream_t)stream);
    g->x_unchanged = false;
    return rc;
}

int pygim_spmm_run_group(int64_t handle, const void *const *B_parts, void *out, void *stream) {
    return pygim_spmm_run_group_x(handle, B_parts, out, 0, stream);
}

int pygim_grande_run_group(int64_t handle, const void *const *B_windows, const int64_t *window_ld, void *out,
                           void *stream) {
    if (int rc = need_init()) return rc;
    Group *g = lookup(handle);
    if (!g) return fail(PYGIM_ERR_INVALID, "unknown group handle");
    if (!window_ld) return fail(PYGIM_ERR_INVALID, "window_ld is required");
    return run_group_common(g, B_windows, window_ld, true, out, (hipStream_t)stream);
}

int pygim_spmv_run_group(int64_t handle, const void *const *B_vectors, void *out, void *stream) {
    if (int rc = need_init()) return rc;
    Group *g = lookup(handle);
    if (!g) return fail(PYGIM_ERR_INVALID, "unknown group handle");
    hipStream_t st = (hipStream_t)stream;
    const size_t es = dtype_size(g->dtype);
    const size_t nvec = g->parts[0].dense_cols.size();
    for (auto &p : g->parts) {
        if (p.dense_cols.size() != nvec) return fail(PYGIM_ERR_INVALID, "spmv group: dense split differs between parts");
        for (auto wdt : p.dense_cols)
            if (wdt != 1) return fail(PYGIM_ERR_INVALID, "spmv group: every dense part must be one column wide");
    }
    static const OperandTexts texts{"null vectors or output", "null vector", "vectors mix host and device memory",
                                    "vectors and output must both be host or both be device memory"};
    bool dev_in = false;
    if (int rc = check_dense_operands(B_vectors, nvec, out, texts, &dev_in)) return rc;
    const bool dev_out = dev_in;   // (checked: both on one side)
    const uint64_t n = (uint64_t)g->total_cols;
    // layout of stage_in: [packed panel n x nvec][raw vectors (host mode only)]
    const size_t panel_bytes = ((size_t)n * nvec * es + 255) & ~(size_t)255;
    const size_t vec_bytes = ((size_t)n * es + 255) & ~(size_t)255;
    const size_t need_in = panel_bytes + (dev_in ? 0 : vec_bytes * nvec);
    if (int rc = ensure(&g->stage_in, &g->stage_in_bytes, std::max<size_t>(need_in, 256))) return rc;
    if (g->d_ptrs_n < nvec) {
        if (g->d_ptrs) HIP_TRY(hipFree(g->d_ptrs));  // (waits for earlier packs)
        g->d_ptrs = nullptr;
        HIP_TRY(hipMalloc((void **)&g->d_ptrs, 2 * nvec * sizeof(void *)));
        g->d_ptrs_n = nvec;
    }
    // pointer table of the pack kernel: page-locked host memory, two slots used in turn, each released by an event
    // recorded behind the pack kernel that read it -- device-pointer calls only enqueue work (no host sync)
    if (g->h_ptrs_n < nvec) {
        if (g->h_ptrs) HIP_TRY(hipHostFree(g->h_ptrs));
        g->h_ptrs = nullptr;
        HIP_TRY(hipHostMalloc((void **)&g->h_ptrs, 2 * nvec * sizeof(void *), hipHostMallocDefault));
        g->h_ptrs_n = nvec;
        for (hipEvent_t &e : g->ev_ptrs)
            if (!e) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    const int slot = g->ptr_slot;
    g->ptr_slot ^= 1;
    HIP_TRY(hipEventSynchronize(g->ev_ptrs[slot]));  // (a never-recorded event is complete)
    const void **src = (const void **)(g->h_ptrs + (size_t)slot * g->h_ptrs_n);
    const double t0 = now_ms();
    for (size_t j = 0; j < nvec; j++) {
        if (dev_in) {
            src[j] = B_vectors[j];
        } else {
            void *d = (char *)g->stage_in + panel_bytes + j * vec_bytes;
            if (n) HIP_TRY(hipMemcpyAsync(d, B_vectors[j], (size_t)n * es, hipMemcpyHostToDevice, st));
            src[j] = d;
        }
    }
    if (!dev_in) HIP_TRY(hipStreamSynchronize(st));  // host mode: the upload time is reported
    HIP_TRY(hipMemcpyAsync(g->d_ptrs + (size_t)slot * nvec, src, nvec * sizeof(void *), hipMemcpyHostToDevice, st));
    const double t1 = now_ms();
    const void *const *tab = (const void *const *)(g->d_ptrs + (size_t)slot * nvec);
    switch (es) {
        case 1: launch_pack<int8_t>(tab, (uint32_t)nvec, n, g->stage_in, st); break;
        case 2: launch_pack<int16_t>(tab, (uint32_t)nvec, n, g->stage_in, st); break;
        case 4: launch_pack<int32_t>(tab, (uint32_t)nvec, n, g->stage_in, st); break;
        case 8: launch_pack<int64_t>(tab, (uint32_t)nvec, n, g->stage_in, st); break;
    }
    HIP_TRY(hipEventRecord(g->ev_ptrs[slot], st));
    void *dout = out;
    if (!dev_out) {
        if (int rc = ensure(&g->stage_out, &g->stage_out_bytes, std::max<size_t>((size_t)g->total_rows * nvec * es, 256))) return rc;
        dout = g->stage_out;
    }
    if (g->merged && g_tune.merge_parts && g->parts.size() > 1) {
        if (int rc = launch_block_any(g, *g->merged, g->stage_in, (int64_t)nvec, dout, (int64_t)nvec, (int64_t)nvec, false, st))
            return rc;
    } else {
        int64_t brow = 0;
        for (size_t i = 0; i < g->parts.size(); i++) {
            Part &p = g->parts[i];
            const char *x = (const char *)g->stage_in + (size_t)brow * nvec * es;
            if (int rc = launch_block_any(g, p, x, (int64_t)nvec, dout, (int64_t)nvec, (int64_t)nvec, i > 0, st)) return rc;
            brow += p.ncols;
        }
    }
    if (!dev_out) {
        HIP_TRY(hipStreamSynchronize(st));
        const double t2 = now_ms();
        const size_t bytes = (size_t)g->total_rows * nvec * es;
        if (bytes) HIP_TRY(hipMemcpyAsync(out, dout, bytes, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        g->timers[0] = t1 - t0;
        g->timers[1] = t2 - t1;
        g->timers[2] = now_ms() - t2;
        g->timers[3] = 0;
    }
    return 0;
}

}  // extern "C"
