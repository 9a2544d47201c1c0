// spmm_multi_dev.hpp -- several statistics of a row's stored entries in ONE gather (PNA-style aggregation), unit weights:
//   S1[r, f] = sum over the stored entries e of row r, in stored order, of X[colind[e], f]        S2[r, f] = the same sum of X * X
//   sum = S1    mean = S1 / n    var = max(S2 / n - mean * mean, 0)    std = sqrt(var + eps)       n = the row's number of stored entries
//   max, min = the winning X[colind[e], f] itself, optionally with the index of the entry that won (arg_max, arg_min)
// A gather kernel waits for the X rows (profiles/exp_reduce.txt), so the per-entry arithmetic of all of these is held in registers beside one
// gather instead of one gather per statistic.  out[r, j * h + f] holds statistic j of the caller's list; which statistics are stored is a
// run-time argument (MultiStats), what a lane carries per feature is chosen by two template switches:
//   MOMENTS  S1 and S2, accumulated in T in exactly the order FoldSum adds (entry order in a run, the xor tree of the lane groups, then
//            the runs in order): sum and mean have the bits of pygim_spmm_reduce MEAN without values
//   BEST     the pairs (max, index) and (min, index) of FoldBest<RD_MAX> and FoldBest<RD_MIN> (spmm_reduce_dev.hpp), joined with rd_better:
//            its tie rule (the lowest entry index) and its NaN rule (a NaN never wins against a number)
// NaN and inf travel through S1 / S2 as IEEE addition carries them, into sum, mean, var and std of that (row, feature) alone; the clamp
// of var keeps a NaN (v < 0 ? 0 : v).
//
// The walk inside k_multi_gather -- batch loop, row search, ballot of row ends, cut into stretches, slot rule -- is a copy of
// k_row_gather's (row_gather_dev.hpp, which lists all the copies and says why they stay), with a tuple of partial results in place of the
// Fold: a change to the walk there has to be made here as well.  k_multi_fixup finds its row with rg_cut_row and launch_multi_gather_v
// picks the launch form with rg_dispatch, both shared with k_row_gather and k_gat_gather.
//
// The workspace holds, per run, two slots of h elements of every component the instantiation carries: S1, S2 (MOMENTS), then the max
// and min values and their two int32 index arrays (BEST); every sub-array starts 16-byte aligned.  A row that lies wholly inside a
// wave's run is stored directly, finished; the at most two rows a run shares with its neighbours leave their raw tuples in the slots
// and k_multi_fixup joins them per row in the order of the runs.  Rows without entries are written by k_multi_empty: 0, sqrt(eps) for
// std (the formula at S1 = S2 = 0), -1 in arg.  No two kernels write the same row, no atomics: the same bits on every launch.
//
// S is the storage type of X and out, T the type of everything else: S = T = float / double, or S = _Float16 / __bf16 with T = float --
// an X piece is widened as it is folded (exact) and every finished value is rounded once, where the row is stored.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "row_gather_dev.hpp"
#include "spmm_reduce_dev.hpp"

namespace pygim {

constexpr int MS_SUM = 0, MS_MEAN = 1, MS_MIN = 2, MS_MAX = 3, MS_VAR = 4, MS_STD = 5, MS_COUNT = 6;   // PYGIM_STAT_*

// which statistics a call stores: col[s] = the first column of statistic s in a row of out (j * h), -1 when it is not asked for
template <typename T> struct MultiStats {
    int32_t col[MS_COUNT];
    T eps;
};

// the sub-arrays of the workspace (null for what the instantiation does not carry)
template <typename T> struct MultiWs {
    T *s1, *s2, *vmax, *vmin;
    int32_t *imax, *imin;
};

__device__ inline float ms_sqrt(float x) { return sqrtf(x); }
__device__ inline double ms_sqrt(double x) { return sqrt(x); }

// The finished-row store of VEC features from column f on, used by the direct flush and by the fix-up alike.  n: the row's stored entries.
template <typename T, typename S, int VEC, bool MOMENTS, bool BEST>
__device__ inline void ms_store_row(S *__restrict__ orow, int32_t *__restrict__ amax_row, int32_t *__restrict__ amin_row, uint32_t f, const T *s1,
                                    const T *s2, const T *vmax, const int32_t *imax, const T *vmin, const int32_t *imin, T n, const MultiStats<T> &st) {
    if constexpr (MOMENTS) {
        if (st.col[MS_SUM] >= 0) rg_store<S, T, VEC>(orow + st.col[MS_SUM] + f, s1);
        T mean[VEC];
#pragma unroll
        for (int i = 0; i < VEC; i++) mean[i] = s1[i] / n;
        if (st.col[MS_MEAN] >= 0) rg_store<S, T, VEC>(orow + st.col[MS_MEAN] + f, mean);
        if (st.col[MS_VAR] >= 0 || st.col[MS_STD] >= 0) {
            T var[VEC];
#pragma unroll
            for (int i = 0; i < VEC; i++) {
                const T v = s2[i] / n - mean[i] * mean[i];
                var[i] = v < T(0) ? T(0) : v;   // a NaN stays
            }
            if (st.col[MS_VAR] >= 0) rg_store<S, T, VEC>(orow + st.col[MS_VAR] + f, var);
            if (st.col[MS_STD] >= 0) {
#pragma unroll
                for (int i = 0; i < VEC; i++) var[i] = ms_sqrt(var[i] + st.eps);
                rg_store<S, T, VEC>(orow + st.col[MS_STD] + f, var);
            }
        }
    }
    if constexpr (BEST) {
        if (st.col[MS_MAX] >= 0) rg_store<S, T, VEC>(orow + st.col[MS_MAX] + f, vmax);
        if (st.col[MS_MIN] >= 0) rg_store<S, T, VEC>(orow + st.col[MS_MIN] + f, vmin);
        if (amax_row) rg_store_idx<VEC>(amax_row + f, imax, true);
        if (amin_row) rg_store_idx<VEC>(amin_row + f, imin, true);
    }
}

// WHOLE: the wave is one lane group (L = 64) that holds NV pieces of VEC features per lane; else NV = 1 and L < 64 is a launch argument.
// arg_max, arg_min: may be null.  Six state registers per feature in the MOMENTS + BEST form beside the gathers in flight: U is set here
// and nowhere else.
template <typename T, typename S, int VEC, int NV, bool WHOLE, bool MOMENTS, bool BEST>
__global__ __launch_bounds__(256) void k_multi_gather(const uint32_t *__restrict__ rowptr, const uint32_t *__restrict__ colind, uint32_t nrows, uint32_t nnz,
                                                      const S *__restrict__ X, uint64_t ldx, uint32_t h, uint32_t L, S *__restrict__ out, uint64_t ldo,
                                                      int32_t *__restrict__ arg_max, int32_t *__restrict__ arg_min, MultiWs<T> ws, MultiStats<T> st) {
    using V = typename SdVec<S, VEC>::type;
    constexpr int U = NV == 1 ? RG_U : RG_U / 2;
    constexpr int NM = MOMENTS ? NV : 1, NB = BEST ? NV : 1;   // the state that is not carried shrinks to one unused piece
    if constexpr (WHOLE) L = 64;
    const uint32_t R = 64 / L;
    const uint32_t lane = threadIdx.x & 63, grp = lane / L, li = lane % L;
    const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint64_t e_begin = wave * RG_EPW;
    if (e_begin >= nnz) return;
    const uint32_t e_end = (uint32_t)(e_begin + RG_EPW < nnz ? e_begin + RG_EPW : nnz);
    uint32_t f[NV];
    bool fok[NV];
#pragma unroll
    for (int v = 0; v < NV; v++) {
        f[v] = ((blockIdx.y * NV + v) * L + li) * VEC;
        fok[v] = f[v] < h;
    }
    uint32_t row_cur = sd_row_of(rowptr, 0, nrows, (uint32_t)e_begin);
    const uint32_t row_hi = sd_row_of(rowptr, row_cur, nrows, e_end - 1) + 1;
    bool head_open = rowptr[row_cur] < (uint32_t)e_begin;   // the first row of the run began in an earlier run
    bool pending = false;
    T s1[NM][VEC], s2[NM][VEC];       // the running sums of x and of x * x ...
    T vmax[NB][VEC], vmin[NB][VEC];   // ... the best values so far ...
    int32_t imax[NB][VEC], imin[NB][VEC];   // ... and the entries that hold them
    const uint64_t slots = wave * 2 * (uint64_t)h;   // the run's two slots, in elements of every sub-array
    const auto reset = [&]() {
#pragma unroll
        for (int v = 0; v < NV; v++)
#pragma unroll
            for (int i = 0; i < VEC; i++) {
                if constexpr (MOMENTS) s1[v][i] = s2[v][i] = T(0);
                if constexpr (BEST) {
                    vmax[v][i] = rd_worst<RD_MAX, T>();
                    vmin[v][i] = rd_worst<RD_MIN, T>();
                    imax[v][i] = imin[v][i] = RD_NONE;
                }
            }
    };
    // join the lane groups, then store: the raw tuple into the workspace slots, or the finished row `row` into out / arg_max / arg_min
    const auto flush = [&](bool to_slot, uint32_t slot, uint32_t row) {
        const uint64_t at = slots + (slot ? h : 0u);
        T cnt = T(1);
        if (!to_slot) cnt = T(rowptr[row + 1] - rowptr[row]);
#pragma unroll
        for (int v = 0; v < NV; v++) {
            if constexpr (!WHOLE) {
                for (uint32_t s = L; s < 64; s <<= 1) {
#pragma unroll
                    for (int i = 0; i < VEC; i++) {
                        if constexpr (MOMENTS) {
                            s1[v][i] = s1[v][i] + rg_shfl_xor(s1[v][i], (int)s);
                            s2[v][i] = s2[v][i] + rg_shfl_xor(s2[v][i], (int)s);
                        }
                        if constexpr (BEST) {
                            const int32_t oa = __shfl_xor(imax[v][i], (int)s, 64), oi = __shfl_xor(imin[v][i], (int)s, 64);
                            FoldBest<RD_MAX>::join(vmax[v][i], imax[v][i], rg_shfl_xor(vmax[v][i], (int)s), oa);
                            FoldBest<RD_MIN>::join(vmin[v][i], imin[v][i], rg_shfl_xor(vmin[v][i], (int)s), oi);
                        }
                    }
                }
            }
            if (grp == 0 && fok[v]) {
                const int m = MOMENTS ? v : 0, b = BEST ? v : 0;
                if (to_slot) {
                    if constexpr (MOMENTS) {
                        rg_store<T, T, VEC>(ws.s1 + at + f[v], s1[m]);
                        rg_store<T, T, VEC>(ws.s2 + at + f[v], s2[m]);
                    }
                    if constexpr (BEST) {
                        rg_store<T, T, VEC>(ws.vmax + at + f[v], vmax[b]);
                        rg_store<T, T, VEC>(ws.vmin + at + f[v], vmin[b]);
                        rg_store_idx<VEC>(ws.imax + at + f[v], imax[b], false);
                        rg_store_idx<VEC>(ws.imin + at + f[v], imin[b], false);
                    }
                } else {
                    ms_store_row<T, S, VEC, MOMENTS, BEST>(out + (uint64_t)row * ldo, arg_max ? arg_max + (uint64_t)row * h : nullptr,
                                                           arg_min ? arg_min + (uint64_t)row * h : nullptr, f[v], s1[m], s2[m], vmax[b], imax[b], vmin[b],
                                                           imin[b], cnt, st);
                }
            }
        }
    };
    reset();

    for (uint32_t base = (uint32_t)e_begin; base < e_end; base += 64) {
        const uint32_t n = (base + 64 < e_end ? base + 64 : e_end) - base;
        const uint32_t my_e = base + lane;
        const bool valid = lane < n;
        const uint32_t my_col = valid ? colind[my_e] : 0u;
        uint32_t my_row = row_cur;
        bool my_end = false;
        if (valid) {
            my_row = sd_row_of(rowptr, row_cur, row_hi, my_e);
            my_end = rowptr[my_row + 1] == my_e + 1;
        }
        const uint64_t endmask = __ballot(my_end);
        uint32_t pos = 0;
        while (pos < n) {
            const uint64_t m = endmask >> pos;
            const bool closes = m != 0;
            const uint32_t last = closes ? pos + (uint32_t)__builtin_ctzll(m) : n - 1;
            for (uint32_t k0 = pos; k0 <= last; k0 += R * U) {
                V x[U][NV];
                bool ok[U];
                int32_t ei[U];
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const uint32_t kk = k0 + (uint32_t)u * R + grp;
                    ok[u] = kk <= last;
                    ei[u] = (int32_t)(base + kk);
                    const uint32_t col = rg_take32<WHOLE>(my_col, ok[u] ? kk : pos);
                    const S *xr = X + (uint64_t)col * ldx;
#pragma unroll
                    for (int v = 0; v < NV; v++) {
                        x[u][v] = V(0);
                        if (ok[u] && fok[v]) x[u][v] = *(const V *)(xr + f[v]);
                    }
                }
#pragma unroll
                for (int u = 0; u < U; u++) {
#pragma unroll
                    for (int v = 0; v < NV; v++)
                        if (ok[u] && fok[v]) {
#pragma unroll
                            for (int i = 0; i < VEC; i++) {
                                const T xv = T(rg_get<S, VEC>(x[u][v], i));
                                if constexpr (MOMENTS) {
                                    s1[v][i] = s1[v][i] + xv;
                                    s2[v][i] = s2[v][i] + xv * xv;
                                }
                                if constexpr (BEST) {
                                    FoldBest<RD_MAX>::join(vmax[v][i], imax[v][i], xv, ei[u]);
                                    FoldBest<RD_MIN>::join(vmin[v][i], imin[v][i], xv, ei[u]);
                                }
                            }
                        }
                }
            }
            if (closes) {
                flush(head_open, 0u, rg_take32<true>(my_row, last));
                reset();
                head_open = false;
            }
            pending = !closes;
            pos = last + 1;
        }
        row_cur = rg_take32<true>(my_row, n - 1);
    }
    if (pending) flush(true, head_open ? 0u : 1u, 0u);   // the run's last row goes on in the next run
}

// one wave per run: the row that goes on after run w = slot 1 of w joined with slot 0 of every later run the row reaches, in order
// (the loop of k_row_gather_fixup on a tuple)
template <typename T, typename S, bool MOMENTS, bool BEST>
__global__ __launch_bounds__(256) void k_multi_fixup(const uint32_t *__restrict__ rowptr, uint32_t nrows, uint32_t nnz, uint32_t h, MultiWs<T> ws,
                                                     S *__restrict__ out, uint64_t ldo, int32_t *__restrict__ arg_max, int32_t *__restrict__ arg_min,
                                                     MultiStats<T> st) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t w = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    uint32_t row, rb, re;
    uint64_t w1;
    if (!rg_cut_row(rowptr, nrows, nnz, w, row, rb, re, w1)) return;
    for (uint32_t f = lane; f < h; f += 64) {
        uint64_t at = (w * 2 + 1) * (uint64_t)h + f;
        T s1 = T(0), s2 = T(0), vmax = T(0), vmin = T(0);
        int32_t imax = RD_NONE, imin = RD_NONE;
        if constexpr (MOMENTS) {
            s1 = ws.s1[at];
            s2 = ws.s2[at];
        }
        if constexpr (BEST) {
            vmax = ws.vmax[at];
            vmin = ws.vmin[at];
            imax = ws.imax[at];
            imin = ws.imin[at];
        }
        for (uint64_t j = w + 1; j <= w1; j++) {
            at = j * 2 * (uint64_t)h + f;
            if constexpr (MOMENTS) {
                s1 = s1 + ws.s1[at];
                s2 = s2 + ws.s2[at];
            }
            if constexpr (BEST) {
                FoldBest<RD_MAX>::join(vmax, imax, ws.vmax[at], ws.imax[at]);
                FoldBest<RD_MIN>::join(vmin, imin, ws.vmin[at], ws.imin[at]);
            }
        }
        ms_store_row<T, S, 1, MOMENTS, BEST>(out + (uint64_t)row * ldo, arg_max ? arg_max + (uint64_t)row * h : nullptr,
                                             arg_min ? arg_min + (uint64_t)row * h : nullptr, f, &s1, &s2, &vmax, &imax, &vmin, &imin, T(re - rb), st);
    }
}

// rows without entries: 0 for sum, mean, var, max and min, sqrt(eps) for std, -1 in arg_max / arg_min
// (the walk of k_row_gather_empty: a change there has to be made here as well)
template <typename T, typename S>
__global__ __launch_bounds__(256) void k_multi_empty(const uint32_t *__restrict__ rowptr, uint32_t nrows, uint32_t h, S *__restrict__ out, uint64_t ldo,
                                                     int32_t *__restrict__ arg_max, int32_t *__restrict__ arg_min, MultiStats<T> st) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t row = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= nrows || rowptr[row] != rowptr[row + 1]) return;
    const S at_std = S(ms_sqrt(T(0) + st.eps));
    for (uint32_t f = lane; f < h; f += 64) {
#pragma unroll
        for (int s = 0; s < MS_COUNT; s++)
            if (st.col[s] >= 0) out[row * ldo + (uint32_t)st.col[s] + f] = s == MS_STD ? at_std : S(0);
        if (arg_max) arg_max[row * h + f] = -1;
        if (arg_min) arg_min[row * h + f] = -1;
    }
}

// ---- the workspace: per run two slots of h elements of S1, S2 (moments), max, min and their two index arrays (best), each 16-byte aligned ----
inline uint64_t multi_sub_bytes(uint64_t nnz, uint64_t h, size_t elem) { return row_gather_index_offset(nnz, h, elem); }
inline uint64_t multi_workspace_bytes(bool moments, bool best, uint64_t nnz, uint64_t h, size_t elem) {
    return (moments ? 2 * multi_sub_bytes(nnz, h, elem) : 0) + (best ? 2 * multi_sub_bytes(nnz, h, elem) + 2 * multi_sub_bytes(nnz, h, sizeof(int32_t)) : 0);
}

// the lane layout: the mean fold's (16-byte pieces of the storage type when every row of X and out starts 16-byte aligned and h fills
// whole pieces -- then every block [j * h, (j + 1) * h) of a row of out starts 16-byte aligned as well)
inline LaunchShape multi_gather_shape(uint32_t h, uint32_t V, bool aligned) { return row_gather_shape(h, h, V, aligned); }

template <typename T, typename S, int VEC, bool MOMENTS, bool BEST>
inline void launch_multi_gather_v(const uint32_t *rowptr, const uint32_t *colind, uint32_t nrows, uint32_t nnz, const S *X, uint64_t ldx, uint32_t h, S *out,
                                  uint64_t ldo, int32_t *arg_max, int32_t *arg_min, const MultiWs<T> &ws, const MultiStats<T> &st, const LaunchShape &g,
                                  hipStream_t stream) {
    rg_dispatch(nnz, g, [&](auto nv, auto whole, dim3 grid, uint32_t L) {
        hipLaunchKernelGGL((k_multi_gather<T, S, VEC, decltype(nv)::value, decltype(whole)::value, MOMENTS, BEST>), grid, dim3(256), 0, stream, rowptr, colind,
                           nrows, nnz, X, ldx, h, L, out, ldo, arg_max, arg_min, ws, st);
    });
}

template <typename T, typename S, bool MOMENTS, bool BEST>
inline void launch_multi_gather_mb(const uint32_t *rowptr, const uint32_t *colind, uint32_t nrows, uint32_t nnz, const S *X, uint64_t ldx, uint32_t h, S *out,
                                   uint64_t ldo, int32_t *arg_max, int32_t *arg_min, void *workspace, const MultiStats<T> &st, hipStream_t stream) {
    constexpr uint32_t V = 16 / sizeof(S);
    MultiWs<T> ws = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    char *p = (char *)workspace;
    const uint64_t sub = multi_sub_bytes(nnz, h, sizeof(T));
    if (MOMENTS) {
        ws.s1 = (T *)p;
        ws.s2 = (T *)(p + sub);
        p += 2 * sub;
    }
    if (BEST) {
        ws.vmax = (T *)p;
        ws.vmin = (T *)(p + sub);
        ws.imax = (int32_t *)(p + 2 * sub);
        ws.imin = (int32_t *)(p + 2 * sub + multi_sub_bytes(nnz, h, sizeof(int32_t)));
    }
    const bool aligned = ldx % V == 0 && ldo % V == 0 && (uintptr_t)X % 16 == 0 && (uintptr_t)out % 16 == 0 && (uintptr_t)workspace % 16 == 0;
    const LaunchShape g = multi_gather_shape(h, V, aligned);
    if (g.vec > 1) launch_multi_gather_v<T, S, (int)V, MOMENTS, BEST>(rowptr, colind, nrows, nnz, X, ldx, h, out, ldo, arg_max, arg_min, ws, st, g, stream);
    else launch_multi_gather_v<T, S, 1, MOMENTS, BEST>(rowptr, colind, nrows, nnz, X, ldx, h, out, ldo, arg_max, arg_min, ws, st, g, stream);
    const uint64_t runs = row_gather_runs(nnz);
    if (runs > 1)
        hipLaunchKernelGGL((k_multi_fixup<T, S, MOMENTS, BEST>), dim3((unsigned)((runs + 2) / 4)), dim3(256), 0, stream, rowptr, nrows, nnz, h, ws, out, ldo,
                           arg_max, arg_min, st);
}

// moments: one of sum, mean, var, std is asked for; best: max or min is (the caller derives both from st.col, and at least one holds)
template <typename T, typename S>
inline void launch_spmm_multi(const uint32_t *rowptr, const uint32_t *colind, uint32_t nrows, uint32_t nnz, const S *X, uint64_t ldx, uint32_t h, S *out,
                              uint64_t ldo, int32_t *arg_max, int32_t *arg_min, void *workspace, const MultiStats<T> &st, bool moments, bool best,
                              hipStream_t stream) {
    if (nrows > 0) hipLaunchKernelGGL((k_multi_empty<T, S>), dim3((nrows + 3) / 4), dim3(256), 0, stream, rowptr, nrows, h, out, ldo, arg_max, arg_min, st);
    if (nnz == 0) return;
    if (moments && best)
        launch_multi_gather_mb<T, S, true, true>(rowptr, colind, nrows, nnz, X, ldx, h, out, ldo, arg_max, arg_min, workspace, st, stream);
    else if (moments)
        launch_multi_gather_mb<T, S, true, false>(rowptr, colind, nrows, nnz, X, ldx, h, out, ldo, arg_max, arg_min, workspace, st, stream);
    else
        launch_multi_gather_mb<T, S, false, true>(rowptr, colind, nrows, nnz, X, ldx, h, out, ldo, arg_max, arg_min, workspace, st, stream);
}

}  // namespace pygim
