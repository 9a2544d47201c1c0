// spmm_reduce_dev.hpp -- the row-wise reductions other than the sum on a caller's CSR, as folds of k_row_gather (row_gather_dev.hpp):
//   out[r, f] = REDUCE over the stored entries e of row r of w[e] * X[colind[e], f],   w[e] = values[e], or 1 without values
// REDUCE = mean (FoldSum<true>: the sum of pygim_spmm_values, in its order, divided by the row's number of stored entries), max or
// min (FoldBest, all six element types; optionally with arg[r, f] = the index, in stored order, of the entry that won), and the
// gradient of max / min with respect to X (k_spmm_reduce_bwd).
//
// The tie rule of max / min: among equal products the LOWEST entry index wins.  A partial result is a pair (value, entry index) and
// rd_better compares pairs -- in the per-lane scan, in the xor tree of the lane groups and in the fix-up alike -- so the winner does
// not depend on how the entries were dealt to lanes, groups and runs.  -0.0 and +0.0 are equal (the lower index wins).
// NaN: a NaN product never wins against a number and a number always replaces a NaN, wherever the NaN stands in the row; if every
// product of a row is NaN the row stores NaN and arg -1 (no entry won).  Integer products wrap like the type's own arithmetic and
// compare as signed values.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <limits>
#include <type_traits>

#include "row_gather_dev.hpp"

namespace pygim {

constexpr int RD_MEAN = 1, RD_MAX = 2, RD_MIN = 3;   // PYGIM_REDUCE_*

// does the pair (pv, pi) beat the pair (bv, bi)?  A total order on pairs with distinct indices, so folds may be regrouped freely.
template <int OP, typename T> __device__ inline bool rd_better(T pv, int32_t pi, T bv, int32_t bi) {
    if constexpr (std::is_floating_point<T>::value) {
        const bool wins = OP == RD_MAX ? !(pv <= bv) : !(pv >= bv);   // true as well when bv is NaN
        return pv == pv && (wins || (pv == bv && pi < bi));
    } else {
        const bool wins = OP == RD_MAX ? pv > bv : pv < bv;
        return wins || (pv == bv && pi < bi);
    }
}

// what every entry beats (with index RD_NONE): NaN for floats, the far end of the type for integers
template <int OP, typename T> __device__ inline T rd_worst() {
    if constexpr (std::is_floating_point<T>::value) return std::numeric_limits<T>::quiet_NaN();
    else return OP == RD_MAX ? std::numeric_limits<T>::min() : std::numeric_limits<T>::max();
}

// max / min: the best product so far and the entry that holds it
template <int OP> struct FoldBest {
    static constexpr bool INDEXED = true, PER_HEAD = false, MEAN = false;
    template <typename T> __device__ static T neutral() { return rd_worst<OP, T>(); }
    template <typename T> __device__ static void join(T &a, int32_t &ai, T b, int32_t bi) {
        if (rd_better<OP, T>(b, bi, a, ai)) {
            a = b;
            ai = bi;
        }
    }
};

inline uint64_t spmm_reduce_workspace_bytes(int op, uint64_t nnz, uint64_t h, size_t elem) {
    return row_gather_index_offset(nnz, h, elem) + (op == RD_MEAN ? 0 : row_gather_slot_bytes(nnz, h, sizeof(int32_t)));
}

// the mean of 16-bit features (S = _Float16 / __bf16): float32 values, sums, slots and division; the quotient is rounded once into out
template <typename S>
inline void launch_spmm_mean16(const uint32_t *rowptr, const uint32_t *colind, uint32_t nrows, uint32_t nnz, const float *values, const S *X, uint64_t ldx,
                               uint32_t h, S *out, uint64_t ldo, void *workspace, hipStream_t st) {
    launch_row_gather<float, FoldSum<true>, S>(rowptr, colind, nrows, nnz, values, 1u, X, ldx, h, out, ldo, nullptr, workspace, st);
}

// op: RD_MEAN (floating types only: the caller checks), RD_MAX or RD_MIN
template <typename T>
inline void launch_spmm_reduce(int op, const uint32_t *rowptr, const uint32_t *colind, uint32_t nrows, uint32_t nnz, const T *values, const T *X, uint64_t ldx,
                               uint32_t h, T *out, uint64_t ldo, int32_t *arg, void *workspace, hipStream_t st) {
    if constexpr (std::is_floating_point<T>::value) {
        if (op == RD_MEAN) return launch_row_gather<T, FoldSum<true>>(rowptr, colind, nrows, nnz, values, 1u, X, ldx, h, out, ldo, nullptr, workspace, st);
    }
    if (op == RD_MAX) launch_row_gather<T, FoldBest<RD_MAX>>(rowptr, colind, nrows, nnz, values, 1u, X, ldx, h, out, ldo, arg, workspace, st);
    else launch_row_gather<T, FoldBest<RD_MIN>>(rowptr, colind, nrows, nnz, values, 1u, X, ldx, h, out, ldo, arg, workspace, st);
}

// ---- the gradient of max / min with respect to X: a gather on the transposed structure ----
//   dX[c, f] = sum over the entries e' of row c of A^T, in order, of (arg[r, f] == e ? w[e] * G[r, f] : 0),  e = perm[e'], r = rows_t[e']
// A lane group of L lanes owns output row c (64 / L rows side by side in a wave when rows are narrow), walks the row's entries in e'
// order with RB_U of them in flight, and reads an arg row beside every G row.  One owner per output row: no atomics, one order.
constexpr int RB_U = 4;

template <typename T, int VEC, int NV>
__global__ __launch_bounds__(256) void k_spmm_reduce_bwd(const uint32_t *__restrict__ rowptr_t, const uint32_t *__restrict__ rows_t,
                                                         const int32_t *__restrict__ perm, uint32_t ncols, const T *__restrict__ values,
                                                         const T *__restrict__ G, uint64_t ldg, const int32_t *__restrict__ arg, uint32_t h, uint32_t L,
                                                         T *__restrict__ dX, uint64_t ldd) {
    using V = typename SdVec<T, VEC>::type;
    using IV = typename RdIdx<VEC>::type;
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t c = t / L;
    const uint32_t li = (uint32_t)(t % L);
    if (c >= ncols) return;
    uint32_t f[NV];
    bool fok[NV];
    T acc[NV][VEC];
#pragma unroll
    for (int v = 0; v < NV; v++) {
        f[v] = ((blockIdx.y * NV + v) * L + li) * VEC;
        fok[v] = f[v] < h;
#pragma unroll
        for (int i = 0; i < VEC; i++) acc[v][i] = T(0);
    }
    const uint32_t k_end = rowptr_t[c + 1];
    for (uint32_t k0 = rowptr_t[c]; k0 < k_end; k0 += RB_U) {
        V g[RB_U][NV];
        IV a[RB_U][NV];
        T w[RB_U];
        int32_t e[RB_U];
        bool ok[RB_U];
#pragma unroll
        for (int u = 0; u < RB_U; u++) {
            ok[u] = k0 + u < k_end;
            const uint32_t k = ok[u] ? k0 + u : k0;
            const uint32_t r = rows_t[k];
            e[u] = perm[k];
            w[u] = values ? values[e[u]] : T(1);
#pragma unroll
            for (int v = 0; v < NV; v++)
                if (ok[u] && fok[v]) {
                    g[u][v] = *(const V *)(G + (uint64_t)r * ldg + f[v]);
                    a[u][v] = *(const IV *)(arg + (uint64_t)r * h + f[v]);
                }
        }
#pragma unroll
        for (int u = 0; u < RB_U; u++) {
#pragma unroll
            for (int v = 0; v < NV; v++)
                if (ok[u] && fok[v]) {
#pragma unroll
                    for (int i = 0; i < VEC; i++) {
                        int32_t ai;
                        if constexpr (VEC == 1) ai = a[u][v];
                        else ai = a[u][v][i];
                        acc[v][i] += ai == e[u] ? w[u] * rg_get<T, VEC>(g[u][v], i) : T(0);
                    }
                }
        }
    }
#pragma unroll
    for (int v = 0; v < NV; v++)
        if (fok[v]) rg_store<T, T, VEC>(dX + c * ldd + f[v], acc[v]);
}

template <typename T, int VEC>
inline void launch_spmm_reduce_bwd_v(const uint32_t *rowptr_t, const uint32_t *rows_t, const int32_t *perm, uint32_t ncols, const T *values, const T *G,
                                     uint64_t ldg, const int32_t *arg, uint32_t h, T *dX, uint64_t ldd, const LaunchShape &g, hipStream_t st) {
    if (g.npl == 1) {
        hipLaunchKernelGGL((k_spmm_reduce_bwd<T, VEC, 1>), dim3((unsigned)(((uint64_t)ncols * g.L + 255) / 256)), dim3(256), 0, st, rowptr_t, rows_t, perm,
                           ncols, values, G, ldg, arg, h, g.L, dX, ldd);
    } else {
        hipLaunchKernelGGL((k_spmm_reduce_bwd<T, VEC, 2>), dim3((unsigned)(((uint64_t)ncols * 64 + 255) / 256), g.chunks), dim3(256), 0, st,
                           rowptr_t, rows_t, perm, ncols, values, G, ldg, arg, h, 64u, dX, ldd);
    }
}

// the row walkers' layout, except that L lanes (not the whole wave) own an output row up to 64 pieces
inline LaunchShape spmm_reduce_bwd_shape(uint32_t h, uint32_t V, bool aligned) { return row_gather_shape(h, h, V, aligned, 64); }

template <typename T>
inline void launch_spmm_reduce_bwd(const uint32_t *rowptr_t, const uint32_t *rows_t, const int32_t *perm, uint32_t ncols, const T *values, const T *G,
                                   uint64_t ldg, const int32_t *arg, uint32_t h, T *dX, uint64_t ldd, hipStream_t st) {
    constexpr uint32_t V = 16 / sizeof(T);
    if (ncols == 0) return;
    const LaunchShape g = spmm_reduce_bwd_shape(h, V, ldg % V == 0 && ldd % V == 0 && (uintptr_t)G % 16 == 0 && (uintptr_t)dX % 16 == 0);
    if (g.vec > 1) launch_spmm_reduce_bwd_v<T, (int)V>(rowptr_t, rows_t, perm, ncols, values, G, ldg, arg, h, dX, ldd, g, st);
    else launch_spmm_reduce_bwd_v<T, 1>(rowptr_t, rows_t, perm, ncols, values, G, ldg, arg, h, dX, ldd, g, st);
}

}  // namespace pygim
