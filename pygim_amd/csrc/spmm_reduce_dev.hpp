// spmm_reduce_dev.hpp -- a row-wise reduction other than the sum on a caller's CSR:
//   out[r, f] = REDUCE over the stored entries e of row r of w[e] * X[colind[e], f],   w[e] = values[e], or 1 without values
// REDUCE = mean (the sum of spmm_values_dev.hpp, in its order, divided by the row's number of stored entries: duplicates count),
// max or min (all six element types; optionally with arg[r, f] = the index, in stored order, of the entry that won), and the
// gradient of max / min with respect to X (k_spmm_reduce_bwd).
//
// Shape: that of k_spmm_values.  A wave owns SV_EPW consecutive entries whatever rows they fall in and walks them in batches of 64;
// lanes lie across the features, 16 bytes each when h, the strides and the pointers allow it; rows narrower than a wave are taken by
// 64 / L lane groups side by side on different entries of one row, joined in a fixed xor tree when the row ends; wider rows go over
// blockIdx.y.  A row inside the wave's run is stored directly; the at most two rows a run shares with its neighbours leave their
// partial result (slot 0: the row that began earlier, slot 1: the row that goes on) in the workspace -- for max / min the value and
// the entry index that holds it -- and k_rd_fixup folds the partials of a row in the order of the runs.  Empty rows: k_rd_empty
// (0, and -1 in arg).  No atomics, no two kernels write the same row, every order is fixed: the same bits on every launch.
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

#include "spmm_values_dev.hpp"

namespace pygim {

constexpr int RD_MEAN = 1, RD_MAX = 2, RD_MIN = 3;   // PYGIM_REDUCE_*
constexpr int32_t RD_NONE = 0x7FFFFFFF;              // "no entry yet": above every entry index (nnz <= 2^31 - 1)

template <int VEC> struct RdIdx { typedef int32_t __attribute__((ext_vector_type(VEC), aligned(4))) type; };
template <> struct RdIdx<1> { typedef int32_t type; };

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

// w * x; integers wrap like the type's own arithmetic (no signed overflow, no promotion past the type)
template <typename T> __device__ inline T rd_mul(T w, T x) {
    if constexpr (std::is_floating_point<T>::value) return w * x;
    else {
        using W = typename std::conditional<sizeof(T) <= 4, uint32_t, uint64_t>::type;
        return (T)((W)w * (W)x);
    }
}

template <typename T> __device__ inline T rd_shfl_xor(T v, int mask) {
    if constexpr (sizeof(T) == 8) {
        uint64_t b;
        __builtin_memcpy(&b, &v, 8);
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)b, mask, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(b >> 32), mask, 64);
        b = (uint64_t)lo | ((uint64_t)hi << 32);
        __builtin_memcpy(&v, &b, 8);
        return v;
    } else if constexpr (std::is_floating_point<T>::value) {
        return __shfl_xor(v, mask, 64);
    } else {
        return (T)__shfl_xor((int)v, mask, 64);
    }
}

template <bool WHOLE, typename T> __device__ inline T rd_take(T v, uint32_t src) {
    if constexpr (sizeof(T) == 8) {
        uint64_t b;
        __builtin_memcpy(&b, &v, 8);
        b = (uint64_t)sv_take32<WHOLE>((uint32_t)b, src) | ((uint64_t)sv_take32<WHOLE>((uint32_t)(b >> 32), src) << 32);
        __builtin_memcpy(&v, &b, 8);
        return v;
    } else if constexpr (std::is_floating_point<T>::value) {
        return __uint_as_float(sv_take32<WHOLE>(__float_as_uint(v), src));
    } else {
        return (T)(int32_t)sv_take32<WHOLE>((uint32_t)(int32_t)v, src);
    }
}

template <typename T, int VEC> __device__ inline T rd_get(const typename SdVec<T, VEC>::type &v, int i) {
    if constexpr (VEC == 1) return v;
    else return v[i];
}

template <typename T, int VEC> __device__ inline void rd_store(T *dst, const T *a) {
    typename SdVec<T, VEC>::type v;
    if constexpr (VEC == 1) v = a[0];
    else {
#pragma unroll
        for (int i = 0; i < VEC; i++) v[i] = a[i];
    }
    *(typename SdVec<T, VEC>::type *)dst = v;
}

// entry indices of VEC features; `final`: RD_NONE (no entry won) becomes -1
template <int VEC> __device__ inline void rd_store_idx(int32_t *dst, const int32_t *a, bool final) {
    typename RdIdx<VEC>::type v;
    if constexpr (VEC == 1) v = (final && a[0] == RD_NONE) ? -1 : a[0];
    else {
#pragma unroll
        for (int i = 0; i < VEC; i++) v[i] = (final && a[i] == RD_NONE) ? -1 : a[i];
    }
    *(typename RdIdx<VEC>::type *)dst = v;
}

// WHOLE: the wave is one lane group (L = 64) that holds NV pieces of VEC features per lane; else NV = 1 and L < 64 is a launch argument.
// values, arg: may be null (unit weights; no index output).  ws_idx: the index half of the workspace (max / min).
template <typename T, int VEC, int NV, bool WHOLE, int OP>
__global__ __launch_bounds__(256) void k_spmm_reduce(const uint32_t *__restrict__ rowptr, const uint32_t *__restrict__ colind, uint32_t nrows, uint32_t nnz,
                                                     const T *__restrict__ values, const T *__restrict__ X, uint64_t ldx, uint32_t h, uint32_t L,
                                                     T *__restrict__ out, uint64_t ldo, int32_t *__restrict__ arg, T *__restrict__ ws,
                                                     int32_t *__restrict__ ws_idx) {
    using V = typename SdVec<T, VEC>::type;
    constexpr bool MEAN = OP == RD_MEAN;
    constexpr int U = NV == 1 ? SV_U : SV_U / 2;
    if constexpr (WHOLE) L = 64;
    const uint32_t R = 64 / L;
    const uint32_t lane = threadIdx.x & 63, grp = lane / L, li = lane % L;
    const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint64_t e_begin = wave * SV_EPW;
    if (e_begin >= nnz) return;
    const uint32_t e_end = (uint32_t)(e_begin + SV_EPW < nnz ? e_begin + SV_EPW : nnz);
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
    T acc[NV][VEC];         // the running sum (mean) or the best product so far (max / min) ...
    int32_t aidx[NV][VEC];  // ... and the entry that holds it
    const auto reset = [&]() {
#pragma unroll
        for (int v = 0; v < NV; v++)
#pragma unroll
            for (int i = 0; i < VEC; i++) {
                if constexpr (MEAN) acc[v][i] = T(0);
                else acc[v][i] = rd_worst<OP, T>();
                aidx[v][i] = RD_NONE;
            }
    };
    // join the lane groups, then store: into the workspace slot (raw partial), or the finished row `row` into out / arg
    const auto flush = [&](bool to_slot, uint32_t slot, uint32_t row) {
        T *dst = to_slot ? ws + (wave * 2 + slot) * (uint64_t)h : out + (uint64_t)row * ldo;
        int32_t *dst_i = to_slot ? ws_idx + (wave * 2 + slot) * (uint64_t)h : (arg ? arg + (uint64_t)row * h : nullptr);
        T cnt = T(1);
        if constexpr (MEAN)
            if (!to_slot) cnt = T(rowptr[row + 1] - rowptr[row]);
#pragma unroll
        for (int v = 0; v < NV; v++) {
            if constexpr (!WHOLE) {
                for (uint32_t s = L; s < 64; s <<= 1) {
#pragma unroll
                    for (int i = 0; i < VEC; i++) {
                        const T ov = rd_shfl_xor(acc[v][i], (int)s);
                        if constexpr (MEAN) acc[v][i] = acc[v][i] + ov;
                        else {
                            const int32_t oi = __shfl_xor(aidx[v][i], (int)s, 64);
                            if (rd_better<OP, T>(ov, oi, acc[v][i], aidx[v][i])) {
                                acc[v][i] = ov;
                                aidx[v][i] = oi;
                            }
                        }
                    }
                }
            }
            if (grp == 0 && fok[v]) {
                if constexpr (MEAN) {
                    if (!to_slot) {
#pragma unroll
                        for (int i = 0; i < VEC; i++) acc[v][i] = acc[v][i] / cnt;
                    }
                    rd_store<T, VEC>(dst + f[v], acc[v]);
                } else {
                    rd_store<T, VEC>(dst + f[v], acc[v]);
                    if (dst_i) rd_store_idx<VEC>(dst_i + f[v], aidx[v], !to_slot);
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
        const T my_val = (valid && values) ? values[my_e] : T(1);
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
                T w[U];
                bool ok[U];
                int32_t ei[U];
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const uint32_t kk = k0 + (uint32_t)u * R + grp;
                    ok[u] = kk <= last;
                    ei[u] = (int32_t)(base + kk);
                    const uint32_t col = sv_take32<WHOLE>(my_col, ok[u] ? kk : pos);
                    w[u] = rd_take<WHOLE, T>(my_val, ok[u] ? kk : pos);
                    const T *xr = X + (uint64_t)col * ldx;
#pragma unroll
                    for (int v = 0; v < NV; v++) {
                        x[u][v] = sv_zero<T, VEC>();
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
                                const T p = rd_mul<T>(w[u], rd_get<T, VEC>(x[u][v], i));
                                if constexpr (MEAN) acc[v][i] += p;
                                else if (rd_better<OP, T>(p, ei[u], acc[v][i], aidx[v][i])) {
                                    acc[v][i] = p;
                                    aidx[v][i] = ei[u];
                                }
                            }
                        }
                }
            }
            if (closes) {
                flush(head_open, 0u, sv_take32<true>(my_row, last));
                reset();
                head_open = false;
            }
            pending = !closes;
            pos = last + 1;
        }
        row_cur = sv_take32<true>(my_row, n - 1);
    }
    if (pending) flush(true, head_open ? 0u : 1u, 0u);   // the run's last row goes on in the next run
}

// one wave per run: the row that goes on after run w = slot 1 of w joined with slot 0 of every later run the row reaches, in order
template <typename T, int OP>
__global__ __launch_bounds__(256) void k_rd_fixup(const uint32_t *__restrict__ rowptr, uint32_t nrows, uint32_t nnz, uint32_t h, const T *__restrict__ ws,
                                                  const int32_t *__restrict__ ws_idx, T *__restrict__ out, uint64_t ldo, int32_t *__restrict__ arg) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t w = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint64_t e_begin = w * SV_EPW;
    if (e_begin + SV_EPW >= nnz) return;   // the last run has no row that goes on
    const uint32_t e_end = (uint32_t)(e_begin + SV_EPW);
    const uint32_t row = sd_row_of(rowptr, 0, nrows, e_end - 1);
    const uint32_t rb = rowptr[row], re = rowptr[row + 1];
    if (re <= e_end || rb < (uint32_t)e_begin) return;
    const uint64_t w1 = (re - 1) / SV_EPW;
    for (uint32_t f = lane; f < h; f += 64) {
        T s = ws[(w * 2 + 1) * (uint64_t)h + f];
        if constexpr (OP == RD_MEAN) {
            for (uint64_t j = w + 1; j <= w1; j++) s += ws[j * 2 * (uint64_t)h + f];
            out[(uint64_t)row * ldo + f] = s / T(re - rb);
        } else {
            int32_t si = ws_idx[(w * 2 + 1) * (uint64_t)h + f];
            for (uint64_t j = w + 1; j <= w1; j++) {
                const T ov = ws[j * 2 * (uint64_t)h + f];
                const int32_t oi = ws_idx[j * 2 * (uint64_t)h + f];
                if (rd_better<OP, T>(ov, oi, s, si)) {
                    s = ov;
                    si = oi;
                }
            }
            out[(uint64_t)row * ldo + f] = s;
            if (arg) arg[(uint64_t)row * h + f] = si == RD_NONE ? -1 : si;
        }
    }
}

// rows without entries: 0, and -1 in arg
template <typename T>
__global__ __launch_bounds__(256) void k_rd_empty(const uint32_t *__restrict__ rowptr, uint32_t nrows, uint32_t h, T *__restrict__ out, uint64_t ldo,
                                                  int32_t *__restrict__ arg) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t row = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= nrows || rowptr[row] != rowptr[row + 1]) return;
    for (uint32_t f = lane; f < h; f += 64) {
        out[row * ldo + f] = T(0);
        if (arg) arg[row * h + f] = -1;
    }
}

// the value half of the workspace: two slots of h elements per run, rounded to 16 bytes; max / min add two slots of h entry indices
inline uint64_t spmm_reduce_value_bytes(uint64_t nnz, uint64_t h, size_t elem) { return ((nnz + SV_EPW - 1) / SV_EPW * 2 * h * elem + 15) / 16 * 16; }
inline uint64_t spmm_reduce_workspace_bytes(int op, uint64_t nnz, uint64_t h, size_t elem) {
    return spmm_reduce_value_bytes(nnz, h, elem) + (op == RD_MEAN ? 0 : (nnz + SV_EPW - 1) / SV_EPW * 2 * h * sizeof(int32_t));
}

template <typename T, int VEC, int OP>
inline void launch_spmm_reduce_v(const uint32_t *rowptr, const uint32_t *colind, uint32_t nrows, uint32_t nnz, const T *values, const T *X, uint64_t ldx,
                                 uint32_t h, T *out, uint64_t ldo, int32_t *arg, T *ws, int32_t *ws_idx, hipStream_t st) {
    const uint64_t waves = ((uint64_t)nnz + SV_EPW - 1) / SV_EPW;
    const unsigned blocks = (unsigned)((waves + 3) / 4);
    const uint32_t pieces = (h + VEC - 1) / VEC;
    if (pieces <= 32) {
        uint32_t L = 1;
        while (L < pieces) L <<= 1;
        hipLaunchKernelGGL((k_spmm_reduce<T, VEC, 1, false, OP>), dim3(blocks), dim3(256), 0, st, rowptr, colind, nrows, nnz, values, X, ldx, h, L, out, ldo,
                           arg, ws, ws_idx);
    } else if (pieces <= 64) {
        hipLaunchKernelGGL((k_spmm_reduce<T, VEC, 1, true, OP>), dim3(blocks), dim3(256), 0, st, rowptr, colind, nrows, nnz, values, X, ldx, h, 64u, out, ldo,
                           arg, ws, ws_idx);
    } else {   // two pieces per lane, the rest of a wider row over blockIdx.y
        hipLaunchKernelGGL((k_spmm_reduce<T, VEC, 2, true, OP>), dim3(blocks, (pieces + 127) / 128), dim3(256), 0, st, rowptr, colind, nrows, nnz, values, X,
                           ldx, h, 64u, out, ldo, arg, ws, ws_idx);
    }
}

// 16-byte pieces when every row of X and out starts 16-byte aligned and h fills whole pieces (arg and the index slots are stored
// with 4-byte alignment, whatever their width)
template <typename T, int OP>
inline void launch_spmm_reduce(const uint32_t *rowptr, const uint32_t *colind, uint32_t nrows, uint32_t nnz, const T *values, const T *X, uint64_t ldx,
                               uint32_t h, T *out, uint64_t ldo, int32_t *arg, void *workspace, hipStream_t st) {
    constexpr uint32_t V = 16 / sizeof(T);
    if (nrows > 0) hipLaunchKernelGGL((k_rd_empty<T>), dim3((nrows + 3) / 4), dim3(256), 0, st, rowptr, nrows, h, out, ldo, arg);
    if (nnz == 0) return;
    T *ws = (T *)workspace;
    int32_t *ws_idx = (int32_t *)((char *)workspace + spmm_reduce_value_bytes(nnz, h, sizeof(T)));
    const bool vec = h % V == 0 && ldx % V == 0 && ldo % V == 0 && (uintptr_t)X % 16 == 0 && (uintptr_t)out % 16 == 0 && (uintptr_t)ws % 16 == 0;
    if (vec) launch_spmm_reduce_v<T, (int)V, OP>(rowptr, colind, nrows, nnz, values, X, ldx, h, out, ldo, arg, ws, ws_idx, st);
    else launch_spmm_reduce_v<T, 1, OP>(rowptr, colind, nrows, nnz, values, X, ldx, h, out, ldo, arg, ws, ws_idx, st);
    const uint64_t waves = ((uint64_t)nnz + SV_EPW - 1) / SV_EPW;
    if (waves > 1) hipLaunchKernelGGL((k_rd_fixup<T, OP>), dim3((unsigned)((waves + 2) / 4)), dim3(256), 0, st, rowptr, nrows, nnz, h, ws, ws_idx, out, ldo, arg);
}

// op: RD_MEAN (floating types only: the caller checks), RD_MAX or RD_MIN
template <typename T>
inline void launch_spmm_reduce_op(int op, const uint32_t *rowptr, const uint32_t *colind, uint32_t nrows, uint32_t nnz, const void *values, const void *X,
                                  uint64_t ldx, uint32_t h, void *out, uint64_t ldo, int32_t *arg, void *workspace, hipStream_t st) {
    if constexpr (std::is_floating_point<T>::value) {
        if (op == RD_MEAN) {
            launch_spmm_reduce<T, RD_MEAN>(rowptr, colind, nrows, nnz, (const T *)values, (const T *)X, ldx, h, (T *)out, ldo, nullptr, workspace, st);
            return;
        }
    }
    if (op == RD_MAX) launch_spmm_reduce<T, RD_MAX>(rowptr, colind, nrows, nnz, (const T *)values, (const T *)X, ldx, h, (T *)out, ldo, arg, workspace, st);
    else launch_spmm_reduce<T, RD_MIN>(rowptr, colind, nrows, nnz, (const T *)values, (const T *)X, ldx, h, (T *)out, ldo, arg, workspace, st);
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
                        acc[v][i] += ai == e[u] ? w[u] * rd_get<T, VEC>(g[u][v], i) : T(0);
                    }
                }
        }
    }
#pragma unroll
    for (int v = 0; v < NV; v++)
        if (fok[v]) rd_store<T, VEC>(dX + c * ldd + f[v], acc[v]);
}

template <typename T, int VEC>
inline void launch_spmm_reduce_bwd_v(const uint32_t *rowptr_t, const uint32_t *rows_t, const int32_t *perm, uint32_t ncols, const T *values, const T *G,
                                     uint64_t ldg, const int32_t *arg, uint32_t h, T *dX, uint64_t ldd, hipStream_t st) {
    const uint32_t pieces = (h + VEC - 1) / VEC;
    if (pieces <= 64) {
        uint32_t L = 1;
        while (L < pieces) L <<= 1;
        hipLaunchKernelGGL((k_spmm_reduce_bwd<T, VEC, 1>), dim3((unsigned)(((uint64_t)ncols * L + 255) / 256)), dim3(256), 0, st, rowptr_t, rows_t, perm,
                           ncols, values, G, ldg, arg, h, L, dX, ldd);
    } else {
        hipLaunchKernelGGL((k_spmm_reduce_bwd<T, VEC, 2>), dim3((unsigned)(((uint64_t)ncols * 64 + 255) / 256), (pieces + 127) / 128), dim3(256), 0, st,
                           rowptr_t, rows_t, perm, ncols, values, G, ldg, arg, h, 64u, dX, ldd);
    }
}

template <typename T>
inline void launch_spmm_reduce_bwd(const uint32_t *rowptr_t, const uint32_t *rows_t, const int32_t *perm, uint32_t ncols, const T *values, const T *G,
                                   uint64_t ldg, const int32_t *arg, uint32_t h, T *dX, uint64_t ldd, hipStream_t st) {
    constexpr uint32_t V = 16 / sizeof(T);
    if (ncols == 0) return;
    const bool vec = h % V == 0 && ldg % V == 0 && ldd % V == 0 && (uintptr_t)G % 16 == 0 && (uintptr_t)dX % 16 == 0;
    if (vec) launch_spmm_reduce_bwd_v<T, (int)V>(rowptr_t, rows_t, perm, ncols, values, G, ldg, arg, h, dX, ldd, st);
    else launch_spmm_reduce_bwd_v<T, 1>(rowptr_t, rows_t, perm, ncols, values, G, ldg, arg, h, dX, ldd, st);
}

}  // namespace pygim
