// spmm_edge_dev.hpp -- aggregation of messages that carry a feature-wide edge feature (GINEConv, GENConv with edge_dim), unit weights:
//   msg[e, f] = act(X[colind[e], f] + E[e, f]) + eps        act: identity or relu; E [nnz, h] in stored CSR order, row stride lde
//   out[r, f] = FOLD over the stored entries e of row r, in stored order, of msg[e, f]        FOLD: sum, mean, max, min
//   out[r, f] = sum_e softmax_e(t[f] * msg[e, f]) * msg[e, f]                                 (the softmax fold, with lse)
// and the gradient of all five with respect to E in one entry-order kernel; the message is additive in x and e, so d msg / dX = d msg / dE
// and dX is the unit-weight sum of the dE rows over the CSR of A^T with perm as column ids: pygim_spmm_values, no kernel here.
//
// Forward.  k_edge_gather is k_row_gather (row_gather_dev.hpp) and k_edge_softmax_gather is k_softmax_gather (spmm_softmax_dev.hpp) with one
// more operand: a wave owns RG_EPW CONSECUTIVE entries, so its rows of E are one contiguous block, and the E piece of entry base + kk is
// loaded beside the gathered X piece in the same unrolled issue block, at E + (base + kk) * lde + f[v], with the same VEC.  The fold
// order is that of the kernel each one copies -- the scan, the xor tree of the lane groups, the runs in order -- and the folds
// (FoldSum<false / true>, FoldBest<OP>, sm_fold / sm_join), the slots, the fix-up and the empty-row kernels are the existing ones, which
// see partials only.  With E = -0.0, no activation and eps = 0 the message is x itself (x + -0.0 == x for every x, signed zeros
// included; eps = 0 is not added, because -0.0 + 0.0 is +0.0) and the call returns the bits of spmm_values / spmm_reduce / spmm_softmax.
// The walk -- batch loop, row search, ballot of row ends, cut into stretches, slot rule -- is copied text as in the seven siblings
// row_gather_dev.hpp lists, and for the reason given there: a change to the walk there has to be made in the three kernels here as well.
//
// Backward.  k_edge_message_grad walks the same runs in the same lane layout.  All entries of a stretch belong to one row r, so G[r] (and
// arg[r], or out[r] and lse[r]) are loaded once per stretch; per entry the lane reads E[e] (a stream) and X[colind[e]] (a gather) and
// writes dE[e, f] = act'(X + E) * c[e, f]:
//   sum: c = G[r, f]     mean: c = G[r, f] / deg(r)     max / min: c = G[r, f] if arg[r, f] == e, else 0
//   softmax: c = G[r, f] * p * (1 + t[f] * (msg - out[r, f])),  p = exp(t[f] * msg - lse[r, f])
// act' is 1 for the identity and (x + e > 0) for relu.  When t needs a gradient the wave also leaves dT_part[run, f] = the sum over
// its entries of G * p * msg * (msg - out): per lane group in entry order, then the fixed xor tree; the caller sums the runs.  Every dE
// row has one writer and there is no slot and no fix-up: nothing is atomic, the same bits on every launch.
// Known cost: sum / mean without relu is a pure broadcast of G[r] over the row's entries and needs neither X nor colind, yet it runs the
// whole walk (the colind load and the row search included; the X and E pieces are declared and zero-filled but not loaded); under relu
// the gathered X row serves only the sign of x + e.  A kernel of its own for the broadcast was not written.
//
// S is the storage type of X, E, G, out and dE, T the type of everything else (eps, t, lse, dT_part, the partials, the slots): S = T =
// float / double, or S = _Float16 / __bf16 with T = float -- an element is widened as it is folded (exact) and a value is rounded once,
// where it is stored.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "row_gather_dev.hpp"
#include "spmm_reduce_dev.hpp"
#include "spmm_softmax_dev.hpp"

namespace pygim {

constexpr int RD_SUM = 4, RD_SOFTMAX = 5;   // PYGIM_REDUCE_SUM, PYGIM_REDUCE_SOFTMAX
constexpr int EM_ACT_NONE = 0, EM_ACT_RELU = 1;   // PYGIM_ACT_*

// what turns the pair (x, e) into a message; relu and eps are wave-uniform kernel arguments
template <typename T> struct EdgeMsg {
    T eps;
    int relu;
    // NaN stays NaN under relu (NaN < 0 is false), -inf becomes 0; eps = 0 is not added (it would turn a message of -0.0 into +0.0)
    __device__ T operator()(T x, T e) const {
        T m = x + e;
        if (relu) m = m < T(0) ? T(0) : m;
        if (eps != T(0)) m = m + eps;
        return m;
    }
    // act'(x + e)
    __device__ bool live(T x, T e) const { return !relu || x + e > T(0); }
};

// k_row_gather without weights, with the E stream.  WHOLE: the wave is one lane group (L = 64) that holds NV pieces of VEC features per
// lane; else NV = 1 and L < 64 is a launch argument.  arg: may be null.  ws_idx: the index half of the workspace.
template <typename T, typename S, int VEC, int NV, bool WHOLE, typename Fold>
__global__ __launch_bounds__(256) void k_edge_gather(const uint32_t *__restrict__ rowptr, const uint32_t *__restrict__ colind, uint32_t nrows, uint32_t nnz,
                                                     const S *__restrict__ X, uint64_t ldx, const S *__restrict__ E, uint64_t lde, EdgeMsg<T> msg, uint32_t h,
                                                     uint32_t L, S *__restrict__ out, uint64_t ldo, int32_t *__restrict__ arg, T *__restrict__ ws,
                                                     int32_t *__restrict__ ws_idx) {
    using V = typename SdVec<S, VEC>::type;
    constexpr int U = NV == 1 ? RG_U : RG_U / 2;
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
    T acc[NV][VEC];         // the running fold ...
    int32_t aidx[NV][VEC];  // ... and, for INDEXED folds, the entry that holds it
    const uint64_t slots = wave * 2 * (uint64_t)h;   // the run's two slots, in elements
    const auto reset = [&]() {
#pragma unroll
        for (int v = 0; v < NV; v++)
#pragma unroll
            for (int i = 0; i < VEC; i++) {
                acc[v][i] = Fold::template neutral<T>();
                aidx[v][i] = RD_NONE;
            }
    };
    // join the lane groups, then store: into the workspace slot (raw partial), or the finished row `row` into out / arg
    const auto flush = [&](bool to_slot, uint32_t slot, uint32_t row) {
        T *dst = nullptr;
        S *dst_out = nullptr;
        if constexpr (std::is_same<S, T>::value) dst = to_slot ? ws + slots + (slot ? h : 0u) : out + (uint64_t)row * ldo;
        else if (to_slot) dst = ws + slots + (slot ? h : 0u);
        else dst_out = out + (uint64_t)row * ldo;
        int32_t *dst_i = nullptr;
        if constexpr (Fold::INDEXED) dst_i = to_slot ? ws_idx + slots + (slot ? h : 0u) : (arg ? arg + (uint64_t)row * h : nullptr);
        T cnt = T(1);
        if constexpr (Fold::MEAN)
            if (!to_slot) cnt = T(rowptr[row + 1] - rowptr[row]);
#pragma unroll
        for (int v = 0; v < NV; v++) {
            if constexpr (!WHOLE) {
                for (uint32_t s = L; s < 64; s <<= 1) {
#pragma unroll
                    for (int i = 0; i < VEC; i++) {
                        int32_t oi = RD_NONE;
                        if constexpr (Fold::INDEXED) oi = __shfl_xor(aidx[v][i], (int)s, 64);
                        Fold::join(acc[v][i], aidx[v][i], rg_shfl_xor(acc[v][i], (int)s), oi);
                    }
                }
            }
            if (grp == 0 && fok[v]) {
                if constexpr (Fold::MEAN) {
                    if (!to_slot) {
#pragma unroll
                        for (int i = 0; i < VEC; i++) acc[v][i] = acc[v][i] / cnt;
                    }
                }
                if (std::is_same<S, T>::value || to_slot) rg_store<T, T, VEC>(dst + f[v], acc[v]);
                else rg_store<S, T, VEC>(dst_out + f[v], acc[v]);
                if constexpr (Fold::INDEXED)
                    if (dst_i) rg_store_idx<VEC>(dst_i + f[v], aidx[v], !to_slot);
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
                V x[U][NV], ev[U][NV];
                bool ok[U];
                int32_t ei[U];
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const uint32_t kk = k0 + (uint32_t)u * R + grp;
                    ok[u] = kk <= last;
                    ei[u] = (int32_t)(base + kk);
                    const uint32_t col = rg_take32<WHOLE>(my_col, ok[u] ? kk : pos);
                    const S *xr = X + (uint64_t)col * ldx;
                    const S *er = E + (uint64_t)(base + kk) * lde;   // read only when ok[u]: base + kk < e_end
#pragma unroll
                    for (int v = 0; v < NV; v++) {
                        x[u][v] = V(0);
                        ev[u][v] = V(0);
                        if (ok[u] && fok[v]) {
                            x[u][v] = *(const V *)(xr + f[v]);
                            ev[u][v] = *(const V *)(er + f[v]);
                        }
                    }
                }
#pragma unroll
                for (int u = 0; u < U; u++) {
#pragma unroll
                    for (int v = 0; v < NV; v++)
                        if (ok[u] && fok[v]) {
#pragma unroll
                            for (int i = 0; i < VEC; i++)
                                Fold::join(acc[v][i], aidx[v][i], msg(T(rg_get<S, VEC>(x[u][v], i)), T(rg_get<S, VEC>(ev[u][v], i))), ei[u]);
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

// 16-byte pieces need every row of X, E and out 16-byte aligned and h to fill whole pieces
inline LaunchShape edge_gather_shape(uint32_t h, uint32_t V, bool aligned) { return row_gather_shape(h, h, V, aligned); }
inline LaunchShape edge_grad_shape(uint32_t h, uint32_t V, bool aligned) { return row_gather_shape(h, h, V, aligned); }

template <typename T, typename S, int VEC, typename Fold>
inline void launch_edge_gather_v(const uint32_t *rowptr, const uint32_t *colind, uint32_t nrows, uint32_t nnz, const S *X, uint64_t ldx, const S *E, uint64_t lde,
                                 const EdgeMsg<T> &msg, uint32_t h, S *out, uint64_t ldo, int32_t *arg, T *ws, int32_t *ws_idx, const LaunchShape &g,
                                 hipStream_t st) {
    rg_dispatch(nnz, g, [&](auto nv, auto whole, dim3 grid, uint32_t L) {
        hipLaunchKernelGGL((k_edge_gather<T, S, VEC, decltype(nv)::value, decltype(whole)::value, Fold>), grid, dim3(256), 0, st, rowptr, colind, nrows, nnz, X,
                           ldx, E, lde, msg, h, L, out, ldo, arg, ws, ws_idx);
    });
}

// the launcher of launch_row_gather with the E stream: the same empty-row kernel, workspace layout and fix-up
template <typename T, typename Fold, typename S = T>
inline void launch_edge_gather(const uint32_t *rowptr, const uint32_t *colind, uint32_t nrows, uint32_t nnz, const S *X, uint64_t ldx, const S *E, uint64_t lde,
                               const EdgeMsg<T> &msg, uint32_t h, S *out, uint64_t ldo, int32_t *arg, void *workspace, hipStream_t st) {
    constexpr uint32_t V = 16 / sizeof(S);
    if (nrows > 0) hipLaunchKernelGGL((k_row_gather_empty<S>), dim3((nrows + 3) / 4), dim3(256), 0, st, rowptr, nrows, h, out, ldo, arg);
    if (nnz == 0) return;
    T *ws = (T *)workspace;
    int32_t *ws_idx = Fold::INDEXED ? (int32_t *)((char *)workspace + row_gather_index_offset(nnz, h, sizeof(T))) : nullptr;
    const bool aligned = ldx % V == 0 && lde % V == 0 && ldo % V == 0 && (uintptr_t)X % 16 == 0 && (uintptr_t)E % 16 == 0 && (uintptr_t)out % 16 == 0 &&
                         (uintptr_t)ws % 16 == 0;
    const LaunchShape g = edge_gather_shape(h, V, aligned);
    if (g.vec > 1) launch_edge_gather_v<T, S, (int)V, Fold>(rowptr, colind, nrows, nnz, X, ldx, E, lde, msg, h, out, ldo, arg, ws, ws_idx, g, st);
    else launch_edge_gather_v<T, S, 1, Fold>(rowptr, colind, nrows, nnz, X, ldx, E, lde, msg, h, out, ldo, arg, ws, ws_idx, g, st);
    const uint64_t runs = row_gather_runs(nnz);
    if (runs > 1)
        hipLaunchKernelGGL((k_row_gather_fixup<T, S, Fold>), dim3((unsigned)((runs + 2) / 4)), dim3(256), 0, st, rowptr, nrows, nnz, h, ws, ws_idx, out, ldo, arg);
}

// the bytes launch_edge_gather needs: those of the fold without E
inline uint64_t spmm_edge_workspace_bytes(int op, uint64_t nnz, uint64_t h, size_t elem) {
    return row_gather_index_offset(nnz, h, elem) + ((op == RD_MAX || op == RD_MIN) ? row_gather_slot_bytes(nnz, h, sizeof(int32_t)) : 0);
}

// op: RD_SUM, RD_MEAN, or (S = T: the caller checks) RD_MAX / RD_MIN
template <typename T, typename S>
inline void launch_spmm_edge(int op, const uint32_t *rowptr, const uint32_t *colind, uint32_t nrows, uint32_t nnz, const S *X, uint64_t ldx, const S *E,
                             uint64_t lde, const EdgeMsg<T> &msg, uint32_t h, S *out, uint64_t ldo, int32_t *arg, void *workspace, hipStream_t st) {
    if (op == RD_SUM) return launch_edge_gather<T, FoldSum<false>, S>(rowptr, colind, nrows, nnz, X, ldx, E, lde, msg, h, out, ldo, nullptr, workspace, st);
    if (op == RD_MEAN) return launch_edge_gather<T, FoldSum<true>, S>(rowptr, colind, nrows, nnz, X, ldx, E, lde, msg, h, out, ldo, nullptr, workspace, st);
    if constexpr (std::is_same<S, T>::value) {
        if (op == RD_MAX) launch_edge_gather<T, FoldBest<RD_MAX>, S>(rowptr, colind, nrows, nnz, X, ldx, E, lde, msg, h, out, ldo, arg, workspace, st);
        else launch_edge_gather<T, FoldBest<RD_MIN>, S>(rowptr, colind, nrows, nnz, X, ldx, E, lde, msg, h, out, ldo, arg, workspace, st);
    }
}

// ---- the softmax fold: k_softmax_gather with the E stream and the message transform ----
template <typename T, typename S, int VEC, int NV, bool WHOLE>
__global__ __launch_bounds__(256) void k_edge_softmax_gather(const uint32_t *__restrict__ rowptr, const uint32_t *__restrict__ colind, uint32_t nrows,
                                                             uint32_t nnz, const S *__restrict__ X, uint64_t ldx, const S *__restrict__ E, uint64_t lde,
                                                             EdgeMsg<T> msg, const T *__restrict__ t, uint32_t h, uint32_t L, S *__restrict__ out, uint64_t ldo,
                                                             T *__restrict__ lse, SoftmaxWs<T> ws) {
    using V = typename SdVec<S, VEC>::type;
    constexpr int U = NV == 1 ? RG_U : RG_U / 2;
    if constexpr (WHOLE) L = 64;
    const uint32_t R = 64 / L;
    const uint32_t lane = threadIdx.x & 63, grp = lane / L, li = lane % L;
    const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint64_t e_begin = wave * RG_EPW;
    if (e_begin >= nnz) return;
    const uint32_t e_end = (uint32_t)(e_begin + RG_EPW < nnz ? e_begin + RG_EPW : nnz);
    uint32_t f[NV];
    bool fok[NV];
    T tv[NV][VEC];   // the temperatures of the lane's features
#pragma unroll
    for (int v = 0; v < NV; v++) {
        f[v] = ((blockIdx.y * NV + v) * L + li) * VEC;
        fok[v] = f[v] < h;
#pragma unroll
        for (int i = 0; i < VEC; i++) tv[v][i] = fok[v] ? t[f[v] + i] : T(0);
    }
    uint32_t row_cur = sd_row_of(rowptr, 0, nrows, (uint32_t)e_begin);
    const uint32_t row_hi = sd_row_of(rowptr, row_cur, nrows, e_end - 1) + 1;
    bool head_open = rowptr[row_cur] < (uint32_t)e_begin;   // the first row of the run began in an earlier run
    bool pending = false;
    T m[NV][VEC], den[NV][VEC], num[NV][VEC];   // the online-softmax triple per feature
    const uint64_t slots = wave * 2 * (uint64_t)h;   // the run's two slots, in elements of every sub-array
    const auto reset = [&]() {
#pragma unroll
        for (int v = 0; v < NV; v++)
#pragma unroll
            for (int i = 0; i < VEC; i++) {
                m[v][i] = es_neg_inf<T>();
                den[v][i] = num[v][i] = T(0);
            }
    };
    // join the lane groups, then store: the raw triple into the workspace slots, or the finished row `row` into out / lse
    const auto flush = [&](bool to_slot, uint32_t slot, uint32_t row) {
        const uint64_t at = slots + (slot ? h : 0u);
#pragma unroll
        for (int v = 0; v < NV; v++) {
            if constexpr (!WHOLE) {
                for (uint32_t s = L; s < 64; s <<= 1) {
#pragma unroll
                    for (int i = 0; i < VEC; i++)
                        sm_join(m[v][i], den[v][i], num[v][i], rg_shfl_xor(m[v][i], (int)s), rg_shfl_xor(den[v][i], (int)s), rg_shfl_xor(num[v][i], (int)s));
                }
            }
            if (grp == 0 && fok[v]) {
                if (to_slot) {
                    rg_store<T, T, VEC>(ws.m + at + f[v], m[v]);
                    rg_store<T, T, VEC>(ws.den + at + f[v], den[v]);
                    rg_store<T, T, VEC>(ws.num + at + f[v], num[v]);
                } else {
                    sm_store_row<T, S, VEC>(out + (uint64_t)row * ldo, lse ? lse + (uint64_t)row * h : nullptr, f[v], m[v], den[v], num[v]);
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
            const uint64_t mk = endmask >> pos;
            const bool closes = mk != 0;
            const uint32_t last = closes ? pos + (uint32_t)__builtin_ctzll(mk) : n - 1;
            for (uint32_t k0 = pos; k0 <= last; k0 += R * U) {
                V x[U][NV], ev[U][NV];
                bool ok[U];
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const uint32_t kk = k0 + (uint32_t)u * R + grp;
                    ok[u] = kk <= last;
                    const uint32_t col = rg_take32<WHOLE>(my_col, ok[u] ? kk : pos);
                    const S *xr = X + (uint64_t)col * ldx;
                    const S *er = E + (uint64_t)(base + kk) * lde;   // read only when ok[u]: base + kk < e_end
#pragma unroll
                    for (int v = 0; v < NV; v++) {
                        x[u][v] = V(0);
                        ev[u][v] = V(0);
                        if (ok[u] && fok[v]) {
                            x[u][v] = *(const V *)(xr + f[v]);
                            ev[u][v] = *(const V *)(er + f[v]);
                        }
                    }
                }
#pragma unroll
                for (int u = 0; u < U; u++) {
#pragma unroll
                    for (int v = 0; v < NV; v++)
                        if (ok[u] && fok[v]) {
#pragma unroll
                            for (int i = 0; i < VEC; i++) {
                                const T mv = msg(T(rg_get<S, VEC>(x[u][v], i)), T(rg_get<S, VEC>(ev[u][v], i)));
                                sm_fold(m[v][i], den[v][i], num[v][i], tv[v][i] * mv, mv);
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

template <typename T, typename S, int VEC>
inline void launch_edge_softmax_gather_v(const uint32_t *rowptr, const uint32_t *colind, uint32_t nrows, uint32_t nnz, const S *X, uint64_t ldx, const S *E,
                                         uint64_t lde, const EdgeMsg<T> &msg, const T *t, uint32_t h, S *out, uint64_t ldo, T *lse, const SoftmaxWs<T> &ws,
                                         const LaunchShape &g, hipStream_t stream) {
    rg_dispatch(nnz, g, [&](auto nv, auto whole, dim3 grid, uint32_t L) {
        hipLaunchKernelGGL((k_edge_softmax_gather<T, S, VEC, decltype(nv)::value, decltype(whole)::value>), grid, dim3(256), 0, stream, rowptr, colind, nrows, nnz,
                           X, ldx, E, lde, msg, t, h, L, out, ldo, lse, ws);
    });
}

// the launcher of launch_spmm_softmax with the E stream: the same empty-row kernel, workspace layout (softmax_workspace_bytes) and fix-up
template <typename T, typename S>
inline void launch_spmm_edge_softmax(const uint32_t *rowptr, const uint32_t *colind, uint32_t nrows, uint32_t nnz, const S *X, uint64_t ldx, const S *E,
                                     uint64_t lde, const EdgeMsg<T> &msg, const T *t, uint32_t h, S *out, uint64_t ldo, T *lse, void *workspace,
                                     hipStream_t stream) {
    constexpr uint32_t V = 16 / sizeof(S);
    if (nrows > 0) hipLaunchKernelGGL((k_softmax_empty<T, S>), dim3((nrows + 3) / 4), dim3(256), 0, stream, rowptr, nrows, h, out, ldo, lse);
    if (nnz == 0) return;
    const uint64_t sub = softmax_sub_bytes(nnz, h, sizeof(T));
    char *p = (char *)workspace;
    const SoftmaxWs<T> ws = {(T *)p, (T *)(p + sub), (T *)(p + 2 * sub)};
    const bool aligned = ldx % V == 0 && lde % V == 0 && ldo % V == 0 && (uintptr_t)X % 16 == 0 && (uintptr_t)E % 16 == 0 && (uintptr_t)out % 16 == 0 &&
                         (uintptr_t)workspace % 16 == 0;
    const LaunchShape g = edge_gather_shape(h, V, aligned);
    if (g.vec > 1) launch_edge_softmax_gather_v<T, S, (int)V>(rowptr, colind, nrows, nnz, X, ldx, E, lde, msg, t, h, out, ldo, lse, ws, g, stream);
    else launch_edge_softmax_gather_v<T, S, 1>(rowptr, colind, nrows, nnz, X, ldx, E, lde, msg, t, h, out, ldo, lse, ws, g, stream);
    const uint64_t runs = row_gather_runs(nnz);
    if (runs > 1)
        hipLaunchKernelGGL((k_softmax_fixup<T, S>), dim3((unsigned)((runs + 2) / 4)), dim3(256), 0, stream, rowptr, nrows, nnz, h, ws, out, ldo, lse);
}

// ---- the backward: dE in entry order ----
constexpr int EG_SUM = 0, EG_BEST = 1, EG_SOFTMAX = 2;   // MODE of k_edge_message_grad (EG_SUM: sum and mean)

// mean: EG_SUM divides G by the row's number of stored entries.  arg: EG_BEST.  t, O, lse: EG_SOFTMAX; dT_part [runs, h] or null.
// X and E are read when the message is needed: under relu, and always for EG_SOFTMAX.
template <typename T, typename S, int VEC, int NV, bool WHOLE, int MODE>
__global__ __launch_bounds__(256) void k_edge_message_grad(const uint32_t *__restrict__ rowptr, const uint32_t *__restrict__ colind, uint32_t nrows, uint32_t nnz,
                                                           const S *__restrict__ X, uint64_t ldx, const S *__restrict__ E, uint64_t lde, EdgeMsg<T> msg,
                                                           int mean, uint32_t h, uint32_t L, const S *__restrict__ G, uint64_t ldg,
                                                           const int32_t *__restrict__ arg, const T *__restrict__ t, const S *__restrict__ O, uint64_t ldo,
                                                           const T *__restrict__ lse, S *__restrict__ dE, uint64_t ldde, T *__restrict__ dT_part) {
    using V = typename SdVec<S, VEC>::type;
    using VT = typename RgPiece<T, VEC>::type;
    using IV = typename RdIdx<VEC>::type;
    constexpr int U = NV == 1 ? RG_U / 2 : RG_U / 4;
    if constexpr (WHOLE) L = 64;
    const uint32_t R = 64 / L;
    const uint32_t lane = threadIdx.x & 63, grp = lane / L, li = lane % L;
    const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint64_t e_begin = wave * RG_EPW;
    if (e_begin >= nnz) return;
    const uint32_t e_end = (uint32_t)(e_begin + RG_EPW < nnz ? e_begin + RG_EPW : nnz);
    const bool need_msg = MODE == EG_SOFTMAX || msg.relu != 0;
    uint32_t f[NV];
    bool fok[NV];
    T tv[NV][VEC], dt[NV][VEC];   // EG_SOFTMAX: the temperatures of the lane's features, and the run's share of dT
#pragma unroll
    for (int v = 0; v < NV; v++) {
        f[v] = ((blockIdx.y * NV + v) * L + li) * VEC;
        fok[v] = f[v] < h;
#pragma unroll
        for (int i = 0; i < VEC; i++) {
            tv[v][i] = T(0);
            dt[v][i] = T(0);
            if constexpr (MODE == EG_SOFTMAX)
                if (fok[v]) tv[v][i] = t[f[v] + i];
        }
    }
    uint32_t row_cur = sd_row_of(rowptr, 0, nrows, (uint32_t)e_begin);
    const uint32_t row_hi = sd_row_of(rowptr, row_cur, nrows, e_end - 1) + 1;

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
            const uint64_t mk = endmask >> pos;
            const bool closes = mk != 0;
            const uint32_t last = closes ? pos + (uint32_t)__builtin_ctzll(mk) : n - 1;
            // what the stretch's row holds for the lane's features: G (divided by the degree for the mean), and arg, or out and lse
            T gr[NV][VEC], orow[NV][VEC], lr[NV][VEC];
            int32_t ar[NV][VEC];
            {
                const uint32_t row = rg_take32<true>(my_row, pos);
                T cnt = T(1);
                if (mean) cnt = T(rowptr[row + 1] - rowptr[row]);
#pragma unroll
                for (int v = 0; v < NV; v++) {
                    V gv = V(0), ov = V(0);
                    VT lv = VT(0);
                    IV av = IV(0);
                    if (fok[v]) {
                        gv = *(const V *)(G + (uint64_t)row * ldg + f[v]);
                        if constexpr (MODE == EG_BEST) av = *(const IV *)(arg + (uint64_t)row * h + f[v]);
                        if constexpr (MODE == EG_SOFTMAX) {
                            ov = *(const V *)(O + (uint64_t)row * ldo + f[v]);
                            lv = *(const VT *)(lse + (uint64_t)row * h + f[v]);
                        }
                    }
#pragma unroll
                    for (int i = 0; i < VEC; i++) {
                        gr[v][i] = T(rg_get<S, VEC>(gv, i));
                        if (mean) gr[v][i] = gr[v][i] / cnt;
                        orow[v][i] = T(rg_get<S, VEC>(ov, i));
                        lr[v][i] = rg_get<T, VEC>(lv, i);
                        if constexpr (VEC == 1) ar[v][i] = av;
                        else ar[v][i] = av[i];
                    }
                }
            }
            for (uint32_t k0 = pos; k0 <= last; k0 += R * U) {
                V x[U][NV], ev[U][NV];
                bool ok[U];
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const uint32_t kk = k0 + (uint32_t)u * R + grp;
                    ok[u] = kk <= last;
                    const uint32_t col = rg_take32<WHOLE>(my_col, ok[u] ? kk : pos);
                    const S *xr = X + (uint64_t)col * ldx;
                    const S *er = E + (uint64_t)(base + kk) * lde;   // read only when ok[u]: base + kk < e_end
#pragma unroll
                    for (int v = 0; v < NV; v++) {
                        x[u][v] = V(0);
                        ev[u][v] = V(0);
                        if (ok[u] && fok[v] && need_msg) {
                            x[u][v] = *(const V *)(xr + f[v]);
                            ev[u][v] = *(const V *)(er + f[v]);
                        }
                    }
                }
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const uint32_t kk = k0 + (uint32_t)u * R + grp;
#pragma unroll
                    for (int v = 0; v < NV; v++)
                        if (ok[u] && fok[v]) {
                            T d[VEC];
#pragma unroll
                            for (int i = 0; i < VEC; i++) {
                                const T xv = T(rg_get<S, VEC>(x[u][v], i)), evv = T(rg_get<S, VEC>(ev[u][v], i));
                                T c = gr[v][i];
                                if constexpr (MODE == EG_BEST) c = ar[v][i] == (int32_t)(base + kk) ? c : T(0);
                                if constexpr (MODE == EG_SOFTMAX) {
                                    const T mv = msg(xv, evv);
                                    const T gp = gr[v][i] * sm_exp(tv[v][i] * mv - lr[v][i]);
                                    const T dm = mv - orow[v][i];
                                    c = gp * (T(1) + tv[v][i] * dm);
                                    dt[v][i] = sm_fma(gp * mv, dm, dt[v][i]);
                                }
                                d[i] = msg.live(xv, evv) ? c : T(0);
                            }
                            rg_store<S, T, VEC>(dE + (uint64_t)(base + kk) * ldde + f[v], d);
                        }
                }
            }
            pos = last + 1;
        }
        row_cur = rg_take32<true>(my_row, n - 1);
    }
    if constexpr (MODE == EG_SOFTMAX) {
        if (dT_part) {
#pragma unroll
            for (int v = 0; v < NV; v++) {
                if constexpr (!WHOLE) {
                    for (uint32_t s = L; s < 64; s <<= 1) {
#pragma unroll
                        for (int i = 0; i < VEC; i++) dt[v][i] = dt[v][i] + rg_shfl_xor(dt[v][i], (int)s);
                    }
                }
                if (grp == 0 && fok[v]) sm_store_loose<T, VEC>(dT_part + wave * (uint64_t)h + f[v], dt[v]);
            }
        }
    }
}

template <typename T, typename S, int VEC, int MODE>
inline void launch_edge_grad_v(const uint32_t *rowptr, const uint32_t *colind, uint32_t nrows, uint32_t nnz, const S *X, uint64_t ldx, const S *E, uint64_t lde,
                               const EdgeMsg<T> &msg, int mean, uint32_t h, const S *G, uint64_t ldg, const int32_t *arg, const T *t, const S *O, uint64_t ldo,
                               const T *lse, S *dE, uint64_t ldde, T *dT_part, const LaunchShape &g, hipStream_t stream) {
    rg_dispatch(nnz, g, [&](auto nv, auto whole, dim3 grid, uint32_t L) {
        hipLaunchKernelGGL((k_edge_message_grad<T, S, VEC, decltype(nv)::value, decltype(whole)::value, MODE>), grid, dim3(256), 0, stream, rowptr, colind, nrows,
                           nnz, X, ldx, E, lde, msg, mean, h, L, G, ldg, arg, t, O, ldo, lse, dE, ldde, dT_part);
    });
}

// 16-byte pieces need every row of X, E, G, dE (and out, lse for the softmax) 16-byte aligned; arg and dT_part are read and stored with the
// alignment of one element
template <typename T, typename S, int MODE>
inline void launch_edge_grad(const uint32_t *rowptr, const uint32_t *colind, uint32_t nrows, uint32_t nnz, const S *X, uint64_t ldx, const S *E, uint64_t lde,
                             const EdgeMsg<T> &msg, int mean, uint32_t h, const S *G, uint64_t ldg, const int32_t *arg, const T *t, const S *O, uint64_t ldo,
                             const T *lse, S *dE, uint64_t ldde, T *dT_part, hipStream_t stream) {
    constexpr uint32_t V = 16 / sizeof(S);
    if (nnz == 0) return;
    bool aligned = ldx % V == 0 && lde % V == 0 && ldg % V == 0 && ldde % V == 0 && (uintptr_t)X % 16 == 0 && (uintptr_t)E % 16 == 0 && (uintptr_t)G % 16 == 0 &&
                   (uintptr_t)dE % 16 == 0;
    if (MODE == EG_SOFTMAX) aligned = aligned && ldo % V == 0 && (uintptr_t)O % 16 == 0 && (uintptr_t)lse % 16 == 0;
    const LaunchShape g = edge_grad_shape(h, V, aligned);
    if (g.vec > 1)
        launch_edge_grad_v<T, S, (int)V, MODE>(rowptr, colind, nrows, nnz, X, ldx, E, lde, msg, mean, h, G, ldg, arg, t, O, ldo, lse, dE, ldde, dT_part, g, stream);
    else
        launch_edge_grad_v<T, S, 1, MODE>(rowptr, colind, nrows, nnz, X, ldx, E, lde, msg, mean, h, G, ldg, arg, t, O, ldo, lse, dE, ldde, dT_part, g, stream);
}

// op: RD_SUM, RD_MEAN, RD_SOFTMAX, or (S = T: the caller checks) RD_MAX / RD_MIN
template <typename T, typename S>
inline void launch_spmm_edge_backward(int op, const uint32_t *rowptr, const uint32_t *colind, uint32_t nrows, uint32_t nnz, const S *X, uint64_t ldx, const S *E,
                                      uint64_t lde, const EdgeMsg<T> &msg, uint32_t h, const S *G, uint64_t ldg, const int32_t *arg, const T *t, const S *O,
                                      uint64_t ldo, const T *lse, S *dE, uint64_t ldde, T *dT_part, hipStream_t stream) {
    if (op == RD_SUM || op == RD_MEAN)
        return launch_edge_grad<T, S, EG_SUM>(rowptr, colind, nrows, nnz, X, ldx, E, lde, msg, op == RD_MEAN, h, G, ldg, nullptr, nullptr, nullptr, 0, nullptr, dE,
                                              ldde, nullptr, stream);
    if (op == RD_SOFTMAX)
        return launch_edge_grad<T, S, EG_SOFTMAX>(rowptr, colind, nrows, nnz, X, ldx, E, lde, msg, 0, h, G, ldg, nullptr, t, O, ldo, lse, dE, ldde, dT_part, stream);
    if constexpr (std::is_same<S, T>::value)
        launch_edge_grad<T, S, EG_BEST>(rowptr, colind, nrows, nnz, X, ldx, E, lde, msg, 0, h, G, ldg, arg, nullptr, nullptr, 0, nullptr, dE, ldde, nullptr, stream);
}

}  // namespace pygim
