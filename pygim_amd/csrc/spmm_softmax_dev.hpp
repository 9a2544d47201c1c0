// spmm_softmax_dev.hpp -- softmax aggregation per feature in ONE gather (PyG's SoftmaxAggregation, GENConv / DeeperGCN), unit weights:
//   s[e, f] = t[f] * X[colind[e], f]          lse[r, f] = log sum over the stored entries e of row r of exp(s[e, f])
//   out[r, f] = sum_e exp(s[e, f] - lse[r, f]) * X[colind[e], f]
// The score of an entry is the gathered feature itself times a temperature per feature, so the softmax runs per (row, feature) and a
// composition from edge_softmax and spmm_values with heads = h needs several [nnz, h] tensors; here nothing of that size exists.
//
// Forward, k_softmax_gather.  Per feature a lane carries the online-softmax triple (m, den, num): the running maximum of s, and
// sum exp(s - m) and sum exp(s - m) * x under that maximum.  One exp per element and entry: with d = s - m and e = exp(-|d|),
//   d > 0:  num = num * e + x, den = den * e + 1, m = s            else:  num += e * x, den += e
// (the first entry of a row meets m = -inf: d = +inf, e = 0).  sm_join folds one triple into another by rescaling the one with the smaller
// maximum; a maximum that equals the joint one is not subtracted from it, so the neutral element (-inf, 0, 0) forms no -inf - (-inf).
// The join is used in the xor tree of the lane groups that share a row, for the two slots a run shares with its neighbours and in
// k_softmax_fixup.  The finished row is num / den, its lse is m + log(den).
// A NaN or +-inf score makes num of that (row, feature) NaN or +-inf (exp(-|d|) of it is NaN or 0, and 0 * inf is NaN) and touches no other
// feature: nothing is skipped or masked.
//
// Backward, k_softmax_grad: one gather on the CSR of A^T.  For an entry of column c that belongs to A-row r the lane gathers G[r], out[r]
// and lse[r] and holds its own row X[c]:
//   p = exp(t[f] * X[c, f] - lse[r, f])      a[c, f] = sum G[r, f] * p      b[c, f] = sum G[r, f] * p * (X[c, f] - out[r, f])
//   dX[c, f] = a + t[f] * b                  dT[c, f] = X[c, f] * b   (optional; the caller sums it over c)
// The partial result is the two plain sums a and b in stored order: the slots and the fix-up are those of a sum fold.
//
// The walk inside both kernels -- batch loop, row search, ballot of row ends, cut into stretches, slot rule -- is a copy of k_row_gather's
// (row_gather_dev.hpp, which lists all the copies and says why they stay): a change to the walk there has to be made here as well.  The
// fix-ups find their row with rg_cut_row and the launchers pick the launch form with rg_dispatch; the lane layout is the mean fold's.
//
// The workspace holds, per run, two slots of h elements of every component (m, den, num forward; a, b backward), every sub-array 16-byte
// aligned.  A row that lies wholly inside a wave's run is stored directly, finished; the at most two rows a run shares with its
// neighbours leave their raw partials in the slots and the fix-up joins them per row in the order of the runs.  Rows without entries are
// written by the *_empty kernels (0, and -inf in lse).  No two kernels write the same row, no atomics: the same bits on every launch.
//
// S is the storage type of X, G, out and dX, T the type of everything else (t, lse, dT, the partials, the slots): S = T = float / double,
// or S = _Float16 / __bf16 with T = float -- an element is widened as it is folded (exact) and a finished row is rounded once, where it is
// stored.  lse and dT are stored with the alignment of one element, whatever the piece (like arg of the indexed folds), so the launch
// shape -- and with it the bits of out and dX -- does not depend on whether they are asked for.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "edge_softmax_dev.hpp"
#include "gat_aggregate_dev.hpp"
#include "row_gather_dev.hpp"

namespace pygim {

// VEC elements of T with the alignment of one element: how lse and dT are stored
template <typename T, int VEC> struct SmLoose { typedef T __attribute__((ext_vector_type(VEC), aligned(sizeof(T)))) type; };
template <typename T> struct SmLoose<T, 1> { typedef T type; };
template <typename T, int VEC> __device__ inline void sm_store_loose(T *dst, const T *a) {
    typename SmLoose<T, VEC>::type v;
    if constexpr (VEC == 1) v = a[0];
    else {
#pragma unroll
        for (int i = 0; i < VEC; i++) v[i] = a[i];
    }
    *(typename SmLoose<T, VEC>::type *)dst = v;
}

__device__ inline float sm_abs(float x) { return fabsf(x); }
__device__ inline double sm_abs(double x) { return fabs(x); }
// exp of an argument <= 0 (a score below its maximum, or below the row's lse).  float32: the hardware exponential of x * log2(e), whose
// relative error grows with |x| 2^-24 -- the Delta term of the bounds in include/pygim_hip.h, where EPS = 1e-5 stands for 2^-24; the
// accurate expf costs about as much as the rest of the fold, and the 16-bit forward is bound by this arithmetic, not by the gather.
__device__ inline float sm_exp(float x) { return __expf(x); }
__device__ inline double sm_exp(double x) { return exp(x); }
// a * b + c with one rounding, written out: the build has contraction off, and the fold should not depend on it
__device__ inline float sm_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ inline double sm_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }

// one entry (score s, value x) into the triple
template <typename T> __device__ inline void sm_fold(T &m, T &den, T &num, T s, T x) {
    const T d = s - m;
    const T e = sm_exp(-sm_abs(d));
    if (d > T(0)) {
        num = sm_fma(num, e, x);
        den = sm_fma(den, e, T(1));
        m = s;
    } else {
        num = sm_fma(e, x, num);
        den = den + e;
    }
}

// the triple (m2, den2, num2) into (m, den, num): the one with the smaller maximum is rescaled; (-inf, 0, 0) is the neutral element
template <typename T> __device__ inline void sm_join(T &m, T &den, T &num, T m2, T den2, T num2) {
    const T M = m > m2 ? m : m2;
    const T a = m == M ? T(1) : sm_exp(m - M);
    const T b = m2 == M ? T(1) : sm_exp(m2 - M);
    den = den * a + den2 * b;
    num = num * a + num2 * b;
    m = M;
}

// the sub-arrays of the forward's workspace
template <typename T> struct SoftmaxWs {
    T *m, *den, *num;
};

// the finished-row store of VEC features from column f on: out = num / den (rounded into S here and nowhere else), lse = m + log(den)
template <typename T, typename S, int VEC>
__device__ inline void sm_store_row(S *__restrict__ orow, T *__restrict__ lse_row, uint32_t f, const T *m, const T *den, const T *num) {
    T o[VEC];
#pragma unroll
    for (int i = 0; i < VEC; i++) o[i] = num[i] / den[i];
    rg_store<S, T, VEC>(orow + f, o);
    if (lse_row) {
#pragma unroll
        for (int i = 0; i < VEC; i++) o[i] = m[i] + gat_log(den[i]);
        sm_store_loose<T, VEC>(lse_row + f, o);
    }
}

// WHOLE: the wave is one lane group (L = 64) that holds NV pieces of VEC features per lane; else NV = 1 and L < 64 is a launch argument.
// lse: [nrows, h] contiguous, or null.
template <typename T, typename S, int VEC, int NV, bool WHOLE>
__global__ __launch_bounds__(256) void k_softmax_gather(const uint32_t *__restrict__ rowptr, const uint32_t *__restrict__ colind, uint32_t nrows, uint32_t nnz,
                                                        const S *__restrict__ X, uint64_t ldx, const T *__restrict__ t, uint32_t h, uint32_t L,
                                                        S *__restrict__ out, uint64_t ldo, T *__restrict__ lse, SoftmaxWs<T> ws) {
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
                V x[U][NV];
                bool ok[U];
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const uint32_t kk = k0 + (uint32_t)u * R + grp;
                    ok[u] = kk <= last;
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
                                sm_fold(m[v][i], den[v][i], num[v][i], tv[v][i] * xv, xv);
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
// (the loop of k_row_gather_fixup on a triple)
template <typename T, typename S>
__global__ __launch_bounds__(256) void k_softmax_fixup(const uint32_t *__restrict__ rowptr, uint32_t nrows, uint32_t nnz, uint32_t h, SoftmaxWs<T> ws,
                                                       S *__restrict__ out, uint64_t ldo, T *__restrict__ lse) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t w = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    uint32_t row, rb, re;
    uint64_t w1;
    if (!rg_cut_row(rowptr, nrows, nnz, w, row, rb, re, w1)) return;
    for (uint32_t f = lane; f < h; f += 64) {
        uint64_t at = (w * 2 + 1) * (uint64_t)h + f;
        T m = ws.m[at], den = ws.den[at], num = ws.num[at];
        for (uint64_t j = w + 1; j <= w1; j++) {
            at = j * 2 * (uint64_t)h + f;
            sm_join(m, den, num, ws.m[at], ws.den[at], ws.num[at]);
        }
        sm_store_row<T, S, 1>(out + (uint64_t)row * ldo, lse ? lse + (uint64_t)row * h : nullptr, f, &m, &den, &num);
    }
}

// rows without entries: 0, and -inf in lse (the walk of k_row_gather_empty: a change there has to be made here as well)
template <typename T, typename S>
__global__ __launch_bounds__(256) void k_softmax_empty(const uint32_t *__restrict__ rowptr, uint32_t nrows, uint32_t h, S *__restrict__ out, uint64_t ldo,
                                                       T *__restrict__ lse) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t row = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= nrows || rowptr[row] != rowptr[row + 1]) return;
    for (uint32_t f = lane; f < h; f += 64) {
        out[row * ldo + f] = S(0);
        if (lse) lse[row * h + f] = es_neg_inf<T>();
    }
}

// ---- the workspace: per run two slots of h elements of every component, each sub-array rounded up to 16 bytes ----
inline uint64_t softmax_sub_bytes(uint64_t nnz, uint64_t h, size_t elem) { return row_gather_index_offset(nnz, h, elem); }
inline uint64_t softmax_workspace_bytes(uint64_t nnz, uint64_t h, size_t elem) { return 3 * softmax_sub_bytes(nnz, h, elem); }
inline uint64_t softmax_backward_workspace_bytes(uint64_t nnz, uint64_t h, size_t elem) { return 2 * softmax_sub_bytes(nnz, h, elem); }

// the lane layout of both kernels: the mean fold's (16-byte pieces of the storage type when every gathered and stored row starts 16-byte
// aligned and h fills whole pieces)
inline LaunchShape softmax_gather_shape(uint32_t h, uint32_t V, bool aligned) { return row_gather_shape(h, h, V, aligned); }
inline LaunchShape softmax_grad_shape(uint32_t h, uint32_t V, bool aligned) { return row_gather_shape(h, h, V, aligned); }

template <typename T, typename S, int VEC>
inline void launch_softmax_gather_v(const uint32_t *rowptr, const uint32_t *colind, uint32_t nrows, uint32_t nnz, const S *X, uint64_t ldx, const T *t,
                                    uint32_t h, S *out, uint64_t ldo, T *lse, const SoftmaxWs<T> &ws, const LaunchShape &g, hipStream_t stream) {
    rg_dispatch(nnz, g, [&](auto nv, auto whole, dim3 grid, uint32_t L) {
        hipLaunchKernelGGL((k_softmax_gather<T, S, VEC, decltype(nv)::value, decltype(whole)::value>), grid, dim3(256), 0, stream, rowptr, colind, nrows, nnz, X,
                           ldx, t, h, L, out, ldo, lse, ws);
    });
}

template <typename T, typename S>
inline void launch_spmm_softmax(const uint32_t *rowptr, const uint32_t *colind, uint32_t nrows, uint32_t nnz, const S *X, uint64_t ldx, const T *t, uint32_t h,
                                S *out, uint64_t ldo, T *lse, void *workspace, hipStream_t stream) {
    constexpr uint32_t V = 16 / sizeof(S);
    if (nrows > 0) hipLaunchKernelGGL((k_softmax_empty<T, S>), dim3((nrows + 3) / 4), dim3(256), 0, stream, rowptr, nrows, h, out, ldo, lse);
    if (nnz == 0) return;
    const uint64_t sub = softmax_sub_bytes(nnz, h, sizeof(T));
    char *p = (char *)workspace;
    const SoftmaxWs<T> ws = {(T *)p, (T *)(p + sub), (T *)(p + 2 * sub)};
    const bool aligned = ldx % V == 0 && ldo % V == 0 && (uintptr_t)X % 16 == 0 && (uintptr_t)out % 16 == 0 && (uintptr_t)workspace % 16 == 0;
    const LaunchShape g = softmax_gather_shape(h, V, aligned);
    if (g.vec > 1) launch_softmax_gather_v<T, S, (int)V>(rowptr, colind, nrows, nnz, X, ldx, t, h, out, ldo, lse, ws, g, stream);
    else launch_softmax_gather_v<T, S, 1>(rowptr, colind, nrows, nnz, X, ldx, t, h, out, ldo, lse, ws, g, stream);
    const uint64_t runs = row_gather_runs(nnz);
    if (runs > 1)
        hipLaunchKernelGGL((k_softmax_fixup<T, S>), dim3((unsigned)((runs + 2) / 4)), dim3(256), 0, stream, rowptr, nrows, nnz, h, ws, out, ldo, lse);
}

// ---- the backward: one gather on the CSR of A^T ----
// the finished-row store of VEC features of column `c`: dX = a + t * b (rounded into S here and nowhere else), dT = x * b
template <typename T, typename S, int VEC>
__device__ inline void sm_store_grad(S *__restrict__ drow, T *__restrict__ dt_row, uint32_t f, const T *a, const T *b, const T *tv, const T *xo) {
    T o[VEC];
#pragma unroll
    for (int i = 0; i < VEC; i++) o[i] = a[i] + tv[i] * b[i];
    rg_store<S, T, VEC>(drow + f, o);
    if (dt_row) {
#pragma unroll
        for (int i = 0; i < VEC; i++) o[i] = xo[i] * b[i];
        sm_store_loose<T, VEC>(dt_row + f, o);
    }
}

// rowptr / colind: the CSR of A^T (ncols rows; colind holds the A-row of every entry).  Three gathers per entry (G, out, lse): half the
// entries in flight of the forward.  dT: [ncols, h] contiguous, or null.
template <typename T, typename S, int VEC, int NV, bool WHOLE>
__global__ __launch_bounds__(256) void k_softmax_grad(const uint32_t *__restrict__ rowptr, const uint32_t *__restrict__ colind, uint32_t nrows, uint32_t nnz,
                                                      const S *__restrict__ X, uint64_t ldx, const T *__restrict__ t, uint32_t h, uint32_t L,
                                                      const S *__restrict__ G, uint64_t ldg, const S *__restrict__ O, uint64_t ldo, const T *__restrict__ lse,
                                                      S *__restrict__ dX, uint64_t ldd, T *__restrict__ dT, T *__restrict__ ws_a, T *__restrict__ ws_b) {
    using V = typename SdVec<S, VEC>::type;
    using VT = typename RgPiece<T, VEC>::type;
    constexpr int U = NV == 1 ? RG_U / 2 : RG_U / 4;
    if constexpr (WHOLE) L = 64;
    const uint32_t R = 64 / L;
    const uint32_t lane = threadIdx.x & 63, grp = lane / L, li = lane % L;
    const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint64_t e_begin = wave * RG_EPW;
    if (e_begin >= nnz) return;
    const uint32_t e_end = (uint32_t)(e_begin + RG_EPW < nnz ? e_begin + RG_EPW : nnz);
    uint32_t f[NV];
    bool fok[NV];
    T tv[NV][VEC];
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
    T a[NV][VEC], b[NV][VEC];     // the two running sums ...
    T xo[NV][VEC], sx[NV][VEC];   // ... the lane's own row X[c] of the stretch at hand and its score t * X[c]
    const uint64_t slots = wave * 2 * (uint64_t)h;
    const auto reset = [&]() {
#pragma unroll
        for (int v = 0; v < NV; v++)
#pragma unroll
            for (int i = 0; i < VEC; i++) a[v][i] = b[v][i] = T(0);
    };
    // join the lane groups, then store: the raw sums into the workspace slots, or the finished row `row` into dX / dT
    const auto flush = [&](bool to_slot, uint32_t slot, uint32_t row) {
        const uint64_t at = slots + (slot ? h : 0u);
#pragma unroll
        for (int v = 0; v < NV; v++) {
            if constexpr (!WHOLE) {
                for (uint32_t s = L; s < 64; s <<= 1) {
#pragma unroll
                    for (int i = 0; i < VEC; i++) {
                        a[v][i] = a[v][i] + rg_shfl_xor(a[v][i], (int)s);
                        b[v][i] = b[v][i] + rg_shfl_xor(b[v][i], (int)s);
                    }
                }
            }
            if (grp == 0 && fok[v]) {
                if (to_slot) {
                    rg_store<T, T, VEC>(ws_a + at + f[v], a[v]);
                    rg_store<T, T, VEC>(ws_b + at + f[v], b[v]);
                } else {
                    sm_store_grad<T, S, VEC>(dX + (uint64_t)row * ldd, dT ? dT + (uint64_t)row * h : nullptr, f[v], a[v], b[v], tv[v], xo[v]);
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
            {   // the stretch's own row: the row of its first entry
                const S *xr = X + (uint64_t)rg_take32<true>(my_row, pos) * ldx;
#pragma unroll
                for (int v = 0; v < NV; v++) {
                    V own = V(0);
                    if (fok[v]) own = *(const V *)(xr + f[v]);
#pragma unroll
                    for (int i = 0; i < VEC; i++) {
                        xo[v][i] = T(rg_get<S, VEC>(own, i));
                        sx[v][i] = tv[v][i] * xo[v][i];
                    }
                }
            }
            for (uint32_t k0 = pos; k0 <= last; k0 += R * U) {
                V g[U][NV], o[U][NV];
                VT l[U][NV];
                bool ok[U];
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const uint32_t kk = k0 + (uint32_t)u * R + grp;
                    ok[u] = kk <= last;
                    const uint32_t r = rg_take32<WHOLE>(my_col, ok[u] ? kk : pos);
                    const S *gr = G + (uint64_t)r * ldg, *orow = O + (uint64_t)r * ldo;
                    const T *lr = lse + (uint64_t)r * h;
#pragma unroll
                    for (int v = 0; v < NV; v++) {
                        g[u][v] = V(0);
                        o[u][v] = V(0);
                        l[u][v] = VT(0);
                        if (ok[u] && fok[v]) {
                            g[u][v] = *(const V *)(gr + f[v]);
                            o[u][v] = *(const V *)(orow + f[v]);
                            l[u][v] = *(const VT *)(lr + f[v]);
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
                                const T gp = T(rg_get<S, VEC>(g[u][v], i)) * sm_exp(sx[v][i] - rg_get<T, VEC>(l[u][v], i));
                                a[v][i] = a[v][i] + gp;
                                b[v][i] = sm_fma(gp, xo[v][i] - T(rg_get<S, VEC>(o[u][v], i)), b[v][i]);
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

// one wave per run: the sums of the row that goes on after run w, in run order, then the row's own X and t close it
template <typename T, typename S>
__global__ __launch_bounds__(256) void k_softmax_grad_fixup(const uint32_t *__restrict__ rowptr, uint32_t nrows, uint32_t nnz, const S *__restrict__ X,
                                                            uint64_t ldx, const T *__restrict__ t, uint32_t h, const T *__restrict__ ws_a,
                                                            const T *__restrict__ ws_b, S *__restrict__ dX, uint64_t ldd, T *__restrict__ dT) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t w = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    uint32_t row, rb, re;
    uint64_t w1;
    if (!rg_cut_row(rowptr, nrows, nnz, w, row, rb, re, w1)) return;
    for (uint32_t f = lane; f < h; f += 64) {
        uint64_t at = (w * 2 + 1) * (uint64_t)h + f;
        T a = ws_a[at], b = ws_b[at];
        for (uint64_t j = w + 1; j <= w1; j++) {
            at = j * 2 * (uint64_t)h + f;
            a = a + ws_a[at];
            b = b + ws_b[at];
        }
        const T tf = t[f], xo = T(X[(uint64_t)row * ldx + f]);
        sm_store_grad<T, S, 1>(dX + (uint64_t)row * ldd, dT ? dT + (uint64_t)row * h : nullptr, f, &a, &b, &tf, &xo);
    }
}

// columns without entries: zeros in dX and dT
template <typename T, typename S>
__global__ __launch_bounds__(256) void k_softmax_grad_empty(const uint32_t *__restrict__ rowptr, uint32_t nrows, uint32_t h, S *__restrict__ dX, uint64_t ldd,
                                                            T *__restrict__ dT) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t row = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= nrows || rowptr[row] != rowptr[row + 1]) return;
    for (uint32_t f = lane; f < h; f += 64) {
        dX[row * ldd + f] = S(0);
        if (dT) dT[row * h + f] = T(0);
    }
}

template <typename T, typename S, int VEC>
inline void launch_softmax_grad_v(const uint32_t *rowptr, const uint32_t *colind, uint32_t nrows, uint32_t nnz, const S *X, uint64_t ldx, const T *t, uint32_t h,
                                  const S *G, uint64_t ldg, const S *O, uint64_t ldo, const T *lse, S *dX, uint64_t ldd, T *dT, T *ws_a, T *ws_b,
                                  const LaunchShape &g, hipStream_t stream) {
    rg_dispatch(nnz, g, [&](auto nv, auto whole, dim3 grid, uint32_t L) {
        hipLaunchKernelGGL((k_softmax_grad<T, S, VEC, decltype(nv)::value, decltype(whole)::value>), grid, dim3(256), 0, stream, rowptr, colind, nrows, nnz, X,
                           ldx, t, h, L, G, ldg, O, ldo, lse, dX, ldd, dT, ws_a, ws_b);
    });
}

// 16-byte pieces need every row of X, G, out, lse and dX 16-byte aligned (lse rows are h elements of T apart)
template <typename T, typename S>
inline void launch_spmm_softmax_backward(const uint32_t *rowptr, const uint32_t *colind, uint32_t ncols, uint32_t nnz, const S *X, uint64_t ldx, const T *t,
                                         uint32_t h, const S *G, uint64_t ldg, const S *O, uint64_t ldo, const T *lse, S *dX, uint64_t ldd, T *dT,
                                         void *workspace, hipStream_t stream) {
    constexpr uint32_t V = 16 / sizeof(S);
    if (ncols > 0) hipLaunchKernelGGL((k_softmax_grad_empty<T, S>), dim3((ncols + 3) / 4), dim3(256), 0, stream, rowptr, ncols, h, dX, ldd, dT);
    if (nnz == 0) return;
    T *ws_a = (T *)workspace, *ws_b = (T *)((char *)workspace + softmax_sub_bytes(nnz, h, sizeof(T)));
    const bool aligned = ldx % V == 0 && ldg % V == 0 && ldo % V == 0 && ldd % V == 0 && (uintptr_t)X % 16 == 0 && (uintptr_t)G % 16 == 0 &&
                         (uintptr_t)O % 16 == 0 && (uintptr_t)lse % 16 == 0 && (uintptr_t)dX % 16 == 0 && (uintptr_t)workspace % 16 == 0;
    const LaunchShape g = softmax_grad_shape(h, V, aligned);
    if (g.vec > 1) launch_softmax_grad_v<T, S, (int)V>(rowptr, colind, ncols, nnz, X, ldx, t, h, G, ldg, O, ldo, lse, dX, ldd, dT, ws_a, ws_b, g, stream);
    else launch_softmax_grad_v<T, S, 1>(rowptr, colind, ncols, nnz, X, ldx, t, h, G, ldg, O, ldo, lse, dX, ldd, dT, ws_a, ws_b, g, stream);
    const uint64_t runs = row_gather_runs(nnz);
    if (runs > 1)
        hipLaunchKernelGGL((k_softmax_grad_fixup<T, S>), dim3((unsigned)((runs + 2) / 4)), dim3(256), 0, stream, rowptr, ncols, nnz, X, ldx, t, h, ws_a, ws_b,
                           dX, ldd, dT);
}

}  // namespace pygim
