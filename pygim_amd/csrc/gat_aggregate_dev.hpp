// gat_aggregate_dev.hpp -- the aggregation of a GAT layer in one pass over the stored entries: scores, softmax and product
//   z[e, k]   = a_dst[r, k] + a_src[colind[e], k]              e over the stored entries of row r, in stored order; k = f / (h / heads)
//   s[e, k]   = z >= 0 ? z : negative_slope * z
//   out[r, f] = sum_e exp(s[e, k] - m[r, k]) * X[colind[e], f] / l[r, k],   m = max_e s,  l = sum_e exp(s - m)
//   lse[r, k] = m[r, k] + log(l[r, k])                         (optional)
// Nothing of size nnz is read besides colind or written at all: every score is a function of two per-node numbers, and the softmax is
// an online one -- a running maximum m, a running sum l and an accumulator that is rescaled when the maximum rises.
//
// Shape: k_row_gather's (row_gather_dev.hpp), a sibling kernel on its helpers so that the folds of spmm_values / spmm_reduce compile to
// what they compiled to before.  A wave owns RG_EPW consecutive entries and walks them in batches of 64; lanes lie across the features
// (16 bytes each when a head's features fill whole pieces), 64 / L lane groups side by side for narrow rows, two pieces per lane and
// blockIdx.y for wide ones, the gathers of up to RG_U entries issued before the first is folded.  What is new:
//   * a lane's piece lies in one head, so the lane carries (m, l) of that head beside the piece's accumulator -- lanes of one head see
//     the same entries in the same order and hold the same bits, no cross-lane traffic;
//   * a_dst[r, k] is loaded once per stretch of a row, a_src[col, k] is one element gathered per entry beside the X row;
//   * the entries in flight are folded as a group: M = max(m, their scores), ONE rescale exp(m - M) of (l, acc), then
//     p = exp(s - M), l += p, acc += p * x per entry, in entry order;
//   * partial results (m, l, acc) meet by gat_merge -- es_merge carrying the accumulator: (-inf, 0, 0) is neutral, an equal maximum
//     scales by exactly 1 -- in the xor tree of the lane groups, and in k_gat_fixup over the slots of the runs a row is cut across;
//   * a row's m starts at es_lowest (the lowest finite number, neutral as well), so scores of -inf -- masked entries -- fold as p = 0
//     wherever they stand, and a (row, head) of nothing else stores NaN and lse = -inf (edge_softmax_dev.hpp on es_lowest);
//   * the workspace slots hold the raw (m, l, acc): h accumulators per slot as in k_row_gather, and behind them 2 numbers per head and
//     slot; the division by l happens only where a finished row is stored.
// No atomics, every order is fixed by the CSR: the same bits on every launch.
//
// The walk inside k_gat_gather -- batch loop, row search, ballot of row ends, cut into stretches, slot rule -- is a copy of
// k_row_gather's (row_gather_dev.hpp, which lists all the copies and says why they stay: a shared device function cost some
// instantiations a wave per SIMD): a change to the walk has to be made there as well.  The fix-up's preamble (rg_cut_row) and the
// choice of launch form (rg_dispatch) are shared.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "attn_dropout_dev.hpp"
#include "edge_softmax_dev.hpp"
#include "row_gather_dev.hpp"

namespace pygim {

__device__ inline float gat_log(float x) { return logf(x); }
__device__ inline double gat_log(double x) { return log(x); }

// the factors that bring two partials with maxima m and m2 onto their common maximum M (exactly 1 for the one that holds it)
template <typename T> __device__ inline void gat_scales(T m, T m2, T &M, T &a, T &b) {
    M = m > m2 ? m : m2;
    a = m == M ? T(1) : es_exp(m - M);
    b = m2 == M ? T(1) : es_exp(m2 - M);
}

// the workspace: the accumulator slots of k_row_gather, then (m, l) per head for each of the 2 slots of a run
inline uint64_t gat_stat_offset(uint64_t nnz, uint64_t h, size_t elem) { return row_gather_index_offset(nnz, h, elem); }
inline uint64_t gat_workspace_bytes(uint64_t nnz, uint64_t h, uint64_t heads, size_t elem) {
    return gat_stat_offset(nnz, h, elem) + row_gather_runs(nnz) * 2 * heads * 2 * elem;
}

// WHOLE: the wave is one lane group (L = 64) that holds NV pieces of VEC features per lane; else NV = 1 and L < 64 is a launch argument.
// lse may be null.  ws: accumulator slots, ws_stat: the (m, l) slots.
// S is the storage type of X and out, T the type of a_dst, a_src, lse, (m, l, acc) and the slots (S = T, or a 16-bit S with T = float:
// an X piece is widened as it is folded, acc / l is rounded once where a finished row is stored).
// DROP: attention dropout (attn_dropout_dev.hpp).  A probability goes into l unchanged and into the accumulate as p * w, w = 1 / (1 - rate) or
// 0 from the mask of (entry index base + kk, the piece's head hv[v]); m, l, lse and everything else are untouched.  dr is read only then.
// EDGE: a per-entry term of the score, z = a_dst + a_src + a_edge[e, k] before the leaky ReLU (the edge features of PyG's GATConv, an
// additive mask).  a_edge is [nnz, heads] in the stored order of A and e = base + kk is the index the dropout hash takes: the 64 entries of
// a batch are 64 * heads consecutive elements, each lane loads the one of its (entry, head) beside the gathered row.  Read only then.
template <typename T, typename S, int VEC, int NV, bool WHOLE, bool DROP = false, bool EDGE = false>
__global__ __launch_bounds__(256) void k_gat_gather(const uint32_t *__restrict__ rowptr, const uint32_t *__restrict__ colind, uint32_t nrows, uint32_t nnz,
                                                    const T *__restrict__ a_dst, const T *__restrict__ a_src, uint32_t heads, T slope,
                                                    const S *__restrict__ X, uint64_t ldx, uint32_t h, uint32_t L, S *__restrict__ out, uint64_t ldo,
                                                    T *__restrict__ lse, T *__restrict__ ws, T *__restrict__ ws_stat, AttnDrop<T> dr,
                                                    const T *__restrict__ a_edge = nullptr) {
    using V = typename SdVec<S, VEC>::type;
    constexpr int U = NV == 1 ? RG_U : RG_U / 2;
    if constexpr (WHOLE) L = 64;
    const uint32_t R = 64 / L;
    const uint32_t lane = threadIdx.x & 63, grp = lane / L, li = lane % L;
    const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint64_t e_begin = wave * RG_EPW;
    if (e_begin >= nnz) return;
    const uint32_t e_end = (uint32_t)(e_begin + RG_EPW < nnz ? e_begin + RG_EPW : nnz);
    const uint32_t hd = h / heads;
    uint32_t f[NV], hv[NV];
    bool fok[NV], first[NV];   // first: the piece opens its head, so its lane stores the head's (m, l) and lse
#pragma unroll
    for (int v = 0; v < NV; v++) {
        f[v] = ((blockIdx.y * NV + v) * L + li) * VEC;
        fok[v] = f[v] < h;
        hv[v] = fok[v] ? f[v] / hd : 0u;
        first[v] = fok[v] && f[v] == hv[v] * hd;
    }
    uint32_t row_cur = sd_row_of(rowptr, 0, nrows, (uint32_t)e_begin);
    const uint32_t row_hi = sd_row_of(rowptr, row_cur, nrows, e_end - 1) + 1;
    bool head_open = rowptr[row_cur] < (uint32_t)e_begin;   // the first row of the run began in an earlier run
    bool pending = false;
    T acc[NV][VEC], m[NV], l[NV];
    const uint64_t slots = wave * 2 * (uint64_t)h;   // the run's two accumulator slots, in elements
    const auto reset = [&]() {
#pragma unroll
        for (int v = 0; v < NV; v++) {
            m[v] = es_lowest<T>();
            l[v] = T(0);
#pragma unroll
            for (int i = 0; i < VEC; i++) acc[v][i] = T(0);
        }
    };
    // join the lane groups, then store: the raw partial into the workspace slot, or the finished row `row` into out / lse
    const auto flush = [&](bool to_slot, uint32_t slot, uint32_t row) {
#pragma unroll
        for (int v = 0; v < NV; v++) {
            if constexpr (!WHOLE) {
                for (uint32_t s = L; s < 64; s <<= 1) {
                    const T m2 = rg_shfl_xor(m[v], (int)s), l2 = rg_shfl_xor(l[v], (int)s);
                    T M, a, b;
                    gat_scales(m[v], m2, M, a, b);
                    l[v] = l[v] * a + l2 * b;
                    m[v] = M;
#pragma unroll
                    for (int i = 0; i < VEC; i++) acc[v][i] = acc[v][i] * a + rg_shfl_xor(acc[v][i], (int)s) * b;
                }
            }
            if (grp == 0 && fok[v]) {
                if (to_slot) {
                    rg_store<T, T, VEC>(ws + slots + (slot ? h : 0u) + f[v], acc[v]);
                    if (first[v]) {
                        T *st = ws_stat + ((wave * 2 + slot) * heads + hv[v]) * 2;
                        st[0] = m[v];
                        st[1] = l[v];
                    }
                } else {
                    const T inv = T(1) / l[v];
#pragma unroll
                    for (int i = 0; i < VEC; i++) acc[v][i] = acc[v][i] * inv;
                    rg_store<S, T, VEC>(out + (uint64_t)row * ldo + f[v], acc[v]);
                    if (lse && first[v]) lse[(uint64_t)row * heads + hv[v]] = m[v] + gat_log(l[v]);
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
            const uint64_t em = endmask >> pos;
            const bool closes = em != 0;
            const uint32_t last = closes ? pos + (uint32_t)__builtin_ctzll(em) : n - 1;
            const uint32_t row = rg_take32<true>(my_row, last);   // the row of the entries pos .. last
            T ad[NV];
#pragma unroll
            for (int v = 0; v < NV; v++) ad[v] = fok[v] ? a_dst[(uint64_t)row * heads + hv[v]] : T(0);
            for (uint32_t k0 = pos; k0 <= last; k0 += R * U) {
                V x[U][NV];
                T s[U][NV];
                T ae[EDGE ? U : 1][NV];   // EDGE: the entry's term, loaded beside its row
                bool ok[U];
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const uint32_t kk = k0 + (uint32_t)u * R + grp;
                    ok[u] = kk <= last;
                    const uint32_t col = rg_take32<WHOLE>(my_col, ok[u] ? kk : pos);
                    const S *xr = X + (uint64_t)col * ldx;
                    const T *ar = a_src + (uint64_t)col * heads;
#pragma unroll
                    for (int v = 0; v < NV; v++) {
                        x[u][v] = V(0);
                        s[u][v] = es_lowest<T>();   // an entry slot that is not in flight: never above M
                        if constexpr (EDGE) ae[u][v] = T(0);
                        if (ok[u] && fok[v]) {
                            x[u][v] = *(const V *)(xr + f[v]);
                            s[u][v] = ar[hv[v]];
                            if constexpr (EDGE) ae[u][v] = a_edge[(uint64_t)(base + kk) * heads + hv[v]];
                        }
                    }
                }
#pragma unroll
                for (int v = 0; v < NV; v++) {
                    T M = m[v];
#pragma unroll
                    for (int u = 0; u < U; u++) {
                        if (ok[u] && fok[v]) {
                            T z = ad[v] + s[u][v];
                            if constexpr (EDGE) z = z + ae[u][v];
                            s[u][v] = z >= T(0) ? z : slope * z;
                        }
                        M = s[u][v] > M ? s[u][v] : M;
                    }
                    const T c = m[v] == M ? T(1) : es_exp(m[v] - M);
                    m[v] = M;
                    l[v] = l[v] * c;
#pragma unroll
                    for (int i = 0; i < VEC; i++) acc[v][i] = acc[v][i] * c;
#pragma unroll
                    for (int u = 0; u < U; u++)
                        if (ok[u] && fok[v]) {
                            T p = es_exp(s[u][v] - M);
                            l[v] = l[v] + p;
                            if constexpr (DROP)
                                p = attn_dropout_keep(base + k0 + (uint32_t)u * R + grp, hv[v], dr.seed_lo, dr.seed_hi, dr.thr) ? p * dr.keep_w : T(0);
#pragma unroll
                            for (int i = 0; i < VEC; i++) acc[v][i] = acc[v][i] + p * T(rg_get<S, VEC>(x[u][v], i));
                        }
                }
            }
            if (closes) {
                flush(head_open, 0u, row);
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

// one wave per run: the row that goes on after run w = slot 1 of w merged with slot 0 of every later run the row reaches, in order,
// then divided by its l
template <typename T, typename S>
__global__ __launch_bounds__(256) void k_gat_fixup(const uint32_t *__restrict__ rowptr, uint32_t nrows, uint32_t nnz, uint32_t h, uint32_t heads,
                                                   const T *__restrict__ ws, const T *__restrict__ ws_stat, S *__restrict__ out, uint64_t ldo,
                                                   T *__restrict__ lse) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t w = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    uint32_t row, rb, re;
    uint64_t w1;
    if (!rg_cut_row(rowptr, nrows, nnz, w, row, rb, re, w1)) return;
    const uint32_t hd = h / heads;
    for (uint32_t f = lane; f < h; f += 64) {
        const uint32_t k = f / hd;
        const T *st = ws_stat + ((w * 2 + 1) * heads + k) * 2;
        T m = st[0], l = st[1], acc = ws[(w * 2 + 1) * (uint64_t)h + f];
        for (uint64_t j = w + 1; j <= w1; j++) {
            st = ws_stat + (j * 2 * heads + k) * 2;
            T M, a, b;
            gat_scales(m, st[0], M, a, b);
            l = l * a + st[1] * b;
            acc = acc * a + ws[j * 2 * (uint64_t)h + f] * b;
            m = M;
        }
        out[(uint64_t)row * ldo + f] = S(acc * (T(1) / l));
        if (lse && f == k * hd) lse[(uint64_t)row * heads + k] = m + gat_log(l);
    }
}

// rows without entries: out = 0, lse = 0
template <typename T, typename S>
__global__ __launch_bounds__(256) void k_gat_empty(const uint32_t *__restrict__ rowptr, uint32_t nrows, uint32_t h, uint32_t heads, S *__restrict__ out,
                                                   uint64_t ldo, T *__restrict__ lse) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t row = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= nrows || rowptr[row] != rowptr[row + 1]) return;
    for (uint32_t f = lane; f < h; f += 64) out[row * ldo + f] = S(0);
    if (lse)
        for (uint32_t k = lane; k < heads; k += 64) lse[row * heads + k] = T(0);
}

template <typename T, typename S, int VEC, bool DROP, bool EDGE>
inline void launch_gat_gather_v(const uint32_t *rowptr, const uint32_t *colind, uint32_t nrows, uint32_t nnz, const T *a_dst, const T *a_src, uint32_t heads,
                                T slope, const S *X, uint64_t ldx, uint32_t h, S *out, uint64_t ldo, T *lse, T *ws, T *ws_stat, const LaunchShape &g,
                                const AttnDrop<T> &dr, const T *a_edge, hipStream_t st) {
    rg_dispatch(nnz, g, [&](auto nv, auto whole, dim3 grid, uint32_t L) {
        hipLaunchKernelGGL((k_gat_gather<T, S, VEC, decltype(nv)::value, decltype(whole)::value, DROP, EDGE>), grid, dim3(256), 0, st, rowptr, colind, nrows, nnz,
                           a_dst, a_src, heads, slope, X, ldx, h, L, out, ldo, lse, ws, ws_stat, dr, a_edge);
    });
}

// 16-byte pieces (of the storage type) under the conditions of launch_row_gather: aligned rows of X and out, and no piece across two heads
// DROP: with attention dropout of (rate, seed) = dr; without it dr is not read.  EDGE: with the per-entry term a_edge [nnz, heads]; without it
// a_edge is not read
template <typename T, typename S = T, bool DROP = false, bool EDGE = false>
inline void launch_gat_aggregate(const uint32_t *rowptr, const uint32_t *colind, uint32_t nrows, uint32_t nnz, const T *a_dst, const T *a_src, uint32_t heads,
                                 T slope, const S *X, uint64_t ldx, uint32_t h, S *out, uint64_t ldo, T *lse, void *workspace, hipStream_t st,
                                 const AttnDrop<T> &dr = AttnDrop<T>(), const T *a_edge = nullptr) {
    constexpr uint32_t V = 16 / sizeof(S);
    if (nrows > 0) hipLaunchKernelGGL((k_gat_empty<T, S>), dim3((nrows + 3) / 4), dim3(256), 0, st, rowptr, nrows, h, heads, out, ldo, lse);
    if (nnz == 0) return;
    T *ws = (T *)workspace;
    T *ws_stat = (T *)((char *)workspace + gat_stat_offset(nnz, h, sizeof(T)));
    const bool aligned = ldx % V == 0 && ldo % V == 0 && (uintptr_t)X % 16 == 0 && (uintptr_t)out % 16 == 0 && (uintptr_t)ws % 16 == 0;
    const LaunchShape g = row_gather_shape(h, h / heads, V, aligned);   // the walker's layout
    if (g.vec > 1) launch_gat_gather_v<T, S, (int)V, DROP, EDGE>(rowptr, colind, nrows, nnz, a_dst, a_src, heads, slope, X, ldx, h, out, ldo, lse, ws, ws_stat, g, dr, a_edge, st);
    else launch_gat_gather_v<T, S, 1, DROP, EDGE>(rowptr, colind, nrows, nnz, a_dst, a_src, heads, slope, X, ldx, h, out, ldo, lse, ws, ws_stat, g, dr, a_edge, st);
    const uint64_t runs = row_gather_runs(nnz);
    if (runs > 1)
        hipLaunchKernelGGL((k_gat_fixup<T, S>), dim3((unsigned)((runs + 2) / 4)), dim3(256), 0, st, rowptr, nrows, nnz, h, heads, ws, ws_stat, out, ldo, lse);
}

}  // namespace pygim
