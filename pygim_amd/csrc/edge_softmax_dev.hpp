// edge_softmax_dev.hpp -- the softmax of per-entry scores over the stored entries of every row of a CSR, per head, and its backward:
//   forward   out[e, k] = exp(s[e, k] - m) / sum_{e' in row} exp(s[e', k] - m),   m = the row's and head's maximum
//   backward  out[e, k] = P[e, k] * (dP[e, k] - sum_{e' in row} P[e', k] * dP[e', k])
// Both are one reduction per (row, head) followed by an element-wise map, streamed over [nnz, heads]; ES_MODE says which.
//
// Shape:
//   * a wave owns ES_EPW consecutive entries and walks them in batches of 64, a lane per entry, the heads of an entry side by side in
//     the lane (16 bytes at a time when heads allows it);
//   * the reduction is a segmented scan over the 64 lanes (six shuffles, a lane joins its neighbour's partial when both lie in the same
//     row) and one more shuffle that fetches the total from the segment's last lane.  A row that lies wholly inside a batch is read
//     once, kept in registers and written once (k_es_batch);
//   * a row that crosses a batch boundary leaves one partial per batch in the workspace -- (maximum, sum of exp) or the plain sum; at
//     most two per batch: slot 0 for the row that began before the batch, slot 1 for the row that goes on after it -- k_es_combine folds
//     the partials of a row in a fixed tree and writes the row's totals back over them, and k_es_finish reads the entries of those rows a
//     second time and maps them.
// No atomics; the shape of every reduction depends on the CSR alone: the same bits on every launch.
//
// Workspace: per batch 2 slots x heads x 2 elements, then one uint32 per batch (the end of the row that goes on after it, or 0).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "sddmm_dev.hpp"

namespace pygim {

constexpr uint32_t ES_EPW = 1024;   // entries per wave (16 batches of 64)

enum { ES_FORWARD = 0, ES_BACKWARD = 1 };

__device__ inline float es_exp(float x) { return expf(x); }
__device__ inline double es_exp(double x) { return exp(x); }
template <typename T> __device__ inline T es_neg_inf() { return -__builtin_huge_val(); }
template <> __device__ inline float es_neg_inf<float>() { return -__builtin_huge_valf(); }
// what is subtracted from the scores under a maximum m: m itself, or 0 when every score so far is -inf (masked), so that such a score
// gives exp(-inf - 0) = 0 and never exp(-inf - -inf) = NaN.  The partial of an all-masked stretch is then the neutral (-inf, 0).
template <typename T> __device__ inline T es_shift(T m) { return m == es_neg_inf<T>() ? T(0) : m; }
// where the running maximum of an online softmax starts (k_gat_gather and its siblings): the lowest FINITE number, not -inf.  No score
// but -inf lies below it, so it changes no maximum; entries that are all -inf (masked) leave M there and give p = exp(-inf - M) = 0
// instead of exp(-inf - -inf) = NaN, with no select in the scan.  (lowest, 0, 0) is neutral in gat_scales like (-inf, 0, 0): against a
// larger maximum it scales by exp(lowest - M) = 0, against itself by exactly 1.  A (row, head) of nothing but -inf ends as (lowest, 0, 0):
// out = 0 * (1 / 0) = NaN, lse = lowest + log(0) = -inf.
template <typename T> __device__ inline T es_lowest() { return -__DBL_MAX__; }
template <> __device__ inline float es_lowest<float>() { return -__FLT_MAX__; }

inline uint64_t edge_softmax_batches(uint64_t nnz) { return (nnz + 63) / 64; }
inline uint64_t edge_softmax_workspace_bytes(uint64_t nnz, uint64_t heads, size_t elem) {
    const uint64_t nb = edge_softmax_batches(nnz);
    return (nb * 4 * heads * elem + 15) / 16 * 16 + nb * 4;
}

// two partials (maximum, sum of exp(. - maximum)) of one row into one; (-inf, 0) is the neutral element
template <typename T> __device__ inline void es_merge(T &m, T &s, T m2, T s2) {
    const T M = m > m2 ? m : m2;
    const T a = m == M ? T(1) : es_exp(m - M);
    const T b = m2 == M ? T(1) : es_exp(m2 - M);
    s = s * a + s2 * b;
    m = M;
}

// inclusive segmented scan over the wave's lanes (a lane takes part with the `ds` lanes before it), then the segment's total from its last lane
template <typename T, bool MAX> __device__ inline T es_segment_total(T v, uint32_t lane, uint32_t ds, uint32_t de) {
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const T o = __shfl_up(v, d, 64);
        if (d <= ds) v = MAX ? (v > o ? v : o) : v + o;
    }
    return __shfl(v, (int)(lane + de), 64);
}

// what a lane knows about its entry's row inside the batch [base, base + n)
struct EsLane {
    uint32_t ds, de;      // lanes of the same row before / after this one inside the batch
    bool head, tail;      // the row began before the batch / goes on after it
    uint32_t row_end;     // rowptr[row + 1]
};

__device__ inline EsLane es_lane(const uint32_t *__restrict__ rowptr, uint32_t row_lo, uint32_t row_hi, uint32_t base, uint32_t n, uint32_t lane,
                                 uint32_t &my_row) {
    EsLane r = {0u, 0u, false, false, 0u};
    my_row = row_lo;
    if (lane < n) {
        const uint32_t e = base + lane;
        my_row = sd_row_of(rowptr, row_lo, row_hi, e);
        const uint32_t rs = rowptr[my_row], re = rowptr[my_row + 1];
        r.head = rs < base;
        r.tail = re > base + n;
        r.ds = e - (r.head ? base : rs);
        r.de = (r.tail ? base + n : re) - 1 - e;
        r.row_end = re;
    }
    return r;
}

// MODE forward: a = scores; backward: a = P, b = dP.  HV heads per step (a 16-byte piece, or 1).
// FINISH false: rows inside a batch are mapped and written, rows across batches leave their partials.
// FINISH true : only the entries of rows across batches, mapped with the row's totals k_es_combine left in the slots.
template <typename T, int HV, int MODE, bool FINISH>
__global__ __launch_bounds__(256) void k_es_batch(const uint32_t *__restrict__ rowptr, uint32_t nrows, uint32_t nnz, const T *__restrict__ a,
                                                  const T *__restrict__ b, uint32_t heads, T *__restrict__ out, T *__restrict__ ws,
                                                  uint32_t *__restrict__ tail_end) {
    using V = typename SdVec<T, HV>::type;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint64_t e_begin = wave * ES_EPW;
    if (e_begin >= nnz) return;
    const uint32_t e_end = (uint32_t)(e_begin + ES_EPW < nnz ? e_begin + ES_EPW : nnz);
    uint32_t row_cur = sd_row_of(rowptr, 0, nrows, (uint32_t)e_begin);
    const uint32_t row_hi = sd_row_of(rowptr, row_cur, nrows, e_end - 1) + 1;
    for (uint32_t base = (uint32_t)e_begin; base < e_end; base += 64) {
        const uint32_t n = (base + 64 < e_end ? base + 64 : e_end) - base;
        const uint64_t batch = base / 64;
        uint32_t my_row;
        const EsLane q = es_lane(rowptr, row_cur, row_hi, base, n, lane, my_row);
        row_cur = (uint32_t)__builtin_amdgcn_readlane((int)my_row, (int)(n - 1));
        const bool valid = lane < n;
        const bool across = q.head || q.tail;
        T *slot = ws + (batch * 2 + (q.head ? 0 : 1)) * 2 * (uint64_t)heads;
        if constexpr (!FINISH) {
            if (lane == n - 1) tail_end[batch] = (q.tail && !q.head) ? q.row_end : 0u;
        } else {
            if (__ballot(valid && across) == 0) continue;
        }
        const uint64_t at = (uint64_t)(base + lane) * heads;
        for (uint32_t k0 = 0; k0 < heads; k0 += HV) {
            T x[HV], y[HV];
#pragma unroll
            for (int i = 0; i < HV; i++) {
                x[i] = MODE == ES_FORWARD ? es_neg_inf<T>() : T(0);
                y[i] = T(0);
            }
            if (valid && (!FINISH || across)) {
                const V xv = *(const V *)(a + at + k0);
                if constexpr (HV == 1) x[0] = xv;
                else
#pragma unroll
                    for (int i = 0; i < HV; i++) x[i] = xv[i];
                if constexpr (MODE == ES_BACKWARD) {
                    const V yv = *(const V *)(b + at + k0);
                    if constexpr (HV == 1) y[0] = yv;
                    else
#pragma unroll
                        for (int i = 0; i < HV; i++) y[i] = yv[i];
                }
            }
            T res[HV];
#pragma unroll
            for (int i = 0; i < HV; i++) {
                T m = T(0), s = T(1);
                if constexpr (FINISH) {
                    if (valid && across) {
                        m = slot[(k0 + i) * 2];
                        s = slot[(k0 + i) * 2 + 1];
                    } else {
                        s = T(1);
                    }
                } else {
                    if constexpr (MODE == ES_FORWARD) {
                        m = es_segment_total<T, true>(x[i], lane, q.ds, q.de);
                        s = es_segment_total<T, false>(valid ? es_exp(x[i] - es_shift(m)) : T(0), lane, q.ds, q.de);
                    } else {
                        s = es_segment_total<T, false>(x[i] * y[i], lane, q.ds, q.de);
                    }
                    if (valid && across && q.de == 0) {   // the segment's last lane parks the partial
                        slot[(k0 + i) * 2] = m;
                        slot[(k0 + i) * 2 + 1] = s;
                    }
                }
                if constexpr (MODE == ES_FORWARD) res[i] = es_exp(x[i] - es_shift(m)) / s;
                else res[i] = x[i] * (y[i] - s);
            }
            if (valid && (FINISH ? across : !across)) {
                V rv;
                if constexpr (HV == 1) rv = res[0];
                else
#pragma unroll
                    for (int i = 0; i < HV; i++) rv[i] = res[i];
                *(V *)(out + at + k0) = rv;
            }
        }
    }
}

// one wave per batch: the row that goes on after batch w = slot 1 of w and slot 0 of the batches up to the row's last; every lane folds the
// partials l, l + 64, ... in order, a fixed xor tree folds the lanes, and the row's totals go back into every one of those slots
template <typename T, int MODE>
__global__ __launch_bounds__(256) void k_es_combine(uint64_t nbatches, uint32_t heads, T *__restrict__ ws, const uint32_t *__restrict__ tail_end) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t w = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= nbatches) return;
    const uint32_t re = tail_end[w];
    if (re == 0) return;
    const uint64_t w1 = (re - 1) / 64;
    const uint64_t count = w1 - w + 1;
    for (uint32_t k = 0; k < heads; k++) {
        T m = MODE == ES_FORWARD ? es_neg_inf<T>() : T(0), s = T(0);
        for (uint64_t j = lane; j < count; j += 64) {
            const T *slot = ws + ((w + j) * 2 + (j == 0 ? 1 : 0)) * 2 * (uint64_t)heads + (uint64_t)k * 2;
            if constexpr (MODE == ES_FORWARD) es_merge(m, s, slot[0], slot[1]);
            else s += slot[1];
        }
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const T m2 = __shfl_xor(m, d, 64), s2 = __shfl_xor(s, d, 64);
            if constexpr (MODE == ES_FORWARD) {
                // both partners must fold in the same order to hold the same bits: the lower lane's partial first
                if (lane & (uint32_t)d) {
                    T mm = m2, ss = s2;
                    es_merge(mm, ss, m, s);
                    m = mm;
                    s = ss;
                } else {
                    es_merge(m, s, m2, s2);
                }
            } else {
                s = (lane & (uint32_t)d) ? s2 + s : s + s2;
            }
        }
        for (uint64_t j = lane; j < count; j += 64) {
            T *slot = ws + ((w + j) * 2 + (j == 0 ? 1 : 0)) * 2 * (uint64_t)heads + (uint64_t)k * 2;
            slot[0] = m;
            slot[1] = s;
        }
    }
}

// k_es_batch: a lane per entry, the entry's heads in steps of a 16-byte piece when `heads` fills whole pieces (every entry's heads then
// start 16-byte aligned when the arrays do) and a, b and out are aligned; else one head per step
inline LaunchShape edge_softmax_shape(uint32_t heads, uint32_t V, bool aligned) {
    LaunchShape g = launch_shape_piece(heads, V, aligned);
    g.chunks = heads / g.vec;   // steps of the loop over the heads
    return g;
}

template <typename T, int MODE>
inline void launch_edge_softmax(const uint32_t *rowptr, uint32_t nrows, uint32_t nnz, const T *a, const T *b, uint32_t heads, T *out, void *workspace,
                                hipStream_t st) {
    constexpr uint32_t V = 16 / sizeof(T);
    const uint64_t nb = edge_softmax_batches(nnz);
    T *ws = (T *)workspace;
    uint32_t *tail_end = (uint32_t *)((char *)workspace + (nb * 4 * heads * sizeof(T) + 15) / 16 * 16);
    const unsigned blocks = (unsigned)((((uint64_t)nnz + ES_EPW - 1) / ES_EPW + 3) / 4);
    const bool vec = edge_softmax_shape(heads, V, (uintptr_t)a % 16 == 0 && (uintptr_t)out % 16 == 0 && (MODE == ES_FORWARD || (uintptr_t)b % 16 == 0)).vec > 1;
    if (vec) hipLaunchKernelGGL((k_es_batch<T, (int)V, MODE, false>), dim3(blocks), dim3(256), 0, st, rowptr, nrows, nnz, a, b, heads, out, ws, tail_end);
    else hipLaunchKernelGGL((k_es_batch<T, 1, MODE, false>), dim3(blocks), dim3(256), 0, st, rowptr, nrows, nnz, a, b, heads, out, ws, tail_end);
    if (nb <= 1) return;
    hipLaunchKernelGGL((k_es_combine<T, MODE>), dim3((unsigned)((nb + 3) / 4)), dim3(256), 0, st, nb, heads, ws, tail_end);
    if (vec) hipLaunchKernelGGL((k_es_batch<T, (int)V, MODE, true>), dim3(blocks), dim3(256), 0, st, rowptr, nrows, nnz, a, b, heads, out, ws, tail_end);
    else hipLaunchKernelGGL((k_es_batch<T, 1, MODE, true>), dim3(blocks), dim3(256), 0, st, rowptr, nrows, nnz, a, b, heads, out, ws, tail_end);
}

}  // namespace pygim
