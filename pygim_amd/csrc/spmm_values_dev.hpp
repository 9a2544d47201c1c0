// spmm_values_dev.hpp -- a row-wise product on a caller's CSR whose edge values are an operand of the call:
//   out[r, f] = sum over the stored entries e of row r of values[e * heads + f / (h / heads)] * X[colind[e], f]
// (the aggregation of an attention layer: the values change on every call, so nothing about them can be compiled into a group).
//
// Shape (the gather of k_sddmm, with a sum per row instead of a dot product per entry):
//   * a wave owns SV_EPW consecutive entries, whatever rows they belong to (a hub row is cut across waves, a run of short rows shares
//     one), and walks them in batches of 64: one coalesced load of the batch's column ids (and values, with one head), one search of
//     every lane's row inside the rows of the wave's run, one ballot of the lanes that end a row;
//   * lanes lie across the features, 16 bytes each when h, the strides and the pointers allow it (h = 256 FLT32: one 1 KiB
//     wave-instruction per X row); rows narrower than a wave are taken by 64 / L lane groups side by side on different entries of the
//     same row, and their sums meet in a fixed xor tree when the row ends; wider rows go over blockIdx.y in chunks;
//   * the gathers of up to SV_U entries are issued back to back before the first product is added;
//   * a row that lies wholly inside the wave's run is stored directly.  The at most two rows a run shares with its neighbours (the one
//     that began before it -- slot 0 -- and the one that goes on after it -- slot 1) leave their partial sums in the workspace, and
//     k_sv_fixup adds them per row in the order of the runs.  Empty rows are zeroed by k_sv_empty.  No two kernels write the same row.
// No atomics; every sum has a fixed order (entry order inside a run, then the runs in order): the same bits on every launch.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "sddmm_dev.hpp"

namespace pygim {

constexpr uint32_t SV_EPW = 512;   // entries per wave (8 batches of 64)
constexpr int SV_U = 8;            // 16-byte gathers in flight per lane

// the value lane `src` holds (src wave-uniform when WHOLE: a readlane; else a per-lane shuffle)
template <bool WHOLE> __device__ inline uint32_t sv_take32(uint32_t v, uint32_t src) {
    if constexpr (WHOLE) return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)__builtin_amdgcn_readfirstlane((int)src));
    else return (uint32_t)__shfl((int)v, (int)(src & 63u), 64);
}
template <bool WHOLE> __device__ inline float sv_take(float v, uint32_t src) { return __uint_as_float(sv_take32<WHOLE>(__float_as_uint(v), src)); }
template <bool WHOLE> __device__ inline double sv_take(double v, uint32_t src) {
    const uint64_t b = (uint64_t)__double_as_longlong(v);
    const uint64_t r = (uint64_t)sv_take32<WHOLE>((uint32_t)b, src) | ((uint64_t)sv_take32<WHOLE>((uint32_t)(b >> 32), src) << 32);
    return __longlong_as_double((long long)r);
}

template <typename T, int VEC> __device__ inline typename SdVec<T, VEC>::type sv_zero() {
    if constexpr (VEC == 1) return T(0);
    else {
        typename SdVec<T, VEC>::type z;
#pragma unroll
        for (int i = 0; i < VEC; i++) z[i] = T(0);
        return z;
    }
}

template <typename T, int VEC> __device__ inline typename SdVec<T, VEC>::type sv_xor(const typename SdVec<T, VEC>::type &a, int mask) {
    if constexpr (VEC == 1) return __shfl_xor(a, mask, 64);
    else {
        typename SdVec<T, VEC>::type r;
#pragma unroll
        for (int i = 0; i < VEC; i++) r[i] = __shfl_xor(a[i], mask, 64);
        return r;
    }
}

// WHOLE: the wave is one lane group (L = 64) that holds NV pieces of VEC features per lane; else NV = 1 and L < 64 is a launch argument
template <typename T, int VEC, int NV, bool WHOLE>
__global__ __launch_bounds__(256) void k_spmm_values(const uint32_t *__restrict__ rowptr, const uint32_t *__restrict__ colind, uint32_t nrows,
                                                     uint32_t nnz, const T *__restrict__ values, uint32_t heads, const T *__restrict__ X, uint64_t ldx,
                                                     uint32_t h, uint32_t L, T *__restrict__ out, uint64_t ldo, T *__restrict__ ws) {
    using V = typename SdVec<T, VEC>::type;
    constexpr int U = NV == 1 ? SV_U : SV_U / 2;
    if constexpr (WHOLE) L = 64;
    const uint32_t R = 64 / L;
    const uint32_t lane = threadIdx.x & 63, grp = lane / L, li = lane % L;
    const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint64_t e_begin = wave * SV_EPW;
    if (e_begin >= nnz) return;
    const uint32_t e_end = (uint32_t)(e_begin + SV_EPW < nnz ? e_begin + SV_EPW : nnz);
    const uint32_t hd = h / heads;
    uint32_t f[NV], hv[NV];
    bool fok[NV];
#pragma unroll
    for (int v = 0; v < NV; v++) {
        f[v] = ((blockIdx.y * NV + v) * L + li) * VEC;
        fok[v] = f[v] < h;
        hv[v] = fok[v] ? f[v] / hd : 0u;
    }
    const bool one_head = heads == 1;
    uint32_t row_cur = sd_row_of(rowptr, 0, nrows, (uint32_t)e_begin);
    const uint32_t row_hi = sd_row_of(rowptr, row_cur, nrows, e_end - 1) + 1;
    bool head_open = rowptr[row_cur] < (uint32_t)e_begin;   // the first row of the run began in an earlier run
    bool pending = false;
    V acc[NV];
#pragma unroll
    for (int v = 0; v < NV; v++) acc[v] = sv_zero<T, VEC>();
    T *slots = ws + wave * 2 * (uint64_t)h;

    for (uint32_t base = (uint32_t)e_begin; base < e_end; base += 64) {
        const uint32_t n = (base + 64 < e_end ? base + 64 : e_end) - base;
        const uint32_t my_e = base + lane;
        const bool valid = lane < n;
        const uint32_t my_col = valid ? colind[my_e] : 0u;
        const T my_val = (valid && one_head) ? values[my_e] : T(0);
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
                T w[U][NV];
                bool ok[U];
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const uint32_t kk = k0 + (uint32_t)u * R + grp;
                    ok[u] = kk <= last;
                    const uint32_t col = sv_take32<WHOLE>(my_col, ok[u] ? kk : pos);
                    const T wv = sv_take<WHOLE>(my_val, ok[u] ? kk : pos);
                    const T *xr = X + (uint64_t)col * ldx;
#pragma unroll
                    for (int v = 0; v < NV; v++) {
                        x[u][v] = sv_zero<T, VEC>();
                        w[u][v] = wv;
                        if (ok[u] && fok[v]) {
                            x[u][v] = *(const V *)(xr + f[v]);
                            if (!one_head) w[u][v] = values[(uint64_t)(base + kk) * heads + hv[v]];
                        }
                    }
                }
#pragma unroll
                for (int u = 0; u < U; u++) {
#pragma unroll
                    for (int v = 0; v < NV; v++)
                        if (ok[u] && fok[v]) acc[v] += w[u][v] * x[u][v];
                }
            }
            if (closes) {
                const uint32_t row = sv_take32<true>(my_row, last);
                T *dst = head_open ? slots : out + (uint64_t)row * ldo;
#pragma unroll
                for (int v = 0; v < NV; v++) {
                    if constexpr (!WHOLE)
                        for (uint32_t s = L; s < 64; s <<= 1) acc[v] = acc[v] + sv_xor<T, VEC>(acc[v], (int)s);
                    if (grp == 0 && fok[v]) *(V *)(dst + f[v]) = acc[v];
                    acc[v] = sv_zero<T, VEC>();
                }
                head_open = false;
            }
            pending = !closes;
            pos = last + 1;
        }
        row_cur = sv_take32<true>(my_row, n - 1);
    }
    if (pending) {   // the run's last row goes on in the next run
        T *dst = slots + (head_open ? 0 : h);
#pragma unroll
        for (int v = 0; v < NV; v++) {
            if constexpr (!WHOLE)
                for (uint32_t s = L; s < 64; s <<= 1) acc[v] = acc[v] + sv_xor<T, VEC>(acc[v], (int)s);
            if (grp == 0 && fok[v]) *(V *)(dst + f[v]) = acc[v];
        }
    }
}

// one wave per run: the row that goes on after run w (slot 1 of w) = slot 1 of w + slot 0 of every later run the row reaches, in order
template <typename T>
__global__ __launch_bounds__(256) void k_sv_fixup(const uint32_t *__restrict__ rowptr, uint32_t nrows, uint32_t nnz, uint32_t h, const T *__restrict__ ws,
                                                  T *__restrict__ out, uint64_t ldo) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t w = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint64_t e_begin = w * SV_EPW;
    if (e_begin + SV_EPW >= nnz) return;   // the last run has no row that goes on
    const uint32_t e_end = (uint32_t)(e_begin + SV_EPW);
    const uint32_t row = sd_row_of(rowptr, 0, nrows, e_end - 1);
    const uint32_t re = rowptr[row + 1];
    if (re <= e_end || rowptr[row] < (uint32_t)e_begin) return;
    const uint64_t w1 = (re - 1) / SV_EPW;
    for (uint32_t f = lane; f < h; f += 64) {
        T s = ws[(w * 2 + 1) * (uint64_t)h + f];
        for (uint64_t j = w + 1; j <= w1; j++) s += ws[j * 2 * (uint64_t)h + f];
        out[(uint64_t)row * ldo + f] = s;
    }
}

// rows without entries: zero
template <typename T>
__global__ __launch_bounds__(256) void k_sv_empty(const uint32_t *__restrict__ rowptr, uint32_t nrows, uint32_t h, T *__restrict__ out, uint64_t ldo) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t row = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= nrows || rowptr[row] != rowptr[row + 1]) return;
    for (uint32_t f = lane; f < h; f += 64) out[row * ldo + f] = T(0);
}

inline uint64_t spmm_values_workspace_bytes(uint64_t nnz, uint64_t h, size_t elem) { return (nnz + SV_EPW - 1) / SV_EPW * 2 * h * elem; }

template <typename T, int VEC>
inline void launch_spmm_values_v(const uint32_t *rowptr, const uint32_t *colind, uint32_t nrows, uint32_t nnz, const T *values, uint32_t heads, const T *X,
                                 uint64_t ldx, uint32_t h, T *out, uint64_t ldo, T *ws, hipStream_t st) {
    const uint64_t waves = ((uint64_t)nnz + SV_EPW - 1) / SV_EPW;
    const unsigned blocks = (unsigned)((waves + 3) / 4);
    const uint32_t pieces = (h + VEC - 1) / VEC;
    if (pieces <= 32) {
        uint32_t L = 1;
        while (L < pieces) L <<= 1;
        hipLaunchKernelGGL((k_spmm_values<T, VEC, 1, false>), dim3(blocks), dim3(256), 0, st, rowptr, colind, nrows, nnz, values, heads, X, ldx, h, L, out,
                           ldo, ws);
    } else if (pieces <= 64) {
        hipLaunchKernelGGL((k_spmm_values<T, VEC, 1, true>), dim3(blocks), dim3(256), 0, st, rowptr, colind, nrows, nnz, values, heads, X, ldx, h, 64u, out,
                           ldo, ws);
    } else {   // two pieces per lane, the rest of a wider row over blockIdx.y
        hipLaunchKernelGGL((k_spmm_values<T, VEC, 2, true>), dim3(blocks, (pieces + 127) / 128), dim3(256), 0, st, rowptr, colind, nrows, nnz, values, heads,
                           X, ldx, h, 64u, out, ldo, ws);
    }
}

// 16-byte pieces when every row of X and out starts 16-byte aligned, h fills whole pieces and no piece lies across two heads
template <typename T>
inline void launch_spmm_values(const uint32_t *rowptr, const uint32_t *colind, uint32_t nrows, uint32_t nnz, const T *values, uint32_t heads, const T *X,
                               uint64_t ldx, uint32_t h, T *out, uint64_t ldo, T *ws, hipStream_t st) {
    constexpr uint32_t V = 16 / sizeof(T);
    if (nrows > 0) hipLaunchKernelGGL((k_sv_empty<T>), dim3((nrows + 3) / 4), dim3(256), 0, st, rowptr, nrows, h, out, ldo);
    if (nnz == 0) return;
    const bool vec = (h / heads) % V == 0 && ldx % V == 0 && ldo % V == 0 && (uintptr_t)X % 16 == 0 && (uintptr_t)out % 16 == 0 && (uintptr_t)ws % 16 == 0;
    if (vec) launch_spmm_values_v<T, (int)V>(rowptr, colind, nrows, nnz, values, heads, X, ldx, h, out, ldo, ws, st);
    else launch_spmm_values_v<T, 1>(rowptr, colind, nrows, nnz, values, heads, X, ldx, h, out, ldo, ws, st);
    const uint64_t waves = ((uint64_t)nnz + SV_EPW - 1) / SV_EPW;
    if (waves > 1) hipLaunchKernelGGL((k_sv_fixup<T>), dim3((unsigned)((waves + 2) / 4)), dim3(256), 0, st, rowptr, nrows, nnz, h, ws, out, ldo);
}

}  // namespace pygim
