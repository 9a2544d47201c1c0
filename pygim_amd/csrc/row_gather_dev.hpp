// row_gather_dev.hpp -- the row-wise gather on a caller's CSR whose edge values are an operand of the call, written once:
//   out[r, f] = FOLD over the stored entries e of row r, in stored order, of w[e, f] * X[colind[e], f]
// and the sum fold on it (pygim_spmm_values: the aggregation of an attention layer, the values change on every call, so nothing
// about them can be compiled into a group):
//   out[r, f] = sum over e of values[e * heads + f / (h / heads)] * X[colind[e], f]
// Mean, max and min are the other folds (spmm_reduce_dev.hpp).
//
// Shape of k_row_gather (the gather of k_sddmm, with a fold per row instead of a dot product per entry):
//   * a wave owns RG_EPW consecutive entries, whatever rows they belong to (a hub row is cut across waves, a run of short rows shares
//     one), and walks them in batches of 64: one coalesced load of the batch's column ids (and weights, when there is one per entry),
//     one search of every lane's row inside the rows of the wave's run, one ballot of the lanes that end a row;
//   * lanes lie across the features, 16 bytes each when h, the strides and the pointers allow it (h = 256 FLT32: one 1 KiB
//     wave-instruction per X row); rows narrower than a wave are taken by 64 / L lane groups side by side on different entries of the
//     same row, and their partial results meet in a fixed xor tree when the row ends; wider rows go over blockIdx.y in chunks;
//   * the gathers of up to RG_U entries are issued back to back before the first product is folded;
//   * a row that lies wholly inside the wave's run is stored directly.  The at most two rows a run shares with its neighbours (the one
//     that began before it -- slot 0 -- and the one that goes on after it -- slot 1) leave their raw partial results in the workspace
//     (two slots of h elements per run; folds that carry an entry index have a second such array of int32 behind the first), and
//     k_row_gather_fixup joins them per row in the order of the runs.  Rows without entries are written by k_row_gather_empty.  No
//     two kernels write the same row.
// No atomics; every fold has a fixed order (entry order inside a run, the xor tree, then the runs in order): the same bits on every
// launch.
//
// What the siblings share with this file, and what they do not:
//   * rg_cut_row -- which row goes on after run w, and up to which run -- is the preamble of k_row_gather_fixup, k_gat_fixup
//     (gat_aggregate_dev.hpp), k_multi_fixup (spmm_multi_dev.hpp), k_softmax_fixup and k_softmax_grad_fixup (spmm_softmax_dev.hpp);
//     rg_dispatch is the host's choice between the three launch forms of row_gather_shape for launch_row_gather_v, launch_gat_gather_v,
//     launch_multi_gather_v, launch_softmax_gather_v and launch_softmax_grad_v.
//   * The walk inside the gather kernel -- batch loop, row search, ballot of row ends, cut into stretches, slot rule -- is still copied
//     text in k_gat_gather, k_multi_gather, k_sa_gather (sparse_attention_dev.hpp), k_gatv2_gather and k_gatv2_grad (gatv2_dev.hpp),
//     k_softmax_gather and k_softmax_grad (spmm_softmax_dev.hpp), k_edge_gather, k_edge_softmax_gather and k_edge_message_grad
//     (spmm_edge_dev.hpp): a change to the walk here has to be made in those ten as well.  One device function for it, taking the kernel's per-batch
//     load, its fold of a stretch and its row close as three lambdas, was written and measured (profiles/walker_refactor_resources.txt):
//     every call inlines and no form uses scratch, but a fold body that is optimised as a function of its own before it is inlined does
//     not come out as the same body written in the kernel, and in every form tried some instantiations lose a wave per SIMD (27 of
//     430 in the best one, k_row_gather and k_gat_gather among them).  Until a form keeps every instantiation's occupancy the
//     copies stay.
//
// A Fold says what the walker cannot know:
//   INDEXED   the partial result is a pair (value, index of the entry that holds it): aidx, the index slots and arg exist
//   PER_HEAD  values holds `heads` weights per entry and feature f takes weight f / (h / heads); else one weight per entry, 1 without values
//   MEAN      the finished row is divided by its number of stored entries, where it is stored into out and nowhere else
//   neutral() what a row starts from (with index RD_NONE)
//   join(a, ai, b, bi)  fold the pair (b, bi) into (a, ai): a product in the scan, a partner's partial in the xor tree, a slot in the fix-up
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "sddmm_dev.hpp"

namespace pygim {

constexpr uint32_t RG_EPW = 512;         // entries per wave (8 batches of 64)
constexpr int RG_U = 8;                  // 16-byte gathers in flight per lane
constexpr int32_t RD_NONE = 0x7FFFFFFF;  // "no entry yet": above every entry index (nnz <= 2^31 - 1); -1 in arg

template <int VEC> struct RdIdx { typedef int32_t __attribute__((ext_vector_type(VEC), aligned(4))) type; };
template <> struct RdIdx<1> { typedef int32_t type; };

// ---- lane exchange and piece access for the six element types ----
// the 32 bits lane `src` holds (src wave-uniform when WHOLE: a readlane; else a per-lane shuffle)
template <bool WHOLE> __device__ inline uint32_t rg_take32(uint32_t v, uint32_t src) {
    if constexpr (WHOLE) return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)__builtin_amdgcn_readfirstlane((int)src));
    else return (uint32_t)__shfl((int)v, (int)(src & 63u), 64);
}

// f applied to each 32-bit half of an element of 8 bytes, to the element widened to 32 bits otherwise
template <typename T, typename F> __device__ inline T rg_by_words(T v, F f) {
    if constexpr (sizeof(T) == 8) {
        uint64_t b;
        __builtin_memcpy(&b, &v, 8);
        b = (uint64_t)f((uint32_t)b) | ((uint64_t)f((uint32_t)(b >> 32)) << 32);
        __builtin_memcpy(&v, &b, 8);
        return v;
    } else if constexpr (std::is_floating_point<T>::value) {
        return __uint_as_float(f(__float_as_uint(v)));
    } else {
        return (T)(int32_t)f((uint32_t)(int32_t)v);
    }
}
template <bool WHOLE, typename T> __device__ inline T rg_take(T v, uint32_t src) {
    return rg_by_words(v, [&](uint32_t x) { return rg_take32<WHOLE>(x, src); });
}
template <typename T> __device__ inline T rg_shfl_xor(T v, int mask) {
    return rg_by_words(v, [&](uint32_t x) { return (uint32_t)__shfl_xor((int)x, mask, 64); });
}

template <typename T, int VEC> __device__ inline T rg_get(const typename SdVec<T, VEC>::type &v, int i) {
    if constexpr (VEC == 1) return v;
    else return v[i];
}

// VEC elements of the compute type T, stored as D: D = T (a workspace slot, or out when storage and compute type are one), or the
// 16-bit storage type of out -- the one place a result is rounded (round-to-nearest-even; v_cvt_pk_bf16_f32 / v_cvt_pk_f16_f32).
// A piece of 8 float32 partials is 32 bytes in a slot whose rows are 16-byte aligned: stored with that alignment.
template <typename D, int VEC> struct RgPiece { typedef D __attribute__((ext_vector_type(VEC), aligned(sizeof(D) * VEC < 16 ? sizeof(D) * VEC : 16))) type; };
template <typename D> struct RgPiece<D, 1> { typedef D type; };

template <typename D, typename T, int VEC> __device__ inline void rg_store(D *dst, const T *a) {
    typename SdVec<T, VEC>::type v;
    if constexpr (VEC == 1) v = a[0];
    else {
#pragma unroll
        for (int i = 0; i < VEC; i++) v[i] = a[i];
    }
    if constexpr (std::is_same<D, T>::value) *(typename RgPiece<T, VEC>::type *)dst = v;
    else if constexpr (VEC == 1) *dst = D(v);
    else *(typename RgPiece<D, VEC>::type *)dst = __builtin_convertvector(v, typename SdVec<D, VEC>::type);
}

// entry indices of VEC features; `final`: RD_NONE (no entry won) becomes -1
template <int VEC> __device__ inline void rg_store_idx(int32_t *dst, const int32_t *a, bool final) {
    typename RdIdx<VEC>::type v;
    if constexpr (VEC == 1) v = (final && a[0] == RD_NONE) ? -1 : a[0];
    else {
#pragma unroll
        for (int i = 0; i < VEC; i++) v[i] = (final && a[i] == RD_NONE) ? -1 : a[i];
    }
    *(typename RdIdx<VEC>::type *)dst = v;
}

// w * x; integers wrap like the type's own arithmetic (no signed overflow, no promotion past the type)
template <typename T> __device__ inline T rd_mul(T w, T x) {
    if constexpr (std::is_floating_point<T>::value) return w * x;
    else {
        using W = typename std::conditional<sizeof(T) <= 4, uint32_t, uint64_t>::type;
        return (T)((W)w * (W)x);
    }
}

// the sum (MEAN: divided by the row's number of stored entries -- duplicates count -- at the one place the row is stored)
template <bool MEAN_> struct FoldSum {
    static constexpr bool INDEXED = false, PER_HEAD = !MEAN_, MEAN = MEAN_;
    template <typename T> __device__ static T neutral() { return T(0); }
    template <typename T> __device__ static void join(T &a, int32_t &, T b, int32_t) { a = a + b; }
};

// WHOLE: the wave is one lane group (L = 64) that holds NV pieces of VEC features per lane; else NV = 1 and L < 64 is a launch argument.
// values (folds with one weight per entry), arg: may be null (unit weights; no index output).  ws_idx: the index half of the workspace.
// S is the storage type of X and out, T the type of everything else (values, accumulators, the xor tree, the slots).  S = T for the six
// element types; S = _Float16 / __bf16 with T = float for 16-bit features: an X piece is widened as it is folded (exact) and a finished
// row is rounded once, where it is stored into out.
template <typename T, typename S, int VEC, int NV, bool WHOLE, typename Fold>
__global__ __launch_bounds__(256) void k_row_gather(const uint32_t *__restrict__ rowptr, const uint32_t *__restrict__ colind, uint32_t nrows, uint32_t nnz,
                                                    const T *__restrict__ values, uint32_t heads, const S *__restrict__ X, uint64_t ldx, uint32_t h,
                                                    uint32_t L, S *__restrict__ out, uint64_t ldo, int32_t *__restrict__ arg, T *__restrict__ ws,
                                                    int32_t *__restrict__ ws_idx) {
    using V = typename SdVec<S, VEC>::type;
    constexpr int U = NV == 1 ? RG_U : RG_U / 2;
    constexpr int NW = Fold::PER_HEAD ? NV : 1;   // weights held per entry in flight
    if constexpr (WHOLE) L = 64;
    const uint32_t R = 64 / L;
    const uint32_t lane = threadIdx.x & 63, grp = lane / L, li = lane % L;
    const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint64_t e_begin = wave * RG_EPW;
    if (e_begin >= nnz) return;
    const uint32_t e_end = (uint32_t)(e_begin + RG_EPW < nnz ? e_begin + RG_EPW : nnz);
    const bool lane_w = !Fold::PER_HEAD || heads == 1;   // the weight of entry base + lane travels with its column id
    uint32_t f[NV], hv[NV];
    bool fok[NV];
#pragma unroll
    for (int v = 0; v < NV; v++) {
        f[v] = ((blockIdx.y * NV + v) * L + li) * VEC;
        fok[v] = f[v] < h;
        hv[v] = (Fold::PER_HEAD && fok[v]) ? f[v] / (h / heads) : 0u;
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
        // one destination when a slot and out hold the same type; else the slot (T) or the row of out (S, rounded by the store)
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
        const T my_val = (valid && values && lane_w) ? values[my_e] : T(1);
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
                T w[U][NW];
                bool ok[U];
                int32_t ei[U];
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const uint32_t kk = k0 + (uint32_t)u * R + grp;
                    ok[u] = kk <= last;
                    ei[u] = (int32_t)(base + kk);
                    const uint32_t col = rg_take32<WHOLE>(my_col, ok[u] ? kk : pos);
                    const T wv = rg_take<WHOLE, T>(my_val, ok[u] ? kk : pos);
                    const S *xr = X + (uint64_t)col * ldx;
#pragma unroll
                    for (int v = 0; v < NV; v++) {
                        x[u][v] = V(0);
                        if (v < NW) w[u][v] = wv;
                        if (ok[u] && fok[v]) {
                            x[u][v] = *(const V *)(xr + f[v]);
                            if constexpr (Fold::PER_HEAD)
                                if (!lane_w) w[u][v] = values[(uint64_t)(base + kk) * heads + hv[v]];
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
                                Fold::join(acc[v][i], aidx[v][i], rd_mul<T>(w[u][v < NW ? v : 0], T(rg_get<S, VEC>(x[u][v], i))), ei[u]);
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

// The fix-up's half of the slot rule, shared by k_row_gather_fixup, k_gat_fixup and k_multi_fixup: does a row go on after run w?  Then
// `row` is that row, [rb, re) its entries and w1 the last run it reaches: the row is slot 1 of run w joined with slot 0 of the runs
// w + 1 .. w1, in that order.  A row that began before run w is the business of the run it began in.
__device__ inline bool rg_cut_row(const uint32_t *__restrict__ rowptr, uint32_t nrows, uint32_t nnz, uint64_t w, uint32_t &row, uint32_t &rb, uint32_t &re,
                                  uint64_t &w1) {
    const uint64_t e_begin = w * RG_EPW;
    if (e_begin + RG_EPW >= nnz) return false;   // the last run has no row that goes on
    const uint32_t e_end = (uint32_t)(e_begin + RG_EPW);
    row = sd_row_of(rowptr, 0, nrows, e_end - 1);
    rb = rowptr[row];
    re = rowptr[row + 1];
    if (re <= e_end || rb < (uint32_t)e_begin) return false;
    w1 = (re - 1) / RG_EPW;
    return true;
}

// one wave per run: the row that goes on after run w = slot 1 of w joined with slot 0 of every later run the row reaches, in order
template <typename T, typename S, typename Fold>
__global__ __launch_bounds__(256) void k_row_gather_fixup(const uint32_t *__restrict__ rowptr, uint32_t nrows, uint32_t nnz, uint32_t h,
                                                          const T *__restrict__ ws, const int32_t *__restrict__ ws_idx, S *__restrict__ out, uint64_t ldo,
                                                          int32_t *__restrict__ arg) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t w = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    uint32_t row, rb, re;
    uint64_t w1;
    if (!rg_cut_row(rowptr, nrows, nnz, w, row, rb, re, w1)) return;
    for (uint32_t f = lane; f < h; f += 64) {
        uint64_t at = (w * 2 + 1) * (uint64_t)h + f;
        T s = ws[at];
        int32_t si = RD_NONE;
        if constexpr (Fold::INDEXED) si = ws_idx[at];
        for (uint64_t j = w + 1; j <= w1; j++) {
            at = j * 2 * (uint64_t)h + f;
            int32_t oi = RD_NONE;
            if constexpr (Fold::INDEXED) oi = ws_idx[at];
            Fold::join(s, si, ws[at], oi);
        }
        if constexpr (Fold::MEAN) s = s / T(re - rb);
        out[(uint64_t)row * ldo + f] = S(s);
        if constexpr (Fold::INDEXED)
            if (arg) arg[(uint64_t)row * h + f] = si == RD_NONE ? -1 : si;
    }
}

// rows without entries: 0, and -1 in arg
template <typename T>
__global__ __launch_bounds__(256) void k_row_gather_empty(const uint32_t *__restrict__ rowptr, uint32_t nrows, uint32_t h, T *__restrict__ out, uint64_t ldo,
                                                          int32_t *__restrict__ arg) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t row = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= nrows || rowptr[row] != rowptr[row + 1]) return;
    for (uint32_t f = lane; f < h; f += 64) {
        out[row * ldo + f] = T(0);
        if (arg) arg[row * h + f] = -1;
    }
}

// the workspace: two slots of h elements per run; the index slots of an INDEXED fold start behind them, rounded up to 16 bytes
inline uint64_t row_gather_runs(uint64_t nnz) { return (nnz + RG_EPW - 1) / RG_EPW; }
inline uint64_t row_gather_slot_bytes(uint64_t nnz, uint64_t h, size_t elem) { return row_gather_runs(nnz) * 2 * h * elem; }
inline uint64_t row_gather_index_offset(uint64_t nnz, uint64_t h, size_t elem) { return (row_gather_slot_bytes(nnz, h, elem) + 15) / 16 * 16; }

// One launch holds LS_MAX_CHUNKS chunks of 128 pieces: the widest row k_row_gather, k_gat_gather and k_spmm_reduce_bwd take on their
// one-element path.  The entry points (and their *_workspace functions) reject a wider h before any launch, whatever the alignment.
constexpr uint64_t RG_MAX_H = (uint64_t)LS_MAX_CHUNKS * 128;

// the lane layout of k_row_gather, k_gat_gather and k_spmm_reduce_bwd: up to `split` pieces a row is taken by L lanes side by side (a
// power of two; 64 / L entries per wave-instruction), up to 64 by the whole wave, beyond that by two pieces per lane and blockIdx.y chunks
// of 128 pieces.  width: what must fill whole pieces (h / heads: no piece lies across two heads).  h <= RG_MAX_H (the caller has checked).
inline LaunchShape row_gather_shape(uint32_t h, uint32_t width, uint32_t V, bool aligned, uint32_t split = 32) {
    LaunchShape g = launch_shape_piece(width, V, aligned);
    const uint32_t pieces = (h + g.vec - 1) / g.vec;
    if (pieces <= split) {
        while (g.L < pieces) g.L <<= 1;
    } else {
        g.L = 64;
        if (pieces > 64) {
            g.npl = 2;
            g.chunks = (pieces + 127) / 128;
        }
    }
    g.LH = g.L;
    if (pieces % g.L != 0) g.flags |= LS_PART_PIECE;
    if (g.chunks > 1 && pieces % 128 != 0) g.flags |= LS_PART_CHUNK;
    return g;
}

// the three launch forms of a row_gather_shape, for k_row_gather, k_gat_gather, k_multi_gather, k_softmax_gather and k_softmax_grad alike:
// launch(integral_constant<int, NV>, bool_constant<WHOLE>, grid, L) starts the kernel's <.., NV, WHOLE, ..> form on that grid
template <typename Launch> inline void rg_dispatch(uint64_t nnz, const LaunchShape &g, Launch &&launch) {
    const unsigned blocks = (unsigned)((row_gather_runs(nnz) + 3) / 4);
    if (g.L < 64) launch(std::integral_constant<int, 1>(), std::false_type(), dim3(blocks), g.L);
    else if (g.npl == 1) launch(std::integral_constant<int, 1>(), std::true_type(), dim3(blocks), 64u);
    else launch(std::integral_constant<int, 2>(), std::true_type(), dim3(blocks, g.chunks), 64u);   // two pieces per lane, the rest of a wider row over blockIdx.y
}

template <typename T, typename S, int VEC, typename Fold>
inline void launch_row_gather_v(const uint32_t *rowptr, const uint32_t *colind, uint32_t nrows, uint32_t nnz, const T *values, uint32_t heads, const S *X,
                                uint64_t ldx, uint32_t h, S *out, uint64_t ldo, int32_t *arg, T *ws, int32_t *ws_idx, const LaunchShape &g, hipStream_t st) {
    rg_dispatch(nnz, g, [&](auto nv, auto whole, dim3 grid, uint32_t L) {
        hipLaunchKernelGGL((k_row_gather<T, S, VEC, decltype(nv)::value, decltype(whole)::value, Fold>), grid, dim3(256), 0, st, rowptr, colind, nrows, nnz, values,
                           heads, X, ldx, h, L, out, ldo, arg, ws, ws_idx);
    });
}

// 16-byte pieces when every row of X and out starts 16-byte aligned, h fills whole pieces and no piece lies across two heads (arg and
// the index slots are stored with 4-byte alignment, whatever their width).  heads: 1 unless Fold::PER_HEAD.  A piece is 16 bytes of the
// STORAGE type: 8 features of a 16-bit one (h = 256: 32 pieces, two entries side by side in a wave instruction).
template <typename T, typename Fold, typename S = T>
inline void launch_row_gather(const uint32_t *rowptr, const uint32_t *colind, uint32_t nrows, uint32_t nnz, const T *values, uint32_t heads, const S *X,
                              uint64_t ldx, uint32_t h, S *out, uint64_t ldo, int32_t *arg, void *workspace, hipStream_t st) {
    constexpr uint32_t V = 16 / sizeof(S);
    if (nrows > 0) hipLaunchKernelGGL((k_row_gather_empty<S>), dim3((nrows + 3) / 4), dim3(256), 0, st, rowptr, nrows, h, out, ldo, arg);
    if (nnz == 0) return;
    T *ws = (T *)workspace;
    int32_t *ws_idx = Fold::INDEXED ? (int32_t *)((char *)workspace + row_gather_index_offset(nnz, h, sizeof(T))) : nullptr;
    const bool aligned = ldx % V == 0 && ldo % V == 0 && (uintptr_t)X % 16 == 0 && (uintptr_t)out % 16 == 0 && (uintptr_t)ws % 16 == 0;
    const LaunchShape g = row_gather_shape(h, h / heads, V, aligned);
    if (g.vec > 1) launch_row_gather_v<T, S, (int)V, Fold>(rowptr, colind, nrows, nnz, values, heads, X, ldx, h, out, ldo, arg, ws, ws_idx, g, st);
    else launch_row_gather_v<T, S, 1, Fold>(rowptr, colind, nrows, nnz, values, heads, X, ldx, h, out, ldo, arg, ws, ws_idx, g, st);
    const uint64_t runs = row_gather_runs(nnz);
    if (runs > 1)
        hipLaunchKernelGGL((k_row_gather_fixup<T, S, Fold>), dim3((unsigned)((runs + 2) / 4)), dim3(256), 0, st, rowptr, nrows, nnz, h, ws, ws_idx, out, ldo, arg);
}

}  // namespace pygim
