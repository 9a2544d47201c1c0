// sparse_attention_dev.hpp -- scaled dot-product attention over the stored entries of a CSR in one pass: scores, softmax and product
//   s[e, k]   = scale * sum_{f in head k} Q[r, f] * K[colind[e], f]     e over the stored entries of row r, in stored order; hd = h / heads, k = f / hd
//   out[r, f] = sum_e exp(s[e, k] - m[r, k]) * V[colind[e], f] / l[r, k],   m = max_e s,  l = sum_e exp(s - m)
//   lse[r, k] = m[r, k] + log(l[r, k])                                   (optional)
// Nothing of size nnz is read besides colind or written at all (the attention of TransformerConv and of graph transformers).
//
// Shape: k_gat_gather's (gat_aggregate_dev.hpp), a sibling kernel on the helpers of row_gather_dev.hpp, edge_softmax_dev.hpp and
// gat_aggregate_dev.hpp, so that the existing kernels compile to what they compiled to before.  A wave owns RG_EPW consecutive entries
// and walks them in batches of 64; the online softmax state (m, l, acc), the fold of the entries in flight as a group, the workspace
// slots, k_gat_fixup and k_gat_empty are those of the GAT aggregation.  What is new: the score is a dot product over a head's features,
// so it needs a reduction across lanes per entry.
//   * lanes lie across the features of a HEAD: a head group is LH lanes (the power of two that covers hd in pieces, at most 64), a lane
//     holds NP pieces of VEC features of its head, piece p at feature (p * LH + lane_in_head) * VEC of the head;
//   * heads lie side by side across the wave, L = heads * LH rounded up to a power of two, at most 64; the heads that do not fit go to
//     blockIdx.y, whole heads only -- every quantity is per head, no exchange between blocks;
//   * where L < 64, the 64 / L lane groups work on different entries of the row and meet in the xor tree with gat_scales;
//   * Q[r] pieces are loaded once per stretch of a row, the K and V pieces of up to RG_U / NP entries are issued before the first is
//     folded;
//   * per entry a lane forms the dot product of its pieces (features in ascending order), lanes past hd hold 0, and an xor butterfly
//     over the LH lanes (distances 1, 2, ..., LH / 2) leaves the sum in every lane of the head: x_i + x_j and x_j + x_i are the same
//     float, so after every step both partners -- and in the end all LH lanes -- hold the same bits, which the redundant (m, l) of the
//     head's lanes rely on.
// No atomics, every order is fixed by the CSR and the launch shape: the same bits on every launch.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "edge_softmax_dev.hpp"
#include "gat_aggregate_dev.hpp"
#include "row_gather_dev.hpp"

namespace pygim {

constexpr uint32_t SA_MAX_HEAD = 256;   // features of one head: 64 lanes x 4 scalar pieces on the narrowest path

// S is the storage type of Q, K, V and out, T the type of the products, the scores, lse, (m, l, acc) and the slots (S = T, or a 16-bit
// S with T = float).  LH: lanes per head, L: lanes per entry (a multiple of LH, 64 / L entries side by side); both powers of two.
// head0: the first head of this launch (blockIdx.y counts chunks of L / LH heads from there).
// DROP: attention dropout as in k_gat_gather -- pr into l unchanged, pr * w into the accumulate, w from (entry index base + kk, the lane's
// head: head0 and the blockIdx.y chunk included, so the mask does not depend on the launch shape).
// EDGE: a per-entry bias of the score, s = scale * dot + a_edge[e, head] after the butterfly and the scaling, before the maximum (the attention
// bias of graph transformers, an additive mask); a_edge is [nnz, heads] in the stored order of A, e = base + kk as for the dropout hash.  Every
// lane of a head loads the same element, so the head's redundant (m, l) stay equal.  Read only then.
template <typename T, typename S, int VEC, int NP, bool DROP = false, bool EDGE = false>
__global__ __launch_bounds__(256) void k_sa_gather(const uint32_t *__restrict__ rowptr, const uint32_t *__restrict__ colind, uint32_t nrows, uint32_t nnz,
                                                   const S *__restrict__ Q, uint64_t ldq, const S *__restrict__ K, uint64_t ldk, const S *__restrict__ Vm,
                                                   uint64_t ldv, uint32_t h, uint32_t heads, uint32_t head0, T scale, uint32_t LH, uint32_t L, S *__restrict__ out,
                                                   uint64_t ldo, T *__restrict__ lse, T *__restrict__ ws, T *__restrict__ ws_stat, AttnDrop<T> dr,
                                                   const T *__restrict__ a_edge = nullptr) {
    using V = typename SdVec<S, VEC>::type;
    constexpr int U = RG_U / NP;
    const uint32_t R = 64 / L;
    const uint32_t lane = threadIdx.x & 63, grp = lane / L, li = lane % L, lh = li % LH;
    const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint64_t e_begin = wave * RG_EPW;
    if (e_begin >= nnz) return;
    const uint32_t e_end = (uint32_t)(e_begin + RG_EPW < nnz ? e_begin + RG_EPW : nnz);
    const uint32_t hd = h / heads;
    const uint32_t head = head0 + blockIdx.y * (L / LH) + li / LH;
    const bool hok = head < heads;
    const bool first = hok && lh == 0;   // the lane that stores the head's (m, l) and lse
    uint32_t f[NP];
    bool pok[NP];
#pragma unroll
    for (int p = 0; p < NP; p++) {
        const uint32_t fh = ((uint32_t)p * LH + lh) * VEC;
        pok[p] = hok && fh < hd;
        f[p] = pok[p] ? head * hd + fh : 0u;
    }
    uint32_t row_cur = sd_row_of(rowptr, 0, nrows, (uint32_t)e_begin);
    const uint32_t row_hi = sd_row_of(rowptr, row_cur, nrows, e_end - 1) + 1;
    bool head_open = rowptr[row_cur] < (uint32_t)e_begin;   // the first row of the run began in an earlier run
    bool pending = false;
    T acc[NP][VEC], m, l;
    const uint64_t slots = wave * 2 * (uint64_t)h;   // the run's two accumulator slots, in elements
    const auto reset = [&]() {
        m = es_lowest<T>();
        l = T(0);
#pragma unroll
        for (int p = 0; p < NP; p++)
#pragma unroll
            for (int i = 0; i < VEC; i++) acc[p][i] = T(0);
    };
    // join the lane groups, then store: the raw partial into the workspace slot, or the finished row `row` into out / lse
    const auto flush = [&](bool to_slot, uint32_t slot, uint32_t row) {
        for (uint32_t s = L; s < 64; s <<= 1) {
            const T m2 = rg_shfl_xor(m, (int)s), l2 = rg_shfl_xor(l, (int)s);
            T M, a, b;
            gat_scales(m, m2, M, a, b);
            l = l * a + l2 * b;
            m = M;
#pragma unroll
            for (int p = 0; p < NP; p++)
#pragma unroll
                for (int i = 0; i < VEC; i++) acc[p][i] = acc[p][i] * a + rg_shfl_xor(acc[p][i], (int)s) * b;
        }
        if (grp != 0) return;
        if (to_slot) {
#pragma unroll
            for (int p = 0; p < NP; p++)
                if (pok[p]) rg_store<T, T, VEC>(ws + slots + (slot ? h : 0u) + f[p], acc[p]);
            if (first) {
                T *st = ws_stat + ((wave * 2 + slot) * heads + head) * 2;
                st[0] = m;
                st[1] = l;
            }
        } else {
            const T inv = T(1) / l;
#pragma unroll
            for (int p = 0; p < NP; p++)
                if (pok[p]) {
#pragma unroll
                    for (int i = 0; i < VEC; i++) acc[p][i] = acc[p][i] * inv;
                    rg_store<S, T, VEC>(out + (uint64_t)row * ldo + f[p], acc[p]);
                }
            if (lse && first) lse[(uint64_t)row * heads + head] = m + gat_log(l);
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
            V q[NP];
#pragma unroll
            for (int p = 0; p < NP; p++) q[p] = pok[p] ? *(const V *)(Q + (uint64_t)row * ldq + f[p]) : V(0);
            for (uint32_t k0 = pos; k0 <= last; k0 += R * U) {
                V kx[U][NP], vx[U][NP];
                T s[U];
                T ae[EDGE ? U : 1];   // EDGE: the entry's bias, loaded beside its rows
                bool ok[U];
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const uint32_t kk = k0 + (uint32_t)u * R + grp;
                    ok[u] = kk <= last;
                    const uint32_t col = rg_take32<false>(my_col, ok[u] ? kk : pos);
                    const S *kr = K + (uint64_t)col * ldk;
                    const S *vr = Vm + (uint64_t)col * ldv;
                    if constexpr (EDGE) ae[u] = ok[u] && hok ? a_edge[(uint64_t)(base + kk) * heads + head] : T(0);
#pragma unroll
                    for (int p = 0; p < NP; p++) {
                        kx[u][p] = V(0);
                        vx[u][p] = V(0);
                        if (ok[u] && pok[p]) {
                            kx[u][p] = *(const V *)(kr + f[p]);
                            vx[u][p] = *(const V *)(vr + f[p]);
                        }
                    }
                }
                // the lane's part of every dot product (0 in lanes past hd), then the butterfly over the head's LH lanes
#pragma unroll
                for (int u = 0; u < U; u++) {
                    s[u] = sd_dot<T, S, VEC>(q[0], kx[u][0]);
#pragma unroll
                    for (int p = 1; p < NP; p++) s[u] += sd_dot<T, S, VEC>(q[p], kx[u][p]);
                }
                for (uint32_t d = 1; d < LH; d <<= 1) {
#pragma unroll
                    for (int u = 0; u < U; u++) s[u] = s[u] + rg_shfl_xor(s[u], (int)d);
                }
                T M = m;
#pragma unroll
                for (int u = 0; u < U; u++) {
                    if constexpr (EDGE) s[u] = ok[u] ? scale * s[u] + ae[u] : es_lowest<T>();
                    else s[u] = ok[u] ? scale * s[u] : es_lowest<T>();   // not in flight: never above M
                    M = s[u] > M ? s[u] : M;
                }
                const T c = m == M ? T(1) : es_exp(m - M);
                m = M;
                l = l * c;
#pragma unroll
                for (int p = 0; p < NP; p++)
#pragma unroll
                    for (int i = 0; i < VEC; i++) acc[p][i] = acc[p][i] * c;
#pragma unroll
                for (int u = 0; u < U; u++)
                    if (ok[u]) {
                        T pr = es_exp(s[u] - M);
                        l = l + pr;
                        if constexpr (DROP)
                            pr = attn_dropout_keep(base + k0 + (uint32_t)u * R + grp, head, dr.seed_lo, dr.seed_hi, dr.thr) ? pr * dr.keep_w : T(0);
#pragma unroll
                        for (int p = 0; p < NP; p++)
#pragma unroll
                            for (int i = 0; i < VEC; i++) acc[p][i] = acc[p][i] + pr * T(rg_get<S, VEC>(vx[u][p], i));
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

// the lane layout of the head-wise kernels (k_sa_gather, k_gatv2_gather, k_gatv2_grad): NP pieces per lane (1 up to 64 pieces per head, then
// 2, then 4; hd <= SA_MAX_HEAD: at most 256 scalar pieces), LH lanes per head, L lanes per entry, L / LH heads per block and the rest of
// the heads over blockIdx.y, LS_MAX_CHUNKS chunks per launch
inline LaunchShape head_gather_shape(uint32_t h, uint32_t heads, uint32_t V, bool aligned) {
    LaunchShape g = launch_shape_piece(h / heads, V, aligned);
    const uint32_t pieces = (h / heads + g.vec - 1) / g.vec;
    g.npl = pieces <= 64 ? 1 : pieces <= 128 ? 2 : 4;
    while (g.LH * g.npl < pieces) g.LH <<= 1;
    for (g.L = g.LH; g.L < 64 && g.L < (uint64_t)heads * g.LH; g.L <<= 1) {}
    g.per = g.L / g.LH;                         // heads per block
    g.chunks = (heads + g.per - 1) / g.per;     // blockIdx.y; a launch takes at most LS_MAX_CHUNKS of them
    g.launches = (g.chunks + LS_MAX_CHUNKS - 1) / LS_MAX_CHUNKS;
    if (pieces != g.npl * g.LH) g.flags |= LS_PART_PIECE;   // some (lane, piece) places of a head hold no feature
    if (heads % g.per != 0) g.flags |= LS_PART_HEADS | (g.chunks > 1 ? LS_PART_CHUNK : 0u);
    return g;
}

template <typename T, typename S, int VEC, bool DROP, bool EDGE>
inline void launch_sa_gather_v(const uint32_t *rowptr, const uint32_t *colind, uint32_t nrows, uint32_t nnz, const S *Q, uint64_t ldq, const S *K, uint64_t ldk,
                               const S *Vm, uint64_t ldv, uint32_t h, uint32_t heads, T scale, S *out, uint64_t ldo, T *lse, T *ws, T *ws_stat,
                               const LaunchShape &g, const AttnDrop<T> &dr, const T *a_edge, hipStream_t st) {
    const unsigned blocks = (unsigned)((row_gather_runs(nnz) + 3) / 4);
#define PYGIM_SA_LAUNCH(NP)                                                                                                                                    \
    for (uint32_t c0 = 0; c0 < g.chunks; c0 += LS_MAX_CHUNKS)                                                                                                  \
    hipLaunchKernelGGL((k_sa_gather<T, S, VEC, NP, DROP, EDGE>), dim3(blocks, g.chunks - c0 < LS_MAX_CHUNKS ? g.chunks - c0 : LS_MAX_CHUNKS), dim3(256), 0, st,   \
                       rowptr, colind, nrows, nnz, Q, ldq, K, ldk, Vm, ldv, h, heads, c0 * g.per, scale, g.LH, g.L, out, ldo, lse, ws, ws_stat, dr, a_edge)
    constexpr uint32_t MAX_NP = (SA_MAX_HEAD + VEC * 64 - 1) / (VEC * 64);   // only the piece counts a head of SA_MAX_HEAD can need
    if (g.npl == 1) PYGIM_SA_LAUNCH(1);
    if constexpr (MAX_NP >= 2)
        if (g.npl == 2) PYGIM_SA_LAUNCH(2);
    if constexpr (MAX_NP >= 4)
        if (g.npl == 4) PYGIM_SA_LAUNCH(4);
#undef PYGIM_SA_LAUNCH
}

// 16-byte pieces (of the storage type) when a head's features fill whole pieces and every row of Q, K, V and out starts 16-byte aligned;
// else one element per lane.  The caller has checked h / heads <= SA_MAX_HEAD.  EDGE: with the per-entry bias a_edge [nnz, heads].
template <typename T, typename S = T, bool DROP = false, bool EDGE = false>
inline void launch_sparse_attention(const uint32_t *rowptr, const uint32_t *colind, uint32_t nrows, uint32_t nnz, const S *Q, uint64_t ldq, const S *K,
                                    uint64_t ldk, const S *Vm, uint64_t ldv, uint32_t h, uint32_t heads, T scale, S *out, uint64_t ldo, T *lse,
                                    void *workspace, hipStream_t st, const AttnDrop<T> &dr = AttnDrop<T>(), const T *a_edge = nullptr) {
    constexpr uint32_t V = 16 / sizeof(S);
    if (nrows > 0) hipLaunchKernelGGL((k_gat_empty<T, S>), dim3((nrows + 3) / 4), dim3(256), 0, st, rowptr, nrows, h, heads, out, ldo, lse);
    if (nnz == 0) return;
    T *ws = (T *)workspace;
    T *ws_stat = (T *)((char *)workspace + gat_stat_offset(nnz, h, sizeof(T)));
    const bool aligned = ldq % V == 0 && ldk % V == 0 && ldv % V == 0 && ldo % V == 0 && (uintptr_t)Q % 16 == 0 && (uintptr_t)K % 16 == 0 &&
                         (uintptr_t)Vm % 16 == 0 && (uintptr_t)out % 16 == 0 && (uintptr_t)ws % 16 == 0;
    const LaunchShape g = head_gather_shape(h, heads, V, aligned);
    if (g.vec > 1) launch_sa_gather_v<T, S, (int)V, DROP, EDGE>(rowptr, colind, nrows, nnz, Q, ldq, K, ldk, Vm, ldv, h, heads, scale, out, ldo, lse, ws, ws_stat, g, dr, a_edge, st);
    else launch_sa_gather_v<T, S, 1, DROP, EDGE>(rowptr, colind, nrows, nnz, Q, ldq, K, ldk, Vm, ldv, h, heads, scale, out, ldo, lse, ws, ws_stat, g, dr, a_edge, st);
    const uint64_t runs = row_gather_runs(nnz);
    if (runs > 1)
        hipLaunchKernelGGL((k_gat_fixup<T, S>), dim3((unsigned)((runs + 2) / 4)), dim3(256), 0, st, rowptr, nrows, nnz, h, heads, ws, ws_stat, out, ldo, lse);
}

}  // namespace pygim
