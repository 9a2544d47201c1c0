// gatv2_dev.hpp -- the aggregation of a GATv2 layer (Brody et al.; PyG's GATv2Conv) over the stored entries of a CSR, forward and backward,
// with nothing of size nnz read (besides colind) or written:
//   z[e, f]   = x_dst[r, f] + x_src[colind[e], f]                      e over the stored entries of row r, in stored order
//   s[e, k]   = sum_{f in head k} att[f] * lrelu(z[e, f])              hd = h / heads, k = f / hd, lrelu(z) = z > 0 ? z : slope * z
//   out[r, f] = sum_e exp(s[e, k] - m[r, k]) * x_src[colind[e], f] / l[r, k],   m = max_e s,  l = sum_e exp(s - m)
//   lse[r, k] = m[r, k] + log(l[r, k])                                 (optional)
// The nonlinearity sits inside the sum over a head's features, so the score is neither a function of two per-node numbers
// (gat_aggregate_dev.hpp) nor a dot product of two rows (sparse_attention_dev.hpp): composed from other operations it needs a tensor of
// [nnz, h].  Here it is formed in registers.
//
// Forward, k_gatv2_gather: a sibling of k_sa_gather on the same helpers (the existing kernels compile to what they compiled to before).
// Entry runs of RG_EPW, lanes across the features of a head (LH lanes per head, NP pieces per lane, heads side by side, the rest on
// blockIdx.y, 64 / L entry groups joined by gat_scales), two workspace slots per run plus ws_stat, k_gat_fixup and k_gat_empty.  What
// differs from k_sa_gather: the lane's part of a score is att * lrelu(x_dst + x_src) instead of q * k (att is loaded as 0 in lanes past
// hd, so they contribute exactly 0 to the butterfly), and the ONE gathered row x_src[c] of an entry serves the score and the accumulate.
//
// Backward, k_gatv2_grad<.., TRANSPOSED>: one gather over "own row i, gathered row j" with z = own[i] + oth[j], run once on the CSR of A
// (own = x_dst; G, lse, delta belong to the own row; it accumulates dx_dst and the partial of datt) and once on the CSR of A^T (own =
// x_src; x_dst, G, lse, delta belong to the gathered row; it accumulates dx_src).  With G = dout, delta[r, k] = sum_{f in head k} G out:
//   p  = exp(s - lse[r, k])      dp = sum_{f in head k} G[r, f] * x_src[c, f]      ds = p * (dp - delta[r, k])
//   t[e, f]      = ds * att[f] * lrelu'(z[e, f])                         lrelu'(z) = z > 0 ? 1 : slope  (z == 0 takes slope, as torch does)
//   dx_dst[r, f] = sum_{e in row r} t                     dx_src[c, f] = sum_{e with col = c} (p * G[r, f] + t)
//   datt[f]      = sum_e ds * lrelu(z[e, f])
// The score code is the forward's (gv2_score_part); s and dp go through the same butterfly passes.  The row results are plain sums: rows
// cut across runs leave raw partials in two slots per run and k_row_gather_fixup adds them in run order, k_row_gather_empty zeroes the
// rows without entries.  datt: every run leaves one partial of h elements (it is not reset at row ends) and k_gatv2_datt_reduce adds
// GV2_RED of them at a time, level by level, in a fixed order.
// No atomics, every order is fixed by the CSR and the launch shape: the same bits on every launch.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "edge_softmax_dev.hpp"
#include "gat_aggregate_dev.hpp"
#include "row_gather_dev.hpp"
#include "sparse_attention_dev.hpp"

namespace pygim {

constexpr uint32_t GV2_MAX_HEAD = SA_MAX_HEAD;   // features of one head: the lane layout is k_sa_gather's
constexpr uint32_t GV2_RED = 256;                // datt partials added per thread and level of k_gatv2_datt_reduce

// the lane's part of an entry's score: att * lrelu(a + b) over its NP pieces, features in ascending order.  a + b and b + a are the same
// float, so the forward (x_dst + x_src) and both backward directions form the same bits.  Lanes past hd hold att = 0 and a = b = 0.
template <typename T, typename S, int VEC, int NP>
__device__ inline T gv2_score_part(const T (&att)[NP][VEC], const typename SdVec<S, VEC>::type (&a)[NP], const typename SdVec<S, VEC>::type (&b)[NP],
                                   T slope) {
    T s = T(0);
#pragma unroll
    for (int p = 0; p < NP; p++)
#pragma unroll
        for (int i = 0; i < VEC; i++) {
            const T z = T(rg_get<S, VEC>(a[p], i)) + T(rg_get<S, VEC>(b[p], i));
            s += att[p][i] * (z > T(0) ? z : slope * z);
        }
    return s;
}

// S is the storage type of x_dst, x_src and out, T the type of att, z, the scores, lse, (m, l, acc) and the slots (S = T, or a 16-bit S
// with T = float).  LH, L, head0, DROP and dr: as in k_sa_gather.
template <typename T, typename S, int VEC, int NP, bool DROP = false>
__global__ __launch_bounds__(256) void k_gatv2_gather(const uint32_t *__restrict__ rowptr, const uint32_t *__restrict__ colind, uint32_t nrows, uint32_t nnz,
                                                      const S *__restrict__ Xd, uint64_t ldxd, const S *__restrict__ Xs, uint64_t ldxs,
                                                      const T *__restrict__ att, uint32_t h, uint32_t heads, uint32_t head0, T slope, uint32_t LH, uint32_t L,
                                                      S *__restrict__ out, uint64_t ldo, T *__restrict__ lse, T *__restrict__ ws, T *__restrict__ ws_stat,
                                                      AttnDrop<T> dr) {
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
    T a[NP][VEC];
#pragma unroll
    for (int p = 0; p < NP; p++) {
        const uint32_t fh = ((uint32_t)p * LH + lh) * VEC;
        pok[p] = hok && fh < hd;
        f[p] = pok[p] ? head * hd + fh : 0u;
#pragma unroll
        for (int i = 0; i < VEC; i++) a[p][i] = pok[p] ? att[f[p] + i] : T(0);
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
            T M, sa, sb;
            gat_scales(m, m2, M, sa, sb);
            l = l * sa + l2 * sb;
            m = M;
#pragma unroll
            for (int p = 0; p < NP; p++)
#pragma unroll
                for (int i = 0; i < VEC; i++) acc[p][i] = acc[p][i] * sa + rg_shfl_xor(acc[p][i], (int)s) * sb;
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
            for (int p = 0; p < NP; p++) q[p] = pok[p] ? *(const V *)(Xd + (uint64_t)row * ldxd + f[p]) : V(0);
            for (uint32_t k0 = pos; k0 <= last; k0 += R * U) {
                V x[U][NP];
                T s[U];
                bool ok[U];
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const uint32_t kk = k0 + (uint32_t)u * R + grp;
                    ok[u] = kk <= last;
                    const uint32_t col = rg_take32<false>(my_col, ok[u] ? kk : pos);
                    const S *xr = Xs + (uint64_t)col * ldxs;
#pragma unroll
                    for (int p = 0; p < NP; p++) {
                        x[u][p] = V(0);
                        if (ok[u] && pok[p]) x[u][p] = *(const V *)(xr + f[p]);
                    }
                }
                // the lane's part of every score (0 in lanes past hd), then the butterfly over the head's LH lanes
#pragma unroll
                for (int u = 0; u < U; u++) s[u] = gv2_score_part<T, S, VEC, NP>(a, q, x[u], slope);
                for (uint32_t d = 1; d < LH; d <<= 1) {
#pragma unroll
                    for (int u = 0; u < U; u++) s[u] = s[u] + rg_shfl_xor(s[u], (int)d);
                }
                T M = m;
#pragma unroll
                for (int u = 0; u < U; u++) {
                    s[u] = ok[u] ? s[u] : es_lowest<T>();   // not in flight: never above M
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
                            for (int i = 0; i < VEC; i++) acc[p][i] = acc[p][i] + pr * T(rg_get<S, VEC>(x[u][p], i));
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

// own / oth: the walked CSR's row operand and the gathered one (x_dst / x_src on the CSR of A, x_src / x_dst on the CSR of A^T).  G, lse
// [., heads] and delta [., heads] belong to the rows of A: the own row when !TRANSPOSED, the gathered row otherwise.  d_own: the gradient
// of own.  ws: two slots of h per run; ws_datt (!TRANSPOSED): h per run.  S stores own, oth, G and d_own; everything else is T.
// DROP: the forward ran with attention dropout dr: dp = w * sum G x_src, and the transposed direction accumulates pr * w * G + t.  w is the
// mask of (entry index IN A, head): entry_ids[walked index] -- the perm of the transposed CSR, loaded per lane beside colind and
// broadcast like my_col -- or the walked index itself when entry_ids is null.
template <typename T, typename S, int VEC, int NP, bool TRANSPOSED, bool DROP = false>
__global__ __launch_bounds__(256) void k_gatv2_grad(const uint32_t *__restrict__ rowptr, const uint32_t *__restrict__ colind, uint32_t nrows, uint32_t nnz,
                                                    const S *__restrict__ own, uint64_t ld_own, const S *__restrict__ oth, uint64_t ld_oth,
                                                    const T *__restrict__ att, uint32_t h, uint32_t heads, uint32_t head0, T slope, const S *__restrict__ G,
                                                    uint64_t ldg, const T *__restrict__ lse, const T *__restrict__ delta, uint32_t LH, uint32_t L,
                                                    S *__restrict__ d_own, uint64_t ldd, T *__restrict__ ws, T *__restrict__ ws_datt,
                                                    const int32_t *__restrict__ entry_ids, AttnDrop<T> dr) {
    using V = typename SdVec<S, VEC>::type;
    // entries in flight: k_sa_gather's RG_U / NP, at most 32 gathered elements per lane (8-element pieces of a 16-bit type are widened to float32
    // for two sums and an accumulate: more of them in flight cost the kernel its second wave per SIMD), half when TRANSPOSED gathers two rows
    constexpr int UF = RG_U / NP < 32 / (VEC * NP) ? RG_U / NP : 32 / (VEC * NP);
    constexpr int U = TRANSPOSED ? (UF >= 2 ? UF / 2 : 1) : UF;
    const uint32_t R = 64 / L;
    const uint32_t lane = threadIdx.x & 63, grp = lane / L, li = lane % L, lh = li % LH;
    const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint64_t e_begin = wave * RG_EPW;
    if (e_begin >= nnz) return;
    const uint32_t e_end = (uint32_t)(e_begin + RG_EPW < nnz ? e_begin + RG_EPW : nnz);
    const uint32_t hd = h / heads;
    const uint32_t head = head0 + blockIdx.y * (L / LH) + li / LH;
    const bool hok = head < heads;
    uint32_t f[NP];
    bool pok[NP];
    T a[NP][VEC];
#pragma unroll
    for (int p = 0; p < NP; p++) {
        const uint32_t fh = ((uint32_t)p * LH + lh) * VEC;
        pok[p] = hok && fh < hd;
        f[p] = pok[p] ? head * hd + fh : 0u;
#pragma unroll
        for (int i = 0; i < VEC; i++) a[p][i] = pok[p] ? att[f[p] + i] : T(0);
    }
    uint32_t row_cur = sd_row_of(rowptr, 0, nrows, (uint32_t)e_begin);
    const uint32_t row_hi = sd_row_of(rowptr, row_cur, nrows, e_end - 1) + 1;
    bool head_open = rowptr[row_cur] < (uint32_t)e_begin;   // the first row of the run began in an earlier run
    bool pending = false;
    T acc[NP][VEC];    // the gradient row of the own row
    T dacc[NP][VEC];   // the run's part of datt: never reset
    const uint64_t slots = wave * 2 * (uint64_t)h;
#pragma unroll
    for (int p = 0; p < NP; p++)
#pragma unroll
        for (int i = 0; i < VEC; i++) acc[p][i] = dacc[p][i] = T(0);
    // add the lane groups, then store: the raw partial into the workspace slot, or the finished row `row` into d_own
    const auto flush = [&](bool to_slot, uint32_t slot, uint32_t row) {
        for (uint32_t s = L; s < 64; s <<= 1) {
#pragma unroll
            for (int p = 0; p < NP; p++)
#pragma unroll
                for (int i = 0; i < VEC; i++) acc[p][i] = acc[p][i] + rg_shfl_xor(acc[p][i], (int)s);
        }
        if (grp == 0) {
#pragma unroll
            for (int p = 0; p < NP; p++)
                if (pok[p]) {
                    if (to_slot) rg_store<T, T, VEC>(ws + slots + (slot ? h : 0u) + f[p], acc[p]);
                    else rg_store<S, T, VEC>(d_own + (uint64_t)row * ldd + f[p], acc[p]);
                }
        }
#pragma unroll
        for (int p = 0; p < NP; p++)
#pragma unroll
            for (int i = 0; i < VEC; i++) acc[p][i] = T(0);
    };

    for (uint32_t base = (uint32_t)e_begin; base < e_end; base += 64) {
        const uint32_t n = (base + 64 < e_end ? base + 64 : e_end) - base;
        const uint32_t my_e = base + lane;
        const bool valid = lane < n;
        const uint32_t my_col = valid ? colind[my_e] : 0u;
        uint32_t my_id = my_e;   // DROP: the entry's index in A
        if constexpr (DROP)
            if (entry_ids) my_id = valid ? (uint32_t)entry_ids[my_e] : 0u;
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
            V o[NP], g[NP];
            T ls_row = T(0), dl_row = T(0);
#pragma unroll
            for (int p = 0; p < NP; p++) {
                o[p] = pok[p] ? *(const V *)(own + (uint64_t)row * ld_own + f[p]) : V(0);
                g[p] = V(0);
                if constexpr (!TRANSPOSED)
                    if (pok[p]) g[p] = *(const V *)(G + (uint64_t)row * ldg + f[p]);
            }
            if constexpr (!TRANSPOSED)
                if (hok) {
                    ls_row = lse[(uint64_t)row * heads + head];
                    dl_row = delta[(uint64_t)row * heads + head];
                }
            for (uint32_t k0 = pos; k0 <= last; k0 += R * U) {
                V x[U][NP], gj[TRANSPOSED ? U : 1][NP];
                T s[U], dp[U], ls[U], dl[U];
                bool ok[U];
                uint32_t id[DROP ? U : 1];
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const uint32_t kk = k0 + (uint32_t)u * R + grp;
                    ok[u] = kk <= last;
                    const uint32_t col = rg_take32<false>(my_col, ok[u] ? kk : pos);
                    if constexpr (DROP) id[u] = rg_take32<false>(my_id, ok[u] ? kk : pos);
                    const S *xr = oth + (uint64_t)col * ld_oth;
                    ls[u] = ls_row;
                    dl[u] = dl_row;
                    if constexpr (TRANSPOSED)
                        if (ok[u] && hok) {
                            ls[u] = lse[(uint64_t)col * heads + head];
                            dl[u] = delta[(uint64_t)col * heads + head];
                        }
#pragma unroll
                    for (int p = 0; p < NP; p++) {
                        x[u][p] = V(0);
                        if constexpr (TRANSPOSED) gj[u][p] = V(0);
                        if (ok[u] && pok[p]) {
                            x[u][p] = *(const V *)(xr + f[p]);
                            if constexpr (TRANSPOSED) gj[u][p] = *(const V *)(G + (uint64_t)col * ldg + f[p]);
                        }
                    }
                }
                // the lane's parts of the score and of dp = G[r] . x_src[c] (0 in lanes past hd), both through one butterfly
#pragma unroll
                for (int u = 0; u < U; u++) {
                    s[u] = gv2_score_part<T, S, VEC, NP>(a, o, x[u], slope);
                    if constexpr (TRANSPOSED) {
                        dp[u] = sd_dot<T, S, VEC>(gj[u][0], o[0]);
#pragma unroll
                        for (int p = 1; p < NP; p++) dp[u] += sd_dot<T, S, VEC>(gj[u][p], o[p]);
                    } else {
                        dp[u] = sd_dot<T, S, VEC>(g[0], x[u][0]);
#pragma unroll
                        for (int p = 1; p < NP; p++) dp[u] += sd_dot<T, S, VEC>(g[p], x[u][p]);
                    }
                }
                for (uint32_t d = 1; d < LH; d <<= 1) {
#pragma unroll
                    for (int u = 0; u < U; u++) {
                        s[u] = s[u] + rg_shfl_xor(s[u], (int)d);
                        dp[u] = dp[u] + rg_shfl_xor(dp[u], (int)d);
                    }
                }
#pragma unroll
                for (int u = 0; u < U; u++)
                    if (ok[u]) {
                        const T pr = es_exp(s[u] - ls[u]);
                        T pw = pr;   // pr * w
                        if constexpr (DROP) {
                            const T w = attn_dropout_keep(id[u], head, dr.seed_lo, dr.seed_hi, dr.thr) ? dr.keep_w : T(0);
                            dp[u] = dp[u] * w;
                            pw = pr * w;
                        }
                        const T ds = pr * (dp[u] - dl[u]);
#pragma unroll
                        for (int p = 0; p < NP; p++)
#pragma unroll
                            for (int i = 0; i < VEC; i++) {
                                const T z = T(rg_get<S, VEC>(o[p], i)) + T(rg_get<S, VEC>(x[u][p], i));
                                const bool pos_z = z > T(0);
                                const T t = ds * a[p][i] * (pos_z ? T(1) : slope);
                                if constexpr (TRANSPOSED) acc[p][i] = acc[p][i] + (pw * T(rg_get<S, VEC>(gj[u][p], i)) + t);
                                else {
                                    acc[p][i] = acc[p][i] + t;
                                    dacc[p][i] = dacc[p][i] + ds * (pos_z ? z : slope * z);
                                }
                            }
                    }
            }
            if (closes) {
                flush(head_open, 0u, row);
                head_open = false;
            }
            pending = !closes;
            pos = last + 1;
        }
        row_cur = rg_take32<true>(my_row, n - 1);
    }
    if (pending) flush(true, head_open ? 0u : 1u, 0u);   // the run's last row goes on in the next run
    if constexpr (!TRANSPOSED) {
        for (uint32_t s = L; s < 64; s <<= 1) {
#pragma unroll
            for (int p = 0; p < NP; p++)
#pragma unroll
                for (int i = 0; i < VEC; i++) dacc[p][i] = dacc[p][i] + rg_shfl_xor(dacc[p][i], (int)s);
        }
        if (grp == 0) {
#pragma unroll
            for (int p = 0; p < NP; p++)
                if (pok[p]) rg_store<T, T, VEC>(ws_datt + wave * (uint64_t)h + f[p], dacc[p]);
        }
    }
}

// dst[b, f] = src[b * GV2_RED, f] + ... + src[min(n, (b + 1) * GV2_RED) - 1, f], in that order (n = 0: zeros); b = blockIdx.y
template <typename T>
__global__ __launch_bounds__(256) void k_gatv2_datt_reduce(const T *__restrict__ src, uint64_t n, uint32_t h, T *__restrict__ dst) {
    const uint32_t f = blockIdx.x * 256 + threadIdx.x;
    if (f >= h) return;
    const uint64_t w0 = (uint64_t)blockIdx.y * GV2_RED;
    const uint64_t w1 = w0 + GV2_RED < n ? w0 + GV2_RED : n;
    T s = T(0);
    for (uint64_t w = w0; w < w1; w++) s = s + src[w * h + f];
    dst[(uint64_t)blockIdx.y * h + f] = s;
}

// the lane layout is head_gather_shape's (sparse_attention_dev.hpp)
template <typename T, typename S, int VEC, bool DROP>
inline void launch_gatv2_gather_v(const uint32_t *rowptr, const uint32_t *colind, uint32_t nrows, uint32_t nnz, const S *Xd, uint64_t ldxd, const S *Xs,
                                  uint64_t ldxs, const T *att, uint32_t h, uint32_t heads, T slope, S *out, uint64_t ldo, T *lse, T *ws, T *ws_stat,
                                  const LaunchShape &g, const AttnDrop<T> &dr, hipStream_t st) {
    const unsigned blocks = (unsigned)((row_gather_runs(nnz) + 3) / 4);
#define PYGIM_GV2_LAUNCH(NP)                                                                                                                          \
    for (uint32_t c0 = 0; c0 < g.chunks; c0 += LS_MAX_CHUNKS)                                                                                         \
    hipLaunchKernelGGL((k_gatv2_gather<T, S, VEC, NP, DROP>), dim3(blocks, g.chunks - c0 < LS_MAX_CHUNKS ? g.chunks - c0 : LS_MAX_CHUNKS), dim3(256), 0, st, \
                       rowptr, colind, nrows, nnz, Xd, ldxd, Xs, ldxs, att, h, heads, c0 * g.per, slope, g.LH, g.L, out, ldo, lse, ws, ws_stat, dr)
    constexpr uint32_t MAX_NP = (GV2_MAX_HEAD + VEC * 64 - 1) / (VEC * 64);   // only the piece counts a head of GV2_MAX_HEAD can need
    if (g.npl == 1) PYGIM_GV2_LAUNCH(1);
    if constexpr (MAX_NP >= 2)
        if (g.npl == 2) PYGIM_GV2_LAUNCH(2);
    if constexpr (MAX_NP >= 4)
        if (g.npl == 4) PYGIM_GV2_LAUNCH(4);
#undef PYGIM_GV2_LAUNCH
}

// 16-byte pieces (of the storage type) when a head's features fill whole pieces and every row of x_dst, x_src and out starts 16-byte
// aligned; else one element per lane.  The caller has checked h / heads <= GV2_MAX_HEAD.  The workspace is gat_aggregate's.
template <typename T, typename S = T, bool DROP = false>
inline void launch_gatv2_aggregate(const uint32_t *rowptr, const uint32_t *colind, uint32_t nrows, uint32_t nnz, const S *Xd, uint64_t ldxd, const S *Xs,
                                   uint64_t ldxs, const T *att, uint32_t h, uint32_t heads, T slope, S *out, uint64_t ldo, T *lse, void *workspace,
                                   hipStream_t st, const AttnDrop<T> &dr = AttnDrop<T>()) {
    constexpr uint32_t V = 16 / sizeof(S);
    if (nrows > 0) hipLaunchKernelGGL((k_gat_empty<T, S>), dim3((nrows + 3) / 4), dim3(256), 0, st, rowptr, nrows, h, heads, out, ldo, lse);
    if (nnz == 0) return;
    T *ws = (T *)workspace;
    T *ws_stat = (T *)((char *)workspace + gat_stat_offset(nnz, h, sizeof(T)));
    const bool aligned = ldxd % V == 0 && ldxs % V == 0 && ldo % V == 0 && (uintptr_t)Xd % 16 == 0 && (uintptr_t)Xs % 16 == 0 &&
                         (uintptr_t)out % 16 == 0 && (uintptr_t)ws % 16 == 0;
    const LaunchShape g = head_gather_shape(h, heads, V, aligned);
    if (g.vec > 1) launch_gatv2_gather_v<T, S, (int)V, DROP>(rowptr, colind, nrows, nnz, Xd, ldxd, Xs, ldxs, att, h, heads, slope, out, ldo, lse, ws, ws_stat, g, dr, st);
    else launch_gatv2_gather_v<T, S, 1, DROP>(rowptr, colind, nrows, nnz, Xd, ldxd, Xs, ldxs, att, h, heads, slope, out, ldo, lse, ws, ws_stat, g, dr, st);
    const uint64_t runs = row_gather_runs(nnz);
    if (runs > 1)
        hipLaunchKernelGGL((k_gat_fixup<T, S>), dim3((unsigned)((runs + 2) / 4)), dim3(256), 0, st, rowptr, nrows, nnz, h, heads, ws, ws_stat, out, ldo, lse);
}

// the backward's workspace: the two accumulator slots per run of k_row_gather, then the datt partials (h per run), then the second
// buffer of their reduction (h per GV2_RED runs); every part starts 16-byte aligned
inline uint64_t gatv2_datt_offset(uint64_t nnz, uint64_t h, size_t elem) { return row_gather_index_offset(nnz, h, elem); }
inline uint64_t gatv2_datt2_offset(uint64_t nnz, uint64_t h, size_t elem) {
    return gatv2_datt_offset(nnz, h, elem) + (row_gather_runs(nnz) * h * elem + 15) / 16 * 16;
}
inline uint64_t gatv2_backward_workspace_bytes(uint64_t nnz, uint64_t h, size_t elem) {
    return gatv2_datt2_offset(nnz, h, elem) + (row_gather_runs(nnz) + GV2_RED - 1) / GV2_RED * h * elem;
}

template <typename T, typename S, int VEC, bool TRANSPOSED, bool DROP>
inline void launch_gatv2_grad_v(const uint32_t *rowptr, const uint32_t *colind, uint32_t nrows, uint32_t nnz, const S *own, uint64_t ld_own, const S *oth,
                                uint64_t ld_oth, const T *att, uint32_t h, uint32_t heads, T slope, const S *G, uint64_t ldg, const T *lse, const T *delta,
                                S *d_own, uint64_t ldd, T *ws, T *ws_datt, const LaunchShape &g, const int32_t *entry_ids, const AttnDrop<T> &dr,
                                hipStream_t st) {
    const unsigned blocks = (unsigned)((row_gather_runs(nnz) + 3) / 4);
#define PYGIM_GV2_LAUNCH(NP)                                                                                                                           \
    for (uint32_t c0 = 0; c0 < g.chunks; c0 += LS_MAX_CHUNKS)                                                                                          \
    hipLaunchKernelGGL((k_gatv2_grad<T, S, VEC, NP, TRANSPOSED, DROP>), dim3(blocks, g.chunks - c0 < LS_MAX_CHUNKS ? g.chunks - c0 : LS_MAX_CHUNKS), dim3(256), 0, st, \
                       rowptr, colind, nrows, nnz, own, ld_own, oth, ld_oth, att, h, heads, c0 * g.per, slope, G, ldg, lse, delta, g.LH, g.L, d_own, ldd, ws,   \
                       ws_datt, entry_ids, dr)
    constexpr uint32_t MAX_NP = (GV2_MAX_HEAD + VEC * 64 - 1) / (VEC * 64);
    if (g.npl == 1) PYGIM_GV2_LAUNCH(1);
    if constexpr (MAX_NP >= 2)
        if (g.npl == 2) PYGIM_GV2_LAUNCH(2);
    if constexpr (MAX_NP >= 4)
        if (g.npl == 4) PYGIM_GV2_LAUNCH(4);
#undef PYGIM_GV2_LAUNCH
}

// one direction of the backward (see k_gatv2_grad).  datt: null when TRANSPOSED; when !TRANSPOSED and null, the reduction is skipped.
// DROP: the forward's attention dropout dr, entry_ids: the index in A of every walked entry (null: the walked index)
template <typename T, typename S, bool TRANSPOSED, bool DROP = false>
inline void launch_gatv2_backward(const uint32_t *rowptr, const uint32_t *colind, uint32_t nrows, uint32_t nnz, const S *own, uint64_t ld_own, const S *oth,
                                  uint64_t ld_oth, const T *att, uint32_t h, uint32_t heads, T slope, const S *G, uint64_t ldg, const T *lse, const T *delta,
                                  S *d_own, uint64_t ldd, T *datt, void *workspace, hipStream_t st, const int32_t *entry_ids = nullptr,
                                  const AttnDrop<T> &dr = AttnDrop<T>()) {
    constexpr uint32_t V = 16 / sizeof(S);
    if (nrows > 0) hipLaunchKernelGGL((k_row_gather_empty<S>), dim3((nrows + 3) / 4), dim3(256), 0, st, rowptr, nrows, h, d_own, ldd, nullptr);
    const uint64_t runs = row_gather_runs(nnz);
    T *ws = (T *)workspace;
    T *part = (T *)((char *)workspace + gatv2_datt_offset(nnz, h, sizeof(T)));
    T *part2 = (T *)((char *)workspace + gatv2_datt2_offset(nnz, h, sizeof(T)));
    if (nnz > 0) {
        const bool aligned = ld_own % V == 0 && ld_oth % V == 0 && ldg % V == 0 && ldd % V == 0 && (uintptr_t)own % 16 == 0 && (uintptr_t)oth % 16 == 0 &&
                             (uintptr_t)G % 16 == 0 && (uintptr_t)d_own % 16 == 0 && (uintptr_t)ws % 16 == 0;
        const LaunchShape g = head_gather_shape(h, heads, V, aligned);
        if (g.vec > 1)
            launch_gatv2_grad_v<T, S, (int)V, TRANSPOSED, DROP>(rowptr, colind, nrows, nnz, own, ld_own, oth, ld_oth, att, h, heads, slope, G, ldg, lse, delta,
                                                                d_own, ldd, ws, part, g, entry_ids, dr, st);
        else
            launch_gatv2_grad_v<T, S, 1, TRANSPOSED, DROP>(rowptr, colind, nrows, nnz, own, ld_own, oth, ld_oth, att, h, heads, slope, G, ldg, lse, delta, d_own, ldd,
                                                           ws, part, g, entry_ids, dr, st);
        if (runs > 1)
            hipLaunchKernelGGL((k_row_gather_fixup<T, S, FoldSum<false>>), dim3((unsigned)((runs + 2) / 4)), dim3(256), 0, st, rowptr, nrows, nnz, h, ws, nullptr,
                               d_own, ldd, nullptr);
    }
    if constexpr (!TRANSPOSED) {
        if (!datt) return;
        // level by level, GV2_RED partials at a time, between the two buffers; the last level writes datt
        const T *src = part;
        uint64_t n = runs;
        for (;;) {
            const uint64_t nb = n > GV2_RED ? (n + GV2_RED - 1) / GV2_RED : 1;
            T *dst = nb == 1 ? datt : (src == part ? part2 : part);
            hipLaunchKernelGGL((k_gatv2_datt_reduce<T>), dim3((h + 255) / 256, (unsigned)nb), dim3(256), 0, st, src, n, h, dst);
            if (nb == 1) break;
            src = dst;
            n = nb;
        }
    }
}

}  // namespace pygim
