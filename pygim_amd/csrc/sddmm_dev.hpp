// sddmm_dev.hpp -- sampled dense-dense product on a caller's CSR: out[e] = sum_f G[row(e), f] * X[colind[e], f] for every stored entry e
// (the gradient of a conv layer's aggregation with respect to the edge values: d(A . X)/dA[r, c] = G[r] . X[c]).
//
// Shape (the gather of the forward's sweep, with one dot product per entry instead of a sum per row):
//   * a wave owns SD_EPW consecutive entries (a hub row is cut across waves; no output is shared, so there are no atomics and every
//     run stores the same bits) and walks them in batches of 64;
//   * a lane group of L lanes (L = the power of two that covers h in 16-byte pieces, at most 64) holds one X row per wave-instruction,
//     16 bytes per lane; 64 / L groups work on different entries side by side, every lane keeps the partial sums of the L entries its
//     group handles in a batch and issues their gathers back to back (several rows in flight);
//   * a batch inside one row keeps G[row] in registers; a batch that crosses rows reads each entry's G row beside its X row;
//   * the L partials of a group are reduced as a reduce-scatter (recursive halving: L - 1 exchanges per lane for L entries, instead of
//     a log2(L)-step tree per entry) that leaves the sum of the group's k-th entry in its k-th lane -- the 64 sums of a batch then sit in
//     64 lanes, and one coalesced store writes them.
// The order of every sum is fixed (per lane: features in ascending order within its pieces; then the halving order): deterministic.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pygim {

constexpr uint32_t SD_EPW = 256;   // entries per wave (4 batches of 64)

// What a launch_* function of the gather family decides, as numbers: computed by the pure host functions *_shape() from the sizes, the
// pieces a 16-byte load holds (V = 16 / sizeof(storage type)) and ONE alignment fact (`aligned`: every stride is a multiple of V and
// every base pointer a multiple of 16 bytes).  The launchers launch what these functions say; pygim_gather_launch_shape
// (include/pygim_hip.h) returns the same numbers without a device.
struct LaunchShape {
    uint32_t vec;        // features per piece: V, or 1
    uint32_t npl;        // pieces a lane holds at once (NV of the row walkers, NP of the head-wise kernels, up to NVC of k_sddmm, 1 else)
    uint32_t LH;         // lanes across one head's features (head-wise kernels); L elsewhere
    uint32_t L;          // lanes per entry: 64 / L entries side by side in a wave
    uint32_t per;        // heads per block (head-wise kernels); 1 elsewhere
    uint32_t chunks;     // blockIdx.y chunks over all launches (k_sddmm: passes of NVC pieces; k_es_batch: steps over the heads)
    uint32_t launches;   // launches of the gather kernel (65535 chunks each at most)
    uint32_t flags;      // LS_* below
};
constexpr uint32_t LS_PART_PIECE = 1;    // the last piece of a lane exists only on some of the lanes (pieces % lanes != 0)
constexpr uint32_t LS_PART_CHUNK = 2;    // the last chunk (pass) holds fewer pieces, or fewer heads, than the others
constexpr uint32_t LS_PART_HEADS = 4;    // a block has lanes for more heads than it is given (heads % per != 0)
constexpr uint32_t LS_SCALAR_SIZE = 8;   // vec == 1 because the width (a head's, or `heads` of edge_softmax) does not fill whole pieces
constexpr uint32_t LS_SCALAR_ALIGN = 16; // vec == 1 because of `aligned` alone
constexpr uint32_t LS_MAX_CHUNKS = 65535;   // gridDim.y

// the piece: V features when `width` fills whole pieces and everything is aligned; else 1, with the reason in flags
inline LaunchShape launch_shape_piece(uint32_t width, uint32_t V, bool aligned) {
    LaunchShape g = {1u, 1u, 1u, 1u, 1u, 1u, 1u, 0u};
    if (width % V != 0) g.flags = LS_SCALAR_SIZE;
    else if (!aligned) g.flags = LS_SCALAR_ALIGN;
    else g.vec = V;
    return g;
}

// k_sddmm: L lanes cover the row's pieces (a power of two, at most 64), a lane holds up to 4 pieces at once and takes longer rows in passes
inline LaunchShape sddmm_shape(uint32_t h, uint32_t V, bool aligned) {
    LaunchShape g = launch_shape_piece(h, V, aligned);
    const uint32_t pieces = (h + g.vec - 1) / g.vec;
    while (g.L < 64 && g.L < pieces) g.L <<= 1;
    g.LH = g.L;
    const uint32_t nv = (pieces + g.L - 1) / g.L;   // pieces per lane and entry
    g.npl = nv < 4 ? nv : 4;
    g.chunks = (nv + 3) / 4;
    if (pieces % g.L != 0) g.flags |= LS_PART_PIECE;
    if (g.chunks > 1 && nv % 4 != 0) g.flags |= LS_PART_CHUNK;
    return g;
}

// the last row r < nrows with rowptr[r] <= e, searched in [lo, nrows)
__device__ inline uint32_t sd_row_of(const uint32_t *__restrict__ rowptr, uint32_t lo, uint32_t nrows, uint32_t e) {
    uint32_t hi = nrows;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (rowptr[mid] <= e) lo = mid;
        else hi = mid;
    }
    return lo;
}

template <typename T, int VEC> struct SdVec { typedef T __attribute__((ext_vector_type(VEC))) type; };
template <typename T> struct SdVec<T, 1> { typedef T type; };

// a . b in T, the operands stored as S (widened element by element: exact)
template <typename T, typename S, int VEC>
__device__ inline T sd_dot(const typename SdVec<S, VEC>::type &a, const typename SdVec<S, VEC>::type &b) {
    if constexpr (VEC == 1) {
        return T(a) * T(b);
    } else {
        T s = T(a[0]) * T(b[0]);
#pragma unroll
        for (int i = 1; i < VEC; i++) s += T(a[i]) * T(b[i]);
        return s;
    }
}

// a wave-uniform value of lane `src` (src a compile-time constant after unrolling when the whole wave is one group)
template <int L> __device__ inline uint32_t sd_take(uint32_t v, uint32_t src) {
    if constexpr (L == 64) return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)src);
    else return (uint32_t)__shfl((int)v, (int)src, 64);
}

// NVC: 16-byte pieces per lane held at once (features per lane and pass = NVC * VEC; wider rows take several passes)
// S is the storage type of G and X, T the type of the products, the sums and out (S = T, or a 16-bit S with T = float: no rounding)
template <typename T, typename S, int VEC, int L, int NVC>
__global__ __launch_bounds__(256) void k_sddmm(const uint32_t *__restrict__ rowptr, const uint32_t *__restrict__ colind, uint32_t nrows, uint32_t nnz,
                                               const S *__restrict__ G, uint64_t ldg, const S *__restrict__ X, uint64_t ldx, uint32_t h, T *__restrict__ out) {
    using V = typename SdVec<S, VEC>::type;
    constexpr int R = 64 / L;   // entries side by side per wave-instruction
    const uint32_t lane = threadIdx.x & 63, grp = lane / L, li = lane % L;
    const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint64_t e_begin = wave * SD_EPW;
    if (e_begin >= nnz) return;
    const uint32_t e_end = (uint32_t)(e_begin + SD_EPW < nnz ? e_begin + SD_EPW : nnz);
    const uint32_t nv = (h + VEC * L - 1) / (VEC * L);   // pieces per lane and entry
    uint32_t row = sd_row_of(rowptr, 0, nrows, (uint32_t)e_begin);
    for (uint32_t base = (uint32_t)e_begin; base < e_end; base += 64) {
        const uint32_t bend = base + 64 < e_end ? base + 64 : e_end;
        if (rowptr[row + 1] <= base) row = sd_row_of(rowptr, row + 1, nrows, base);
        const bool one_row = rowptr[row + 1] >= bend;   // wave-uniform
        // entry base + lane: its column (and, when the batch crosses rows, its row); the groups take theirs from these lanes
        const uint32_t my_e = base + lane;
        const uint32_t my_col = my_e < bend ? colind[my_e] : 0u;
        uint32_t my_row = row;
        if (!one_row && my_e < bend) my_row = sd_row_of(rowptr, row, nrows, my_e);
        T p[L];
#pragma unroll
        for (int k = 0; k < L; k++) p[k] = T(0);
        for (uint32_t c0 = 0; c0 < nv; c0 += NVC) {
            V gv[NVC];
            if (one_row) {
                const S *gr = G + (uint64_t)row * ldg;
#pragma unroll
                for (int v = 0; v < NVC; v++) {
                    const uint32_t f = ((c0 + v) * L + li) * VEC;
                    gv[v] = (c0 + v < nv && f < h) ? *(const V *)(gr + f) : V(0);
                }
            }
#pragma unroll
            for (int k = 0; k < L; k++) {
                const uint32_t src = grp + (uint32_t)(R * k);
                const bool valid = base + src < bend;
                const uint32_t col = sd_take<L>(my_col, src);
                const S *xr = X + (uint64_t)col * ldx;
                const S *gr = G + (uint64_t)(one_row ? row : sd_take<L>(my_row, src)) * ldg;
#pragma unroll
                for (int v = 0; v < NVC; v++) {
                    const uint32_t f = ((c0 + v) * L + li) * VEC;
                    if (valid && c0 + v < nv && f < h) {
                        const V xv = *(const V *)(xr + f);
                        const V gg = one_row ? gv[v] : *(const V *)(gr + f);
                        p[k] += sd_dot<T, S, VEC>(gg, xv);
                    }
                }
            }
        }
        // reduce-scatter over the group's L lanes: after the step of distance s a lane keeps the half of its partials whose index has
        // bit s equal to its own lane bit s, and adds the partner's copy of that half -- in the end lane li holds entry li's sum
#pragma unroll
        for (int s = L / 2; s >= 1; s >>= 1) {
            const bool hi = (li & (uint32_t)s) != 0;
#pragma unroll
            for (int j = 0; j < s; j++) {
                const T send = hi ? p[j] : p[j + s];
                const T keep = hi ? p[j + s] : p[j];
                p[j] = keep + __shfl_xor(send, s, 64);
            }
        }
        const uint32_t e = base + grp + (uint32_t)R * li;   // a permutation of the batch's 64 entries over the 64 lanes
        if (e < bend) out[e] = p[0];
    }
}

template <typename T, typename S, int VEC, int L>
inline void launch_sddmm_l(const uint32_t *rowptr, const uint32_t *colind, uint32_t nrows, uint32_t nnz, const S *G, uint64_t ldg, const S *X, uint64_t ldx,
                           uint32_t h, T *out, hipStream_t st) {
    const uint64_t waves = ((uint64_t)nnz + SD_EPW - 1) / SD_EPW;
    // pieces held at once: the whole row up to 4 pieces (h = 256 FLT32 / DBL64 with 64 lanes: 1 / 2), longer rows in passes of 4
    hipLaunchKernelGGL((k_sddmm<T, S, VEC, L, 4>), dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, rowptr, colind, nrows, nnz, G, ldg, X, ldx, h, out);
}

template <typename T, typename S, int VEC>
inline void launch_sddmm_v(const uint32_t *rowptr, const uint32_t *colind, uint32_t nrows, uint32_t nnz, const S *G, uint64_t ldg, const S *X, uint64_t ldx,
                           uint32_t h, T *out, uint32_t L, hipStream_t st) {
    if (L == 1) launch_sddmm_l<T, S, VEC, 1>(rowptr, colind, nrows, nnz, G, ldg, X, ldx, h, out, st);
    else if (L == 2) launch_sddmm_l<T, S, VEC, 2>(rowptr, colind, nrows, nnz, G, ldg, X, ldx, h, out, st);
    else if (L == 4) launch_sddmm_l<T, S, VEC, 4>(rowptr, colind, nrows, nnz, G, ldg, X, ldx, h, out, st);
    else if (L == 8) launch_sddmm_l<T, S, VEC, 8>(rowptr, colind, nrows, nnz, G, ldg, X, ldx, h, out, st);
    else if (L == 16) launch_sddmm_l<T, S, VEC, 16>(rowptr, colind, nrows, nnz, G, ldg, X, ldx, h, out, st);
    else if (L == 32) launch_sddmm_l<T, S, VEC, 32>(rowptr, colind, nrows, nnz, G, ldg, X, ldx, h, out, st);
    else launch_sddmm_l<T, S, VEC, 64>(rowptr, colind, nrows, nnz, G, ldg, X, ldx, h, out, st);
}

// 16-byte pieces (of the storage type) when every row of G and X starts 16-byte aligned and h fills whole pieces; else one element per lane
template <typename T, typename S = T>
inline void launch_sddmm(const uint32_t *rowptr, const uint32_t *colind, uint32_t nrows, uint32_t nnz, const S *G, uint64_t ldg, const S *X, uint64_t ldx,
                         uint32_t h, T *out, hipStream_t st) {
    constexpr uint32_t V = 16 / sizeof(S);
    const bool aligned = ldg % V == 0 && ldx % V == 0 && (uintptr_t)G % 16 == 0 && (uintptr_t)X % 16 == 0;
    const LaunchShape g = sddmm_shape(h, V, aligned);
    if (g.vec > 1) launch_sddmm_v<T, S, (int)V>(rowptr, colind, nrows, nnz, G, ldg, X, ldx, h, out, g.L, st);
    else launch_sddmm_v<T, S, 1>(rowptr, colind, nrows, nnz, G, ldg, X, ldx, h, out, g.L, st);
}

}  // namespace pygim
