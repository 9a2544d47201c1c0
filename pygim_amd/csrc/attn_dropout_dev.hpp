// attn_dropout_dev.hpp -- the mask of attention dropout: a pure function of (seed, entry index in A, head), specified bit for bit in
// include/pygim_hip.h ("attention dropout").  It keeps no state and depends neither on the launch shape nor on the direction the CSR
// is walked, so the fused forwards, both directions of the GATv2 backward, the elementwise mask kernel and the host mirror
// (pygim_attention_dropout_host) all call the ONE function below and drop the same entries.
//   fmix(x):  x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16              (uint32)
//   u(e, k)  = fmix(fmix(e ^ seed_lo) + seed_hi + k * 0x9E3779B9)                                           (mod 2^32)
//   keep     = u >= T,   T = min(2^32 - 1, floor(p * 2^32))
// The inner fmix depends on the entry alone: a lane that holds pieces of two heads pays it once (the compiler shares it).
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PYGIM_HOST_DEVICE __host__ __device__
#else
#define PYGIM_HOST_DEVICE
#endif

namespace pygim {

// what a kernel needs of (p, seed): the seed's halves, the threshold T and the weight 1 / (1 - p) of a kept entry
template <typename T> struct AttnDrop {
    uint32_t seed_lo, seed_hi, thr;
    T keep_w;
};

PYGIM_HOST_DEVICE inline bool attn_dropout_keep(uint32_t e, uint32_t k, uint32_t seed_lo, uint32_t seed_hi, uint32_t thr) {
    uint32_t x = e ^ seed_lo;
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    x += seed_hi + k * 0x9E3779B9u;
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x >= thr;
}

// T of a rate 0 <= p < 1 (the caller has checked it)
inline uint32_t attn_dropout_threshold(double p) {
    const double t = p * 4294967296.0;
    return t >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)t;
}

template <typename T> inline AttnDrop<T> attn_dropout_args(double p, uint64_t seed) {
    return AttnDrop<T>{(uint32_t)(seed & 0xFFFFFFFFull), (uint32_t)(seed >> 32), attn_dropout_threshold(p), (T)(1.0 / (1.0 - p))};
}

#if defined(__HIPCC__)
// w[i, k] = keep(entry_ids ? entry_ids[i] : i, k) ? 1 / (1 - p) : 0 for i < nnz, k < heads; [nnz, heads] contiguous
template <typename T>
__global__ __launch_bounds__(256) void k_attn_dropout_mask(uint64_t total, uint32_t heads, const int32_t *__restrict__ entry_ids, AttnDrop<T> dr,
                                                           T *__restrict__ mask) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const uint64_t e = i / heads;
    const uint32_t k = (uint32_t)(i - e * heads);
    const uint32_t id = entry_ids ? (uint32_t)entry_ids[e] : (uint32_t)e;
    mask[i] = attn_dropout_keep(id, k, dr.seed_lo, dr.seed_hi, dr.thr) ? dr.keep_w : T(0);
}
#endif

}  // namespace pygim
