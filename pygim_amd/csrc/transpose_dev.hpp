// transpose_dev.hpp -- A^T of a group's input on the device (the backward product dX = A^T . G of a conv layer's aggregation).
// A is what pygim_group_create's arguments describe: the column blocks side by side, nrows[0] x sum(ncols).  Row c of A^T lists the
// entries of global column c in the order they have in A (ascending row, stored order among duplicates): a stable sort of the row-major
// entries by global column -- np.argsort(col, kind="stable"), torch_sparse's t().  One-time set-up steps, bandwidth-bound passes over the
// entries; the sort is the code-stream encoder's (lds_codegen_dev.hpp cg_radix_sort) with the global column as key and the entry as payload.
#pragma once
#include <hip/hip_runtime.h>

#include "lds_codegen_dev.hpp"

namespace pygim {

// keys, payload, row ids and values of one part, written at entry offset e0 of the concatenation of all parts
// (T: an unsigned type of the element's size -- values are only moved; `one` is the bit pattern of 1 in the group's type)
template <typename T>
__global__ __launch_bounds__(256) void k_tr_keys(const uint32_t *__restrict__ idx0, const uint32_t *__restrict__ colind, const T *__restrict__ vals,
                                                 uint32_t nnz, uint32_t nrows, int is_csr, uint32_t col0, uint32_t e0, T one, uint64_t *__restrict__ keys,
                                                 uint32_t *__restrict__ pay, uint32_t *__restrict__ rows, T *__restrict__ vcat) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nnz) return;
    uint32_t r;
    if (is_csr) {
        // the last row that starts at or before entry i (rowptr[0] = 0 <= i < nnz = rowptr[nrows]: validated)
        uint32_t lo = 0, hi = nrows;
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (idx0[mid] <= (uint32_t)i) lo = mid;
            else hi = mid;
        }
        r = lo;
    } else {
        r = idx0[i];
    }
    keys[e0 + i] = (uint64_t)colind[i] + col0;
    pay[e0 + i] = e0 + (uint32_t)i;
    rows[e0 + i] = r;
    if (vcat) vcat[e0 + i] = vals ? vals[i] : one;
}

// entry j of A^T: column id = the row of the entry the sort put at j, value = its value; the sorted key as a 32-bit row index of A^T
template <typename T>
__global__ __launch_bounds__(256) void k_tr_gather(const uint64_t *__restrict__ skeys, const uint32_t *__restrict__ perm, const uint32_t *__restrict__ rows,
                                                   const T *__restrict__ vcat, uint64_t n, uint32_t *__restrict__ key32, uint32_t *__restrict__ colT,
                                                   T *__restrict__ valsT) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint32_t src = perm[j];
    key32[j] = (uint32_t)skeys[j];
    colT[j] = rows[src];
    if (vcat) valsT[j] = vcat[src];
}

// Input of one part on the device (validated: k_check_csr / k_check_coo passed).
struct TrPart {
    const uint32_t *idx0, *colind;
    const void *vals;   // nullptr = all ones
    uint32_t nrows, ncols, nnz;
    int is_csr;         // idx0 is a row pointer (else a row index per entry)
};

// Builds A^T as one CSR part: *rowptrT (ncolsT + 1 words), *colT and *valsT (nnzT entries; both nullptr when nnzT = 0, *valsT also when
// no part has values).  Everything is allocated here and handed to the caller; on failure nothing is left allocated.
template <typename T>
int tr_build_t(const std::vector<TrPart> &parts, T one, uint32_t **rowptrT, uint32_t **colT, void **valsT, uint64_t *ncolsT_out, uint64_t *nnzT_out,
               hipStream_t st, std::string *err) {
    uint64_t ncolsT = 0, nnzT = 0;
    bool valued = false;
    for (const TrPart &p : parts) {
        ncolsT += p.ncols;
        nnzT += p.nnz;
        valued |= p.vals != nullptr;
    }
    *rowptrT = *colT = nullptr;
    *valsT = nullptr;
    *ncolsT_out = ncolsT;
    *nnzT_out = nnzT;
    std::vector<void *> tmp;
    bool failed = false;
    auto dalloc = [&](size_t bytes) -> void * {
        void *q = nullptr;
        if (hipMalloc(&q, bytes ? bytes : 16) != hipSuccess) {
            (void)hipGetLastError();
            failed = true;
            return nullptr;
        }
        return q;
    };
    auto tfree = [&]() {
        for (void *q : tmp)
            if (q) (void)hipFree(q);
        tmp.clear();
    };
    auto bail = [&](const char *what) {
        (void)hipStreamSynchronize(st);
        tfree();
        for (void *q : {(void *)*rowptrT, (void *)*colT, *valsT})
            if (q) (void)hipFree(q);
        *rowptrT = *colT = nullptr;
        *valsT = nullptr;
        *err = what;
        return PYGIM_ERR_HIP;
    };
    *rowptrT = (uint32_t *)dalloc((ncolsT + 1) * 4);
    if (failed) return bail("transpose: out of device memory (row pointer)");
    if (nnzT == 0) {
        if (hipMemsetAsync(*rowptrT, 0, (ncolsT + 1) * 4, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return bail("transpose: empty row pointer");
        return 0;
    }
    uint64_t *keys_a = (uint64_t *)dalloc(nnzT * 8), *keys_b = (uint64_t *)dalloc(nnzT * 8);
    uint32_t *pay_a = (uint32_t *)dalloc(nnzT * 4), *pay_b = (uint32_t *)dalloc(nnzT * 4), *rows = (uint32_t *)dalloc(nnzT * 4);
    T *vcat = valued ? (T *)dalloc(nnzT * sizeof(T)) : nullptr;
    const uint32_t sort_tiles = cg_sort_tiles(nnzT);
    uint32_t *d_hist = (uint32_t *)dalloc(((size_t)256 * sort_tiles + 1) * 4);
    uint32_t *d_scan = (uint32_t *)dalloc(cg_scan_scratch_words((uint64_t)256 * sort_tiles) * 4);
    tmp = {keys_a, keys_b, pay_a, pay_b, rows, vcat, d_hist, d_scan};
    if (failed) return bail("transpose: out of device memory (sort)");
    uint64_t e0 = 0, c0 = 0;
    for (const TrPart &p : parts) {
        if (p.nnz > 0)
            hipLaunchKernelGGL((k_tr_keys<T>), dim3((unsigned)(((uint64_t)p.nnz + 255) / 256)), dim3(256), 0, st, p.idx0, p.colind, (const T *)p.vals, p.nnz,
                               p.nrows, p.is_csr, (uint32_t)c0, (uint32_t)e0, one, keys_a, pay_a, rows, vcat);
        e0 += p.nnz;
        c0 += p.ncols;
    }
    uint32_t key_bits = 0;
    while (key_bits < 64 && (ncolsT >> key_bits) != 0) key_bits++;
    cg_radix_sort(&keys_a, &keys_b, &pay_a, &pay_b, nnzT, std::max<uint32_t>(key_bits, 1), d_hist, d_scan, st);
    uint32_t *key32 = (uint32_t *)keys_b;   // (the other key buffer is free after the sort)
    *colT = (uint32_t *)dalloc(nnzT * 4);
    if (valued) *valsT = dalloc(nnzT * sizeof(T));
    if (failed) return bail("transpose: out of device memory (result)");
    hipLaunchKernelGGL((k_tr_gather<T>), dim3((unsigned)((nnzT + 255) / 256)), dim3(256), 0, st, (const uint64_t *)keys_a, (const uint32_t *)pay_a,
                       (const uint32_t *)rows, (const T *)vcat, nnzT, key32, *colT, (T *)*valsT);
    hipLaunchKernelGGL(k_coo_rowptr, dim3((unsigned)((nnzT + 1 + 255) / 256)), dim3(256), 0, st, (const uint32_t *)key32, (uint32_t)nnzT, (uint32_t)ncolsT,
                       *rowptrT);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return bail("transpose: kernels failed");
    tfree();
    return 0;
}

}  // namespace pygim
