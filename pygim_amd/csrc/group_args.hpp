// group_args.hpp -- what pygim_group_create and pygim_group_create_transposed refuse, written once: the argument checks both make before any
// device work, and which error the validation kernels' flags stand for.  Pure: pointers are only compared with null, never followed past the
// tables the caller hands over.  tests/native/sweep_plan_main.cpp asks both on a CPU.
//
// Host-only C++17: no device header, no runtime state.
#pragma once
#include "../../include/pygim_hip.h"

#include <cstddef>
#include <cstdint>

namespace pygim {

struct ArgError {
    int code = 0;                // 0: nothing to refuse
    const char *text = nullptr;
};

// es: the bytes of an element of `dtype`, 0 for an unknown one.  The order is the order of the refusals: the call as a whole, then part by part
// equal rows, sizes that fit 32 bits, n_dense, a negative width, widths that add to h_size, a null index, a null colind.
inline ArgError check_group_args(int format, size_t es, int n_parts, const int32_t *const *idx0, const int32_t *const *colind, const int64_t *nrows,
                                 const int64_t *ncols, const int64_t *nnz, const int64_t *n_dense, const int64_t *dense_cols, int64_t h_size,
                                 const int64_t *out_handle) {
    if (format != PYGIM_CSR && format != PYGIM_COO) return {PYGIM_ERR_INVALID, "format must be CSR(0) or COO(1)"};
    if (es == 0) return {PYGIM_ERR_INVALID, "unknown dtype"};
    if (n_parts <= 0 || !idx0 || !colind || !nrows || !ncols || !nnz || !n_dense || !dense_cols || !out_handle)
        return {PYGIM_ERR_INVALID, "null argument or n_parts <= 0"};
    if (h_size <= 0) return {PYGIM_ERR_INVALID, "h_size must be positive"};
    size_t dpos = 0;
    for (int i = 0; i < n_parts; i++) {
        if (nrows[i] != nrows[0]) return {PYGIM_ERR_INVALID, "all sparse parts must have the same number of rows"};
        if (nrows[i] < 0 || ncols[i] < 0 || nnz[i] < 0 || nnz[i] > 0xFFFFFFFFll || nrows[i] >= 0xFFFFFFFFll || ncols[i] > 0xFFFFFFFFll)
            return {PYGIM_ERR_INVALID, "part sizes must fit 32-bit indices (the reference's uint32 matrices)"};
        if (n_dense[i] <= 0) return {PYGIM_ERR_INVALID, "n_dense must be positive"};
        int64_t sum = 0;
        for (int64_t j = 0; j < n_dense[i]; j++) {
            if (dense_cols[dpos + j] < 0) return {PYGIM_ERR_INVALID, "negative dense width"};
            sum += dense_cols[dpos + j];
        }
        dpos += (size_t)n_dense[i];
        if (sum != h_size) return {PYGIM_ERR_INVALID, "dense widths of a part must add up to h_size"};
        if (!idx0[i] && (format == PYGIM_CSR || nnz[i] > 0)) return {PYGIM_ERR_INVALID, "null index array"};
        if (!colind[i] && nnz[i] > 0) return {PYGIM_ERR_INVALID, "null colind"};
    }
    return {};
}

// flags: what k_check_csr / k_check_coo left behind -- [0] order (COO: rows not sorted; CSR: rowptr no prefix array), [1] an index out of range
inline ArgError group_validation_error(int format, const int *flags) {
    if (flags[1]) return {PYGIM_ERR_INVALID, "index out of range in a sparse part"};
    if (flags[0] && format == PYGIM_COO) return {PYGIM_ERR_UNSORTED, "COO row indices are not sorted (pass a coalesced tensor)"};
    if (flags[0]) return {PYGIM_ERR_INVALID, "rowptr is not a non-decreasing prefix array ending at nnz"};
    return {};
}

}  // namespace pygim
