/*
 * pygim_hip.h -- C ABI of the MI355X (gfx950) aggregation backend.
 *
 * This is the drop-in boundary for PyGim's backend_pim SpMM/SpMV path: every
 * entry point replaces one function the reference reaches through
 * torch.ops.pim_ops.* (registered in backend_pim/<variant>/pytorch_api.cpp).
 * Plain pointers and sizes only; no torch types.  All functions return 0 on
 * success and a non-zero pygim_status otherwise; pygim_last_error() then holds a
 * message (thread-local).
 *
 * Pointer convention: every data pointer may be a HOST pointer or a DEVICE (HIP)
 * pointer; the library asks the HIP runtime which.  Host data is staged through
 * device buffers owned by the group (one-time for the sparse arrays -- the
 * reference's copy_sparse_csr/copy_sparse_coo -- and per call for dense parts).
 * Device data is used in place: the caller keeps it alive for the lifetime of
 * the group, the same ownership rule the reference has for the raw data_ptr()s
 * it stores (spmm_default/pytorch_api.cpp:230-232, 312-314).
 *
 * Threading: like the reference (one process-global `dpus` singleton,
 * spmm_default/pytorch_api.cpp:152) the library holds one device context per
 * process; calls are not re-entrant for the same group handle.  The tunables are
 * process-global.  The slice-major copy of X that the panel sweep gathers from lives in
 * one buffer per (device, launch stream), so products on different streams do not
 * disturb each other; at most four are kept (least recently used goes first) and all
 * are freed with the last group.  A caller that runs several products on the SAME
 * unchanged X says so per call (the x_unchanged argument of pygim_spmm_run_group_x /
 * pygim_block_run_x): the copy made by the most recent product on exactly that operand
 * (pointer, stride, shape) is then shared instead of repeated; the caller orders the
 * streams itself (an event after the first product, as bench.py does) and must not
 * pass the flag after writing to X.
 * Scratch buffers are sized on first use (hipMalloc), so capture a product into a hipGraph only after one warm-up call.
 * A captured graph bakes in the addresses of the slice-major buffer of its capture stream and of the group's scratch
 * buffers: while such a graph may still be replayed, do not run products on four or more OTHER streams of the same
 * device (the least recently used slice-major buffer is freed), do not run a LARGER product on the capture stream
 * (its buffer is re-allocated) and do not free the group -- inference.py --graph 1 keeps to one stream and one shape.
 */
#ifndef PYGIM_HIP_H
#define PYGIM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    PYGIM_OK = 0,
    PYGIM_ERR_INVALID = 1,   /* bad argument / shape / dtype / handle          */
    PYGIM_ERR_NO_DEVICE = 2, /* no HIP device, or pygim_init not called         */
    PYGIM_ERR_HIP = 3,       /* a HIP runtime call failed                       */
    PYGIM_ERR_UNSORTED = 4   /* COO input not sorted by row (must be coalesced) */
} pygim_status;

/* val_dt of the reference (spmm_default/support/common.h:39-60), chosen at run
 * time here instead of one library per type. */
typedef enum {
    PYGIM_INT8 = 0,
    PYGIM_INT16 = 1,
    PYGIM_INT32 = 2,
    PYGIM_INT64 = 3,
    PYGIM_FLT32 = 4,
    PYGIM_DBL64 = 5,
    /* 16-bit FEATURE types (IEEE binary16, bfloat16).  Valid only for pygim_sddmm, pygim_spmm_values, pygim_gat_aggregate,
     * pygim_sparse_attention, pygim_gatv2_aggregate, pygim_gatv2_backward (and the *_dropout forms of these four, pygim_gat_aggregate_edge, pygim_sparse_attention_bias), pygim_spmm_reduce with PYGIM_REDUCE_MEAN and their *_workspace functions ("16-bit features" below); every other entry
     * point -- group creation, edge softmax, the max / min reductions and their backward, the quantisers -- rejects them like
     * an unknown type. */
    PYGIM_FLT16 = 6,
    PYGIM_BF16 = 7
} pygim_dtype;

/* ---- 16-bit features ----
 * With PYGIM_FLT16 / PYGIM_BF16 the feature matrices are STORED in 16 bits and everything else is float32:
 *   pygim_sddmm          G, X 16-bit;      out [nnz] float32 (nothing is rounded)
 *   pygim_spmm_values    X, out 16-bit;    values float32
 *   pygim_gat_aggregate  X, out 16-bit;    a_dst, a_src, lse float32
 *   pygim_sparse_attention  Q, K, V, out 16-bit;  products, scores and lse float32
 *   pygim_gatv2_aggregate   x_dst, x_src, out 16-bit;  att, z, scores and lse float32
 *   pygim_gatv2_backward    x_own, x_oth, G, d_own 16-bit;  att, lse, delta, datt float32
 *   pygim_spmm_reduce   X, out 16-bit;    values float32 or NULL; PYGIM_REDUCE_MEAN only (MAX / MIN: PYGIM_ERR_INVALID)
 * Strides (ldx, ldo, ldg) count 16-bit elements.  An element of X is widened to float32 as it is read (exact) and the arithmetic is
 * the FLT32 arithmetic of the call: accumulators, the exchange between lane groups, the workspace slots of rows cut across waves and
 * the kernels that join them, the online-softmax state (m, l, acc), the mean's division and lse are float32 -- so the *_workspace
 * functions return the FLT32 sizes for these codes.  A result is rounded ONCE, round-to-nearest-even, where a finished row is
 * stored into out (NaN stays NaN; a FLT16 result beyond 65504 becomes +-inf).  Empty rows store 16-bit zeros (lse = 0.0f).
 * Bounds, with u = 2^-11 (FLT16) / 2^-8 (BF16), the half-ulp of that one rounding, and `exact` the exact result on the 16-bit inputs:
 *   spmm_values, mean     |out - exact| <= u |exact| + the FLT32 bound of the call (1e-5 sum |value . x|; the mean's divided by the count)
 *   gat_aggregate         |out - exact| <= u |exact| + 2e-5 sum_e p[e] |x[e]|;  lse as for FLT32
 *   sparse_attention, gatv2_aggregate   |out - exact| <= u |exact| + the FLT32 bound of the call;  lse as for FLT32
 *   sddmm                 the FLT32 bound (1e-5 sum_f |G . X|)
 * 16-byte gathers need (h / heads) % 8 == 0, strides that are multiples of 8 elements and 16-byte aligned X / G / out; otherwise a
 * lane reads one element.  No atomics and fixed orders as for FLT32: the same bits on every launch. */

typedef enum { PYGIM_CSR = 0, PYGIM_COO = 1 } pygim_format;

/* ---- device set-up --------------------------------------------------------
 * pygim_init_ranks replaces dpu_init_ranks (spmm_default/pytorch_api.cpp:154,
 * spmv_sparseP/pytorch_api.cpp:132; grande's int[]-returning form
 * spmm_grande/pytorch_api.cpp:157-166).  nr_ranks = number of (sparse part x
 * dense part) partitions the caller will create.  If units_per_rank is not NULL
 * it receives nr_ranks entries: the number of feature windows the grande layout
 * should cut per sparse part (grande's "DPUs per rank"; here one window per XCD).
 * pygim_init_units replaces dpu_init_dpus (:158 / grande :168-177).
 * pygim_release replaces dpu_release (:162): frees every live group.          */
int pygim_init_ranks(int64_t nr_ranks, int64_t *units_per_rank);
int pygim_init_units(int64_t nr_units, int64_t *units_per_rank, int64_t *nr_ranks_out);
int pygim_release(void);
/* number of pygim_release calls so far: a handle made under an earlier generation is dead (every group was freed),
 * even when the allocator hands the same address out again -- wrappers that cache a handle compare this. */
int64_t pygim_generation(void);
/* creation serial of a live group (1, 2, 3 ... over the life of the process, never reused): a handle is an address, and the allocator may hand
 * a freed group's address to the next one -- a wrapper that frees what it created (the reference's spmm_free_group,
 * spmm_default/pytorch_api.cpp:198-201, is the caller's to call) remembers the serial and frees only while it still matches. */
int pygim_group_serial(int64_t handle, int64_t *out);
int pygim_is_initialized(void);
const char *pygim_last_error(void);
/* name / CU count / bytes of HBM of the device in use */
int pygim_device_info(char *name, int name_len, int *cu_count, int64_t *hbm_bytes);

/* ---- sparse group: create / free -------------------------------------------
 * Replaces spmm_csr_to_device_group / spmm_coo_to_device_group
 * (spmm_default/pytorch_api.cpp:204-243, 286-329), grande's
 * spmm_csr_to_device_group (spmm_grande/pytorch_api.cpp:221-264) and
 * spmv_coo_to_device_group (spmv_sparseP/pytorch_api.cpp:184-228).
 *
 *  n_parts          sparse column blocks of A (backend_pim/spmm.py:127-136);
 *                   block i is nrows[i] x ncols[i] with LOCAL column ids.
 *  idx0[i]          CSR: rowptr, nrows[i]+1 int32;  COO: row index, nnz[i] int32,
 *                   sorted by (row, col) as torch's coalesce() leaves it.
 *  colind[i]        nnz[i] int32.
 *  values[i]        nnz[i] elements of `dtype`; values == NULL or values[i] ==
 *                   NULL means all-ones (backend_pim/spmm.py:36-37, 48-49).
 *  n_dense[i]       number of dense (feature) parts paired with sparse part i.
 *                   Default/spmv layout: the same list for every part -- pass the
 *                   count in n_dense[0..n_parts) and the widths once per part.
 *  dense_cols       concatenated widths, sum_i n_dense[i] entries; for each part
 *                   they must add up to h_size.
 *  out_handle       opaque handle (the reference returns its csr_info_group*
 *                   as an int64, pytorch_api.cpp:240).
 */
int pygim_group_create(int format, int dtype, int n_parts,
                       const int32_t *const *idx0, const int32_t *const *colind,
                       const void *const *values, const int64_t *nrows, const int64_t *ncols,
                       const int64_t *nnz, const int64_t *n_dense, const int64_t *dense_cols,
                       int64_t h_size, int64_t *out_handle);
/* Replaces spmm_free_group (spmm_default/pytorch_api.cpp:198-201). */
int pygim_group_free(int64_t handle);
/* The group of A^T, for the backward product dX = A^T . G of an aggregation: exactly pygim_group_create's arguments,
 * where A is the matrix they describe (the column blocks side by side, nrows[0] x sum(ncols)).  The input is validated
 * with the same checks and error codes, host arrays are uploaded once and device arrays read in place (they need not
 * outlive the call), and the transpose runs on the device.  Row c of A^T lists the entries of global column c in the
 * order they have in A: ascending row, stored order among duplicates (a stable sort by column, torch_sparse's t());
 * part i's columns become the rows from sum_{j<i} ncols[j] on.  The result is an ordinary group -- one CSR sparse part of
 * sum(ncols) x nrows[0], the same dtype and h_size, one dense part of width h_size -- built by the same creation path
 * (unit weights, plans, code streams and fallbacks as for any group) with its own serial; pygim_group_free or
 * pygim_release frees it.  All six types, CSR or COO input.                                                          */
int pygim_group_create_transposed(int format, int dtype, int n_parts,
                                  const int32_t *const *idx0, const int32_t *const *colind,
                                  const void *const *values, const int64_t *nrows, const int64_t *ncols,
                                  const int64_t *nnz, const int64_t *n_dense, const int64_t *dense_cols,
                                  int64_t h_size, int64_t *out_handle);

/* ---- run -----------------------------------------------------------------
 * pygim_spmm_run_group replaces spmm_csr_run_group / spmm_coo_run_group
 * (spmm_default/pytorch_api.cpp:248-280, 332-367): B_parts[j] is a row-major
 * [total_cols, dense_cols[j]] array holding feature block j of X for ALL sparse
 * parts (sparse part i reads the rows that start at the sum of the previous
 * parts' ncols, spmm_mul_csr.c:356-363); out is row-major [nrows[0], h_size] and
 * is fully overwritten (the reference returns a fresh torch::zeros + merge).
 *
 * pygim_grande_run_group replaces grande's spmm_csr_run_group
 * (spmm_grande/pytorch_api.cpp:269-321): B_windows holds, part after part, one
 * window per dense part of that sparse part, each row-major
 * [ncols[i], window_ld[k]] of which the first dense_cols[k] columns are used
 * (backend_pim/grande.py:12-23 pads windows to 8 bytes).
 *
 * pygim_spmv_run_group replaces spmv_coo_run_group
 * (spmv_sparseP/pytorch_api.cpp:231-266): B_vectors[j] is vector j ([ncols,1]);
 * out is [nrows[0], n_dense] -- one SpMV result per column.
 *
 * stream: a hipStream_t (NULL = the default stream).  With device pointers the
 * call only enqueues work; with host pointers it returns after the result has
 * been copied back.
 *
 * Non-finite operands (FLT32 / DBL64; every form of the product -- row per wave,
 * long-row segments, native COO, the SpMV end, the panel sweep, the LDS-staged
 * forms, the density split, merged and unmerged parts, host windows, the
 * transposed group -- is held to this by tests/test_group_nonfinite_gpu.py):
 *   - a NaN or infinite feature or value reaches exactly the outputs the CPU
 *     loop (oracle/spmm_oracle.c) gives it to: NaN where that loop has NaN, the
 *     loop's bits everywhere else -- lanes, tokens and slots that do no work add
 *     nothing, whatever X holds in the column they point at;
 *   - a stored 0 times an infinity is NaN;
 *   - no explicit zero is dropped, at creation or in a kernel;
 *   - a product never returns -0.0: every sum starts from +0.
 * (Finite sums that mix magnitudes round by the order a form adds them in; that
 * is each form's tolerance, stated with it, and not part of this contract.)   */
int pygim_spmm_run_group(int64_t handle, const void *const *B_parts, void *out, void *stream);
/* the same with x_unchanged (see "Threading" above): 1 = B_parts hold exactly what the most
 * recent product on the same pointers held, its slice-major copy may be reused.   */
int pygim_spmm_run_group_x(int64_t handle, const void *const *B_parts, void *out, int x_unchanged,
                           void *stream);
int pygim_grande_run_group(int64_t handle, const void *const *B_windows, const int64_t *window_ld,
                           void *out, void *stream);
int pygim_spmv_run_group(int64_t handle, const void *const *B_vectors, void *out, void *stream);

/* One block product on resident data, the building brick of the three calls
 * above and of the multi-GPU layer: C[0:nrows, c_col0 : c_col0+width] (+)=
 * A_part . X[:, 0:width] with row strides ldx / ldc in elements.  X and C must
 * be device pointers.                                                         */
int pygim_block_run(int64_t handle, int part, const void *X, int64_t ldx, void *C, int64_t ldc,
                    int64_t width, int accumulate, void *stream);
int pygim_block_run_x(int64_t handle, int part, const void *X, int64_t ldx, void *C, int64_t ldc,
                      int64_t width, int accumulate, int x_unchanged, void *stream);

/* ---- quantise -> aggregate -> dequantise (the step either side of the product in every conv layer,
 * models/pyg_gcn_conv.py:130-137 with models/quantize.py:20-42), on device in one call:
 *   scale = max|X| * 2 / 2^k (k = 5 / 10 / 20 for INT8 / INT16 / INT32 groups; 20 for FLT32),
 *   X_q = round_half_even(X / scale) in the group's type, out_q = A . X_q, out = float(out_q) * scale.
 * X: float32 [total_cols, h] (row stride ldx), out: float32 [nrows, h]; device pointers.
 * scale_out (device float, may be NULL) receives the scale.                     */
int pygim_quant_spmm_run(int64_t handle, const float *X, int64_t ldx, float *out, float *scale_out, void *stream);
/* the same with a per-column epilogue applied in the last store of every row (the sweep's, or the LDS-staged kernel's):
 *   out[r, f] = col_mul[f] * out[r, f] + col_add[f], then max(., 0) when relu != 0
 * (what follows the aggregation in a GCN layer -- + bias, eval-mode BatchNorm, ReLU, models/models.py:30-38 -- folded into
 * one affine map per feature; col_mul / col_add: device float[h]; both NULL = no epilogue).                              */
int pygim_quant_spmm_run_post(int64_t handle, const float *X, int64_t ldx, float *out, float *scale_out,
                              const float *col_mul, const float *col_add, int relu, void *stream);

/* The same quantiser in its three steps, for callers that exchange the QUANTISED features between them
 * (row-sharded multi-GPU inference: every rank quantises its row block with the global scale, the blocks
 * are all-gathered in the narrow type, each rank aggregates its rows and dequantises them).
 *   absmax_bits: device uint32 holding the bit pattern of max|X| (a non-negative float orders like an
 *   unsigned integer, so ranks combine it with an integer MAX all-reduce); pygim_quant_absmax
 *   max-accumulates into it, the caller zeroes it first.
 *   pygim_quantize: Xq[rows, width] contiguous in `dtype` (INT8/INT16/INT32/FLT32) = round_half_even(X / scale).
 *   pygim_dequantize: out[i] = float(Q[i]) * scale.                                     */
int pygim_quant_absmax(const float *X, int64_t ldx, int64_t rows, int64_t width, uint32_t *absmax_bits, void *stream);
int pygim_quantize(int dtype, const float *X, int64_t ldx, int64_t rows, int64_t width, const uint32_t *absmax_bits,
                   void *Xq, float *scale_out, void *stream);
int pygim_dequantize(int dtype, const void *Q, int64_t n, const uint32_t *absmax_bits, float *out, void *stream);
/* the last two of those steps in one sweep: out = float(A . Xq) * scale, Xq [total_cols, h] already quantised in the
 * group's type (row stride ldx), the dequantisation done by the sweep's last store per row (no integer result matrix). */
int pygim_spmm_run_dequant(int64_t handle, const void *Xq, int64_t ldx, float *out, const uint32_t *absmax_bits, void *stream);

/* ---- sampled dense-dense product (the gradient of an aggregation with respect to the edge values) ----
 *   out[e] = sum_f G[row(e), f] * X[colind[e], f]   for every stored entry e of the CSR (rowptr: nrows + 1, colind: nnz),
 * in stored order.  G: [nrows, h] with row stride ldg, X: [max column + 1, h] with row stride ldx, out: nnz elements; any
 * h >= 1, nnz = 0 and empty rows allowed.  FLT32 and DBL64 (FLT16 / BF16: G and X 16-bit, out float32 -- "16-bit features" above), else
 * PYGIM_ERR_INVALID; device pointers only, the
 * caller guarantees a valid CSR (rowptr non-decreasing from 0 to nnz, column ids inside X).  Every entry owns its output:
 * no atomics, the same bits on every run; each sum is a fixed-order sum over the features (within 1e-5 (FLT32) /
 * 1e-12 (DBL64) of sum_f |G . X| of the exact value).  Only enqueues work on `stream`.                                */
int pygim_sddmm(int dtype, int64_t nrows, const int32_t *rowptr, const int32_t *colind, int64_t nnz, const void *G,
                int64_t ldg, const void *X, int64_t ldx, int64_t h, void *out, void *stream);

/* ---- products and softmax whose edge values are an operand of the call (attention, gates, learned normalisation) ----
 * Functional entry points on a caller's CSR like pygim_sddmm: no group handle, device pointers only, FLT32 and DBL64 only (else
 * PYGIM_ERR_INVALID; pygim_spmm_values also takes FLT16 / BF16 with float32 values -- "16-bit features" above), int32 rowptr / colind with nnz <= 2^31 - 1, a valid CSR guaranteed by the caller.  nnz = 0, empty rows and any
 * h >= 1 are allowed.  They only enqueue work on `stream`: no allocation, no synchronisation.  Scratch comes from the caller:
 * `workspace` holds at least the bytes the matching *_workspace function returns (a function of its arguments alone, never of the
 * CSR's contents; -1 for bad arguments), is 16-byte aligned, and must not be shared by calls that may overlap.  No float atomics:
 * rows cut across waves leave partial results in the workspace and a second kernel folds them in a fixed order, so every launch
 * stores the same bits.
 *
 *   pygim_spmm_values:  out[r, f] = sum over the entries e of row r of values[e * heads + f / (h / heads)] * X[colind[e], f]
 *     values: [nnz, heads] contiguous, heads >= 1 divides h; X: row stride ldx >= h; out[0:nrows, 0:h] (row stride ldo >= h) is
 *     overwritten, empty rows with zeros.  Within 1e-5 (FLT32) / 1e-12 (DBL64) of sum |value . x| of the exact value.
 *   pygim_edge_softmax:  out[e, k] = exp(s[e, k] - m) / sum_{e' in row(e)} exp(s[e', k] - m), m the row's and head's maximum;
 *     scores and out: [nnz, heads] contiguous; the sum runs over the row's stored entries (duplicates are separate entries); stable
 *     for finite scores of any magnitude.
 *     Non-finite scores (here and in pygim_gat_aggregate and pygim_sparse_attention below, whose scores are computed from a_src / K;
 *     pygim_gatv2_aggregate has no masking input: x_src is score and value at once, so a non-finite x_src makes NaN the (row, head)s
 *     that gather it, and only those): a score of -inf masks its entry --
 *     its probability is exactly 0 and the softmax of the (row, head) runs over the rest, wherever the masked entries stand in the row;
 *     heads are independent.  A (row, head) whose scores are ALL -inf is 0 / 0: NaN probabilities / NaN out over the head's features,
 *     lse = -inf (torch.softmax, torch.logsumexp).  One +inf or NaN score makes its (row, head) NaN and nothing else.  Non-finite
 *     features (X, V) stay in the outputs they are summed into: NaN and +-inf propagate as in a plain sum, nowhere else (a masked
 *     entry's features are still multiplied by its probability 0, so they must be finite).
 *   pygim_edge_softmax_backward:  out[e, k] = P[e, k] * (dP[e, k] - sum_{e' in row(e)} P[e', k] * dP[e', k]).                          */
int64_t pygim_spmm_values_workspace(int dtype, int64_t nrows, int64_t nnz, int64_t h, int64_t heads);
int pygim_spmm_values(int dtype, int64_t nrows, const int32_t *rowptr, const int32_t *colind, int64_t nnz, const void *values,
                      int64_t heads, const void *X, int64_t ldx, int64_t h, void *out, int64_t ldo, void *workspace,
                      int64_t workspace_bytes, void *stream);
int64_t pygim_edge_softmax_workspace(int dtype, int64_t nrows, int64_t nnz, int64_t heads);
int pygim_edge_softmax(int dtype, int64_t nrows, const int32_t *rowptr, int64_t nnz, const void *scores, int64_t heads, void *out,
                       void *workspace, int64_t workspace_bytes, void *stream);
int pygim_edge_softmax_backward(int dtype, int64_t nrows, const int32_t *rowptr, int64_t nnz, const void *P, const void *dP,
                                int64_t heads, void *out, void *workspace, int64_t workspace_bytes, void *stream);
/*   pygim_gat_aggregate:  the aggregation of a GAT layer in one pass over the stored entries -- scores, softmax and product, with
 *     nothing of size nnz read (besides colind) or written:
 *       s[e, k]   = leaky_relu(a_dst[r, k] + a_src[colind[e], k], negative_slope)     e over the entries of row r, k = f / (h / heads)
 *       out[r, f] = sum_e exp(s[e, k] - m[r, k]) * X[colind[e], f] / l[r, k],   m = max_e s,  l = sum_e exp(s - m)
 *       lse[r, k] = m[r, k] + log(l[r, k])        when lse is not NULL ([nrows, heads] contiguous)
 *     The contract of pygim_spmm_values: FLT32 and DBL64 (FLT16 / BF16: X and out 16-bit, a_dst / a_src / lse float32), device pointers only, a valid CSR guaranteed by the caller, nnz = 0,
 *     empty rows and any h >= 1 allowed, heads >= 1 divides h, row strides ldx, ldo >= h, work is only enqueued on `stream`, scratch
 *     from the caller (pygim_gat_aggregate_workspace bytes: a function of its arguments alone, -1 for bad arguments; 16-byte
 *     aligned), no atomics, the same bits on every launch.  a_dst: [nrows, heads], a_src: [max column + 1, heads], both contiguous.
 *     Duplicates are separate entries; empty rows store out = 0 and lse = 0; out has the same bits with and without lse.  An online
 *     softmax (running maximum, rescaled sum and accumulator): stable for finite scores of any magnitude.  Within 2e-5 (FLT32) /
 *     2e-12 (DBL64) of sum_e p[e] * |x[e]| of the exact value, p the exact probabilities: the bounds of pygim_edge_softmax and
 *     pygim_spmm_values added.  PYGIM_ERR_INVALID: an integer type, heads not dividing h, a workspace too small or misaligned.    */
int64_t pygim_gat_aggregate_workspace(int dtype, int64_t nrows, int64_t nnz, int64_t h, int64_t heads);
int pygim_gat_aggregate(int dtype, int64_t nrows, const int32_t *rowptr, const int32_t *colind, int64_t nnz,
                        const void *a_dst /* [nrows, heads] */, const void *a_src /* [ncols, heads] */, int64_t heads,
                        double negative_slope, const void *X, int64_t ldx, int64_t h, void *out, int64_t ldo,
                        void *lse /* [nrows, heads] or NULL */, void *workspace, int64_t workspace_bytes, void *stream);
/*   pygim_sparse_attention:  scaled dot-product attention over the stored entries (TransformerConv, graph transformers) in one pass
 *     -- scores, softmax and product, with nothing of size nnz read (besides colind) or written:
 *       s[e, k]   = scale * sum_{f in head k} Q[r, f] * K[colind[e], f]      e over the entries of row r, hd = h / heads, k = f / hd
 *       out[r, f] = sum_e exp(s[e, k] - m[r, k]) * V[colind[e], f] / l[r, k],   m = max_e s,  l = sum_e exp(s - m)
 *       lse[r, k] = m[r, k] + log(l[r, k])        when lse is not NULL ([nrows, heads] contiguous)
 *     The contract of pygim_gat_aggregate: FLT32 and DBL64 (FLT16 / BF16: Q, K, V and out 16-bit, lse float32), device pointers only,
 *     a valid CSR guaranteed by the caller, nnz = 0 and empty rows allowed (out = 0, lse = 0), heads >= 1 divides h, Q: [nrows, h],
 *     K and V: [max column + 1, h], row strides ldq, ldk, ldv, ldo >= h, work is only enqueued on `stream`, scratch from the caller
 *     (pygim_sparse_attention_workspace bytes, 16-byte aligned), no atomics, the same bits on every launch, out has the same bits
 *     with and without lse.  A head is at most 256 features wide (h / heads <= 256; any heads >= 1): wider heads are rejected.  The
 *     dot product of an entry is a fixed-order sum (a lane's features in ascending order, then an xor butterfly over the head's
 *     lanes); the softmax is the online one of pygim_gat_aggregate, stable for finite scores of any magnitude.
 *     Bounds, with EPS = 1e-5 (FLT32, FLT16, BF16) / 1e-12 (DBL64), p the exact probabilities and
 *     Delta[r, k] = EPS * |scale| * max_e sum_{f in head k} |Q[r, f] * K[colind[e], f]|   (the pygim_sddmm bound on a score):
 *       |out - exact| <= (2 EPS + 2 Delta[r, k]) * sum_e p[e] * |v[e]|     (a score error of Delta moves a probability by at most
 *                                                                           e^(2 Delta) - 1)
 *       |lse - exact| <= 2 EPS * (1 + |exact|) + Delta[r, k]
 *     and for FLT16 / BF16 the one rounding of out added: u |exact|, u = 2^-11 / 2^-8, exact on the 16-bit inputs.
 *     PYGIM_ERR_INVALID (-1 from the workspace function): an integer type, heads not dividing h, h / heads > 256, a workspace too
 *     small or misaligned.                                                                                                          */
int64_t pygim_sparse_attention_workspace(int dtype, int64_t nrows, int64_t nnz, int64_t h, int64_t heads);
int pygim_sparse_attention(int dtype, int64_t nrows, const int32_t *rowptr, const int32_t *colind, int64_t nnz,
                           const void *Q, int64_t ldq, const void *K, int64_t ldk, const void *V, int64_t ldv,
                           int64_t h, int64_t heads, double scale, void *out, int64_t ldo,
                           void *lse /* [nrows, heads] or NULL */, void *workspace, int64_t workspace_bytes, void *stream);
/*   pygim_gatv2_aggregate:  the aggregation of a GATv2 layer (Brody et al.; PyG's GATv2Conv) in one pass -- scores, softmax and
 *     product, with nothing of size nnz read (besides colind) or written:
 *       z[e, f]   = x_dst[r, f] + x_src[colind[e], f]                   e over the entries of row r, hd = h / heads, k = f / hd
 *       s[e, k]   = sum_{f in head k} att[f] * lrelu(z[e, f])           lrelu(z) = z > 0 ? z : negative_slope * z
 *       out[r, f] = sum_e exp(s[e, k] - m[r, k]) * x_src[colind[e], f] / l[r, k],   m = max_e s,  l = sum_e exp(s - m)
 *       lse[r, k] = m[r, k] + log(l[r, k])        when lse is not NULL ([nrows, heads] contiguous)
 *     The contract of pygim_sparse_attention: FLT32 and DBL64 (FLT16 / BF16: x_dst, x_src and out 16-bit; att, z, the scores and lse
 *     float32), device pointers only, a valid CSR guaranteed by the caller, nnz = 0 and empty rows allowed (out = 0, lse = 0),
 *     heads >= 1 divides h, x_dst: [nrows, h], x_src: [max column + 1, h], att: [h] contiguous, row strides ld_dst, ld_src, ldo >= h,
 *     work is only enqueued on `stream`, scratch from the caller (pygim_gatv2_aggregate_workspace bytes, 16-byte aligned), no
 *     atomics, the same bits on every launch, out has the same bits with and without lse.  A head is at most 256 features wide
 *     (h / heads <= 256): wider heads are rejected.  One gathered row per entry serves the score and the product.  A score is a
 *     fixed-order sum (a lane's features in ascending order, then an xor butterfly over the head's lanes); the softmax is the online
 *     one of pygim_gat_aggregate.  Bounds: those of pygim_sparse_attention with
 *       Delta[r, k] = EPS * max_e sum_{f in head k} |att[f] * lrelu(z[e, f])|,   EPS = 1e-5 (FLT32, FLT16, BF16) / 1e-12 (DBL64):
 *       |out - exact| <= (2 EPS + 2 Delta[r, k]) * sum_e p[e] * |x_src[e]|       |lse - exact| <= 2 EPS * (1 + |exact|) + Delta[r, k]
 *     and for FLT16 / BF16 the one rounding of out added: u |exact|, u = 2^-11 / 2^-8, exact on the 16-bit inputs.
 *     PYGIM_ERR_INVALID (-1 from the workspace function): an integer type, heads not dividing h, h / heads > 256, a workspace too
 *     small or misaligned.
 *   pygim_gatv2_backward:  one direction of its backward, a gather over "own row i, gathered row j" of the CSR it is given, with
 *     z = x_own[i] + x_oth[j]; the probabilities are recomputed from lse, nothing of size nnz is read or written.  With G = dout
 *     ([rows of A, h], row stride ldg), lse as the forward stored it and delta[r, k] = sum_{f in head k} G[r, f] * out[r, f] (both
 *     [rows of A, heads] contiguous, computed by the caller; for FLT16 / BF16 float32, delta from the stored, once-rounded out as
 *     FlashAttention's backward takes it):
 *       p = exp(s - lse[r, k])     dp = sum_{f in head k} G[r, f] * x_src[c, f]     ds = p * (dp - delta[r, k])
 *       t[e, f] = ds * att[f] * lrelu'(z[e, f])          lrelu'(z) = z > 0 ? 1 : negative_slope  (z == 0 takes the slope, as torch does)
 *     transposed = 0, on the CSR of A (nrows = rows of A): x_own = x_dst, x_oth = x_src; G, lse, delta belong to the own row;
 *       d_own[r, f] = dx_dst = sum_{e in row r} t[e, f];   datt[f] = sum_e ds * lrelu(z[e, f])   ([h] contiguous; NULL: not computed)
 *     transposed = 1, on the CSR of A^T (nrows = columns of A, colind = the A-row of every entry; no permutation is needed): x_own =
 *       x_src, x_oth = x_dst; G, lse, delta belong to the gathered row;  d_own[c, f] = dx_src = sum_{e with col = c} (p * G[r, f] + t[e, f]);
 *       datt must be NULL.
 *     d_own[0:nrows, 0:h] (row stride ldd >= h) is overwritten, rows without entries with zeros; nnz = 0 stores zeros, datt included.
 *     Types, pointers, strides, the head cap and the stream as for pygim_gatv2_aggregate (FLT16 / BF16: x_own, x_oth, G and d_own
 *     16-bit, each row of d_own rounded once; att, lse, delta, datt and every sum float32).  Row sums are fixed-order sums, rows cut
 *     across waves meet in the workspace in wave order; datt is summed per wave, then level by level in a fixed order: no atomics,
 *     the same bits on every launch.  pygim_gatv2_backward_workspace serves both directions.  PYGIM_ERR_INVALID: as for
 *     pygim_gatv2_aggregate, and datt non-NULL with transposed.                                                                      */
int64_t pygim_gatv2_aggregate_workspace(int dtype, int64_t nrows, int64_t nnz, int64_t h, int64_t heads);
int pygim_gatv2_aggregate(int dtype, int64_t nrows, const int32_t *rowptr, const int32_t *colind, int64_t nnz,
                          const void *x_dst, int64_t ld_dst, const void *x_src, int64_t ld_src, const void *att /* [h] */,
                          int64_t h, int64_t heads, double negative_slope, void *out, int64_t ldo,
                          void *lse /* [nrows, heads] or NULL */, void *workspace, int64_t workspace_bytes, void *stream);
int64_t pygim_gatv2_backward_workspace(int dtype, int64_t nrows, int64_t nnz, int64_t h, int64_t heads);
int pygim_gatv2_backward(int dtype, int transposed, int64_t nrows, const int32_t *rowptr, const int32_t *colind, int64_t nnz,
                         const void *x_own, int64_t ld_own, const void *x_oth, int64_t ld_oth, const void *att /* [h] */,
                         int64_t h, int64_t heads, double negative_slope, const void *G, int64_t ldg, const void *lse,
                         const void *delta, void *d_own, int64_t ldd, void *datt /* [h]; NULL when transposed */,
                         void *workspace, int64_t workspace_bytes, void *stream);

/* ---- attention dropout: dropout on the attention coefficients, inside the fused kernels ----
 * The `dropout=` of PyG's GATConv, GATv2Conv and TransformerConv.  With pr[e, k] the softmax probability of stored entry e and head k
 * and p the rate, the coefficients are dropped after the softmax and before the product with the gathered row:
 *     w[e, k]   = keep(e, k) ? 1 / (1 - p) : 0
 *     out[r, f] = sum_e pr[e, k] * w[e, k] * v[e, f]                      k = head of f
 * The running maximum, the normalisation l and lse run over ALL entries, dropped ones included: lse has the bits of the call without
 * dropout.  A non-empty row whose entries are all dropped for a head stores exact zeros for that head (never NaN); scores of -inf
 * stay masked as in the base calls.  Backward, with G = dout:
 *     dpr[e, k] = w[e, k] * sum_{f in head k} G[r, f] * v[e, f]           delta[r, k] = sum_e pr * dpr = sum_{f in head k} G[r, f] * out[r, f]
 *     ds        = pr * (dpr - delta[r, k])                                dv[c, f]    = sum_{e with col c} pr * w * G[r, f]
 * delta is still formed from G and out, because out already contains w.
 *
 * The mask is a pure function of (seed, entry index in A, head).  It keeps no state and depends neither on the launch shape nor on
 * the direction the CSR is walked.  All arithmetic is uint32, mod 2^32; seed = seed_hi:seed_lo is 64 bits; e is the index of the
 * entry in the stored order of A (0 .. nnz - 1), k the head:
 *     fmix(x):    x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16
 *     u(e, k)    = fmix( fmix(e ^ seed_lo) + seed_hi + k * 0x9E3779B9 )
 *     keep(e, k) = u(e, k) >= T,      T = min(2^32 - 1, floor(p * 2^32)),      0 <= p < 1
 * (two 32-bit multiplies per fmix; the inner fmix depends on the entry alone).  One inline function, attn_dropout_keep of
 * pygim_amd/csrc/attn_dropout_dev.hpp, is what every kernel and pygim_attention_dropout_host call.
 *
 *   pygim_gat_aggregate_dropout, pygim_sparse_attention_dropout, pygim_gatv2_aggregate_dropout: the base entry point with (p, seed)
 *     appended.  Everything of the base contract holds: types, pointers, strides, bounds (with p[e] read as pr * w), determinism, the
 *     launch shape (pygim_gather_launch_shape of the base kind answers for them).  The EXISTING workspace functions serve them:
 *     pygim_gat_aggregate_workspace, pygim_sparse_attention_workspace, pygim_gatv2_aggregate_workspace.
 *   pygim_gatv2_backward_dropout: pygim_gatv2_backward with (entry_ids, p, seed) appended; pygim_gatv2_backward_workspace serves it.
 *     dp becomes w * sum G x_src, the transposed direction accumulates pr * w * G + t.  entry_ids (int32 [nnz], device): the index in A of
 *     every entry of the CSR that is walked -- for transposed = 1 the permutation that made A^T (entry i of A^T is entry entry_ids[i]
 *     of A: the stable sort of A's entries by column); NULL means identity, for the CSR of A itself.  delta comes from the caller as
 *     before, from G and the out of the dropout forward.
 *   p = 0 launches the instantiation of the base entry point and stores its bits (seed and entry_ids are not read).  p < 0, p >= 1
 *     or NaN: PYGIM_ERR_INVALID, checked before anything else (no device is needed for that answer).
 *   pygim_attention_dropout_mask: mask[i, k] = w[entry_ids ? entry_ids[i] : i, k] for i < nnz, k < heads, [nnz, heads] contiguous,
 *     FLT32 or DBL64, device pointers, enqueued on `stream`.  What the unfused compositions and composed backwards multiply by.
 *   pygim_attention_dropout_host: keep[i * heads + k] = keep(e0 + i, k) as 0 / 1 bytes, host memory, for i < nnz.  Host only: it needs
 *     no device and no pygim_init_*; it calls the same inline function as the kernels (e0 + nnz <= 2^32).
 * Not covered: a captured graph replays the seed it was captured with; multi-GPU; heads wider than 256 features (the fused
 * sparse-attention / GATv2 kernels reject them with or without dropout: the unfused composition with the mask kernel serves them). */
int pygim_gat_aggregate_dropout(int dtype, int64_t nrows, const int32_t *rowptr, const int32_t *colind, int64_t nnz,
                                const void *a_dst, const void *a_src, int64_t heads, double negative_slope, const void *X,
                                int64_t ldx, int64_t h, void *out, int64_t ldo, void *lse, void *workspace,
                                int64_t workspace_bytes, void *stream, double p, uint64_t seed);
int pygim_sparse_attention_dropout(int dtype, int64_t nrows, const int32_t *rowptr, const int32_t *colind, int64_t nnz,
                                   const void *Q, int64_t ldq, const void *K, int64_t ldk, const void *V, int64_t ldv,
                                   int64_t h, int64_t heads, double scale, void *out, int64_t ldo, void *lse,
                                   void *workspace, int64_t workspace_bytes, void *stream, double p, uint64_t seed);
int pygim_gatv2_aggregate_dropout(int dtype, int64_t nrows, const int32_t *rowptr, const int32_t *colind, int64_t nnz,
                                  const void *x_dst, int64_t ld_dst, const void *x_src, int64_t ld_src, const void *att,
                                  int64_t h, int64_t heads, double negative_slope, void *out, int64_t ldo, void *lse,
                                  void *workspace, int64_t workspace_bytes, void *stream, double p, uint64_t seed);
int pygim_gatv2_backward_dropout(int dtype, int transposed, int64_t nrows, const int32_t *rowptr, const int32_t *colind,
                                 int64_t nnz, const void *x_own, int64_t ld_own, const void *x_oth, int64_t ld_oth,
                                 const void *att, int64_t h, int64_t heads, double negative_slope, const void *G, int64_t ldg,
                                 const void *lse, const void *delta, void *d_own, int64_t ldd, void *datt, void *workspace,
                                 int64_t workspace_bytes, void *stream, const int32_t *entry_ids /* [nnz] or NULL */, double p,
                                 uint64_t seed);
int pygim_attention_dropout_mask(int dtype, int64_t nnz, int64_t heads, const int32_t *entry_ids /* [nnz] or NULL */, double p,
                                 uint64_t seed, void *mask /* [nnz, heads] */, void *stream);
int pygim_attention_dropout_host(int64_t nnz, int64_t heads, int64_t e0, double p, uint64_t seed, uint8_t *keep /* [nnz, heads] */);

/* ---- edge terms: one scalar per (stored entry, head) inside the score of the fused attention kernels ----
 * The edge features of PyG's GATConv(edge_dim=), the learned attention bias of graph transformers, and additive masks.  The term is
 * [nnz, heads], contiguous, in the stored order of A (entry e of the CSR, the index the dropout hash takes), read inside the gather
 * beside the gathered row; nothing else of size nnz is read or written.
 *   pygim_gat_aggregate_edge:    z[e, k] = a_dst[r, k] + a_src[colind[e], k] + a_edge[e, k],  s = z >= 0 ? z : negative_slope * z
 *     (the term is added BEFORE the leaky ReLU), then the softmax and product of pygim_gat_aggregate.
 *   pygim_sparse_attention_bias: s[e, k] = scale * sum_{f in head k} Q[r, f] * K[colind[e], f] + bias[e, k]
 *     (the term is added after the scaling), then the softmax and product of pygim_sparse_attention.
 * The signatures are those of the *_dropout forms with the term inserted before (p, seed).  The term's type is the compute type:
 * FLT32 / DBL64 = the feature type, FLT32 beside FLT16 / BF16 features.  Everything of the base contract holds: device pointers,
 * strides, nnz = 0 (the term may then be NULL), empty rows, lse optional, bounds, determinism (no atomics, the same bits on every
 * launch), the launch shape (pygim_gather_launch_shape of the base kind); the EXISTING workspace functions serve them
 * (pygim_gat_aggregate_workspace, pygim_sparse_attention_workspace).  Dropout is that of the *_dropout forms: p = 0 runs the
 * instantiation without dropout and does not read seed.
 *   PYGIM_ERR_INVALID, answered before any launch: a NULL term with nnz > 0; p < 0, p >= 1 or NaN; everything the base call rejects
 *     (heads not dividing h, a head wider than 256 features for sparse attention, bad sizes, strides, pointers or workspace).
 *   A term of -inf masks its (entry, head) exactly as a -inf node term does: probability 0 wherever it stands; a (row, head) with no
 *     other entries stores NaN and lse = -inf.
 *   A term of +inf or NaN makes that row and head NaN and nothing else.
 *   A term of exactly 0 everywhere stores the bits of the base call (of the *_dropout call for p > 0): z + 0 and scale * s + 0 are exact.
 * Not covered: feature-wide ([nnz, h]) edge embeddings -- key_j + e / value_j + e of PyG's TransformerConv(edge_dim), e inside the
 * per-feature leaky ReLU of GATv2Conv(edge_dim); multi-GPU; a fused backward (the gradient of the term is the ds [nnz, heads] the
 * composed backwards already form); heads wider than 256 features in the fused sparse-attention kernel. */
int pygim_gat_aggregate_edge(int dtype, int64_t nrows, const int32_t *rowptr, const int32_t *colind, int64_t nnz,
                             const void *a_dst, const void *a_src, int64_t heads, double negative_slope, const void *X,
                             int64_t ldx, int64_t h, void *out, int64_t ldo, void *lse, void *workspace,
                             int64_t workspace_bytes, void *stream, const void *a_edge /* [nnz, heads] */, double p,
                             uint64_t seed);
int pygim_sparse_attention_bias(int dtype, int64_t nrows, const int32_t *rowptr, const int32_t *colind, int64_t nnz,
                                const void *Q, int64_t ldq, const void *K, int64_t ldk, const void *V, int64_t ldv,
                                int64_t h, int64_t heads, double scale, void *out, int64_t ldo, void *lse,
                                void *workspace, int64_t workspace_bytes, void *stream, const void *bias /* [nnz, heads] */,
                                double p, uint64_t seed);

/* ---- reductions other than the sum over a row's stored entries (mean / max aggregation of GraphSAGE, PNA, GIN variants) ----
 *   pygim_spmm_reduce:  out[r, f] = REDUCE over the stored entries e of row r of w[e] * X[colind[e], f],  w[e] = values[e], or 1
 *     when values is NULL.  The contract of pygim_spmm_values: device pointers only, a valid CSR guaranteed by the caller, nnz = 0,
 *     empty rows and any h >= 1 allowed, row strides ldx, ldo >= h, work is only enqueued on `stream`, scratch from the caller
 *     (pygim_spmm_reduce_workspace bytes: a function of its arguments alone, -1 for bad arguments; 16-byte aligned), no atomics, the
 *     same bits on every launch.  Empty rows store 0.
 *     MEAN (FLT32 / DBL64; FLT16 / BF16 with float32 values -- "16-bit features" above): the sum of pygim_spmm_values, in its order and within its bound, divided by the row's number of stored
 *       entries (duplicates count separately; not the sum of the values).  arg must be NULL.
 *     MAX / MIN (all six types): integers compare as signed values of their type and the integer product wraps like the type's own
 *       arithmetic; a float result is exactly one of the products.  arg, when not NULL ([nrows, h] int32, contiguous), receives the
 *       index in stored order of the entry that won, -1 for empty rows.  Among equal products the LOWEST entry index wins (-0.0 and
 *       +0.0 are equal).  A NaN product never wins against a number, wherever it stands in the row; a row whose products are all NaN
 *       stores NaN and arg -1.
 *   pygim_spmm_reduce_backward (FLT32 / DBL64): the gradient of MAX / MIN with respect to X, as a gather on the transposed structure:
 *       dX[c, f] = sum over the entries e' of row c of A^T, in order, of (arg[r, f] == e ? w[e] * G[r, f] : 0),  e = perm[e'], r = rows_t[e']
 *     rowptr_t [ncols + 1], rows_t [nnz] (the A-row of every entry of A^T) and perm [nnz] (its index in A: the stable sort of A's
 *     entries by column) describe A^T; values are in A's order or NULL; arg is the forward's.  dX[0:ncols, 0:h] (row stride ldd) is
 *     overwritten; every output row has one owner.  Within 1e-5 (FLT32) / 1e-12 (DBL64) of sum |w . G| of the exact value.
 *   PYGIM_ERR_INVALID: an unknown op, an integer type with MEAN or with the backward, a 16-bit type with MAX / MIN or with the backward,
 *     arg with MEAN, a workspace that is too small. */
#define PYGIM_REDUCE_MEAN 1
#define PYGIM_REDUCE_MAX 2
#define PYGIM_REDUCE_MIN 3
int64_t pygim_spmm_reduce_workspace(int dtype, int op, int64_t nrows, int64_t nnz, int64_t h);
int pygim_spmm_reduce(int dtype, int op, int64_t nrows, const int32_t *rowptr, const int32_t *colind, int64_t nnz,
                      const void *values /* [nnz] or NULL */, const void *X, int64_t ldx, int64_t h, void *out, int64_t ldo,
                      int32_t *arg /* [nrows, h] or NULL; max / min only */, void *workspace, int64_t workspace_bytes, void *stream);
int pygim_spmm_reduce_backward(int dtype, int64_t ncols, const int32_t *rowptr_t, const int32_t *rows_t, const int32_t *perm,
                               int64_t nnz, const void *values /* A's order, or NULL */, const void *G, int64_t ldg,
                               const int32_t *arg, int64_t h, void *dX, int64_t ldd, void *stream);

/* ---- several statistics of a row's stored entries in one gather (PNA-style aggregation: mean, min, max, std side by side) ----
 *   pygim_spmm_multi_reduce:  out[r, j * h + f] = statistic stats[j] over the stored entries e of row r of X[colind[e], f]   (unit
 *     weights: there is no values operand).  One pass over the stored entries, whatever the list: a lane carries S1 = sum x and
 *     S2 = sum x * x (when SUM, MEAN, VAR or STD is asked for) and the pairs (max, entry) and (min, entry) (when MAX or MIN is) beside
 *     one gather of X.  With n = the row's number of stored entries (duplicates count separately):
 *       SUM  = S1          MEAN = S1 / n          VAR = max(S2 / n - MEAN * MEAN, 0)          STD = sqrt(VAR + eps)
 *       MAX, MIN = the winning element of X itself; arg_max / arg_min, when not NULL ([nrows, h] int32, contiguous), receive the index
 *       in stored order of the entry that won
 *     The contract of pygim_spmm_reduce: device pointers only (stats is a HOST array of 1..6 distinct PYGIM_STAT_* codes), a valid CSR
 *     guaranteed by the caller, nnz = 0, empty rows and any h >= 1 allowed, row strides ldx >= h and ldo >= nstats * h (columns of out
 *     beyond nstats * h are not touched), work is only enqueued on `stream`, scratch from the caller (pygim_spmm_multi_reduce_workspace
 *     bytes: a function of its arguments alone, -1 for bad arguments; 16-byte aligned; per run of 512 entries two slots of h elements of
 *     every component carried, nothing else of size nnz), no atomics, no two kernels write the same row, the same bits on every launch.
 *     Empty rows store 0 for SUM, MEAN, VAR, MAX and MIN, sqrt(eps) for STD (the formula at S1 = S2 = 0) and -1 in arg_max / arg_min.
 *     Types: FLT32 and DBL64 compute in themselves.  FLT16 / BF16 ("16-bit features" above): X and out are stored in 16 bits, an element
 *       of X is widened as it is folded (exact), S1, S2, the division, VAR and STD are float32, and every stored value is rounded once,
 *       where its row is stored; MAX / MIN are elements of X, so their rounding is exact.
 *     Bounds, with u = 1e-5 (float32 arithmetic) or 1e-12 (DBL64):
 *       SUM, MEAN   the bits of pygim_spmm_reduce(PYGIM_REDUCE_MEAN, values = NULL) on the same operands (SUM: its numerator): the same
 *                   order of additions and the same division, for the 16-bit types too
 *       MAX, MIN, arg_max, arg_min   the bits of pygim_spmm_reduce MAX / MIN with values = NULL (16-bit X: of that call on X widened
 *                   to FLT32): the lowest entry index wins a tie, a NaN never wins against a number, all NaN stores NaN and arg -1
 *       VAR         within 3 u mean(x^2) of the two-pass value (S2 / n within u mean(x^2), MEAN^2 within 2 u mean(|x|)^2; the clamp only
 *                   moves towards it)
 *       STD         within bound(VAR) / STD + 2 epsilon STD, epsilon the machine epsilon of the arithmetic; STD >= sqrt(eps)
 *       16-bit out  2^-8 |exact| (BF16) or 2^-11 |exact| (FLT16) more, for the one rounding
 *       NaN and inf in X travel through S1 / S2 as IEEE addition carries them, into SUM, MEAN, VAR and STD of that (row, feature) alone.
 *   PYGIM_ERR_INVALID: an integer type, an unknown or repeated statistic, nstats outside 1..6, arg_max / arg_min without MAX / MIN in
 *     stats, STD with eps not finite or <= 0, ldo < nstats * h, h > 65535 * 128, a workspace that is too small or misaligned. */
#define PYGIM_STAT_SUM 0
#define PYGIM_STAT_MEAN 1
#define PYGIM_STAT_MIN 2
#define PYGIM_STAT_MAX 3
#define PYGIM_STAT_VAR 4
#define PYGIM_STAT_STD 5
int64_t pygim_spmm_multi_reduce_workspace(int dtype, const int *stats, int nstats, int64_t nrows, int64_t nnz, int64_t h);
int pygim_spmm_multi_reduce(int dtype, const int *stats /* host, 1..6 distinct */, int nstats, double eps, int64_t nrows,
                            const int32_t *rowptr, const int32_t *colind, int64_t nnz, const void *X, int64_t ldx, int64_t h,
                            void *out /* [nrows, nstats * h] */, int64_t ldo, int32_t *arg_max, int32_t *arg_min /* [nrows, h] or NULL */,
                            void *workspace, int64_t workspace_bytes, void *stream);

/* ---- softmax aggregation per feature in one gather (PyG's SoftmaxAggregation: GENConv / DeeperGCN, aggr = "softmax") ----
 *   pygim_spmm_softmax:  with s[e, f] = t[f] * X[colind[e], f] over the stored entries e of row r (unit weights: no values operand)
 *       lse[r, f] = log sum_e exp(s[e, f])      p[e, f] = exp(s[e, f] - lse[r, f])      out[r, f] = sum_e p[e, f] * X[colind[e], f]
 *     t: [h] on the device, a temperature per feature (0: the mean; large: towards the max).  lse: [nrows, h] contiguous, or NULL.
 *     One pass over the stored entries: per feature a lane carries the online-softmax triple (maximum, denominator, numerator) beside
 *     one gather of X, one exp per element and entry; nothing of size nnz * h exists.  Duplicates count separately.
 *     The contract of pygim_spmm_multi_reduce: device pointers only, a valid CSR guaranteed by the caller, nnz = 0, nrows = 0, empty rows
 *     and any h >= 1 allowed, row strides ldx >= h and ldo >= h (columns of out beyond h are not touched), work is only enqueued on
 *     `stream`, scratch from the caller (pygim_spmm_softmax_workspace bytes: a function of its arguments alone, -1 for bad arguments;
 *     16-byte aligned; per run of 512 entries two slots of h elements of each of the three components, every sub-array 16-byte aligned),
 *     no atomics, no two kernels write the same row, the same bits on every launch, and out has the same bits with and without lse.
 *     Empty rows store 0, and -inf in lse.
 *     Types: FLT32 and DBL64 compute in themselves.  FLT16 / BF16: X and out are stored in 16 bits, an element is widened as it is
 *       folded (exact); t, lse, the triple and every intermediate are float32; out is rounded once, where the row is stored.
 *     Non-finite inputs: a (row, feature) that gathers a NaN or +-inf score stores a non-finite out (NaN or +-inf, never a finite
 *       number; its lse is unspecified); entries are never skipped.  Every other (row, feature) keeps the bits it has when that
 *       element is replaced by 0.
 *     Bounds, in the form of pygim_sparse_attention, with EPS = 1e-5 (float32 arithmetic) or 1e-12 (DBL64) and
 *     Delta[r, f] = EPS * max_e |s[e, f]|:
 *       |out - exact| <= (2 EPS + 2 Delta) * sum_e p[e] |x[e]|      (+ u |exact| for 16-bit out, u = 2^-8 BF16 / 2^-11 FLT16)
 *       |lse - exact| <= 2 EPS (1 + |exact|) + Delta
 *     (float32 arithmetic takes exp(x), x <= 0, as the hardware exponential of x * log2(e): a relative error of about |x| 2^-24,
 *     which is what Delta allows for; DBL64 calls exp.)
 *   pygim_spmm_softmax_backward:  one gather on the CSR of A^T (rowptr_t [ncols + 1], rows_t [nnz]: the A-row of every entry; no
 *     permutation, nothing of size nnz allocated).  For an entry of column c that belongs to A-row r:
 *       p = exp(t[f] * X[c, f] - lse[r, f])     a[c, f] = sum G[r, f] * p     b[c, f] = sum G[r, f] * p * (X[c, f] - out[r, f])
 *       dX[c, f] = a + t[f] * b                 dT[c, f] = X[c, f] * b        (dT: [ncols, h] contiguous, or NULL)
 *     The gradient of t is the column sum of dT, formed by the caller (= sum_r G * (E_p[x^2] - out^2)).  out and lse are what the forward
 *     stored ([.., ldo] and [nrows, h] contiguous).  The partial result is the two plain sums a and b in stored order (workspace: two
 *     slots of h elements of each per run).  dX has the same bits with and without dT; columns without entries get zeros.
 *     FLT16 / BF16: X, G, out and dX are 16-bit (out the stored, once-rounded one), t, lse, dT and all sums float32.
 *     Determinism, stream and scratch rules as for the forward.
 *   PYGIM_ERR_INVALID (both): an integer type, h > 65535 * 128, a row stride below h, a workspace that is too small or misaligned. */
int64_t pygim_spmm_softmax_workspace(int dtype, int64_t nrows, int64_t nnz, int64_t h);
int pygim_spmm_softmax(int dtype, int64_t nrows, const int32_t *rowptr, const int32_t *colind, int64_t nnz, const void *X, int64_t ldx,
                       const void *t /* [h] device */, int64_t h, void *out, int64_t ldo, void *lse /* [nrows, h] contiguous or NULL */,
                       void *workspace, int64_t workspace_bytes, void *stream);
int64_t pygim_spmm_softmax_backward_workspace(int dtype, int64_t ncols, int64_t nnz, int64_t h);
int pygim_spmm_softmax_backward(int dtype, int64_t ncols, const int32_t *rowptr_t, const int32_t *rows_t, int64_t nnz, const void *X,
                                int64_t ldx, const void *t, int64_t h, const void *G, int64_t ldg, const void *out, int64_t ldo,
                                const void *lse, void *dX, int64_t ldd, void *dT /* [ncols, h] contiguous or NULL */, void *workspace,
                                int64_t workspace_bytes, void *stream);

/* ---- feature-wide edge features in the message (GINEConv; GENConv / DeeperGCN with edge_dim) ----
 * With E [nnz, h] (row stride lde) in stored CSR order -- the order of rowptr / colind, and of the a_edge term of pygim_gat_aggregate_edge --
 *       msg[e, f] = act(X[colind[e], f] + E[e, f]) + eps        act: PYGIM_ACT_NONE (identity) or PYGIM_ACT_RELU; eps a finite or
 *                                                               infinite number, taken to the compute type; unit weights, no values
 *   pygim_spmm_edge:          out[r, f] = FOLD over the stored entries e of row r, in stored order, of msg[e, f]
 *     op: PYGIM_REDUCE_SUM, _MEAN, _MAX or _MIN.  It is the kernel of pygim_spmm_values / pygim_spmm_reduce with one more operand: the wave
 *     that owns 512 consecutive entries reads its 512 rows of E as one contiguous stream beside the gathered rows of X, and the fold, its
 *     order (the scan, the xor tree of the lane groups, the runs in order), the slots, the fix-up and the tie rule of max / min (the
 *     lowest entry index wins; arg [nrows, h] int32 or NULL, -1 for empty rows) are those of the fold without E.  With E = -0.0,
 *     PYGIM_ACT_NONE and eps = 0 (which is not added) the message is X[colind[e], f] itself and out and arg have the BITS of
 *     pygim_spmm_values with unit values (SUM) or pygim_spmm_reduce (MEAN, MAX, MIN).  Workspace: pygim_spmm_edge_workspace bytes (what
 *     the fold without E needs), 16-byte aligned.
 *   pygim_spmm_edge_softmax:  out[r, f] = sum_e softmax_e(t[f] * msg[e, f]) * msg[e, f], lse[r, f] = log sum_e exp(t[f] * msg[e, f])
 *     pygim_spmm_softmax with msg in place of X[colind[e], f]: the same triple, fix-up, launch shape, workspace size, bounds (with x := msg)
 *     and, for E = -0.0 / no activation / eps = 0, the same bits of out and lse.
 *   pygim_spmm_edge_backward: the gradient with respect to E, one entry-order kernel, for G [nrows, ldg] and row r of entry e
 *       dE[e, f] = act'(X[colind[e], f] + E[e, f]) * c[e, f]        act' = 1, or (x + e > 0) for relu
 *       SUM: c = G[r, f]      MEAN: c = G[r, f] / (stored entries of row r)      MAX / MIN: c = G[r, f] if arg[r, f] == e, else 0
 *       PYGIM_REDUCE_SOFTMAX: c = G[r, f] * p * (1 + t[f] * (msg - out[r, f])),  p = exp(t[f] * msg - lse[r, f])
 *     (arg, or out and lse, are what the forward stored; pointers an op does not use are ignored).  The message is additive in X and E, so
 *     the gradient of X is the sum of the dE rows per column: pygim_spmm_values on the CSR of A^T with the permutation as column ids,
 *     unit values and X := dE -- no kernel of its own.  dT_part ([runs, h] contiguous in the compute type, runs =
 *     pygim_spmm_edge_backward_workspace = ceil(nnz / 512); or NULL): run w stores the sum over its entries of G * p * msg * (msg - out),
 *     per lane group in entry order, then the fixed xor tree; the gradient of t is the column sum, formed by the caller.  Every dE row has
 *     one writer; no workspace, no atomics, the same bits on every launch; dE has the same bits with and without dT_part.
 *     Known cost: SUM / MEAN with PYGIM_ACT_NONE is a broadcast of G[r] over the row's entries; it reads neither X nor E but still walks
 *     colind and searches the rows like the other modes.
 *   Contract (all three): that of pygim_spmm_softmax -- device pointers only, a valid CSR guaranteed by the caller, nnz = 0, nrows = 0,
 *     empty rows (out 0, arg -1, lse -inf) and any h >= 1 allowed, every row stride >= h, work only enqueued on `stream`.
 *   Types: FLT32, DBL64, FLT16, BF16 for SUM, MEAN and the softmax; FLT32 / DBL64 for MAX / MIN.  16-bit: X, E, G, out and dE are stored in
 *     16 bits, widened as they are read (exact); eps, t, lse, dT_part, the slots and all arithmetic are float32; a value is rounded once,
 *     where it is stored.
 *   Non-finite inputs: the underlying fold applied to msg.  relu keeps NaN (NaN < 0 is false) and turns -inf into 0, so E = -inf under
 *     relu gives msg = eps and a gradient of 0; a NaN or +-inf in E reaches only its own (row, feature).  MAX / MIN: a NaN message never
 *     wins against a number; all-NaN rows store NaN and arg -1.
 *   PYGIM_ERR_INVALID before any launch: E NULL with nnz > 0, an unknown op or act, NaN eps, a type the fold does not take (integers;
 *     16-bit MAX / MIN), h > 65535 * 128, arg with SUM / MEAN, a row stride below h, a workspace that is too small or misaligned.
 *   Measured (profiles/exp_edge_message.txt; Reddit-shaped graph at h = 32, products-mini at h = 256, two rounds; X stays in cache at
 *     both, so the stream of E is the cost): the expectation was one gather plus one stream of nnz * h elements, about 2 x the plain
 *     fold.  FLT32: the sum is 1.73 - 1.97 x pygim_spmm_values and reads E at 3.4 - 3.5 TB/s; the softmax is 1.61 x pygim_spmm_softmax on
 *     products-mini but 2.12 x on the Reddit shape (E at 2.5 TB/s), SLOWER than expected: its arithmetic does not hide behind the
 *     stream.  BF16: 1.57 - 1.75 x (sum) and 1.42 - 1.92 x (softmax), E at 1.4 - 2.9 TB/s: 16-bit storage does not halve the time.
 *     Against the composition through [nnz, h] tensors: forward 5.9 - 33 x, forward + backward 4 - 35 x faster, at a peak of one dE above
 *     the operands. */
#define PYGIM_REDUCE_SUM 4
#define PYGIM_REDUCE_SOFTMAX 5 /* pygim_spmm_edge_backward only */
#define PYGIM_ACT_NONE 0
#define PYGIM_ACT_RELU 1
int64_t pygim_spmm_edge_workspace(int dtype, int op, int64_t nrows, int64_t nnz, int64_t h);
int pygim_spmm_edge(int dtype, int op, int act, double eps, int64_t nrows, const int32_t *rowptr, const int32_t *colind, int64_t nnz,
                    const void *X, int64_t ldx, const void *E, int64_t lde, int64_t h, void *out, int64_t ldo,
                    int32_t *arg /* [nrows, h] or NULL */, void *workspace, int64_t workspace_bytes, void *stream);
int64_t pygim_spmm_edge_softmax_workspace(int dtype, int64_t nrows, int64_t nnz, int64_t h);
int pygim_spmm_edge_softmax(int dtype, int act, double eps, int64_t nrows, const int32_t *rowptr, const int32_t *colind, int64_t nnz,
                            const void *X, int64_t ldx, const void *E, int64_t lde, const void *t /* [h] device */, int64_t h, void *out,
                            int64_t ldo, void *lse /* [nrows, h] contiguous or NULL */, void *workspace, int64_t workspace_bytes,
                            void *stream);
int64_t pygim_spmm_edge_backward_workspace(int dtype, int op, int64_t nrows, int64_t nnz, int64_t h); /* runs: rows of dT_part */
int pygim_spmm_edge_backward(int dtype, int op /* PYGIM_REDUCE_* incl. _SOFTMAX */, int act, double eps, int64_t nrows,
                             const int32_t *rowptr, const int32_t *colind, int64_t nnz, const void *X, int64_t ldx, const void *E,
                             int64_t lde, const void *G, int64_t ldg, const int32_t *arg, const void *t, const void *out, int64_t ldo,
                             const void *lse, int64_t h, void *dE, int64_t ldde, void *dT_part, void *stream);

/* ---- which kernel instantiation and lane layout a call of the entry points above gets ----
 * The decision their launchers take, from the host functions the launchers themselves call: no device is touched and nothing is
 * launched (like the *_workspace functions it works without a GPU and without pygim_init_*).  `kind` names the entry point, `dtype`
 * the storage type, `aligned` != 0 says that every row stride is a multiple of a 16-byte piece and every base pointer (the
 * workspace included) a multiple of 16 bytes.  heads is ignored by SDDMM, SPMM_REDUCE and SPMM_REDUCE_BACKWARD, h by EDGE_SOFTMAX;
 * SPMM_MULTI_REDUCE (FLT32, DBL64, FLT16, BF16: the lane layout of the mean fold, whatever the statistics) has no heads and takes
 * heads = 1 alone (anything else: PYGIM_ERR_INVALID); so do SPMM_SOFTMAX and SPMM_SOFTMAX_BACKWARD (the same types and the same lane
 * layout; `aligned` covers lse as well for the backward), and SPMM_EDGE (pygim_spmm_edge and pygim_spmm_edge_softmax; `aligned` covers E and
 * lde) and SPMM_EDGE_BACKWARD (`aligned` covers E, G, dE and, for the softmax, out and lse): the four gather types, the lane layout of
 * SPMM_REDUCE and SPMM_SOFTMAX for the same numbers
 * (forward and backward are one kind: the backward only has one more pointer that must be aligned).
 *   out[0] vec       features per piece (per lane and load): 16 / element size, or 1
 *   out[1] pieces    pieces a lane holds at once: 1 or 2 (row walkers: SPMM_VALUES, SPMM_REDUCE, GAT_AGGREGATE, SPMM_REDUCE_BACKWARD,
 *                    SPMM_MULTI_REDUCE, SPMM_SOFTMAX, SPMM_SOFTMAX_BACKWARD),
 *                    1, 2 or 4 (head-wise: SPARSE_ATTENTION, GATV2_*), 1 .. 4 (SDDMM), 1 (EDGE_SOFTMAX)
 *   out[2] LH        lanes across the features of one head (head-wise kernels); L for the others
 *   out[3] L         lanes per entry (a power of two; 64 / L entries side by side in a wave)
 *   out[4] per       heads per block, L / LH (head-wise kernels); 1 for the others
 *   out[5] chunks    blockIdx.y chunks over all launches: of 128 pieces (row walkers), of `per` heads (head-wise); SDDMM: passes of 4
 *                    pieces per lane; EDGE_SOFTMAX: steps over an entry's heads
 *   out[6] launches  launches of the gather kernel (65535 chunks each at most; more than one only for the head-wise kernels)
 *   out[7] flags     PYGIM_SHAPE_PART_PIECE  a lane's last piece exists only on some lanes (row walkers, SDDMM: pieces % L != 0;
 *                                            head-wise: a head's pieces < out[1] * LH)
 *                    PYGIM_SHAPE_PART_CHUNK  the last chunk (SDDMM: pass) holds fewer pieces, or fewer heads, than the others
 *                    PYGIM_SHAPE_PART_HEADS  heads % per != 0: a block has lanes for heads that do not exist
 *                    PYGIM_SHAPE_SCALAR_SIZE / _ALIGN  why vec == 1: the width (h, h / heads where a piece must not lie across two
 *                                            heads, `heads` for EDGE_SOFTMAX) does not fill whole pieces / `aligned` is 0
 * Returns PYGIM_ERR_INVALID for what the entry point itself rejects for these numbers: an unknown kind, a type it does not take,
 * heads not dividing h, h / heads > 256 (head-wise), and h > 65535 * 128 for the row walkers -- one launch holds 65535 chunks, so
 * pygim_spmm_values, pygim_spmm_reduce, pygim_spmm_multi_reduce, pygim_spmm_softmax, pygim_spmm_softmax_backward, pygim_gat_aggregate, their
 * *_workspace functions (-1) and pygim_spmm_reduce_backward reject a wider row before any launch, whatever the alignment.                                                               */
#define PYGIM_SHAPE_SPMM_VALUES 0
#define PYGIM_SHAPE_SPMM_REDUCE 1
#define PYGIM_SHAPE_GAT_AGGREGATE 2
#define PYGIM_SHAPE_SPARSE_ATTENTION 3
#define PYGIM_SHAPE_GATV2_AGGREGATE 4
#define PYGIM_SHAPE_GATV2_BACKWARD 5
#define PYGIM_SHAPE_SDDMM 6
#define PYGIM_SHAPE_EDGE_SOFTMAX 7
#define PYGIM_SHAPE_SPMM_REDUCE_BACKWARD 8
#define PYGIM_SHAPE_SPMM_MULTI_REDUCE 9
#define PYGIM_SHAPE_SPMM_SOFTMAX 10
#define PYGIM_SHAPE_SPMM_SOFTMAX_BACKWARD 11
#define PYGIM_SHAPE_SPMM_EDGE 12
#define PYGIM_SHAPE_SPMM_EDGE_BACKWARD 13
#define PYGIM_SHAPE_PART_PIECE 1
#define PYGIM_SHAPE_PART_CHUNK 2
#define PYGIM_SHAPE_PART_HEADS 4
#define PYGIM_SHAPE_SCALAR_SIZE 8
#define PYGIM_SHAPE_SCALAR_ALIGN 16
int pygim_gather_launch_shape(int kind, int dtype, int64_t h, int64_t heads, int aligned, int64_t out[8]);

/* ---- introspection -----------------------------------------------------------
 * Milliseconds of the last host-pointer run, in the reference's Timer buckets
 * (support/timer.h; printed as [DATA] lines, spmm_mul_csr.c:563-580):
 * [0] load_dense (H2D)  [1] kernel  [2] retrieve (D2H)  [3] merge (always 0: no
 * host merge here)  [4] one-time sparse upload + analysis of the group.       */
int pygim_group_timers(int64_t handle, double out_ms[5]);
/* shape / plan of a group: total_rows, total_cols, h, n_parts, n_long_rows (rows cut into
 * segments over several waves), all_ones flag, column panels of part 0's L2-blocked plan
 * (0 = no plan), work items of that plan.                                       */
int pygim_group_info(int64_t handle, int64_t out[8]);
/* With tunable "kernel_events" = 1 every block product brackets its dominant kernel (the
 * row-gather kernel, not the long-row tail kernels) with HIP events on the launch stream.
 * This call waits for the pending pairs and returns the accumulated milliseconds and the
 * number of launches since the last reset.                                      */
int pygim_group_kernel_ms(int64_t handle, double *sum_ms, int64_t *count, int reset);
/* the same switch for ONE group (what bench.py uses; the tunable is the process-wide default for A/B scripts) */
int pygim_group_kernel_events(int64_t handle, int on);
/* plan of the matrix the run entry points sweep (the merged matrix of a multi-part group, else part 0):
 * column panels (0 = no panel plan), columns per panel, work items, 16-bit panel-local column ids built (0/1),
 * wave-cooperative (long) items, segment-kernel tasks, merged (0/1), has a non-unit-weight correction part (0/1) */
int pygim_group_plan(int64_t handle, int64_t out[8]);
/* schedule of the LDS-staged product (k_lds_spmm; the reference's scratchpad loop spmm_default/dpu_kernels/
 * spmm_mul_csr_dpu.c:108-126 with X chunks in LDS and the running sums of a tile of rows in registers) of the same matrix:
 * row tiles (0 = no such plan), 80 KiB (320-column) chunk fills per 64-feature slice and product, tokens incl. padding, stored entries */
int pygim_group_lds_plan(int64_t handle, int64_t out[4]);
/* the same schedule compiled into gfx950 machine code (the code-stream form of the product, k_lds_code_*: one straight-line
 * instruction stream per (row tile, wave), 1.5 instructions per stored entry): bytes of code (0 = none), stored entries that share
 * an LDS instruction with a neighbour, 1 when products take this form (tunable "lds_code"), 1 when the stream was generated on the
 * device from the resident CSR (round 5, tunable "lds_codegen") rather than by the host encoder */
int pygim_group_lds_code(int64_t handle, int64_t out[4]);
/* which rows share a tile of that schedule (round 5; the reference hands a DPU consecutive rows, support/partition.c:51-99): 1 when the
 * rows were ordered by similarity (label propagation over the graph, tunable "lds_tile_order") instead of by index, the number of labels
 * the propagation ended with, the rows of the largest one; and whether the L2 sweep's work items are in locality order (0 = by length alone,
 * 1 = blocks of consecutive rows: the stored ids are local, 2 = blocks of the propagated order; tunable "panel_locality") */
int pygim_group_lds_tiles(int64_t handle, int64_t out[4]);
/* how many products (or blocks of pygim_block_run) the LDS-staged kernels have served for this group since it was created: a plan existing
 * (pygim_group_lds_plan) does not say that a given call took it -- widths, alignment and accumulation decide per call (the reference has one
 * kernel per build, spmm_default/dpu_kernels/spmm_mul_csr_dpu.c, so nothing to ask there) */
int pygim_group_lds_runs(int64_t handle, int64_t *out);
/* host operands (the reference driver's default call, spmm_test.py:29-35 with CPU tensors; spmm_default/pytorch_api.cpp:269-271 returns one): how many
 * feature windows the LAST run of this group moved as a pipeline -- window k + 1 uploaded while window k is multiplied and its result travels back
 * (tunable "host_windows"); 1 = upload, product and download one after the other; 0 = no run with host operands yet.  A window is a column range of X
 * and of C: every row's sum keeps its stored order.  *direct (may be NULL): 1 when the windows' products stored their rows straight into the caller's
 * page-locked result (tunable "host_direct"), 0 when the result was staged in device memory and copied down */
int pygim_group_host_windows(int64_t handle, int64_t *windows, int64_t *direct);
/* geometry of that schedule, as the library planned it (callers price staged bytes from THIS, not from assumed constants):
 * waves per workgroup, accumulators (rows) per wave, columns per chunk (chunk bytes = 256 x this), chunk buffers of the LDS ring,
 * staged columns per group of reads and x-register sets of a code stream (0 0 for a token plan), stored entries served by another
 * entry's LDS read (code streams: entries of different rows of one wave that share a column of a chunk), column ranges per row tile,
 * slices of X an XCD runs side by side in a product of the group's full width (1, 2 or 4: "lds_xcd_slices"), and whether the workgroups that
 * run one code stream side by side share its touches ("lds_touch_share": 1 = one wave pulls a stream's lines into the L2, its partners ask for
 * one dword per touch; 0 = every wave touches every line -- also what a plan reports whose x registers reach the touch register) */
int pygim_group_lds_geometry(int64_t handle, int64_t out[10]);
/* which form of the product the group got at creation and, when it is not the fastest one, why (text, NUL-terminated, at most cap - 1
 * characters): "code-stream form" | "code-stream form not available: <reason>; products take the token form ..." | "... the L2 sweep
 * serves this group".  The ladder is code stream -> token kernels -> sweep; nothing falls back silently. */
int pygim_group_lds_note(int64_t handle, char *out, int64_t cap);
/* Kernel tunables (for A/B runs): name in {"long_row_threshold", "long_segment", "force_vec_bytes",
 * "csr_kernel", "coo_chunk", "coo_via_rowptr", "panel_mode", "panel_bytes", "panel_min_seg",
 * "panel_coop", "panel_block", "panel_lds_pad", "panel_pack", "panel_locality", "panel_col16", "slice_group_bytes", "fuse_windows",
 * "split_unit_pattern", "narrow_vals" (INT64 / DBL64 values that all fit int32 / float exactly are streamed in 4 bytes), "merge_parts", "vec_kernel", "vec_lds", "vec_lds_min_seg", "kernel_events",
 * "lds_mode" (LDS-staged product: 0 = by the reuse rule, 1 = whenever planned, 2 = never), "lds_min_reuse_x100",
 * "lds_min_width", "lds_threads", "lds_waves" (8 | 16 waves per workgroup of the kernel the plan is made for),
 * "lds_round_tiles", "lds_code" (1 = FLT32 (valued too) / INT32 / INT16 unit-weight plans are compiled into machine code at creation and run by k_lds_code_*,
 * 0 = the token kernels), "lds_col_split" (short row shares: tiles split into column ranges, partial sums reduced in range order; 0 = automatic,
 * 1 = never, S), "lds_col_split_f32" (FLT32 shares too -- their sums are then sums of per-range sums, inside the path's 1e-5 of |A|.|x| but not the CPU loop's bits:
 * 1 = parts of 2^20 entries and more (the default since round 6), 2 = any part, 0 = never), "lds_row_tail" (percent of a share's rows that may stay outside its LDS plan -- summed by the
 * tail kernels from the same staged copy -- when that leaves exactly one workgroup per compute unit; 0 = never), "lds_fill_tiles", "lds_split_order" (round 6: tile counts / tile order of
 * column-split plans), "lds_half_split" (round 6: 1 = products of at most 32 lanes of a 4-byte type fold two column ranges into the halves of a wave -- half the staged bytes; the plan is
 * written by the host encoder, so 0 is the default), "lds_code_nbuf" (its LDS ring: 0 = by width and geometry, 2 = two buffers of 320 columns with a barrier at every slot boundary,
 * 3 / 4 / 5 ... 10 = 192 / 160 / 128 ... 64 columns; the default is 5 x 128 for the 8-wave geometry), "lds_code_boundary" (rings of three or more
 * buffers: 0 / 1 = the workgroup meets at every slot boundary with nbuf - 1 chunks in flight, 2 = once in the middle of a slot with nbuf - 2),
 * "lds_code_waves" (waves per workgroup of a code-stream plan: 16 x 96 accumulators, 8 x 228 = taller tiles and fewer rounds of workgroups, 0 = automatic),
 * "lds_code_kc" (columns per chunk, 0 = by the ring), "lds_code_gsize" / "lds_code_nsets" (staged columns per group of LDS reads / x-register sets: the
 * reads run nsets - 1 groups ahead of the adds; 0 = default), "lds_codegen" (code streams: 1 = generated on the device from the resident CSR -- the default --, 0 = by
 * the host encoder, 2 = on the device and checked word for word against the host encoder), "lds_tile_order" (which rows share a tile: 0 = consecutive
 * rows, 1 = rows ordered by similarity, 2 = automatic: similarity for square parts of a million entries and more), "lds_lp_rounds", "lds_hybrid" (density split of a community-structured part whose ids carry no locality: the dense (tile, chunk) cells through the LDS-staged kernel, the rest through the sweep; 0 = off, 1 = integer types, 2 = floats too -- their sums are then reordered), "lds_hybrid_min" (entries a cell must hold), "lds_xcd_slices" (code-stream products: slices of X per XCD -- 0 = automatic (the default), 1 = an XCD streams one slice through
 * its L2; 2 / 4 = the workgroups an XCD runs side by side are slices of the same tile and share its code stream in L2), "lds_touch_share" (8-wave code-stream products with 2 / 4 slices per XCD: 1 = the workgroups that run one stream side by side share its touches -- the default --, 0 = every wave touches), "lds_long_slots", "lds_ablate" (timing experiments, wrong results)};
 * returns the previous value, or -1 for an unknown name (pygim_last_error() says which).
 * READ AT GROUP CREATION (they shape the plan; changing them afterwards does not touch existing groups, and switching "lds_code" off
 * after a code-stream group was created sends that group's products to the sweep): panel_*, long_*, split_unit_pattern, narrow_vals,
 * merge_parts, lds_code, lds_codegen, lds_tile_order, lds_lp_rounds, lds_hybrid, lds_hybrid_min, lds_code_waves, lds_code_nbuf, lds_code_kc, lds_code_gsize, lds_code_nsets, lds_code_boundary, lds_waves, lds_col_split,
 * lds_col_split_f32, lds_row_tail, lds_fill_tiles, lds_split_order, lds_half_split, lds_min_width, lds_round_tiles, lds_long_slots, lds_min_reuse_x100 and lds_mode (whether a plan is made at all), lds_threads.
 * The others are read per product.  */
int64_t pygim_set_tunable(const char *name, int64_t value);

#ifdef __cplusplus
}
#endif
#endif /* PYGIM_HIP_H */
