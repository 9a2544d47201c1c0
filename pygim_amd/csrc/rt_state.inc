// rt_state.inc -- part of pygim_hip.hip (included inside its anonymous namespace): error text, tunables, the Part / Group / Context records, the
// slice-major staging buffers, executable device memory (HSA pool), freeing.  Split out in round 5 (VERDICT r04 weak 9); one translation unit still.
thread_local std::string g_err;
int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}
#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess) {                                                                \
            (void)hipGetLastError();                                                           \
            return fail(PYGIM_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));     \
        }                                                                                      \
    } while (0)

size_t dtype_size(int dt) {
    switch (dt) {
        case PYGIM_INT8: return 1;
        case PYGIM_INT16: return 2;
        case PYGIM_INT32: return 4;
        case PYGIM_INT64: return 8;
        case PYGIM_FLT32: return 4;
        case PYGIM_DBL64: return 8;
    }
    return 0;
}

struct Tunables {
    int64_t long_row_threshold = 4096;  // rows with more entries are cut into segments
    int64_t long_segment = 512;         // entries per segment (one wave each) of such a row
    int64_t force_vec_bytes = 0;        // 0 = pick by alignment
    int64_t csr_kernel = 0;             // 0 = auto, 1 = force wide, 2 = force sub-wave
    int64_t coo_chunk = 512;            // entries per wave in the nnz-split COO kernel
    int64_t coo_via_rowptr = 0;         // 1 = run COO groups through the CSR kernels (derived rowptr)
    int64_t panel_mode = 0;             // 0 = auto (cost rule), 1 = force the L2-blocked panel kernel, 2 = never
    int64_t panel_bytes = 4 << 20;      // L2 budget of one (column panel x 128-byte feature slice)
    int64_t panel_min_seg = 8;          // auto: least average entries per (row, panel) worth a panel sweep
    int64_t panel_block = 256;          // threads per block of the sweep kernel (64, 128 or 256)
    int64_t panel_lds_pad = 0;          // (experiment) unused dynamic LDS per sweep block: fewer resident blocks per CU
    int64_t panel_coop = 512;           // items longer than this are walked by a whole wave (8 lane groups)
    int64_t panel_pack = 1;             // 1 = gather from a slice-major copy of X (made per product)
    int64_t slice_group_bytes = 640ll << 20;  // sweep at most this many bytes of slice-major X per launch (0 = all slices at once)
    int64_t vec_kernel = 1;             // 1 = rows of X of at most 4 elements (SpMV) take the CSR-vector kernel
    int64_t vec_lds = 1;                // 1 = ... and, when a column panel of X fits, the LDS-staged form of it (k_spmv_lds)
    int64_t vec_lds_min_seg = 14;       // ... from this many entries per (row, panel) on average
    int64_t merge_parts = 1;            // 1 = groups of several sparse parts also get the merged matrix (used by the run entry points)
    int64_t narrow_vals = 1;            // 1 = INT64 / DBL64 values that are all exactly 4-byte representable are streamed as int32 / float by the sweep
    int64_t split_unit_pattern = 1;     // 1 = integer weights that are 1 almost everywhere: unit pattern + a small correction part
    int64_t panel_locality = 1;         // (2 = always, whatever the size or the labels' quality: tests) 1 = the sweep's work items in LOCALITY order (blocks of 2048 rows of the similarity / id order, longest first inside a block) when the graph has structure; 0 = by length alone
    int64_t panel_col16 = 1;            // 1 = the sweep reads 16-bit panel-local column ids (built with the plan)
    int64_t fuse_windows = 1;           // 1 = the dense windows of a sparse part become ONE block product of the full width
    int64_t host_windows = 0;           // host operands (the reference driver's default call): feature windows of X go up, are multiplied and come down as a pipeline over the
                                        // two directions of PCIe -- 0 = automatic (windows of 512 bytes of a row when X and C are 32 MB and more and the result tensor is
                                        // page-locked), 1 = never (upload, product, download one after the other), n > 1 = n windows whatever the sizes
    int64_t host_direct = 1;            // ... the windows' products may STORE their rows straight into the caller's page-locked tensor (one pass of the LDS-staged kernel; no staged C,
                                        // no copy down): 0 = never, 2 = whenever possible, 1 = for the later calls of a group whose downloads turned out slow (rt_run.inc)
    int64_t kernel_events = 0;          // 1 = bracket the dominant kernel of every block product with HIP events
    int64_t lds_mode = 0;               // LDS-staged product (k_lds_spmm): 0 = auto (reuse rule), 1 = whenever a part has the plan, 2 = never
    int64_t lds_min_reuse_x100 = 75;    // auto: least stored entries per staged column of X (x 100) for the LDS-staged product (measured crossing: between 0.48 and 0.96, profiles/r04_exp_share.txt; round 3's kernel: 1.1; round 6, scripts/exp_narrow_rule.py: ~0.45 at 256 and 64 features, ~0.6 at 16 -- 0.75 is on the safe side)
    int64_t lds_min_width = 5;          // narrower products (lanes: 4-byte units of a row) keep the sweep and the SpMV kernels.  Round 6, last session: 17 -> 5 -- measured on the
                                        // Reddit-shaped graph, all rows: 16 / 12 / 8 FLT32 features 0.86 / 0.93 / 0.85 ms on the sweep, 0.46 / 0.45 / 0.43 on the LDS-staged kernel (half-split
                                        // plan; 0.56-0.58 with a plain plan); INT16 / INT8 of 16 lanes 0.68 against 0.86 / 0.91.  Narrow products weigh the staged columns against FEWER
                                        // gathered bytes per entry -- and still the crossing sits where the wide products' does (lds_min_reuse_narrow_x100)
    int64_t lds_min_width8 = 33;        // ... the 8-byte types (features of a 512-byte slice): 32 DBL64 features 1.82 ms on the LDS-staged kernel against 1.67 on the sweep, 64: 1.83 against 3.26
    int64_t lds_min_reuse_narrow_x100 = 75;    // products of at most 32 lanes: least stored entries per staged column (x 100) for an LDS-staged plan; a half-split plan stages half the
                                               // columns and needs 1.6 x this.  Measured (scripts/exp_narrow_rule.py, Reddit-sized graphs with 1/1 .. 1/5 of the entries, 16 and 32 FLT32
                                               // features): the LDS-staged kernel stays ahead of the sweep down to 0.77 entries per staged column (0.26 against 0.38 ms) -- the same
                                               // crossing as the wide products', so the same number
    int64_t lds_threads = 0;            // host threads of the schedule builder (0 = all)
    int64_t lds_waves = 16;             // waves per workgroup of the LDS-staged kernel the plan is made for (8 or 16)
    int64_t lds_long_slots = 128;       // tokens per (wave, chunk) from which the 16-token-batch geometry is planned (0 = never)
    int64_t lds_code = 1;               // 1 = FLT32 / INT32 unit-weight plans are also compiled into machine code (lds_plan.hpp lds_code_from_plan) and run by k_lds_code_*; 0 = the token kernels
    int64_t lds_col_split = 0;          // column-split workgroup tiles for short row shares: 0 = automatic (integers; FLT32 with lds_col_split_f32), 1 = never, S > 1 = S ranges
    int64_t lds_col_split_f32 = 1;      // FLT32 shares may be split too (a row's sum is then the sum of its column ranges' sums: the norm-wise contract, not the bit-identical one):
                                        // 1 (default, round 6) = parts of a million entries and more, 2 = any part, 0 = never (stored-order sums everywhere)
    int64_t lds_row_tail = 3;           // column-split plans: up to this many percent of a share's rows may stay outside the plan (k_lds_tail) when that buys a whole
                                        // column range more with every compute unit busy (0 = never)
    int64_t lds_half_split = 1;         // 1 = products of at most 32 lanes (4-byte types, unit weights; FLT32 under the column-split rule) fold two column ranges into the halves of a
                                        // wave: half the staged bytes, all rows x 32 FLT32 features 0.58 -> 0.51 ms (then bound by the entries: twice as many per chunk).  On by
                                        // default since the device code generator writes these plans too (the host encoder took 1.2 s for the Reddit-shaped graph); 0 = never
    int64_t lds_direct_x = 1;           // 1 = a one-slice product whose rows of X are exactly the staged row reads the caller's matrix in place (no slice-major copy)
    int64_t lds_split_order = 1;        // column-split plans of one round keep their tiles in (row tile, range) order: an XCD then streams one column range
    int64_t lds_fill_tiles = 1;         // column-split plans: more, lighter row tiles when tall x slices x ranges leaves compute units idle
    int64_t lds_code_nbuf = 0;          // chunk buffers of a code-stream plan: 0 = by the product's width (3 x 192 columns up to two slices, else 2 x 320), 2, 3
    int64_t lds_code_waves = 0;         // waves per workgroup of a code-stream plan: 16 (x 96 accumulators), 8 (x 228: taller tiles, fewer rounds of workgroups), 0 = automatic
    int64_t lds_code_kc = 0;            // columns per chunk of a code-stream plan (0 = by the ring: 320 / 192 / 160 / 128 for 2 / 3 / 4 / 5 buffers)
    int64_t lds_code_gsize = 0;         // staged columns per group of reads of a code stream (0 = lds_plan.hpp lds_code_regs)
    int64_t lds_code_nsets = 0;         // x-register sets of a code stream: the reads run nsets - 1 groups ahead of the adds (0 = default)
    int64_t lds_round_tiles = 1;        // 1 = tile height chosen so that tiles x slices fill whole rounds of workgroups
    int64_t lds_tile_order = 2;         // code-stream plans: which rows share a tile -- 0 = consecutive rows, 1 = similarity order (label propagation, lds_reorder_dev.hpp), 2 = automatic (similarity for square parts of >= 1 M entries)
    int64_t lds_lp_rounds = 12;         // rounds of the label propagation (products-shaped SBM: 3 271 labels after 6, 882 after 12 -- 1 200 planted; sweep 11.7 -> 10.9 ms)
    int64_t lds_codegen = 1;            // code streams: 1 = generated on the device from the resident CSR (lds_codegen_dev.hpp), 0 = by the host encoder, 2 = on the device AND checked word for word against the host encoder (tests)
    int64_t lds_xcd_slices = 0;         // code-stream kernels: slices of X per XCD (0 = automatic; 1 = an XCD streams one slice; 2 / 4: a tile's slices side by side on one XCD share its code in L2)
    int64_t lds_touch_share = 1;        // 8-wave code-stream kernels with 2 / 4 slices per XCD: 1 = of the workgroups that run one stream side by side a single wave pulls its lines
                                        // through the L1 ahead of the sequencer, its partners' touches ask for one dword (LdsArgs.touch_share); 0 = every wave touches every line
    int64_t lds_code_boundary = 0;      // rings of >= 3 buffers: 0 / 1 = the workgroup meets at the slot boundary (one more chunk in flight, the last group's adds cross the barrier), 2 = in the middle of a slot
    int64_t lds_code_exp = 0;           // (timing experiments, WRONG results) code streams without barriers (1) / without the chunk DMA (2)
    int64_t lds_hybrid = 1;             // density split of community-structured parts (lds_hybrid_dev.hpp): 0 off, 1 integer types (exact), 2 floats too (the order of a row's sums changes)
    int64_t lds_hybrid_contig = 1;      // ... the dense half's tiles in row order, an XCD running a contiguous range of them (0: heaviest first, interleaved)
    int64_t lds_hybrid_min = 128;       // ... entries a (tile, chunk) cell must hold to be staged through LDS rather than gathered
    int64_t lds_stamp = 0;              // (measurement) device address of a uint64 buffer [blocks][8 waves][4]: k_lds_code8_f32 runs as its _ts build and stamps the 100 MHz clock
    int64_t lds_fail = 0;               // (tests) force a step of the code-stream set-up to fail: 1 = code generation, 2 = executable memory, 4 = schedule build (host); 8 = a large transient allocation of the DEVICE code generator
    int64_t lds_ablate = 0;             // (timing experiments) 1..4: kernel variants with parts of the loop removed -- WRONG results
} g_tune;

struct LongPlan {
    uint32_t n_long = 0, n_tasks = 0, thresh = 0;
    uint32_t *d_tasks = nullptr;  // (row, s, e) x n_tasks
    uint32_t *d_desc = nullptr;   // (row, first_task, n_tasks) x n_long
};

struct Part {
    int64_t nrows = 0, ncols = 0, nnz = 0;
    uint32_t *rowptr = nullptr;  // CSR rowptr, or derived from the COO row index
    uint32_t *rowind = nullptr;  // COO only
    uint32_t *colind = nullptr;
    void *vals = nullptr;        // nullptr when all ones
    void *vals_narrow = nullptr; // 8-byte element types whose values all fit 4 bytes exactly: the sweep streams these (narrow_values)
    bool own_rowptr = false, own_rowind = false, own_colind = false, own_vals = false;
    // long-row plans (rows cut into segments over many waves).  lp_base: used by the row-per-wave kernels; lp_panel: used with the panel sweep, where a row is
    // only "long" when its share of ONE panel would be (threshold x npanels): segment kernels gather
    // whole rows of X past the L2 blocking, so the panel sweep keeps as many rows as it can
    LongPlan lp_base, lp_panel;
    // L2-blocked plan: per column panel, the list of (row, first entry, length|FIRST) work items
    // sorted by length (rows without entries in a panel do not appear in its list)
    uint32_t *d_items = nullptr;            // [3][n_items]: rows | begins | lens
    size_t n_items = 0;
    std::vector<size_t> panel_off;          // npanels + 1 offsets into the item arrays
    std::vector<uint32_t> panel_coop;       // per panel: leading items long enough for the wave-cooperative mode
    uint32_t npanels = 0, panel_cols = 0;
    unsigned short *col16 = nullptr;        // panel-local 16-bit column ids (panels of <= 65536 columns), same order as colind
    std::vector<uint32_t> panel_long128;    // per panel: leading items with more than 256 / 128 / 64 / 32 entries, 4 counts each (the
                                            // LDS-staged SpMV kernel's length classes)
    std::vector<uint64_t> panel_nnz;        // per panel: entries of its items
    SpmvUnit *d_spmv_units = nullptr;       // the LDS-staged SpMV kernel's (panel, slot) table, built at its first launch
    uint32_t n_spmv_units = 0;
    std::vector<int64_t> dense_cols;
    // integer weights that are 1 almost everywhere (a coalesced multigraph, backend_pim/spmm.py:40-42): this part keeps
    // the PATTERN only (unit weights: no value array, no multiplies, packed 8/16-bit sums) and `extra` holds the few
    // entries with weight v != 1 as (v - 1); A.X = pattern.X + extra.X exactly in modular arithmetic
    std::unique_ptr<Part> extra;
    // density split (round 5, lds_hybrid_dev.hpp): this part = hy_dense (LDS-staged, columns renamed to positions of the similarity order, X staged in that
    // order through lds_col_order) + hy_sparse (the L2 sweep, adding); the part's own plans stay for the calls the LDS kernel does not take
    std::unique_ptr<Part> hy_dense, hy_sparse;
    bool lds_forced = false;               // the dense half of a density split: an LDS plan whatever the reuse rule says, tiles in the order the part brings along (sim_order)
    bool lds_contig_tiles = false;         // the LDS plan's tiles are in row order and an XCD runs a contiguous range of them (set before the plan is built)
    uint32_t *lds_col_order = nullptr;     // (owned by the part that holds it: hy_dense) row `pos` of the staged copy = X[lds_col_order[pos]]
    std::string hy_note;
    // LDS-staged product (lds_plan.hpp): token streams and tile table on the device; lds_tiles == nullptr: no such plan
    uint32_t *lds_tok = nullptr, *lds_nb = nullptr, *lds_chunks = nullptr, *lds_rowmap = nullptr;
    LdsTile *lds_tiles = nullptr;
    int cols_sorted = -1;   // stored order inside every row is column order: -1 = not checked yet, 0 / 1
    uint32_t lds_ntiles = 0, lds_nw = 8, lds_batch = 8, lds_wdelta = 0;   // lds_wdelta != 0: the plan carries the entries' values
    char *lds_code = nullptr;              // the schedule as gfx950 machine code (EXECUTABLE device memory from the HSA pool), or nullptr
    uint64_t *lds_code_start = nullptr;    // [ntiles][16]: byte offset of a (tile, wave) stream
    uint64_t lds_code_bytes = 0, lds_code_pairs = 0;
    uint32_t lds_rows = 0;                 // 0 = the plan's tiles cover every row; else the first lds_rows rows, the others take k_lds_tail (round 6: a share whose rows
                                           // all but fit tall x slices x S = one workgroup per compute unit)
    uint32_t lds_half = 0;                 // > 0: a HALF-SPLIT plan (LdsGeometry::half_split): H, the rows of its staged copy (row j = [X[j] | X[j + H]], 32 lanes each)
    uint32_t *lds_tail_segs = nullptr;     // [3][nseg]: row | first entry | end -- the rows behind lds_rows cut into segments of <= LDS_TAIL_SEG entries
    uint32_t *lds_tail_rowseg = nullptr;   // [ntail + 1]: first segment of every such row
    uint32_t lds_tail_nseg = 0;
    uint32_t lds_col_splits = 1;           // > 1: the plan's tiles are (row tile, column range) pairs writing partial sums (launch_lds reduces them)
    uint32_t lds_code_piece = 0;           // bytes of a chunk one wave DMAs (the code plan's ring geometry)
    uint32_t lds_kc = 0, lds_nbuf = 0;     // the plan's ring: columns per chunk, buffers
    uint32_t lds_row_bytes = 256, lds_ka = 0;   // bytes of a staged row (512: the 8-byte element form), accumulators (rows) per wave
    uint32_t lds_code_gsize = 0, lds_code_nsets = 0;
    uint64_t lds_code_shared = 0;          // entries of the code stream served by another entry's read
    std::string lds_note;                  // which form of the product this part got, and why not a faster one
    bool lds_codegen_device = false;       // its code stream was generated on the device
    // which rows are alike (round 5, lds_reorder_dev.hpp): found once per part, used by the LDS plan's tiles and by the sweep's item order
    bool panel_locality_used = false;      // the sweep's items are in locality order
    int sim_kind = -1;                     // -1 = not looked at, 0 = no structure found, 1 = the stored ids are local already (consecutive order), 2 = label propagation
    std::vector<uint32_t> sim_order;       // kind 2: the rows ordered by (label, id)
    uint32_t sim_labels = 0, sim_largest = 0;
    double sim_agree = 0.0;                // kind 2: share of the stored entries whose column carries its row's label
    std::string sim_why;
    uint32_t lds_tile_labels = 0, lds_tile_largest = 0;   // similarity tiles: labels the propagation ended with, rows of the largest (0 = consecutive rows)
    std::string lds_codegen_why;           // ... or why not
    bool lds_is_code = false;              // the LDS plan of this part is in the code-stream geometry (three 192-column buffers): k_lds_code_* only
    uint64_t lds_slots = 0, lds_tokens = 0;   // 80 KiB chunk fills per slice and product; tokens incl. padding
    bool is_extra = false;  // widths of the dense parts paired with this part
    bool no_pack = false;   // the sweep of this part gathers from the caller's row-major X (the sparse half of a density split: gathers that miss every cache gain
                            // nothing from the slice-major copy, which costs a pass over X: 8.8 -> 8.4 ms)
    bool timed = false;     // an adding part whose kernels are part of the product's time all the same (the sparse half of a density split)
};

struct Group {
    int format = 0, dtype = 0;
    int64_t h = 0, total_rows = 0, total_cols = 0;
    std::vector<Part> parts;
    // the sparse parts are column blocks of ONE matrix (spmm.py:127-136) whose partial products are summed: merged here
    // (global column ids, rows concatenated in block order = sorted) so that the group product is one sweep with the
    // plan that suits the whole matrix, whatever sp_parts the caller chose (32 parts of Reddit: 10.3 -> 6.8 ms)
    std::unique_ptr<Part> merged;
    bool all_ones = true;
    // scratch (device), grown on demand
    void *scratch = nullptr;
    size_t scratch_bytes = 0;
    void *stage_in = nullptr;
    size_t stage_in_bytes = 0;
    void *stage_out = nullptr;
    size_t stage_out_bytes = 0;
    void *xq = nullptr;       // quantised features / integer result of pygim_quant_spmm_run
    size_t xq_bytes = 0;
    void *oq = nullptr;
    size_t oq_bytes = 0;
    // slice-major copy made (or reused) by the block product in flight: its correction part (Part::extra) gathers from
    // the same copy instead of repeating it
    const void *packed_src = nullptr;
    void *packed_buf = nullptr;
    int64_t packed_ld = 0, packed_w = 0;
    // per-call options of the entry point in flight (a group serves one call at a time)
    bool x_unchanged = false;        // the caller vouches: same X, same contents as the product that last packed it
    int64_t serial = 0;              // creation serial (pygim_group_serial): never reused, unlike the address that is the handle
    int64_t lds_runs = 0;            // products (or blocks) the LDS-staged kernels served since the group was created (pygim_group_lds_runs)
    const void *pre_xs = nullptr;    // slice-major copy already made by the caller of launch_block_any (fused quantiser)
    float *deq_out = nullptr;        // fused dequantisation: rows' LAST items store float(sum) * scale here
    int64_t deq_ld = 0;
    const uint32_t *deq_amax = nullptr;
    int deq_log2 = 0;
    const float *post_mul = nullptr, *post_add = nullptr;  // per-column epilogue of the fused store (nullptr = none)
    int post_relu = 0;
    // pinned pointer tables of the SpMV pack (two slots, each guarded by an event)
    void **h_ptrs = nullptr;
    size_t h_ptrs_n = 0;
    hipEvent_t ev_ptrs[2] = {nullptr, nullptr};
    int ptr_slot = 0;
    void *xcat = nullptr;     // dense windows of one sparse part laid side by side (fused block product)
    size_t xcat_bytes = 0;
    void **d_ptrs = nullptr;  // device array of pointers (spmv pack)
    size_t d_ptrs_n = 0;
    int *d_flags = nullptr;
    // long rows run beside the main sweep on a forked stream (fork/join with events)
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // host operands as a pipeline of feature windows (run_group_windows): upload and download streams, an event pair per window
    hipStream_t pipe_up = nullptr, pipe_down = nullptr;   // (the process's pair for this device: Context::pipe_streams)
    std::vector<hipEvent_t> pipe_ev;
    int64_t host_windows_used = 0;   // windows of the last call with host operands (1 = the serial path)
    int64_t host_direct_used = 0;    // ... 1 = their products stored straight into the caller's page-locked tensor
    bool host_copies_slow = false;   // a pipelined call of this group saw its last download run below 40 GB/s: later calls store directly (host_direct = 1)
    double timers[5] = {0, 0, 0, 0, 0};
    // HIP-event pairs around the dominant kernel (tunable kernel_events), resolved on query
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pending;
    bool kernel_events = false;  // pygim_group_kernel_events
    double ev_ms = 0;
    int64_t ev_count = 0;
};

struct Context {
    bool inited = false;
    int device = 0;
    int cu_count = 0;
    int64_t nr_ranks = 0;
    std::set<Group *> groups;
    std::mutex mu;
    // slice-major copies of X for the panel sweep: one buffer per (device, launch stream) -- products on different
    // streams never share a buffer -- each with a record of what it holds, for callers that pass x_unchanged.
    // At most XS_MAX buffers are kept (least recently used goes first); all are freed with the last group.
    struct XsKey {   // what a buffer holds (the LDS-staged product compares and records it as a whole, lds_stage_x)
        const void *src = nullptr;  // X pointer, stride, rows, width, element size
        int64_t ld = 0, rows = 0, w = 0;
        const void *order = nullptr;   // the copy's rows are X[order[pos]] (a density-split part), or X's own order
        uint64_t rows_pad = 0;  // kind 1 / 3 / 5: rows of a slice in THIS copy (whole chunks of the part that packed it) -> its slice stride
        size_t es = 0;
        int kind = 0;  // 0 = 128-byte slices (sweep), 1 = 256-byte slices, rows padded to whole chunks (LDS-staged product; 3: INT8 widened, 5: half-split)
        bool operator==(const XsKey &o) const {
            return src == o.src && ld == o.ld && rows == o.rows && w == o.w && order == o.order && rows_pad == o.rows_pad && es == o.es && kind == o.kind;
        }
    };
    struct XsBuf : XsKey {
        void *ptr = nullptr;
        size_t bytes = 0;
        uint64_t stamp = 0;
        int in_use = 0;  // handed to a call that has not enqueued its kernels yet: not an eviction victim
    };
    static constexpr size_t XS_MAX = 4;
    std::map<std::pair<int, hipStream_t>, XsBuf> xs_bufs;
    uint64_t xs_clock = 0;
    std::map<int, std::pair<hipStream_t, hipStream_t>> pipe_streams;   // per device: upload / download streams of the host-operand pipeline (run_group_windows)
    int64_t group_serial = 0;  // creation serial of the newest group (pygim_group_serial)
    int64_t generation = 0;  // bumped by pygim_release: handles made before it are dead even if an address comes back
} g_ctx;

void free_xs_buffers_locked() {
    for (auto &kv : g_ctx.xs_bufs)
        if (kv.second.ptr) (void)hipFree(kv.second.ptr);
    g_ctx.xs_bufs.clear();
}

// the slice-major buffer of (current device, stream), at least `need` bytes; evicts the least recently used buffer
// when more than XS_MAX exist.  Caller holds g_ctx.mu.
int xs_buffer_locked(hipStream_t st, size_t need, Context::XsBuf **out) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    const auto key = std::make_pair(dev, st);
    if (!g_ctx.xs_bufs.count(key) && g_ctx.xs_bufs.size() >= Context::XS_MAX) {
        auto victim = g_ctx.xs_bufs.end();
        for (auto it = g_ctx.xs_bufs.begin(); it != g_ctx.xs_bufs.end(); ++it)
            if (it->second.in_use == 0 && (victim == g_ctx.xs_bufs.end() || it->second.stamp < victim->second.stamp)) victim = it;
        if (victim != g_ctx.xs_bufs.end()) {  // (all busy: grow past the cap rather than pull a buffer from under a caller)
            if (victim->second.ptr) (void)hipFree(victim->second.ptr);  // hipFree waits for the work that uses it
            g_ctx.xs_bufs.erase(victim);
        }
    }
    Context::XsBuf &b = g_ctx.xs_bufs[key];
    if (b.bytes < need) {
        if (b.ptr) (void)hipFree(b.ptr);
        b = Context::XsBuf();
        if (hipMalloc(&b.ptr, need) != hipSuccess) {
            (void)hipGetLastError();
            g_ctx.xs_bufs.erase(key);
            return fail(PYGIM_ERR_HIP, "slice-major buffer alloc");
        }
        b.bytes = need;
    }
    b.stamp = ++g_ctx.xs_clock;
    b.in_use++;
    *out = &b;
    return 0;
}

// a slice-major buffer stays pinned (not evictable by other threads' calls) until the kernels that read it are enqueued;
// after that hipFree's implicit wait protects it
struct XsPin {
    void *ptr = nullptr;
    void hold(void *p) { ptr = p; }
    ~XsPin() {
        if (!ptr) return;
        std::lock_guard<std::mutex> lk(g_ctx.mu);
        for (auto &kv : g_ctx.xs_bufs)
            if (kv.second.ptr == ptr && kv.second.in_use > 0) kv.second.in_use--;
    }
};

bool is_device_ptr(const void *p) {
    if (!p) return false;
    hipPointerAttribute_t attr;
    hipError_t e = hipPointerGetAttributes(&attr, p);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged;
}

int ensure(void **buf, size_t *have, size_t need) {
    if (*have >= need) return 0;
    if (*buf) HIP_TRY(hipFree(*buf));
    *buf = nullptr;
    *have = 0;
    HIP_TRY(hipMalloc(buf, need));
    *have = need;
    return 0;
}

// bring an array to the device (copy if it is host memory, alias if already there)
template <typename P> int to_device(const void *src, size_t bytes, P **dst, bool *owned, hipStream_t st) {
    if (bytes == 0) {
        // keep a valid non-null pointer so kernels can take it
        HIP_TRY(hipMalloc((void **)dst, 16));
        *owned = true;
        return 0;
    }
    if (is_device_ptr(src)) {
        *dst = (P *)const_cast<void *>(src);
        *owned = false;
        return 0;
    }
    HIP_TRY(hipMalloc((void **)dst, bytes));
    *owned = true;
    HIP_TRY(hipMemcpyAsync(*dst, src, bytes, hipMemcpyHostToDevice, st));
    return 0;
}

// Executable device memory for the code-stream kernels: hipMalloc memory is not executable (an instruction fetch from it faults),
// the HSA runtime's coarse-grained GPU pool with HSA_AMD_MEMORY_POOL_EXECUTABLE_FLAG is (it is what the loader puts kernels in).
struct ExecPool {
    bool tried = false, ok = false;
    hsa_agent_t agent{};
    hsa_amd_memory_pool_t pool{};
};
static std::map<int, ExecPool> g_exec_pools;   // per HIP device ordinal (guarded by g_ctx.mu)
static ExecPool *exec_pool_locked(int dev) {
    ExecPool &ep = g_exec_pools[dev];
    if (ep.tried) return ep.ok ? &ep : nullptr;
    ep.tried = true;
    if (hsa_init() != HSA_STATUS_SUCCESS) return nullptr;   // (reference-counted: HIP holds the runtime open already)
    // the HSA agent of this HIP device: by PCI address (HIP_VISIBLE_DEVICES renumbers HIP's devices, not the runtime's agents);
    // by ordinal only when the address cannot be had
    struct Find { int want, seen; int bdf, domain; hsa_agent_t agent, nth; bool found, have_nth; } f{dev, 0, -1, -1, {}, {}, false, false};
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) == hipSuccess) {
        f.bdf = (prop.pciBusID << 8) | (prop.pciDeviceID << 3);
        f.domain = prop.pciDomainID;
    }
    hsa_iterate_agents([](hsa_agent_t a, void *d) -> hsa_status_t {
        Find *f = (Find *)d;
        hsa_device_type_t t;
        if (hsa_agent_get_info(a, HSA_AGENT_INFO_DEVICE, &t) != HSA_STATUS_SUCCESS || t != HSA_DEVICE_TYPE_GPU) return HSA_STATUS_SUCCESS;
        if (f->seen++ == f->want) { f->nth = a; f->have_nth = true; }
        uint32_t bdf = 0, domain = 0;
        if (f->bdf >= 0 && hsa_agent_get_info(a, (hsa_agent_info_t)HSA_AMD_AGENT_INFO_BDFID, &bdf) == HSA_STATUS_SUCCESS &&
            hsa_agent_get_info(a, (hsa_agent_info_t)HSA_AMD_AGENT_INFO_DOMAIN, &domain) == HSA_STATUS_SUCCESS &&
            (int)(bdf & ~7u) == f->bdf && (int)domain == f->domain) {
            f->agent = a;
            f->found = true;
            return HSA_STATUS_INFO_BREAK;
        }
        return HSA_STATUS_SUCCESS;
    }, &f);
    if (!f.found) {
        if (!f.have_nth) return nullptr;
        f.agent = f.nth;
    }
    struct FindPool { hsa_amd_memory_pool_t pool; bool found; } fp{{}, false};
    hsa_amd_agent_iterate_memory_pools(f.agent, [](hsa_amd_memory_pool_t p, void *d) -> hsa_status_t {
        FindPool *fp = (FindPool *)d;
        hsa_amd_segment_t seg;
        uint32_t flags = 0;
        bool alloc = false;
        hsa_amd_memory_pool_get_info(p, HSA_AMD_MEMORY_POOL_INFO_SEGMENT, &seg);
        hsa_amd_memory_pool_get_info(p, HSA_AMD_MEMORY_POOL_INFO_GLOBAL_FLAGS, &flags);
        hsa_amd_memory_pool_get_info(p, HSA_AMD_MEMORY_POOL_INFO_RUNTIME_ALLOC_ALLOWED, &alloc);
        if (seg == HSA_AMD_SEGMENT_GLOBAL && alloc && (flags & HSA_AMD_MEMORY_POOL_GLOBAL_FLAG_COARSE_GRAINED)) {
            fp->pool = p;
            fp->found = true;
            return HSA_STATUS_INFO_BREAK;
        }
        return HSA_STATUS_SUCCESS;
    }, &fp);
    if (!fp.found) return nullptr;
    ep.agent = f.agent;
    ep.pool = fp.pool;
    ep.ok = true;
    return &ep;
}
// executable device memory from the HSA pool (hipMalloc memory faults on instruction fetch); nullptr + *why when there is none
static void *exec_alloc(size_t bytes, std::string *why = nullptr) {
    auto say = [&](const char *m) { if (why) *why = m; };
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { say("no current HIP device"); return nullptr; }
    ExecPool *ep;
    {
        std::lock_guard<std::mutex> lk(g_ctx.mu);
        ep = exec_pool_locked(dev);
    }
    if (!ep) { say("the HSA runtime offers no executable device memory pool"); return nullptr; }
    void *ptr = nullptr;
    if (hsa_amd_memory_pool_allocate(ep->pool, bytes, HSA_AMD_MEMORY_POOL_EXECUTABLE_FLAG, &ptr) != HSA_STATUS_SUCCESS) {
        say("the executable pool could not allocate the code");
        return nullptr;
    }
    return ptr;
}
static void *exec_alloc_upload(const void *host, size_t bytes, std::string *why = nullptr) {
    auto say = [&](const char *m) { if (why) *why = m; };
    // the code goes up through HIP (a bounded staging buffer and a copy kernel: the executable allocation is a device address like any
    // other inside a kernel); the HSA runtime is asked for the memory only
    const size_t piece = std::min<size_t>(bytes, (size_t)64 << 20);   // 64 MiB at a time: no second full-size allocation beside the code
    void *ptr = exec_alloc(bytes, why), *stage = nullptr;
    if (!ptr) return nullptr;
    if (hipMalloc(&stage, std::max<size_t>(piece, 256)) != hipSuccess) {
        (void)hipGetLastError();
        (void)hsa_amd_memory_pool_free(ptr);
        say("out of device memory for the staging buffer of the code upload");
        return nullptr;
    }
    bool ok = true;
    for (size_t off = 0; off < bytes && ok; off += piece) {
        const size_t nb = std::min(piece, bytes - off);
        ok = hipMemcpy(stage, (const char *)host + off, nb, hipMemcpyHostToDevice) == hipSuccess;
        const uint64_t n16 = nb / 16;   // (the code blob is a multiple of 256 bytes)
        if (ok && n16) {
            hipLaunchKernelGGL(k_copy16, dim3((unsigned)((n16 + 255) / 256)), dim3(256), 0, 0, (const u32x4_t *)stage, (u32x4_t *)((char *)ptr + off), n16);
            ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess;   // (the staging buffer is re-used)
        }
    }
    (void)hipFree(stage);
    if (!ok) {
        (void)hsa_amd_memory_pool_free(ptr);
        say("copying the code to the device failed");
        return nullptr;
    }
    return ptr;
}

void free_part(Part &p) {
    if (p.own_rowptr && p.rowptr) (void)hipFree(p.rowptr);
    if (p.own_rowind && p.rowind) (void)hipFree(p.rowind);
    if (p.own_colind && p.colind) (void)hipFree(p.colind);
    if (p.own_vals && p.vals) (void)hipFree(p.vals);
    if (p.vals_narrow) (void)hipFree(p.vals_narrow);
    p.vals_narrow = nullptr;
    for (LongPlan *lp : {&p.lp_base, &p.lp_panel}) {
        if (lp->d_tasks) (void)hipFree(lp->d_tasks);
        if (lp->d_desc) (void)hipFree(lp->d_desc);
    }
    if (p.d_items) (void)hipFree(p.d_items);
    if (p.col16) (void)hipFree(p.col16);
    if (p.d_spmv_units) (void)hipFree(p.d_spmv_units);
    for (void *q : {(void *)p.lds_tok, (void *)p.lds_nb, (void *)p.lds_chunks, (void *)p.lds_rowmap, (void *)p.lds_tiles})
        if (q) (void)hipFree(q);
    p.lds_tok = p.lds_nb = p.lds_chunks = p.lds_rowmap = nullptr;
    p.lds_tiles = nullptr;
    if (p.lds_code) (void)hsa_amd_memory_pool_free(p.lds_code);
    if (p.lds_code_start) (void)hipFree(p.lds_code_start);
    p.lds_code = nullptr;
    p.lds_code_start = nullptr;
    p.lds_is_code = false;
    p.lds_row_bytes = 256;
    p.lds_col_splits = 1;
    p.lds_rows = 0;
    p.lds_half = 0;
    if (p.lds_tail_segs) (void)hipFree(p.lds_tail_segs);
    if (p.lds_tail_rowseg) (void)hipFree(p.lds_tail_rowseg);
    p.lds_tail_segs = p.lds_tail_rowseg = nullptr;
    p.lds_tail_nseg = 0;
    if (p.extra) free_part(*p.extra);
    if (p.hy_dense) free_part(*p.hy_dense);
    if (p.hy_sparse) free_part(*p.hy_sparse);
    if (p.lds_col_order) {
        // (a staged copy made in this order must not be taken for another part's whose order array lands at the same address later)
        std::lock_guard<std::mutex> lk(g_ctx.mu);
        for (auto &kv : g_ctx.xs_bufs)
            if (kv.second.order == (const void *)p.lds_col_order) { kv.second.src = nullptr; kv.second.order = nullptr; }
        (void)hipFree(p.lds_col_order);
    }
    p.lds_col_order = nullptr;
}

void free_group(Group *g) {
    for (auto &p : g->parts) free_part(p);
    if (g->merged) free_part(*g->merged);
    if (g->scratch) (void)hipFree(g->scratch);
    if (g->stage_in) (void)hipFree(g->stage_in);
    if (g->stage_out) (void)hipFree(g->stage_out);
    if (g->xcat) (void)hipFree(g->xcat);
    if (g->xq) (void)hipFree(g->xq);
    if (g->oq) (void)hipFree(g->oq);
    if (g->d_ptrs) (void)hipFree(g->d_ptrs);
    if (g->h_ptrs) (void)hipHostFree(g->h_ptrs);
    for (hipEvent_t e : g->ev_ptrs)
        if (e) (void)hipEventDestroy(e);
    if (g->d_flags) (void)hipFree(g->d_flags);
    if (g->side) (void)hipStreamDestroy(g->side);
    for (hipEvent_t e : g->pipe_ev)
        if (e) (void)hipEventDestroy(e);
    if (g->ev_fork) (void)hipEventDestroy(g->ev_fork);
    if (g->ev_join) (void)hipEventDestroy(g->ev_join);
    for (auto &e : g->ev_pending) {
        (void)hipEventDestroy(e.first);
        (void)hipEventDestroy(e.second);
    }
    delete g;
}

Group *lookup(int64_t handle) {
    Group *g = reinterpret_cast<Group *>(static_cast<uintptr_t>(handle));
    std::lock_guard<std::mutex> lk(g_ctx.mu);
    return g_ctx.groups.count(g) ? g : nullptr;
}
