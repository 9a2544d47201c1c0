"""The plan of the L2 sweep restated in numpy from its rules (not from pygim_amd/csrc/sweep_plan.hpp): tests/test_sweep_plan.py compares the header's
answers with it element for element, tests/test_parity_gpu.py a created group's plan.

The rules: panels hold ceil(ncols / npan) columns, npan from the byte budget; panels that do not pay, or columns stored out of order, mean ONE panel.
A row whose share of one panel exceeds 16 x the long-row threshold is heavy: it is in no panel and is cut into segments.  Every other row is an item of
each panel it has entries in, an empty row an item of panel 0 (not in a part that only adds).  A panel's items are in a stable order, longest first;
with a locality rank, the items behind the wave-cooperative prefix are regrouped by blocks of 2048 ranks, keeping their order inside a block."""
import numpy as np

KNOBS = dict(panel_mode=0, panel_bytes=4 << 20, panel_min_seg=8, panel_coop=512, panel_locality=1, panel_col16=1, vec_lds=1, vec_kernel=1,
             long_row_threshold=4096, long_segment=512)   # the library's defaults
FIRST, LAST = 0x80000000, 0x40000000


def ceil_div(a, b):
    return -(-a // b)


def panel_count(nrows, ncols, nnz, es, h_hint, k, cols_sorted):
    """(a plan is built, wanted panels, the sortedness is asked, panels, columns per panel)"""
    if k["panel_mode"] == 2 or nrows <= 0 or nnz <= 0:
        return False, 0, False, 0, 0
    budget = max(1, k["panel_bytes"] // 128)
    if 1 <= h_hint <= 4 and k["vec_lds"] and k["vec_kernel"]:
        budget = max(1, min(budget, 65536, (128 * 1024 - 64) // (h_hint * es)))
    npan = max(1, ceil_div(ncols, budget))
    worth = k["panel_mode"] == 1 or npan == 1 or nnz / (nrows * npan) >= k["panel_min_seg"]
    want = npan if worth else 1
    ask = want > 1
    npan = 1 if ask and not cols_sorted else want
    return True, want, ask, npan, ceil_div(ncols, npan)


def segments(rowptr, rows, seg):
    """(row, first entry, end) of the segments the given rows are cut into"""
    return [(int(r), a, min(int(rowptr[r + 1]), a + seg)) for r in rows for a in range(int(rowptr[r]), int(rowptr[r + 1]), seg)]


def plan(rowptr, col, ncols, es=4, h_hint=64, is_extra=False, sim_kind=0, sim_order=None, **knobs):
    k = dict(KNOBS, **knobs)
    rowptr, col = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    nrows, nnz = len(rowptr) - 1, len(col)
    deg = np.diff(rowptr)
    row_of = np.repeat(np.arange(nrows), deg)
    inside = np.ones(nnz, dtype=bool)
    inside[rowptr[:-1][deg > 0]] = False   # an entry that is not its row's first ...
    cols_sorted = not np.any(inside[1:] & (col[1:] < col[:-1])) if nnz > 1 else True   # ... is not below the entry before it
    built, want, ask, npan, panel_cols = panel_count(nrows, ncols, nnz, es, h_hint, k, cols_sorted)
    base_thresh = min(max(k["long_row_threshold"], 64), 0x7FFFFFFF)
    seg = min(base_thresh, max(64, k["long_segment"]))
    out = dict(plan=int(built), want_npan=want, ask_sorted=int(ask), n_panels=npan, panel_cols=panel_cols, base_thresh=base_thresh, seg=seg,
               base_tasks=[x for t in segments(rowptr, np.nonzero(deg > base_thresh)[0], seg) for x in t])
    if not built:
        return out
    # entries of every row in every panel; with one panel the columns are not looked at
    count = np.zeros((npan, nrows), dtype=np.int64)
    if npan == 1:
        count[0] = deg
    else:
        np.add.at(count, (col // panel_cols, row_of), 1)
    begin = rowptr[:-1][None, :] + np.cumsum(count, axis=0) - count
    heavy = (count > 16 * base_thresh).any(axis=0)
    want_sim = bool(k["panel_locality"]) and not 1 <= h_hint <= 4 and (not is_extra or sim_kind == 2)
    rank = None
    if want_sim and sim_kind == 1:
        rank = np.arange(nrows)
    elif want_sim and sim_kind == 2:
        rank = np.empty(nrows, dtype=np.int64)
        rank[np.asarray(sim_order)] = np.arange(nrows)
    coop_cap = max(64, k["panel_coop"])
    rows, beg, lens, off, coop, long128, pnnz = [], [], [], [0], [], [], []
    for q in range(npan):
        item = ~heavy & (count[q] > 0)
        if q == 0 and not is_extra:
            item |= ~heavy & (deg == 0)
        r = np.nonzero(item)[0]
        r = r[np.argsort(-count[q][r], kind="stable")]
        nco = int((count[q][r] > coop_cap).sum())
        if rank is not None:
            tail = r[nco:]
            r = np.concatenate([r[:nco], tail[np.argsort(rank[tail] >> 11, kind="stable")]])
        length = count[q][r]
        coop.append(nco)
        long128 += [int((length > b).sum()) for b in (256, 128, 64, 32)]
        pnnz.append(int(length.sum()))
        flags = np.where(begin[q][r] == rowptr[r], FIRST, 0) | np.where(begin[q][r] + length == rowptr[r + 1], LAST, 0)
        rows += r.tolist()
        beg += begin[q][r].tolist()
        lens += (length | flags).tolist()
        off.append(len(rows))
    out.update(heavy=np.nonzero(heavy)[0].tolist(), segment_tasks=[x for t in segments(rowptr, np.nonzero(heavy & (deg > 0))[0], seg) for x in t],
               want_sim=int(want_sim), locality=int(rank is not None), n_items=len(rows), rows=rows, beg=beg, lens=lens, panel_off=off, panel_coop=coop,
               panel_long128=long128, panel_nnz=pnnz, col16=int(bool(k["panel_col16"]) and panel_cols <= 65536 and nnz > 0 and len(rows) > 0), col16_bytes=nnz * 2 + 64)
    return out
