"""The glue of the resident frame step (pl-svo_amd/csrc/chain_kernels.hip) in the reference's own sequential form, plain NumPy float64:
which candidates are filed in the grids (Reprojector::reproject, src/reprojector.cpp:389-423), which of their matches become features
of the new frame (reprojectMap's two cell loops and refineBestCandidate, :188-276) and what a feature hands to the pose optimiser
(Reprojector::refine :311, :373 and the Feature constructors, src/feature.cpp:103-104).  Written from those lines, not from the kernel:
lists that are appended to and walked, counters that are incremented and compared, one candidate at a time.

Candidate order of one stream, as everywhere in the C ABI: [points | segment start points | segment end points]."""
import numpy as np


def active_rule(active_in, cell, n_pt, n_seg):
    """Which candidates are filed at all.  A point: the caller wants it (active_in; None = every one) and its projection is in frame
    (`cell` >= 0, the 8-pixel border of reproject :393).  A segment: that for BOTH end points (:410-411); both of its entries carry the
    answer.  Returns a bool array over the candidates."""
    cell = np.asarray(cell)
    want = np.ones(n_pt + 2 * n_seg, bool) if active_in is None else np.asarray(active_in).astype(bool)
    out = np.zeros(n_pt + 2 * n_seg, bool)
    for k in range(n_pt):
        out[k] = bool(want[k]) and cell[k] >= 0
    for s in range(n_seg):
        a, e = n_pt + s, n_pt + n_seg + s
        ok = bool(want[a]) and cell[a] >= 0 and bool(want[e]) and cell[e] >= 0
        out[a] = out[e] = ok
    return out


def _visit(cells, order, success, limit):
    """reprojectMap's loop over one grid (:188-198, :201-208): cells in visit order; refineBestCandidate walks the cell's list and returns
    at the first candidate that refines (:243-254); the visit ends AFTER the match that makes the counter exceed the limit"""
    out, n_matches = [], 0
    for i in range(len(cells)):
        for cand in cells[int(order[i])]:
            if success(cand):
                out.append(cand)
                n_matches += 1
                break
        if n_matches > limit:
            break
    return np.array(out, np.int32)


def select_points(found, active, cell, n_pt, cell_order=None, max_fts=None, n_cells=None):
    """Point features of the new frame, as indices into the point candidates, in the order they are created.  With a grid (n_cells
    given): filed candidates are pushed onto their cell's list in the caller's order (:399), the cells are visited in cell_order (None:
    0, 1, ...) under max_fts.  Without: every filed candidate that matched, in candidate order."""
    found, active, cell = np.asarray(found).astype(bool), np.asarray(active).astype(bool), np.asarray(cell)
    if n_cells is None:
        return np.array([k for k in range(n_pt) if active[k] and found[k]], np.int32)
    cells = [[] for _ in range(n_cells)]
    for k in range(n_pt):
        if active[k]:
            cells[int(cell[k])].append(k)
    order = np.arange(n_cells) if cell_order is None else cell_order
    return _visit(cells, order, lambda k: bool(found[k]), max_fts)


def segment_cells(proj_px, n_pt, n_seg, seg_cell_size, seg_n_cols):
    """(sk, ek): the cells of the segment grid a segment's projected start and end points fall in (:413-416)"""
    proj_px = np.asarray(proj_px, np.float64)
    sk, ek = np.zeros(n_seg, np.int64), np.zeros(n_seg, np.int64)
    for s in range(n_seg):
        sp, ep = proj_px[n_pt + s], proj_px[n_pt + n_seg + s]
        with np.errstate(invalid="ignore", over="ignore"):
            sk[s] = int(sp[1] / seg_cell_size) * seg_n_cols + int(sp[0] / seg_cell_size) if np.all(np.isfinite(sp)) else -1
            ek[s] = int(ep[1] / seg_cell_size) * seg_n_cols + int(ep[0] / seg_cell_size) if np.all(np.isfinite(ep)) else -1
    return sk, ek


def select_segments(found, active, proj_px, n_pt, n_seg, seg_cell_size=0, seg_n_cols=0, seg_cell_order=None, max_fts_segs=None, seg_n_cells=None):
    """Segment features of the new frame, as indices into the segment candidates, in the order they are created.  A segment matched
    when both of its end points refined (matcher.cpp:250-274).  With the segments' grid (seg_n_cells given): a filed segment is pushed
    onto the list of its start point's cell AND of its end point's cell (:418-419), cells are visited in seg_cell_order under
    max_fts_segs, and a segment that is the first success of both of its cells becomes a feature twice (refine adds a LineFeat per
    success, :373-374).  Without: every filed segment that matched, in candidate order."""
    found, active = np.asarray(found).astype(bool), np.asarray(active).astype(bool)
    ok = lambda s: bool(found[n_pt + s]) and bool(found[n_pt + n_seg + s])
    filed = lambda s: bool(active[n_pt + s]) and bool(active[n_pt + n_seg + s])
    if seg_n_cells is None:
        return np.array([s for s in range(n_seg) if filed(s) and ok(s)], np.int32)
    sk, ek = segment_cells(proj_px, n_pt, n_seg, seg_cell_size, seg_n_cols)
    cells = [[] for _ in range(seg_n_cells)]
    for s in range(n_seg):
        if filed(s):
            cells[int(sk[s])].append(s)
            cells[int(ek[s])].append(s)
    order = np.arange(seg_n_cells) if seg_cell_order is None else seg_cell_order
    return _visit(cells, order, ok, max_fts_segs)


def bearing(cam, px):
    """Feature::f: cam2world of the pixel, normalised (the Feature constructors)"""
    fx, fy, cx, cy = [float(v) for v in cam[:4]]
    x, y = (float(px[0]) - cx) / fx, (float(px[1]) - cy) / fy
    n = np.sqrt(x * x + y * y + 1.0)
    return np.array([x / n, y / n, 1.0 / n])


def features(cam, px, search_level, pos, n_pt, n_seg, sel_pt, sel_seg):
    """What the selected matches hand to the pose optimiser, in selection order: PointFeat(frame, px, search_level_) -> unit bearing,
    landmark position, level; LineFeat(frame, spx, epx, search_level_) -> line = sf x ef scaled by its image-plane norm
    (feature.cpp:103-104), the landmark's two end positions, level.  The level is Matcher::search_level_ as the match left it: for a
    segment that is the END point's (matcher.cpp:264 runs last, reprojector.cpp:373 reads it afterwards).  A level is used as a shift,
    so the -1 of a rejected candidate never reaches a feature; max(level, 0) only keeps the array well formed."""
    px, pos, search_level = np.asarray(px, np.float64), np.asarray(pos, np.float64), np.asarray(search_level)
    out = dict(pt_f=np.zeros((len(sel_pt), 3)), pt_pos=np.zeros((len(sel_pt), 3)), pt_level=np.zeros(len(sel_pt), np.int32),
               seg_line=np.zeros((len(sel_seg), 3)), seg_spos=np.zeros((len(sel_seg), 3)), seg_epos=np.zeros((len(sel_seg), 3)),
               seg_level=np.zeros(len(sel_seg), np.int32))
    for i, k in enumerate(sel_pt):
        out["pt_f"][i] = bearing(cam, px[k])
        out["pt_pos"][i] = pos[k]
        out["pt_level"][i] = max(int(search_level[k]), 0)
    for i, s in enumerate(sel_seg):
        a, e = n_pt + int(s), n_pt + n_seg + int(s)
        line = np.cross(bearing(cam, px[a]), bearing(cam, px[e]))
        out["seg_line"][i] = line / np.sqrt(line[0] * line[0] + line[1] * line[1])
        out["seg_spos"][i], out["seg_epos"][i] = pos[a], pos[e]
        out["seg_level"][i] = max(int(search_level[e]), 0)
    return out


def brute_force_selection(found, active, cell, n_pt, order, limit, n_seg=0, seg_cells=None):
    """The same selections stated the other way round, for tests/test_chain_host.py: per cell the set of filed candidates that matched,
    its minimum the cell's winner; the winning cells sorted by their place in the visit order; the first limit + 1 of them.
    seg_cells = (sk, ek): segments (a candidate belongs to two cells), else points."""
    found, active = np.asarray(found).astype(bool), np.asarray(active).astype(bool)
    order = np.asarray(order)
    rank = np.empty(len(order), np.int64)
    rank[order] = np.arange(len(order))
    if seg_cells is None:
        matched = np.nonzero(found[:n_pt] & active[:n_pt])[0]
        member = [(int(cell[k]), int(k)) for k in matched]
    else:
        sk, ek = seg_cells
        ok = found[n_pt:n_pt + n_seg] & found[n_pt + n_seg:n_pt + 2 * n_seg] & active[n_pt:n_pt + n_seg] & active[n_pt + n_seg:n_pt + 2 * n_seg]
        member = [(int(c), int(s)) for s in np.nonzero(ok)[0] for c in {int(sk[s]), int(ek[s])}]
    winner = {}
    for c, k in member:
        winner[c] = min(winner.get(c, k), k)
    won = sorted(winner, key=lambda c: rank[c])
    return np.array([winner[c] for c in won[:limit + 1]], np.int32)
