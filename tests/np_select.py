"""Restatement of the second half of Reprojector::reprojectMap, loop for loop like the reference (test infrastructure only):

  Reprojector::setMapCandidates     src/reprojector.cpp:116-131   n_failed_reproj_ += 3 for a candidate that does not project, above 30 deleted and erased
  Reprojector::reprojectMap         src/reprojector.cpp:185-216   the cells in cell_order, the stop after the match that exceeds maxFts / maxFtsSegs
  Reprojector::refineBestCandidate  src/reprojector.cpp:236-276   cell.sort(qualityComparator), n_trials_, erase, first success returns
  Reprojector::refine               src/reprojector.cpp:278-387   the counters, promotion, deletion, the new feature
  Map::safeDeletePoint / safeDeleteSegment                 src/map.cpp:116-139   ftr->feat3D = NULL in every keyframe, TYPE_DELETED
  MapPointCandidates::deleteCandidatePoint (and segments)  src/map.cpp:311-324, :403-416   only a listed landmark is deleted
  [ext] Eigen's normalize() of a 2-vector: two divisions by sqrt(x*x + y*y)

Written as the reference is: a list per cell filled in filing order, list.sort with the comparator at the moment of the visit, the head
of the list tried and erased, landmarks mutated as it goes.  The kernel's formulation (lowest index per cell, a prefix over the visit
order, keys) is deliberately NOT used here.

select() works on the stream dict of tests/np_candidates.py, extended by pt_nfail / pt_nsucc / seg_nfail / seg_nsucc (quality()), and
MUTATES it: types, counters, the keyframes' feature lists, the candidate lists -- what the next frame's candidates() must see.  The
matcher's results are inputs: `match` holds found / px / search_level per entry [points | start points | end points] in the output order
of candidates(); `A` maps a point's output index to Matcher::A_cur_ref_ (row-major, needed for edgelet observations only).
The observation lists of a deleted landmark are left alone (the reference clears them; a deleted landmark is never matched)."""
import functools
import math

import np_candidates as N

EVENT_PROMOTED, EVENT_DELETED = 1, 2
FTR_CORNER, FTR_EDGELET = 0, 1


def quality(st):
    """the counters of a freshly staged stream: zero"""
    for name, n in (("pt", len(st["pt_pos"])), ("seg", len(st["seg_spos"]))):
        st.setdefault(name + "_nfail", [0] * n)
        st.setdefault(name + "_nsucc", [0] * n)
    return st


def n_cells(cam, cell_size):
    return (-(-int(cam[4]) // cell_size)) * (-(-int(cam[5]) // cell_size))


def _quality_comparator(types):
    """pointQualityComparator / lineQualityComparator as list.sort's cmp: lhs before rhs iff lhs.type_ > rhs.type_"""
    comp = lambda lhs, rhs: types[lhs["lm"]] > types[rhs["lm"]]
    return functools.cmp_to_key(lambda a, b: -1 if comp(a, b) else (1 if comp(b, a) else 0))


def select(st, r, match, cam, cell_size, seg_cell_size, max_fts, max_fts_segs, cell_order=None, seg_cell_order=None, A=None, promote=True):
    """one stream, one frame.  r: candidates(st, ...) of this frame, computed BEFORE the call.  promote=False leaves out the promotion to
    TYPE_GOOD (a knob for the tests: what the result would be were the cells' order not decided at visit time)."""
    quality(st)
    n_pt, n_seg = r["n_filed_pt"], r["n_filed_seg"]
    events = dict(pt=[0] * len(st["pt_pos"]), seg=[0] * len(st["seg_spos"]))
    out = dict(n_matches=0, n_ls_matches=0, n_trials=0, pt_lm=[], pt_px=[], pt_level=[], pt_type=[], pt_grad=[], seg_lm=[], seg_px=[], seg_level=[],
               tried_pt=[], tried_seg=[], visited_cells=[], visited_seg_cells=[])

    # ---- setMapCandidates (:116-131): the failures, in list order
    for name in ("pt", "seg"):
        lst, failed = st[name + "_cand"], r[name + "_cand_failed"]
        it = j = 0
        while it != len(lst):
            lm = lst[it]
            if failed[j]:
                st[name + "_nfail"][lm] += 3
                if st[name + "_nfail"][lm] > 30:
                    st[name + "_type"][lm] = N.TYPE_DELETED           # deleteCandidate
                    events[name][lm] |= EVENT_DELETED
                    del lst[it]                                       # it = candidates_.erase(it)
                    j += 1
                    continue
            it += 1
            j += 1

    def safe_delete(name, lm):                                        # Map::safeDeletePoint / safeDeleteSegment
        for fts in st["kf_" + name]:
            for k, v in enumerate(fts):
                if v == lm:
                    fts[k] = -1                                       # ftr->feat3D = NULL
        st[name + "_type"][lm] = N.TYPE_DELETED
        events[name][lm] |= EVENT_DELETED

    def delete_candidate(name, lm):                                   # deleteCandidatePoint / deleteCandidateSegment
        lst = st[name + "_cand"]
        for it, v in enumerate(lst):
            if v == lm:
                st[name + "_type"][lm] = N.TYPE_DELETED
                events[name][lm] |= EVENT_DELETED
                del lst[it]
                return True
        return False

    def quality_logic(name, lm, found_match):                         # refine :291-308, :352-370
        types, nfail, nsucc = st[name + "_type"], st[name + "_nfail"], st[name + "_nsucc"]
        if not found_match:
            nfail[lm] += 1
            if types[lm] == N.TYPE_UNKNOWN and nfail[lm] > 15:
                safe_delete(name, lm)
            if types[lm] == N.TYPE_CANDIDATE and nfail[lm] > 30:
                delete_candidate(name, lm)
            return False
        nsucc[lm] += 1
        if types[lm] == N.TYPE_UNKNOWN and nsucc[lm] > 10 and promote:
            types[lm] = N.TYPE_GOOD
            events[name][lm] |= EVENT_PROMOTED
        return True

    def refine_pt(c):
        lm, i = c["lm"], c["i"]
        if st["pt_type"][lm] == N.TYPE_DELETED:
            return False
        found_match = bool(r["pt_has_view"][i]) and bool(match["found"][i])          # findMatchDirect: getCloseViewObs first
        if not quality_logic("pt", lm, found_match):
            return False
        out["pt_lm"].append(lm); out["pt_px"].append([float(v) for v in match["px"][i]]); out["pt_level"].append(int(match["search_level"][i]))
        ref = st["pt_obs"][lm][r["pt_obs"][i]]                        # matcher_.ref_ftr_
        if ref["type"] == FTR_EDGELET:
            a = A[i]
            g = [a[0] * ref["grad"][0] + a[1] * ref["grad"][1], a[2] * ref["grad"][0] + a[3] * ref["grad"][1]]
            n = math.sqrt(g[0] * g[0] + g[1] * g[1])
            out["pt_type"].append(FTR_EDGELET); out["pt_grad"].append([N._div(g[0], n), N._div(g[1], n)])
        else:
            out["pt_type"].append(FTR_CORNER); out["pt_grad"].append([1.0, 0.0])
        return True

    def refine_seg(c):
        lm, i = c["lm"], c["i"]
        if st["seg_type"][lm] == N.TYPE_DELETED:
            return False
        s, e = n_pt + i, n_pt + n_seg + i
        found_match = bool(r["seg_has_view"][i]) and bool(match["found"][s]) and bool(match["found"][e])
        if not quality_logic("seg", lm, found_match):
            return False
        out["seg_lm"].append(lm); out["seg_px"].append([float(v) for v in match["px"][s]] + [float(v) for v in match["px"][e]])
        out["seg_level"].append(int(match["search_level"][e]))       # search_level_ after the END point's match
        return True

    def refine_best_candidate(cell, types, refine, tried):
        cell.sort(key=_quality_comparator(types))
        while cell:
            out["n_trials"] += 1
            c = cell[0]
            tried.append(c["lm"])
            success = refine(c)
            del cell[0]
            if success:
                return True
        return False

    # ---- the grids, as reproject() filled them: in filing order
    grid = [[] for _ in range(n_cells(cam, cell_size))]
    for lm in r["filing_pt"]:
        i = r["pt_lm"].index(lm)
        grid[r["pt_cell"][i]].append(dict(lm=lm, i=i))
    gridls = [[] for _ in range(n_cells(cam, seg_cell_size))]
    for lm in r["filing_seg"]:
        i = r["seg_lm"].index(lm)
        gridls[r["seg_cell"][i][0]].append(dict(lm=lm, i=i))
        gridls[r["seg_cell"][i][1]].append(dict(lm=lm, i=i))

    for k in range(len(grid)):                                        # :188-199
        cell = k if cell_order is None else int(cell_order[k])
        out["visited_cells"].append(cell)
        if refine_best_candidate(grid[cell], st["pt_type"], refine_pt, out["tried_pt"]):
            out["n_matches"] += 1
        if out["n_matches"] > max_fts:
            break
    for k in range(len(gridls)):                                      # :201-208
        cell = k if seg_cell_order is None else int(seg_cell_order[k])
        out["visited_seg_cells"].append(cell)
        if refine_best_candidate(gridls[cell], st["seg_type"], refine_seg, out["tried_seg"]):
            out["n_ls_matches"] += 1
        if out["n_ls_matches"] > max_fts_segs:
            break
    out["pt_event"], out["seg_event"] = events["pt"], events["seg"]
    return out
