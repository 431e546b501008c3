"""Restatement of the map-candidate stage in plain float64, loop for loop like the reference (test infrastructure only):

  Reprojector::reprojectMap        src/reprojector.cpp:157-183   the loop over the overlap keyframes, then the map's candidates
  Reprojector::setKfCandidates     src/reprojector.cpp:92-109    feat3D == NULL skipped, last_projected_kf_id_: a landmark once
  Reprojector::setMapCandidates    src/reprojector.cpp:111-133   no first-visit test; the failures are reported per entry
  Reprojector::reproject           src/reprojector.cpp:389-423   world2cam(T * pos), isInFrame(px.cast<int>(), 8), the cell
  Point::getCloseViewObs / LineSeg::getCloseViewObs   src/feature3D.cpp:80-125 (called first by the matcher, src/matcher.cpp:165, :239)
  cell.sort(pointQualityComparator)                   src/reprojector.cpp:219-276: a stable sort, descending type_
  [ext] Eigen's normalize() (three divisions by the norm), dot() and norm() as (x*x + y*y) + z*z

Written as the reference is: sequential loops over lists, a `last_projected` mark per landmark, a stable sort by type.  The kernel's
formulation (lowest visit index, ranks from class counts) is deliberately NOT used here, so that the two stay independent.

A stream is a dict of Python lists (see tests/candidates_cases.py):
  kf_T [n_kf][7], kf_slot [n_kf], kf_pt / kf_seg: per keyframe the list of its features' landmark indices (-1 = feat3D is NULL),
  pt_pos, pt_type, pt_obs: per point the list of its observations, each a dict(kf, px, f, level, type, grad),
  seg_spos, seg_epos, seg_type, seg_obs: each observation a dict(kf, spx, epx, sf, ef, level), pt_cand, seg_cand: landmark indices.
Two places the reference leaves open are pinned: an empty observation list gives observation -1 and has_view 0; a projection that is
NaN or beyond 1e9 is out of frame (the reference casts it to int)."""
import math

import np_keyframe as K

TYPE_DELETED, TYPE_CANDIDATE, TYPE_UNKNOWN, TYPE_GOOD = 0, 1, 2, 3


def _div(a, b):
    """IEEE division of two floats (Python raises on a zero divisor)"""
    if b != 0.0:
        return a / b
    if a != a or a == 0.0:
        return math.nan
    return math.copysign(math.inf, a) * math.copysign(1.0, b)


def reproject(T, pos, cam, cell_size, boundary=8):
    """Reprojector::reproject for one position: (px, cell), cell -1 = not in frame; plsvo_reproject's contract"""
    fx, fy, cx, cy, width, height = cam
    c = K.se3_act(T, pos)
    px = [fx * _div(c[0], c[2]) + cx, fy * _div(c[1], c[2]) + cy]
    cell = -1
    if px[0] == px[0] and px[1] == px[1] and abs(px[0]) < 1e9 and abs(px[1]) < 1e9:
        ox, oy = int(px[0]), int(px[1])                               # cast<int>: truncation
        if boundary <= ox < width - boundary and boundary <= oy < height - boundary:
            n_cols = -(-int(width) // cell_size)                      # ceil(width / cell_size), reprojector.cpp:59
            cell = int(px[1] / cell_size) * n_cols + int(px[0] / cell_size)
    return px, cell


def _normalized(v):
    n = K.norm3(v[0], v[1], v[2])
    return [_div(v[0], n), _div(v[1], n), _div(v[2], n)]


def close_view_obs(framepos, pos, obs, kf_pos):
    """getCloseViewObs: (index into obs, has_view)"""
    if not obs:
        return -1, 0
    obs_dir = _normalized([framepos[k] - pos[k] for k in range(3)])
    min_it, min_cos_angle = 0, 0.0
    for it, o in enumerate(obs):
        d = _normalized([kf_pos[o["kf"]][k] - pos[k] for k in range(3)])
        cos_angle = (obs_dir[0] * d[0] + obs_dir[1] * d[1]) + obs_dir[2] * d[2]
        if cos_angle > min_cos_angle:
            min_cos_angle, min_it = cos_angle, it
    if min_cos_angle < 0.5:
        return min_it, 0
    return min_it, 1


def candidates(st, T, overlap, cam, cell_size, seg_cell_size, boundary=8):
    """one stream, one frame: the outputs of plsvo_cand_out as lists, plus `visits` (diagnostics for the tests' input conditions)"""
    T = [float(v) for v in T]
    last_projected_pt = [False] * len(st["pt_pos"])                   # last_projected_kf_id_ == frame->id_
    last_projected_seg = [False] * len(st["seg_spos"])
    filed_pt, filed_seg = [], []                                      # what the grid's cells hold, in filing order
    kf_count = []
    visits = dict(pt=0, pt_repeat=0, seg=0, seg_repeat=0)

    def reproject_pt(lm):
        px, cell = reproject(T, st["pt_pos"][lm], cam, cell_size, boundary)
        if cell < 0:
            return False
        filed_pt.append(dict(lm=lm, px=px, cell=cell))
        return True

    def reproject_seg(lm):
        spx, scell = reproject(T, st["seg_spos"][lm], cam, seg_cell_size, boundary)
        epx, ecell = reproject(T, st["seg_epos"][lm], cam, seg_cell_size, boundary)
        if scell < 0 or ecell < 0:
            return False
        filed_seg.append(dict(lm=lm, px=spx + epx, cell=[scell, ecell]))
        return True

    for k in overlap:                                                 # reprojectMap :157-172
        counter = 0
        for lm in st["kf_pt"][k]:                                     # setKfCandidates(frame, ref_frame->pt_fts_)
            if lm < 0:
                continue
            visits["pt"] += 1
            if last_projected_pt[lm]:
                visits["pt_repeat"] += 1
                continue
            last_projected_pt[lm] = True
            if reproject_pt(lm):
                counter += 1
        for lm in st["kf_seg"][k]:                                    # setKfCandidates(frame, ref_frame->seg_fts_)
            if lm < 0:
                continue
            visits["seg"] += 1
            if last_projected_seg[lm]:
                visits["seg_repeat"] += 1
                continue
            last_projected_seg[lm] = True
            if reproject_seg(lm):
                counter += 1
        kf_count.append(counter)
    pt_cand_failed = [0 if reproject_pt(lm) else 1 for lm in st["pt_cand"]]       # setMapCandidates
    seg_cand_failed = [0 if reproject_seg(lm) else 1 for lm in st["seg_cand"]]

    framepos = K.se3_inv(T)[4:]                                       # Frame::pos()
    kf_pos = [K.se3_inv(Tk)[4:] for Tk in st["kf_T"]]
    for c in filed_pt:
        c["type"] = st["pt_type"][c["lm"]]
        c["obs"], c["has_view"] = close_view_obs(framepos, st["pt_pos"][c["lm"]], st["pt_obs"][c["lm"]], kf_pos)
    for c in filed_seg:
        c["type"] = st["seg_type"][c["lm"]]
        s, e = st["seg_spos"][c["lm"]], st["seg_epos"][c["lm"]]
        cpos = [0.5 * (s[k] + e[k]) for k in range(3)]
        c["obs"], c["has_view"] = close_view_obs(framepos, cpos, st["seg_obs"][c["lm"]], kf_pos)
    out = dict(kf_count=kf_count, pt_cand_failed=pt_cand_failed, seg_cand_failed=seg_cand_failed, visits=visits,
               filing_pt=[c["lm"] for c in filed_pt], filing_seg=[c["lm"] for c in filed_seg])
    for name, filed in (("pt", filed_pt), ("seg", filed_seg)):
        ordered = sorted(filed, key=lambda c: -c["type"])             # list::sort(qualityComparator) is stable
        for c in ordered:
            c["active"] = 1 if (c["type"] != TYPE_DELETED and c["has_view"]) else 0     # refine() :280, :341; findMatchDirect's first test
        out["n_filed_" + name] = len(ordered)
        for f in ("lm", "px", "cell", "obs", "has_view", "active", "type"):
            out[name + "_" + f] = [c[f] for c in ordered]
    return out
