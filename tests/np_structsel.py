"""Restatement of FrameHandlerBase::optimizeStructure (src/frame_handler_base.cpp:192-237) on the stream dict of tests/np_candidates.py
(test infrastructure only), in the reference's sequential form:

  the deque of the frame's features that still hold a landmark (feat3D != NULL behind the pose optimiser's cull), points then segments;
  a segment that won both of its cells is a feature twice and is in the deque twice;
  std::nth_element by last_structure_optim_, PINNED where it leaves the choice open: ties go to the earlier feature (a stable order by
  (key, feature position)); with no more entries than the cap every one is taken;
  Point::optimize / LineSeg::optimize (tests/np_structopt.py) of the chosen entries one after the other on the keyframe poses and the
  landmark's observation list -- a segment chosen twice runs twice, the second time from the first's result -- and
  last_structure_optim_ = frame id behind each, also when the optimiser rolled back (:221).

The chosen entries are visited and reported in feature order (the landmarks are independent, so the order changes no result).
optimize_structure() MUTATES the stream: positions and the keys `pt_last_optim` / `seg_last_optim`, which keys() adds."""
import numpy as np

import np_structopt as O


def keys(st):
    """the stream with last_structure_optim_ = 0 for every landmark, as the reference's constructors set it"""
    st.setdefault("pt_last_optim", [0] * len(st["pt_pos"]))
    st.setdefault("seg_last_optim", [0] * len(st["seg_spos"]))
    st["pt_last_optim"] += [0] * (len(st["pt_pos"]) - len(st["pt_last_optim"]))
    st["seg_last_optim"] += [0] * (len(st["seg_spos"]) - len(st["seg_last_optim"]))
    return st


def choose(lms, last_optim, max_n):
    """positions in the deque `lms` that nth_element leaves in front, ties to the earlier entry; in deque order"""
    n = min(max_n, len(lms))
    order = sorted(range(len(lms)), key=lambda i: (last_optim[lms[i]], i))
    return sorted(order[:n])


def optimize_structure(st, feats, pt_keep, seg_keep, frame_id, max_n_pts=20, n_iter_pts=5, max_n_segs=20, n_iter_segs=5):
    """feats: the selection's features in the order refine() added them.  Returns dict(pt_lm, pt_iters, pt_pos, seg_lm, seg_iters,
    seg_spos, seg_epos): the chosen entries in feature order, each with the position(s) behind its own run."""
    keys(st)
    T = np.asarray(st["kf_T"], np.float64).reshape(-1, 7)
    out = dict(pt_lm=[], pt_iters=[], pt_pos=[], seg_lm=[], seg_iters=[], seg_spos=[], seg_epos=[])
    # Point features
    pts = [int(lm) for i, lm in enumerate(feats["pt_lm"]) if pt_keep[i]]
    for i in choose(pts, st["pt_last_optim"], max_n_pts):
        lm = pts[i]
        obs = st["pt_obs"][lm]
        pos, iters, _ = O.point_optimize(T, st["pt_pos"][lm], [o["kf"] for o in obs], [o["f"] for o in obs], n_iter_pts)
        st["pt_pos"][lm] = [float(v) for v in pos]
        st["pt_last_optim"][lm] = int(frame_id)
        out["pt_lm"].append(lm); out["pt_iters"].append(iters); out["pt_pos"].append(list(st["pt_pos"][lm]))
    # Line features
    segs = [int(lm) for i, lm in enumerate(feats["seg_lm"]) if seg_keep[i]]
    for i in choose(segs, st["seg_last_optim"], max_n_segs):
        lm = segs[i]
        obs = st["seg_obs"][lm]
        sp, ep, iters, _ = O.segment_optimize(T, st["seg_spos"][lm], st["seg_epos"][lm], [o["kf"] for o in obs], [o["sf"] for o in obs], [o["ef"] for o in obs], n_iter_segs)
        st["seg_spos"][lm] = [float(v) for v in sp]; st["seg_epos"][lm] = [float(v) for v in ep]
        st["seg_last_optim"][lm] = int(frame_id)
        out["seg_lm"].append(lm); out["seg_iters"].append(iters); out["seg_spos"].append(list(st["seg_spos"][lm])); out["seg_epos"].append(list(st["seg_epos"][lm]))
    return dict(pt_lm=np.array(out["pt_lm"], np.int32), pt_iters=np.array(out["pt_iters"], np.int32), pt_pos=np.array(out["pt_pos"], np.float64).reshape(-1, 3),
                seg_lm=np.array(out["seg_lm"], np.int32), seg_iters=np.array(out["seg_iters"], np.int32), seg_spos=np.array(out["seg_spos"], np.float64).reshape(-1, 3),
                seg_epos=np.array(out["seg_epos"], np.float64).reshape(-1, 3))


def gathered_job(st, pt_lms, seg_lms):
    """the landmarks' tables flattened into the arrays of plsvo_structopt_in (each listed landmark once, from the positions as they stand)"""
    d = dict(frame_T=np.asarray(st["kf_T"], np.float64).reshape(-1, 7), pt_pos=np.array([st["pt_pos"][i] for i in pt_lms], np.float64).reshape(-1, 3),
             seg_spos=np.array([st["seg_spos"][i] for i in seg_lms], np.float64).reshape(-1, 3), seg_epos=np.array([st["seg_epos"][i] for i in seg_lms], np.float64).reshape(-1, 3))
    for name, lms, fields in (("pt", pt_lms, (("f", "pt_obs_f"),)), ("seg", seg_lms, (("sf", "seg_obs_sf"), ("ef", "seg_obs_ef")))):
        off, fr, cols = [0], [], {dst: [] for _, dst in fields}
        for lm in lms:
            for o in st[name + "_obs"][lm]:
                fr.append(o["kf"])
                for src, dst in fields:
                    cols[dst].append(o[src])
            off.append(len(fr))
        d[name + "_obs_off"] = np.array(off, np.int32); d[name + "_obs_frame"] = np.array(fr, np.int32)
        for dst, v in cols.items():
            d[dst] = np.array(v, np.float64).reshape(-1, 3)
    return d
