"""Restatement of what the reference does when a depth-filter seed converges, loop for loop (test infrastructure only):

  DepthFilter::updatePointSeeds / updateLineSeeds: new Point(xyz_world, ftr) / new LineSeg(..)   src/depth_filter.cpp:334-355, :439-462
  Point::Point / LineSeg::LineSeg: obs_.push_front(ftr), both reprojection counters 0            src/point.cpp:41-55, :198-212
  MapPointCandidates::newCandidatePoint / MapSegmentCandidates::newCandidateSegment              src/map.cpp:285-290, :377-382
      type_ = TYPE_CANDIDATE, candidates_.push_back                                             (bound at src/frame_handler_mono.cpp:88-95)

Written as the reference is: Python lists, one loop per reference loop.  add() works on the stream dict of tests/np_candidates.py with the
counters of np_select.quality() -- the dicts tests/np_insert.py and tests/insert_cases.py use -- and MUTATES it.

The seed's feature does not enter its keyframe's feature list here (it does when the candidate joins: np_insert step 3).  The callbacks'
depth_sigma2 arguments are unused by the reference and do not appear.  The landmark's position is an input (what plsvo_update_seeds
reports as xyz_world).  Points and segments are separate landmark spaces; within a kind input order = landmark index order =
candidate-list order.  Rows are never reclaimed: a landmark deleted later keeps its index."""
import np_candidates as N

EVENT_NEW = 8


def add(st, new):
    """new: dict(pt=[dict(pos, obs=dict(kf, px, f, level, type, grad))], seg=[dict(spos, epos, obs=dict(kf, spx, epx, sf, ef, level))]).
    Returns dict(first_pt, first_seg, n_added_pt, n_added_seg, pt_event, seg_event) -- the event bytes of ALL landmarks, 0 for the old ones."""
    first = dict(pt=-1, seg=-1)
    events = dict(pt=[0] * len(st["pt_pos"]), seg=[0] * len(st["seg_spos"]))
    for p in new.get("pt", ()):                                       # updatePointSeeds: one converged seed after the other
        lm = len(st["pt_pos"])
        st["pt_pos"].append([float(v) for v in p["pos"]])             # new Point(xyz_world, ftr)
        st["pt_obs"].append([])
        st["pt_obs"][lm].insert(0, _pt_obs(p["obs"]))                 #   obs_.push_front(ftr)
        st["pt_nfail"].append(0); st["pt_nsucc"].append(0)            #   n_failed_reproj_(0), n_succeeded_reproj_(0)
        st["pt_type"].append(N.TYPE_CANDIDATE)                        # newCandidatePoint: type_ = TYPE_CANDIDATE
        st["pt_cand"].append(lm)                                      #   candidates_.push_back
        events["pt"].append(EVENT_NEW)
        if first["pt"] < 0:
            first["pt"] = lm
    for s in new.get("seg", ()):                                      # updateLineSeeds
        lm = len(st["seg_spos"])
        st["seg_spos"].append([float(v) for v in s["spos"]]); st["seg_epos"].append([float(v) for v in s["epos"]])
        st["seg_obs"].append([])
        st["seg_obs"][lm].insert(0, _seg_obs(s["obs"]))
        st["seg_nfail"].append(0); st["seg_nsucc"].append(0)
        st["seg_type"].append(N.TYPE_CANDIDATE)
        st["seg_cand"].append(lm)
        events["seg"].append(EVENT_NEW)
        if first["seg"] < 0:
            first["seg"] = lm
    return dict(first_pt=first["pt"], first_seg=first["seg"], n_added_pt=len(new.get("pt", ())), n_added_seg=len(new.get("seg", ())),
                pt_event=events["pt"], seg_event=events["seg"])


def _pt_obs(o):
    f2 = lambda v: [float(x) for x in v]
    return dict(kf=int(o["kf"]), px=f2(o["px"]), f=f2(o["f"]), level=int(o["level"]), type=int(o["type"]), grad=f2(o["grad"]))


def _seg_obs(o):
    f2 = lambda v: [float(x) for x in v]
    return dict(kf=int(o["kf"]), spx=f2(o["spx"]), epx=f2(o["epx"]), sf=f2(o["sf"]), ef=f2(o["ef"]), level=int(o["level"]))
