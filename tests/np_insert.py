"""Restatement of what the reference does to its map when a frame becomes a keyframe, loop for loop (test infrastructure only):

  PoseOptimizer: a feature the optimiser rejects loses its landmark   src/pose_optimizer.cpp:218, :239
  FrameHandlerMono::processFrame: addFrameRef of every feature        src/frame_handler_mono.cpp:358-369; include/plsvo/feature3D.h:202-206 (push_front)
  MapPointCandidates::addCandidatePointToFrame (and segments)         src/map.cpp:292-309, :384-401
  Map::safeDeleteFrame, removePtFrameRef / removeLsFrameRef           src/map.cpp:53-114
  Map::safeDeletePoint / safeDeleteSegment                            src/map.cpp:116-139
  MapPointCandidates::removeFrameCandidates                           src/map.cpp:326-340
  Map::addKeyframe                                                    src/map.cpp:153-156

Written as the reference is: Python lists, one loop per reference loop, lists mutated as it goes.  The kernel's formulation (a decision per
landmark, prefix sums, gathers) is deliberately NOT used here.

insert() works on the stream dict of tests/np_candidates.py with the counters of np_select.quality() and MUTATES it.  Keyframes are table
indices: the new frame is index n_kf while the loops run; removing a keyframe closes the table up at the end.

Pinned where the reference leaves the result open (include/plsvo_hip.h):
  * a feature of the new frame whose landmark is TYPE_DELETED when the frame becomes a keyframe has no landmark;
  * segment candidates of the removed keyframe are deleted and erased like point candidates (the reference forgets them);
  * the observation list of a landmark deleted HERE is emptied; a landmark deleted earlier keeps its list, less the observations that sit
    in the removed keyframe (its row is gone)."""
import math

import np_candidates as N

EVENT_PROMOTED, EVENT_DELETED, EVENT_JOINED = 1, 2, 4


def bearing(px, cam):
    """[ext] vk::PinholeCamera::cam2world, normalised as Feature's constructor does"""
    x, y = (px[0] - cam[2]) / cam[0], (px[1] - cam[3]) / cam[1]
    n = math.sqrt((x * x + y * y) + 1.0)
    return [x / n, y / n, 1.0 / n]


def insert(st, feats, pt_keep, seg_keep, T, slot, remove_kf, cam):
    """feats: the selection's features in the order refine() added them (np_select.select()'s output or plsvo_cand_select_out's rows).
    Returns dict(new_kf, n_joined_pt, n_joined_seg, n_deleted_pt, n_deleted_seg, pt_event, seg_event)."""
    new = len(st["kf_T"])                                             # the new frame, not in the keyframe list yet
    events = dict(pt=[0] * len(st["pt_pos"]), seg=[0] * len(st["seg_spos"]))
    joined, deleted = dict(pt=0, seg=0), dict(pt=0, seg=0)

    # ---- 1. the new frame's feature lists
    new_fts = dict(pt=[], seg=[])
    for name, keep in (("pt", pt_keep), ("seg", seg_keep)):
        for i, lm in enumerate(feats[name + "_lm"]):
            lm = int(lm)
            if not keep[i] or st[name + "_type"][lm] == N.TYPE_DELETED:
                lm = -1
            new_fts[name].append(lm)
    lists = dict(pt=st["kf_pt"] + [new_fts["pt"]], seg=st["kf_seg"] + [new_fts["seg"]])   # every frame's features, the new one last

    # ---- 2. addFrameRef: push_front, in list order
    for i, lm in enumerate(new_fts["pt"]):
        if lm >= 0:
            px = [float(v) for v in feats["pt_px"][i]]
            st["pt_obs"][lm].insert(0, dict(kf=new, px=px, f=bearing(px, cam), level=int(feats["pt_level"][i]), type=int(feats["pt_type"][i]),
                                            grad=[float(v) for v in feats["pt_grad"][i]]))
    for i, lm in enumerate(new_fts["seg"]):
        if lm >= 0:
            px = [float(v) for v in feats["seg_px"][i]]
            st["seg_obs"][lm].insert(0, dict(kf=new, spx=px[0:2], epx=px[2:4], sf=bearing(px[0:2], cam), ef=bearing(px[2:4], cam), level=int(feats["seg_level"][i])))

    # ---- 3. addCandidatePointToFrame / addCandidateSegmentToFrame
    for name in ("pt", "seg"):
        lst = st[name + "_cand"]
        it = 0
        while it != len(lst):
            lm = lst[it]
            obs = st[name + "_obs"][lm]
            if obs and obs[0]["kf"] == new:
                st[name + "_type"][lm] = N.TYPE_UNKNOWN
                st[name + "_nfail"][lm] = 0
                lists[name][obs[-1]["kf"]].append(lm)                 # it->second->frame->addFeature(it->second)
                events[name][lm] |= EVENT_JOINED
                joined[name] += 1
                del lst[it]
            else:
                it += 1

    # ---- 4. safeDeleteFrame
    def safe_delete(name, lm):                                        # safeDeletePoint / safeDeleteSegment
        for fts in lists[name]:
            for k, v in enumerate(fts):
                if v == lm:
                    fts[k] = -1
        st[name + "_obs"][lm].clear()
        st[name + "_type"][lm] = N.TYPE_DELETED
        events[name][lm] |= EVENT_DELETED
        deleted[name] += 1

    if remove_kf >= 0:
        for name in ("pt", "seg"):
            fts = lists[name][remove_kf]
            for k in range(len(fts)):                                 # removePtFrameRef / removeLsFrameRef
                lm = fts[k]
                if lm < 0:
                    continue
                fts[k] = -1
                obs = st[name + "_obs"][lm]
                if len(obs) <= 2:
                    safe_delete(name, lm)
                    continue
                for o in range(len(obs)):                             # deleteFrameRef: the first observation in that frame
                    if obs[o]["kf"] == remove_kf:
                        del obs[o]
                        break
        for name in ("pt", "seg"):                                    # removeFrameCandidates (segments: pinned)
            lst = st[name + "_cand"]
            it = 0
            while it != len(lst):
                lm = lst[it]
                obs = st[name + "_obs"][lm]
                if obs and obs[-1]["kf"] == remove_kf:
                    st[name + "_type"][lm] = N.TYPE_DELETED
                    events[name][lm] |= EVENT_DELETED
                    deleted[name] += 1
                    obs.clear()
                    del lst[it]
                else:
                    it += 1
        for name in ("pt", "seg"):                                    # the row is gone: landmarks deleted earlier drop what they held in it
            for lm, obs in enumerate(st[name + "_obs"]):
                if st[name + "_type"][lm] == N.TYPE_DELETED:
                    obs[:] = [o for o in obs if o["kf"] != remove_kf]

    # ---- 5. addKeyframe, and the table closes up
    st["kf_T"].append([float(v) for v in T]); st["kf_slot"].append(int(slot))
    st["kf_pt"], st["kf_seg"] = lists["pt"], lists["seg"]
    if remove_kf >= 0:
        for f in ("kf_T", "kf_slot", "kf_pt", "kf_seg"):
            del st[f][remove_kf]
        for name in ("pt", "seg"):
            for obs in st[name + "_obs"]:
                for o in obs:
                    assert o["kf"] != remove_kf
                    if o["kf"] > remove_kf:
                        o["kf"] -= 1
    return dict(new_kf=len(st["kf_T"]) - 1, n_joined_pt=joined["pt"], n_joined_seg=joined["seg"], n_deleted_pt=deleted["pt"], n_deleted_seg=deleted["seg"],
                pt_event=events["pt"], seg_event=events["seg"])
