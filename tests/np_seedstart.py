"""Restatement of the creating half of DepthFilter::initializeSeeds in the reference's sequential form (test infrastructure only):

  DepthFilter::initializeSeeds                                  src/depth_filter.cpp:151-191
      feature_detector_->setExistingFeatures(frame->pt_fts_)        :161   (src/feature_detection.cpp:106-113)
      feature_detector_->detect(..)                                 :162-165 (src/feature_detection.cpp:53-104: tests/np_fast.detect)
      seeds_.push_back(PointSeed(ftr, mean, min)) per new feature   :184-186 (tests/np_seedlist.keyframe)
  DepthFilter::updatePointSeeds' setGridOccpuancy(matcher_.px_cur_)  src/depth_filter.cpp:327-331 (src/feature_detection.cpp:115-121)
  PointFeat::PointFeat(frame, px, level)                        include/plsvo/feature.h: f = cam2world(px), type CORNER, grad (1, 0)

One keyframe event of one stream, in the device's order: removeKeyframe, ++batch_counter, the detector's grid, the detection on the
keyframe's pyramid, one point seed per valid cell in cell-index order, the uploaded line seeds.

Pins (where this and the device depart from the reference on purpose), beside those of tests/np_seedlist.py:
  * a position that is negative, not finite, or at or beyond the image size marks no cell (the reference's .at() would throw);
  * no room is all-or-nothing per stream: when the live point seeds plus the new ones exceed the stream's rows, nothing of either kind is
    appended and the report says so; the removal and the counter are applied either way.  The caller restages with room and repeats
    the event with removed_kf = -1, new_batch = False: the lists are then the reference's."""
import math

import np_fast as F
import np_seedlist as SL

OCC_SELECTED, OCC_UPDATED = 1, 2
MARKING = (SL.UPDATED, SL.CONVERGED, SL.NAN)             # the statuses of an update's rows whose px_cur marked a cell (:327-331 comes before :334, :356)


def _cam4(cam):
    return (cam.fx, cam.fy, cam.cx, cam.cy) if hasattr(cam, "fx") else tuple(cam[:4])


def marks(width, height, px):
    """the pin: may this position mark a cell at all"""
    x, y = float(px[0]), float(px[1])
    return math.isfinite(x) and math.isfinite(y) and 0.0 <= x < width and 0.0 <= y < height


def occupancy(width, height, cell, caller=None, selected_px=None, update_rows=None):
    """the detector's grid before detect(): bytes, one per cell.  caller: bytes OR-ed in; selected_px: the point features of the new
    frame (setExistingFeatures, :161), culled ones included; update_rows: (statuses, px_cur) of the last update's rows in list order"""
    cols, rows = F.grid(width, height, cell)
    occ = [0] * (cols * rows)
    if caller is not None:
        for k, v in enumerate(caller):
            if v:
                occ[k] = 1
    if selected_px is not None:
        for px in selected_px:                                      # std::for_each(fts.begin(), fts.end(), ..) (src/feature_detection.cpp:108-112)
            if marks(width, height, px):
                occ[F.cell_index(cols, cell, float(px[0]), float(px[1]))] = 1
    if update_rows is not None:
        for st, px in zip(*update_rows):                            # one call per seed whose epipolar search succeeded (:327-331)
            if int(st) in MARKING and marks(width, height, px):
                occ[F.cell_index(cols, cell, float(px[0]), float(px[1]))] = 1
    return occ


def bearing(cam, px):
    """cam2world(px) with the expressions of select_device.hpp's sel_bearing, in this order, uncontracted"""
    fx, fy, cx, cy = _cam4(cam)
    x, y = (px[0] - cx) / fx, (px[1] - cy) / fy
    n = math.sqrt((x * x + y * y) + 1.0)
    return [x / n, y / n, 1.0 / n]


def corner_features(corners, cam):
    """new PointFeat(frame, px, level) per record of np_fast.detect (src/feature_detection.cpp:95-101), in cell-index order"""
    out = []
    for c in corners:
        px = [float(int(c["x"])), float(int(c["y"]))]
        out.append(dict(px=px, f=bearing(cam, px), level=int(c["level"]), type=0, grad=[1.0, 0.0]))
    return out


def keyframe_detect(seeds, levels, cam, cell, lim_pt=None, removed_kf=-1, new_batch=False, new_kf=0, depth_mean=1.0, depth_min=1.0, caller=None, selected_px=None,
                    update_rows=None, new_seg=(), fast_threshold=20, detection_threshold=20.0):
    """one stream's event on its lists (mutated).  levels: the keyframe's pyramid, as many levels as the detector reads; lim_pt: the point
    rows the stream may hold (None: unlimited).  Returns the report of plsvo_seeds_keyframe_fetch"""
    SL.keyframe(seeds, removed_kf=removed_kf, new_batch=new_batch)    # these need no room
    h0, w0 = levels[0].shape
    occ = occupancy(w0, h0, cell, caller, selected_px, update_rows)
    corners = F.detect(levels, cell, fast_threshold, detection_threshold, occ)
    new_pt = corner_features(corners, cam)
    no_room = lim_pt is not None and len(seeds["pt"]) + len(new_pt) > lim_pt
    if not no_room:
        SL.keyframe(seeds, new_kf=new_kf, depth_mean=depth_mean, depth_min=depth_min, new_pt=new_pt, new_seg=new_seg)
    return dict(n_new_pt=0 if no_room else len(new_pt), n_new_seg=0 if no_room else len(new_seg), n_pt_seeds=len(seeds["pt"]), n_seg_seeds=len(seeds["seg"]),
                batch_counter=seeds["batch_counter"], no_room=int(no_room), n_occupied=sum(occ), reserved0=0)
