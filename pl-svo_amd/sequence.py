"""The sequence harness: the one place where the resident stages are chained the way FrameHandlerMono::processFrame chains them
(src/frame_handler_mono.cpp:266-340), frame after frame on a synthetic sequence -- a textured plane carrying point and line-segment
landmarks, observed in keyframe 0, frame 0 the keyframe with the true pose (make_sequence).  Tests check the stages end to end through
it, tools/run_sequence.py runs it on the card, and it emits trajectory files in the reference harness's format.

run_sequence() checks its flags against one table (_PREREQUISITES) and hands them to a run object, _Run, whose process_frame() reads as
the step list of processFrame; each step is a method that carries the rules of the reference and the contract with the backend it
implements.  In call order:

    relocalize_frame      relocalizeFrame: closest keyframe, gating alignment, alignment from the keyframe        (relocalize)
    align                 1. sparse image alignment, previous frame -> new frame                                   plsvo_sparse_align
    track_map_*           2. reprojection of the map, 3. direct matching against the reference observations        plsvo_reproject, plsvo_match_direct
                          -- keyframe 0's; the map-candidate stage, with the cell selection; or 1-4 as one call    plsvo_candidates_*, plsvo_frame_step_batch
    pose_optimize_host    4. motion-only pose optimisation on the matches                                          plsvo_pose_optimize
    gate                  the gates of processFrame and setTrackingQuality                                         (relocalize)
    decide_keyframe*      scene depth, new-keyframe test, the frame's five key points                              plsvo_keyframe_decide
    structure_resident    5. structure optimisation on the resident tables, every frame                            plsvo_candidates_optimize_structure
    insert_keyframe       the frame joins the resident tables; image seeds; compaction (join_keyframe_host: the restaging path)
    structure_host        5. structure optimisation of the 20 least recently refined landmarks, at a keyframe       plsvo_structure_optimize   (:340)
    update_seeds          6. depth-filter update of the seeds with the new frame                                   plsvo_update_seeds         (depth_filter.cpp:262)
    image_seeds_host      7. the seeds from the image's own corners                                                (detect)
    queue_next_align      the next frame's alignment job from this frame's selection                               (align)

and the trajectory record (TUM line of T_f_w^-1, plsvo_trajectory_record) is written from the result by the caller.  What lives from
frame to frame is held by small state classes: _MapTables (the map tables the harness follows beside the device's, and the row <->
landmark maps), _SeedRows (the resident seed rows), _Keyframes (the keyframe table without keystage), _RelocState (the stage machine);
what one step hands to a later one travels in the frame's _Frame.  It is not a VO system: the map is synthetic and its truth is known.

`backend` is duck-typed: load_frames(list of level-0 images; HipBackend also takes raw frames with rectify=), sparse_align(job),
reproject(job), match_direct(job), pose_optimize(job), and per flag the methods run_sequence's table names.  The product backend is
HipBackend (C ABI on the GPU, no fallback), HipChainBackend with steps 1-4 as one resident call; tests pass an oracle-backed one to check
the whole chain end to end."""
import copy
import math
import types

import numpy as np

from . import abi, synth


class HipBackend:
    def __init__(self, ctx, n_levels=4, rectify=None):
        self.ctx, self.n_levels, self.rectify = ctx, n_levels, rectify

    def load_frames(self, images, rectify=None):
        """images: level-0 frames, already rectified -- or, with rectify = an abi.PinholeRadtan (or (camera, flip_vertical)), the raw
        frames of that camera, rectified on the device into their pyramid slots (plsvo_hip_rectify_build_pyramid).  rectify=None falls
        back to the one given to the constructor."""
        h, w = images[0].shape
        self.ctx.config_pyramids(len(images), w, h, self.n_levels)
        rectify = rectify if rectify is not None else self.rectify
        if rectify is None:
            for k, img in enumerate(images):
                self.ctx.build_pyramid(k, img, 0)
            return
        cam, flip = rectify if isinstance(rectify, tuple) else (rectify, False)
        mid = self.ctx.config_rectify(cam, flip_vertical=flip)
        for k, img in enumerate(images):
            self.ctx.rectify_build_pyramid(mid, k, img, 0)

    def sparse_align(self, job):
        return self.ctx.sparse_align(job)

    def align_ties(self):
        """Gauss-Newton iterations of the LAST alignment whose accept / roll-back decision was taken on the exact float chi2 sums (a frame
        that met none cannot have left its path on a last-bit tie)"""
        return int(self.ctx.align_chi2_ties()[1])

    def reproject(self, job):
        return self.ctx.reproject(job)

    def match_direct(self, job):
        return self.ctx.match_direct(job)

    def pose_optimize(self, job):
        return self.ctx.pose_optimize(job)

    def structure_optimize(self, job):
        return self.ctx.structure_optimize(job)

    def update_seeds(self, job):
        return self.ctx.update_seeds(job)

    def close_keyframes(self, job):
        return self.ctx.close_keyframes([job])[0]

    def keyframe_decide(self, job):
        return self.ctx.keyframe_decide([job])[0]

    def map_candidates(self, map_job, frame_job, cam, n_pyr_levels, cell_size=30, seg_cell_size=30):
        """the map-candidate stage and the resident match for one stream: map_job (abi.CandidateMapJob) = the tables to (re)stage, None =
        they have not changed since the last call.  -> (the stage's result, the matcher's) as capi.Context returns them"""
        if map_job is not None:
            self.ctx.candidates_stage([map_job], cam, cell_size, seg_cell_size, 8, n_pyr_levels, 10)
        self.ctx.candidates_run([frame_job])
        r = self.ctx.candidates_fetch()[0]
        self.ctx.candidates_match()
        return r, self.ctx.candidates_match_fetch([(r["n_filed_pt"], r["n_filed_seg"])])[0]

    def map_select(self, map_job, frame_job, cam, n_pyr_levels, select, carry=None, cell_size=30, seg_cell_size=30, close=None, key_pts=False, poses_dev=None):
        """the map part of a frame as one enqueue sequence on the resident tables: candidates, match, cell selection, pose optimisation
        (plsvo_candidates_run .. plsvo_candidates_pose_optimize).  map_job as in map_candidates; carry: the counters to put back after a
        restage (a candidates_fetch_quality() record), select: the keyword arguments of capi.Context.candidates_select.
        close = max_n_kfs: the overlap list is decided on the device from the resident key-point table (plsvo_candidates_run_close; what
        close_keyframes() reports is left in self.last_close), which a (re)stage gives its rows first: key_pts [n_kf, 5], or None for
        setKeyPoints from five NULLs on the device (False: the table is not touched).
        poses_dev: a device pointer to the frame's pose, read instead of frame_job's (plsvo_candidates_align_poses_dev).
        -> (the stage's result, the matcher's, the selection, the pose optimiser's result, the quality state after the frame)"""
        if map_job is not None:
            self.ctx.candidates_stage([map_job], cam, cell_size, seg_cell_size, 8, n_pyr_levels, 10)
            self._align_reserved = False
            if carry is not None:
                self.ctx.candidates_set_quality([dict(pt_n_failed=carry["pt_n_failed"], pt_n_succeeded=carry["pt_n_succeeded"],
                                                      seg_n_failed=carry["seg_n_failed"], seg_n_succeeded=carry["seg_n_succeeded"])])
        if map_job is not None and key_pts is not False:
            self.ctx.candidates_set_keypts(None if key_pts is None else [key_pts])
        if close is None:
            self.ctx.candidates_run([frame_job], poses_dev=poses_dev)
        else:
            self.ctx.candidates_run_close([frame_job], close, poses_dev=poses_dev)
            self.last_close = self.ctx.candidates_close_fetch()[0]
        self.ctx.candidates_match()
        self.ctx.candidates_select(**select)
        self.ctx.candidates_pose_optimize()
        r = self.ctx.candidates_fetch()[0]
        mr = self.ctx.candidates_match_fetch([(r["n_filed_pt"], r["n_filed_seg"])])[0]
        sel = self.ctx.candidates_select_fetch()[0]
        pr = self.ctx.candidates_pose_fetch([(sel["n_matches"], sel["n_ls_matches"])])[0]
        return r, mr, sel, pr, self.ctx.candidates_fetch_quality()[0]

    def align_build(self, ref_slot, cur_slot, max_level, min_level, cap_pts, cap_seg, slot_cap=2048):
        """the next frame's alignment job from the selection of the last map_select, on the device (plsvo_candidates_align_build, DESIGN.md
        3.20), with the keep masks and the optimised pose the resident pose optimiser left there; the capacities are reserved when the
        tables were staged since the last build.  Enqueue only"""
        if not getattr(self, "_align_reserved", False):
            self.ctx.candidates_align_reserve(max_level, min_level, cap_pts, cap_seg, slot_cap)
            self._align_reserved = True
        self.ctx.candidates_align_build([dict(ref_slot=ref_slot, cur_slot=cur_slot)])

    def align_built(self):
        """the built job run and its pose composed (plsvo_align_run, plsvo_candidates_align_compose).
        -> (the alignment's result, the composed T_f_w as a host copy for the records, the device pointer the next stage reads it from)"""
        self.ctx.align_run()
        self.ctx.candidates_align_compose()
        ar = self.ctx.align_fetch()[0]
        if self.ctx.candidates_align_fetch()[0]["status"] != abi.ALIGN_JOB_OK:
            raise RuntimeError("align_built: the stream did not fit the reserved alignment batch (plsvo_candidates_align_reserve)")
        return ar, self.ctx.candidates_align_fetch_job(0)["T_f_w"], self.ctx.candidates_align_poses_dev()

    def align_kf(self, ref_kf, cur_slot, T_init, max_level, min_level, cap_pts, cap_seg, slot_cap=2048, T_last=None, last_dev=None):
        """the alignment against keyframe row ref_kf of the resident tables (plsvo_candidates_align_build_kf), run and
        composed.  ref_kf None: the closest keyframe, picked on the device from T_last (or the device pointer last_dev) on the live
        key-point table; T_init None: the keyframe's own pose.
        -> (the alignment's result or None without a keyframe, the row, the composed T_f_w as a host copy, its device pointer)"""
        if not getattr(self, "_align_reserved", False):
            self.ctx.candidates_align_reserve(max_level, min_level, cap_pts, cap_seg, slot_cap)
            self._align_reserved = True
        j = dict(ref_kf=ref_kf, cur_slot=cur_slot, T_init=T_init)
        if ref_kf is None:
            j.update(last_dev=last_dev) if last_dev else j.update(T_last=T_last)
        self.ctx.candidates_align_build_kf([j])
        self.ctx.align_run()
        self.ctx.candidates_align_compose()
        ar = self.ctx.align_fetch()[0]
        rep = self.ctx.candidates_align_fetch()[0]
        if rep["status"] == abi.ALIGN_JOB_NO_KEYFRAME:
            return None, -1, None, None
        if rep["status"] != abi.ALIGN_JOB_OK:
            raise RuntimeError("align_kf: the keyframe did not fit the reserved alignment batch (plsvo_candidates_align_reserve)")
        return ar, rep["ref_kf"], self.ctx.candidates_align_fetch_job(0)["T_f_w"], self.ctx.candidates_align_poses_dev()

    def track_gate(self, **job):
        """the gates of processFrame behind the last map_select, on the device (plsvo_candidates_track_gate).
        -> (the 32-byte record, the pose carried forward as a host copy, its device pointer)"""
        self.ctx.candidates_track_gate([job])
        recs, T = self.ctx.candidates_gate_fetch(poses=True)
        return recs[0], T[0].copy(), self.ctx.candidates_gate_poses_dev()

    def map_fetch(self):
        """the resident tables as they stand (plsvo_candidates_fetch_map)"""
        return self.ctx.candidates_fetch_map()[0]

    def map_set_keypts(self, key_pts=None):
        """Frame::key_pts_ of the staged keyframes as a resident table (plsvo_candidates_set_keypts): [n_kf, 5] positions in
        the keyframes' point-feature lists, or None: setKeyPoints from five NULLs on the device.  Live until the next stage; the selection
        and the insertion keep it up.  -> the table as it stands"""
        self.ctx.candidates_set_keypts(None if key_pts is None else [key_pts])
        return self.map_fetch_keypts()

    def map_fetch_keypts(self):
        return self.ctx.candidates_fetch_keypts()[0]

    def map_candidates_close(self, frame_job, max_n_kfs=10):
        """plsvo_candidates_run_close on the staged tables: getCloseKeyframes from the live key-point table and the landmarks' positions as
        they lie now, sorted and cut, feeding the candidate launch in the same enqueue (frame_job: no overlap list).
        -> (what close_keyframes() reports, the candidate stage's result)"""
        self.ctx.candidates_run_close([frame_job], max_n_kfs)
        return self.ctx.candidates_close_fetch()[0], self.ctx.candidates_fetch()[0]

    def map_keyframe_decide(self, T_last_w, kfselect_mindist_t=0.06, kfselect_mindist_r=3.0):
        """the keyframe decision behind the last map_select, on the resident selection (plsvo_candidates_keyframe_decide): nothing but
        T_last_w travels, one record comes back.  -> what keyframe_decide() reports, key_pts in selection order"""
        self.ctx.candidates_keyframe_decide([dict(T_last_w=T_last_w, kfselect_mindist_t=kfselect_mindist_t, kfselect_mindist_r=kfselect_mindist_r)])
        return self.ctx.candidates_decide_fetch()[0]

    def map_reserve(self, **room):
        """room per stream for the insertions to come (plsvo_candidates_reserve; no arguments: the tight layout again)"""
        self.ctx.candidates_reserve(**room)

    def map_insert(self, remove_kf, kf_slot):
        """the frame of the last map_select becomes a keyframe of the resident tables (plsvo_candidates_insert_keyframe), with the pose and
        the keep masks the resident pose optimiser left on the device; remove_kf: -1 or the row Map::safeDeleteFrame takes out.
        -> (the tables as they now stand: capi.Context.candidates_fetch_map's record, the quality state, what the insertion did)"""
        self.ctx.candidates_insert_keyframe([dict(remove_kf=remove_kf, kf_slot=kf_slot)])
        return self.ctx.candidates_fetch_map()[0], self.ctx.candidates_fetch_quality()[0], self.ctx.candidates_insert_fetch()[0]

    def map_set_positions(self, pt_idx, pt_pos):
        """moved point landmarks into the resident tables (plsvo_candidates_set_positions)"""
        self.ctx.candidates_set_positions([dict(pt_idx=pt_idx, pt_pos=pt_pos)])

    def map_optimize_structure(self, frame_id, **params):
        """FrameHandlerBase::optimizeStructure on the resident tables (plsvo_candidates_optimize_structure) behind the last
        map_select, with the keep masks the resident pose optimiser left on the device; params: max_n_pts, n_iter_pts, max_n_segs,
        n_iter_segs (20 / 5 / 20 / 5).  -> what was refined: capi.Context.candidates_structure_fetch's record"""
        self.ctx.candidates_optimize_structure([dict(frame_id=frame_id)], **params)
        return self.ctx.candidates_structure_fetch()[0]

    def map_set_last_optim(self, pt_last_optim, seg_last_optim):
        """the landmarks' last_structure_optim_ carried over a restage (plsvo_candidates_set_last_optim)"""
        self.ctx.candidates_set_last_optim([dict(pt_last_optim=pt_last_optim, seg_last_optim=seg_last_optim)])

    def map_reserve_landmarks(self, **room):
        """landmark rows per stream for the candidates to come (plsvo_candidates_reserve_landmarks; no arguments: today's layout again)"""
        self.ctx.candidates_reserve_landmarks(**room)

    def map_add_candidates(self, new):
        """converged seeds become candidate landmarks of the resident tables (plsvo_candidates_add); new: the arrays of plsvo_cand_new as
        capi.Context.candidates_add takes them.  -> (what the add did: capi.Context.candidates_add_fetch's record, the quality state)"""
        self.ctx.candidates_add([new])
        return self.ctx.candidates_add_fetch()[0], self.ctx.candidates_fetch_quality()[0]

    def map_compact(self, mode="always", min_room_pt=0, min_room_seg=0):
        """the resident tables close up over their deleted landmark rows (plsvo_candidates_compact); mode: "always", or
        "room" -- a kind only where fewer than min_room rows of it are free.  -> (the tables as they now stand, the quality state, what the
        compaction did with pt_remap / seg_remap over the old rows: capi.Context.candidates_compact_fetch's record)"""
        self.ctx.candidates_compact([(mode, min_room_pt, min_room_seg)])
        return self.ctx.candidates_fetch_map()[0], self.ctx.candidates_fetch_quality()[0], self.ctx.candidates_compact_fetch()[0]

    def seeds_stage(self, lists, cam, room=None, **params):
        """the stream's seed lists become a resident table beside the staged map tables (plsvo_seeds_stage); lists: the
        arrays of plsvo_seed_list and batch_counter as capi.Context.seeds_stage takes them; room: extra_pt / extra_seg rows for the seeds
        later keyframes start; params: max_n_kfs and the matcher's options"""
        self.ctx.seeds_reserve(**(room or {}))
        self.ctx.seeds_stage([lists], cam, **params)

    def seeds_update(self, cur_slot, T_f_w=None):
        """the resident seeds updated with the frame in cur_slot, aged, erased and handed over to the resident map tables on the device
        (plsvo_seeds_update .. _update_fetch); T_f_w None: the optimised pose the resident pose optimiser left on the device.
        -> (the report: capi.Context.seeds_update_fetch's record, the update's rows: capi.Context.seeds_fetch_rows', the quality state)"""
        self.ctx.seeds_update([dict(cur_slot=cur_slot, T_f_w=T_f_w)])
        return self.ctx.seeds_update_fetch()[0], self.ctx.seeds_fetch_rows()[0], self.ctx.candidates_fetch_quality()[0]

    def seeds_keyframe(self, **event):
        """a keyframe event on the resident seed lists (plsvo_seeds_keyframe): removed_kf, new_batch, new_kf, depth_mean, depth_min and the
        new seeds' arrays"""
        self.ctx.seeds_keyframe([event])

    def seeds_keyframe_detect(self, cell_size=25, n_levels=3, detection_threshold=20.0, fast_threshold=20, **event):
        """a keyframe event whose point seeds start on the device from the corners of the keyframe's own pyramid slot
        (plsvo_seeds_keyframe_detect): removed_kf, new_batch, new_kf, depth_mean, depth_min, occ_sources (default: the
        last selection's features and the last update's matches), d_occupancy and the line seeds' arrays.  Enqueue only.
        -> nothing; seeds_keyframe_fetch() has the report"""
        self.ctx.seeds_keyframe_detect([event], cell_size, n_levels, fast_threshold, detection_threshold)

    def seeds_keyframe_fetch(self):
        """what the last seeds_keyframe_detect did (plsvo_seeds_keyframe_fetch): capi.Context.seeds_keyframe_fetch's record"""
        return self.ctx.seeds_keyframe_fetch()[0]

    def seeds_fetch_lists(self):
        """the resident seed lists as they stand (plsvo_seeds_fetch_lists)"""
        return self.ctx.seeds_fetch_lists()[0]

    def detect_corners(self, slot, occupancy=None, cell_size=25, n_levels=3, detection_threshold=20.0, fast_threshold=20):
        """FastDetector::detect on the frame in `slot` (plsvo_hip_detect_fast): abi.CORNER_DTYPE records in cell order"""
        return self.ctx.detect_fast(slot, 1, cell_size, n_levels, fast_threshold, detection_threshold, None if occupancy is None else occupancy[None])[0]

    # ---- bootstrap: KLT track of the first keyframe's corners (plsvo_klt_*; one stream) ----
    def klt_first_frame(self, slot, cam, px, extra_px=None, extra_f=None, cap_pts=None, max_level=4):
        """addFirstFrame on the frame in `slot`: the lists from a host list of pixels (and extra points with their bearings)"""
        n = len(px) + (0 if extra_px is None else len(extra_px))
        self.ctx.klt_reserve(1, max(int(cap_pts or n), 1), max_level=max_level)
        fx, fy, cx, cy, w, h = cam
        self.ctx.klt_first_frame([dict(slot=slot, cam=abi.Pinhole(fx, fy, cx, cy, int(w), int(h)), px=px, extra_px=extra_px, extra_f=extra_f)])
        return self.ctx.klt_fetch()[0]

    def klt_second_frame(self, slot, init_min_tracked=40, init_min_disparity=40.0):
        """addSecondFrame up to the disparity gate on the frame in `slot`: the report"""
        self.ctx.klt_second_frame([slot], init_min_tracked, init_min_disparity)
        return self.ctx.klt_fetch()[0]

    def klt_tracks(self):
        return self.ctx.klt_fetch_tracks(0)


class HipChainBackend(HipBackend):
    """The same product backend with steps 1-4 of a frame -- alignment, reprojection, matching, pose optimisation -- as ONE resident
    call (plsvo_frame_step_batch): poses, candidates, matches and keep masks stay in HBM between the kernels."""

    def frame_step(self, job, T_prev, kf_T, kf_slot, n_pt, n_seg, pos_all, ref_px, ref_f, active, cam, n_pyr_levels, reproj_thresh):
        cj = abi.ChainJob(job, T_prev, kf_T, kf_slot, n_pt, n_seg, pos_all, ref_px, ref_f, active=active)
        return self.ctx.frame_step_batch([cj], cam, n_pyr_levels=n_pyr_levels, reproj_thresh=reproj_thresh)[0]


def make_sequence(seed, n_frames=6, W=320, H=240, n_pts=120, n_seg=30, step_scale=0.5, total=None):
    """Camera moving smoothly over the textured plane of synth.make_align_stream.  Returns a dict with the level-0
    images, the camera, the true poses T_f_w of every frame and the map: landmark positions with their keyframe-0
    observations.  Per-frame motion is step_scale x (3 % of the scene depth, 0.01 rad) in a random direction, or -- with
    `total` -- whatever divides a whole-sequence motion of total x (scene depth, 0.25 rad) into n_frames - 1 equal steps
    (long sequences must keep the keyframe's landmarks in view)."""
    st = synth.make_align_stream(seed, W, H, n_pts, n_seg, 3, motion_scale=step_scale)
    rng = np.random.default_rng(seed + 300000)
    d0 = st.plane_d / st.plane_n[2]
    xi = np.concatenate([rng.uniform(-0.03, 0.03, 3) * d0, rng.uniform(-0.01, 0.01, 3)]) * step_scale
    if total is not None:
        dirs = rng.uniform(-1.0, 1.0, 6)
        xi = np.concatenate([dirs[:3] / np.linalg.norm(dirs[:3]) * total * d0, dirs[3:] / np.linalg.norm(dirs[3:]) * total * 0.25]) / max(n_frames - 1, 1)
    subs, T_rel = [], []
    for k in range(1, n_frames):
        s = copy.copy(st)
        s.T_true = synth.se3_exp(k * xi)        # frame k from frame 0
        subs.append(s)
        T_rel.append(s.T_true)
    imgs = synth.render_streams([st] + subs).numpy()
    images = [imgs[0, 0]] + [imgs[k, 1] for k in range(1, n_frames)]
    poses = [st.T_ref_w] + [synth.se3_mul(T, st.T_ref_w) for T in T_rel]
    return dict(images=images, cam=st.cam, poses_true=np.stack(poses), stream=st,
                pt_pos=st.pt_pos_w, pt_px0=st.pt_px, pt_f0=st.pt_f,
                seg_spos=st.seg_spos_w, seg_epos=st.seg_epos_w, seg_spx0=st.seg_spx, seg_epx0=st.seg_epx, seg_sf0=st.seg_sf, seg_ef0=st.seg_ef)


def klt_bootstrap(backend, images, cam, init_min_tracked=40, init_min_disparity=40.0, detect=None, extra_px=None, extra_f=None, cap_pts=None, max_level=4):
    """KltHomographyInit up to computeHomography (src/initialization.cpp:40-69): the first image's corners (FastDetector::detect on its
    pyramid slot, `detect` = keyword arguments of backend.detect_corners) and the caller's extra points become the lists, then every
    following image is a second frame until the result is TRACKED (ready for the homography) or FAILURE.  Returns (reports, tracks):
    one report per frame played -- abi.KltReport's fields -- and the final lists (px_ref, px_cur, f_ref, f_cur, disparity).
    backend: load_frames, detect_corners, klt_first_frame, klt_second_frame, klt_tracks."""
    backend.load_frames(images)
    corners = backend.detect_corners(0, **(detect or {}))
    px = np.stack([corners["x"], corners["y"]], axis=1).astype(np.float32)
    reports = [backend.klt_first_frame(0, cam, px, extra_px, extra_f, cap_pts, max_level)]
    if reports[0]["result"] == abi.KLT_FIRST:
        for k in range(1, len(images)):
            reports.append(backend.klt_second_frame(k, init_min_tracked, init_min_disparity))
            if reports[-1]["result"] in (abi.KLT_TRACKED, abi.KLT_FAILURE):
                break
    return reports, backend.klt_tracks()


def _bearing(cam, px):
    fx, fy, cx, cy = cam[:4]
    r = np.stack([(px[:, 0] - cx) / fx, (px[:, 1] - cy) / fy, np.ones(len(px))], axis=1)
    return r / np.linalg.norm(r, axis=1, keepdims=True)


def _q_rot(q, v):
    """Eigen::Quaternion::_transformVector on Python floats, in the device's operation order (plsvo_math.hpp::quat_rotate)"""
    qx, qy, qz, qw = q
    ux, uy, uz = qy * v[2] - qz * v[1], qz * v[0] - qx * v[2], qx * v[1] - qy * v[0]
    ux += ux; uy += uy; uz += uz
    return [v[0] + qw * ux + (qy * uz - qz * uy), v[1] + qw * uy + (qz * ux - qx * uz), v[2] + qw * uz + (qx * uy - qy * ux)]


def _se3_inv_s(T):
    T = [float(v) for v in T]
    qc = [-T[0], -T[1], -T[2], T[3]]
    return qc + _q_rot(qc, [-T[4], -T[5], -T[6]])


def _se3_mul_s(A, B):
    """Sophus::SE3::operator* on Python floats (plsvo_math.hpp::se3_mul): what the device's compose kernel computes, bit for bit"""
    A, B = [float(v) for v in A], [float(v) for v in B]
    ax, ay, az, aw = A[:4]
    bx, by, bz, bw = B[:4]
    w = aw * bw - ax * bx - ay * by - az * bz
    x = aw * bx + ax * bw + ay * bz - az * by
    y = aw * by + ay * bw + az * bx - ax * bz
    z = aw * bz + az * bw + ax * by - ay * bx
    n = math.sqrt(x * x + y * y + z * z + w * w)
    rt = _q_rot(A[:4], B[4:])
    return [x / n, y / n, z / n, w / n, A[4] + rt[0], A[5] + rt[1], A[6] + rt[2]]


def align_job_host(cam, max_level, min_level, sel, pt_keep, seg_keep, pt_type, seg_type, pt_pos, seg_spos, seg_epos, T_ref, ref_slot, cur_slot):
    """The alignment job plsvo_candidates_align_build writes on the device, restated on the host in scalar float64 with the device's
    operation order (the slot layout is plsvo_align_stage's): the selection's point features whose keep byte is set and
    whose landmark row is not TYPE_DELETED, closed up; ALL its segment features, those without a landmark flagged and zeroed;
    f * ||pos - ref_pos|| with the three squares added in order; T0 = T_ref * T_ref^-1.  -> abi.AlignJob"""
    T_ref = [float(v) for v in T_ref]
    T_inv = _se3_inv_s(T_ref)
    ref = T_inv[4:]

    def scaled(px, pos):
        x, y = (px[0] - cam[2]) / cam[0], (px[1] - cam[3]) / cam[1]
        n = math.sqrt((x * x + y * y) + 1.0)
        dx, dy, dz = pos[0] - ref[0], pos[1] - ref[1], pos[2] - ref[2]
        d = math.sqrt(dx * dx + dy * dy + dz * dz)
        return [x / n * d, y / n * d, 1.0 / n * d]
    px, xyz = [], []
    for i, lm in enumerate(sel["pt_lm"]):
        if pt_keep[i] and pt_type[int(lm)] != abi.LM_DELETED:
            p = [float(v) for v in sel["pt_px"][i]]
            px.append(p); xyz.append(scaled(p, [float(v) for v in pt_pos[int(lm)]]))
    spx, epx, length, p_ref, q_ref, alive = [], [], [], [], [], []
    for i, lm in enumerate(sel["seg_lm"]):
        s4 = [float(v) for v in sel["seg_px"][i]]
        a = bool(seg_keep[i]) and seg_type[int(lm)] != abi.LM_DELETED
        dx, dy = s4[2] - s4[0], s4[3] - s4[1]
        spx.append(s4[:2]); epx.append(s4[2:]); length.append(math.sqrt(dx * dx + dy * dy)); alive.append(int(a))
        p_ref.append(scaled(s4[:2], [float(v) for v in seg_spos[int(lm)]]) if a else [0.0] * 3)
        q_ref.append(scaled(s4[2:], [float(v) for v in seg_epos[int(lm)]]) if a else [0.0] * 3)
    arr = lambda v, cols: np.array(v, float).reshape(-1, cols)
    return abi.AlignJob(cam, max_level, min_level, 30, 1e-6, _se3_mul_s(T_ref, T_inv), arr(px, 2), arr(xyz, 3), arr(spx, 2), arr(epx, 2), np.array(length, float),
                        arr(p_ref, 3), arr(q_ref, 3), np.array(alive, np.uint8), ref_slot=ref_slot, cur_slot=cur_slot)


def align_kf_job_host(cam, max_level, min_level, t, ref_kf, T_init, cur_slot):
    """The alignment job plsvo_candidates_align_build_kf writes on the device from keyframe row ref_kf, assembled on the host from one
    stream's fetched tables (capi.Context.candidates_fetch_map) in scalar float64 with the device's operation order (the
    slot layout is plsvo_align_stage's): the keyframe's point features that hold a landmark which is not TYPE_DELETED and has an
    observation in this keyframe -- the first one: its px and its STORED bearing -- closed up; ALL its segment features, a dead one
    zeroed; T0 = T_init * T_kf^-1 (T_init None: the keyframe's own pose).  The path the device build replaces.  -> abi.AlignJob"""
    T_ref = [float(v) for v in np.asarray(t["kf_T"], float).reshape(-1, 7)[ref_kf]]
    T_inv = _se3_inv_s(T_ref)
    ref = T_inv[4:]

    def first_obs(kind, lm, types):
        if lm < 0 or int(types[lm]) == abi.LM_DELETED:
            return -1
        off, kf = t[kind + "_obs_off"], t[kind + "_obs_kf"]
        return next((o for o in range(int(off[lm]), int(off[lm + 1])) if int(kf[o]) == ref_kf), -1)

    def scaled(f, pos):
        dx, dy, dz = float(pos[0]) - ref[0], float(pos[1]) - ref[1], float(pos[2]) - ref[2]
        d = math.sqrt(dx * dx + dy * dy + dz * dz)
        return [float(f[0]) * d, float(f[1]) * d, float(f[2]) * d]
    rows = lambda f, w: np.asarray(t[f], float).reshape(-1, w)
    pt_pos, obs_px, obs_f = rows("pt_pos", 3), rows("pt_obs_px", 2), rows("pt_obs_f", 3)
    px, xyz = [], []
    for i in range(int(t["kf_pt_off"][ref_kf]), int(t["kf_pt_off"][ref_kf + 1])):
        lm = int(t["kf_pt_lm"][i])
        o = first_obs("pt", lm, t["pt_type"])
        if o >= 0:
            px.append([float(v) for v in obs_px[o]]); xyz.append(scaled(obs_f[o], pt_pos[lm]))
    s_spx, s_epx, s_sf, s_ef, spos, epos = rows("seg_obs_spx", 2), rows("seg_obs_epx", 2), rows("seg_obs_sf", 3), rows("seg_obs_ef", 3), rows("seg_spos", 3), rows("seg_epos", 3)
    spx, epx, length, p_ref, q_ref, alive = [], [], [], [], [], []
    for i in range(int(t["kf_seg_off"][ref_kf]), int(t["kf_seg_off"][ref_kf + 1])):
        lm = int(t["kf_seg_lm"][i])
        o = first_obs("seg", lm, t["seg_type"])
        alive.append(int(o >= 0))
        if o < 0:                                      # no pixels in the tables for a feature without a landmark: zeros
            spx.append([0.0] * 2); epx.append([0.0] * 2); length.append(0.0); p_ref.append([0.0] * 3); q_ref.append([0.0] * 3)
            continue
        a, b = [float(v) for v in s_spx[o]], [float(v) for v in s_epx[o]]
        dx, dy = b[0] - a[0], b[1] - a[1]
        spx.append(a); epx.append(b); length.append(math.sqrt(dx * dx + dy * dy))
        p_ref.append(scaled(s_sf[o], spos[lm])); q_ref.append(scaled(s_ef[o], epos[lm]))
    arr = lambda v, cols: np.array(v, float).reshape(-1, cols)
    return abi.AlignJob(cam, max_level, min_level, 30, 1e-6, _se3_mul_s(T_ref if T_init is None else T_init, T_inv), arr(px, 2), arr(xyz, 3), arr(spx, 2), arr(epx, 2),
                        np.array(length, float), arr(p_ref, 3), arr(q_ref, 3), np.array(alive, np.uint8), ref_slot=int(t["kf_slot"][ref_kf]), cur_slot=cur_slot)


def track_gate_host(n_matches, n_ls_matches, num_obs_pt, num_obs_ls, num_obs_last_pt, num_obs_last_ls, relocalizing=False, quality_min_fts=20, quality_max_drop_fts=50,
                    max_fts=100, max_fts_segs=100):
    """The comparisons plsvo_candidates_track_gate makes on the device, on fetched counts (the selection's n_matches / n_ls_matches, the
    pose optimisation's num_obs): src/frame_handler_mono.cpp:315-321, :335, FrameHandlerBase::setTrackingQuality.  -> (result
    abi.GATE_*, tracking quality abi.TRACKING_*, whether the frame's pose is reset to the last one)"""
    if n_matches + n_ls_matches < quality_min_fts:
        return abi.GATE_FAIL_MATCHES, abi.TRACKING_INSUFFICIENT, True
    if num_obs_pt + num_obs_ls < 10:
        return abi.GATE_FAIL_EDGES, abi.TRACKING_INSUFFICIENT, bool(relocalizing)
    bad = num_obs_pt + num_obs_ls < quality_min_fts or min(num_obs_last_pt, max_fts) - num_obs_pt > quality_max_drop_fts
    return abi.GATE_OK, abi.TRACKING_BAD if bad else abi.TRACKING_GOOD, False


def seeds_from_corners(corners, cam, depth_mean, depth_min):
    """Point seeds for detected corners (abi.CORNER_DTYPE records), as DepthFilter::initializeSeeds creates them
    (src/depth_filter.cpp:161-172): a feature `new PointFeat(frame, px, level)` -- f = cam2world(px), type CORNER, grad (1, 0) -- in a
    PointSeed(ftr, depth_mean, depth_min) (src/depth_filter.cpp:53-61: float arguments, a = b = 10, mu = 1.0 / depth_mean,
    z_range = 1.0 / depth_min, sigma2 = z_range * z_range / 36, all stored as float).  -> the point half of plsvo_seeds_in without the
    frame indices: a dict for abi.SeedsJob's `pt` once `ref_frame` / `cur_frame` are added."""
    f32 = np.float32
    n = len(corners)
    px = np.stack([corners["x"].astype(np.float64), corners["y"].astype(np.float64)], axis=1) if n else np.zeros((0, 2))
    z_range = f32(1.0 / float(f32(depth_min)))
    return dict(px=px, f=_bearing(cam, px) if n else np.zeros((0, 3)), level=corners["level"].astype(np.int32), type=np.zeros(n, np.uint8),
                grad=np.tile(np.array([1.0, 0.0]), (n, 1)), a=np.full(n, 10, f32), b=np.full(n, 10, f32),
                mu=np.full(n, f32(1.0 / float(f32(depth_mean))), f32), z_range=np.full(n, z_range, f32),
                sigma2=np.full(n, f32(z_range * z_range) / f32(36), f32))


def _occupancy(px, w, h, cell):
    """FastDetector::setExistingFeatures: the grid cells of the features a frame already has"""
    cols, rows = -(-w // cell), -(-h // cell)
    occ = np.zeros(cols * rows, np.uint8)
    inside = (px[:, 0] >= 0) & (px[:, 0] < w) & (px[:, 1] >= 0) & (px[:, 1] < h)
    occ[(px[inside, 1] / cell).astype(np.int64) * cols + (px[inside, 0] / cell).astype(np.int64)] = 1
    return occ


def candidate_map_job(cm):
    """the harness's map tables (lists, as tests/np_candidates.py reads them) flattened into the CSR arrays of plsvo_cand_map"""
    def csr(lists):
        off = np.zeros(len(lists) + 1, np.int32)
        off[1:] = np.cumsum([len(l) for l in lists])
        return off
    po = [o for l in cm["pt_obs"] for o in l]
    so = [o for l in cm["seg_obs"] for o in l]
    col = lambda obs, f: [o[f] for o in obs]
    return abi.CandidateMapJob(
        kf_T=cm["kf_T"], kf_slot=cm["kf_slot"], kf_pt_off=csr(cm["kf_pt"]), kf_pt_lm=[v for l in cm["kf_pt"] for v in l],
        kf_seg_off=csr(cm["kf_seg"]), kf_seg_lm=[v for l in cm["kf_seg"] for v in l],
        pt_pos=cm["pt_pos"], pt_type=cm["pt_type"], pt_obs_off=csr(cm["pt_obs"]), pt_obs_kf=col(po, "kf"), pt_obs_px=col(po, "px"), pt_obs_f=col(po, "f"),
        pt_obs_level=col(po, "level"), pt_obs_type=col(po, "type"), pt_obs_grad=col(po, "grad"),
        seg_spos=cm["seg_spos"], seg_epos=cm["seg_epos"], seg_type=cm["seg_type"], seg_obs_off=csr(cm["seg_obs"]), seg_obs_kf=col(so, "kf"),
        seg_obs_spx=col(so, "spx"), seg_obs_epx=col(so, "epx"), seg_obs_sf=col(so, "sf"), seg_obs_ef=col(so, "ef"), seg_obs_level=col(so, "level"),
        pt_cand=cm["pt_cand"], seg_cand=cm["seg_cand"])


def candidate_map_tables(t):
    """the inverse of candidate_map_job: the CSR arrays of plsvo_cand_map (capi.Context.candidates_fetch_map's record) as the harness's
    lists"""
    f3 = lambda a: [[float(x) for x in v] for v in a]
    cut = lambda v, off: [[int(x) for x in v[off[k]:off[k + 1]]] for k in range(len(off) - 1)]
    po, so = t["pt_obs_off"], t["seg_obs_off"]
    pt_obs = [[dict(kf=int(t["pt_obs_kf"][o]), px=[float(x) for x in t["pt_obs_px"][o]], f=[float(x) for x in t["pt_obs_f"][o]], level=int(t["pt_obs_level"][o]),
                    type=int(t["pt_obs_type"][o]), grad=[float(x) for x in t["pt_obs_grad"][o]]) for o in range(po[k], po[k + 1])] for k in range(len(po) - 1)]
    seg_obs = [[dict(kf=int(t["seg_obs_kf"][o]), spx=[float(x) for x in t["seg_obs_spx"][o]], epx=[float(x) for x in t["seg_obs_epx"][o]],
                     sf=[float(x) for x in t["seg_obs_sf"][o]], ef=[float(x) for x in t["seg_obs_ef"][o]], level=int(t["seg_obs_level"][o])) for o in range(so[k], so[k + 1])]
               for k in range(len(so) - 1)]
    return dict(kf_T=f3(t["kf_T"]), kf_slot=[int(v) for v in t["kf_slot"]], kf_pt=cut(t["kf_pt_lm"], t["kf_pt_off"]), kf_seg=cut(t["kf_seg_lm"], t["kf_seg_off"]),
                pt_pos=f3(t["pt_pos"]), pt_type=[int(v) for v in t["pt_type"]], pt_obs=pt_obs, seg_spos=f3(t["seg_spos"]), seg_epos=f3(t["seg_epos"]),
                seg_type=[int(v) for v in t["seg_type"]], seg_obs=seg_obs, pt_cand=[int(v) for v in t["pt_cand"]], seg_cand=[int(v) for v in t["seg_cand"]])


def _set_key_points(cam, px, alive, prev):
    """Frame::setKeyPoints / checkKeyPoints (src/frame.cpp:87-141) on indices, -1 = NULL: holders without a landmark are dropped, then every
    feature that holds one challenges the five slots in list order (slots 3 and 4 compare x with cv, as written there)"""
    key = [int(h) if h >= 0 and alive[h] else -1 for h in prev]
    cu, cv = int(cam[4]) // 2, int(cam[5]) // 2
    prod = lambda i: (float(px[i][0]) - cu) * (float(px[i][1]) - cv)
    centre = lambda i: max(abs(float(px[i][0]) - cu), abs(float(px[i][1]) - cv))
    for f in range(len(px)):
        if not alive[f]:
            continue
        x, y = float(px[f][0]), float(px[f][1])
        if key[0] < 0 or centre(f) < centre(key[0]):
            key[0] = f
        for s, ok in enumerate((x >= cu and y >= cv, x >= cu and y < cv, x < cv and y < cv, x < cv and y >= cv)):
            if ok and (key[s + 1] < 0 or prod(f) > prod(key[s + 1])):
                key[s + 1] = f
    return key


def _key_point_upkeep(cm, tab, cam, fresh=()):
    """the key-point table on the tables as they now stand: a keyframe one of whose holders has lost its landmark (and every row of `fresh`,
    from five NULLs) runs setKeyPoints over its features; a feature's px is its landmark's observation in that keyframe.
    -> (the table, the rows rebuilt)"""
    out, rebuilt = [], 0
    for k, (fts, row) in enumerate(zip(cm["kf_pt"], tab)):
        row = [-1] * 5 if k in fresh else [int(h) if h < len(fts) else -1 for h in row]
        if k in fresh or any(h >= 0 and fts[h] < 0 for h in row):
            px, alive = [], []
            for lm in fts:
                o = next((o for o in cm["pt_obs"][lm] if o["kf"] == k), None) if lm >= 0 else None
                px.append(o["px"] if o else (0.0, 0.0)); alive.append(o is not None)
            row = _set_key_points(cam, px, alive, row)
            rebuilt += k not in fresh
        out.append(row)
    return out, rebuilt


def run_sequence(backend, seq, max_level=3, min_level=1, n_pyr_levels=3, reproj_thresh=2.0, mapping=False, known_frac=0.6,
                 pos_noise=0.005, map_seed=0, kf_every=5, detect=False, detect_cell_size=25, kf_select=False, kfselect_mindist_t=0.06,
                 kfselect_mindist_r=3.0, max_n_kfs=10, map_candidates=False, record_candidates=False, cell_select=False, select_params=None, kf_insert=False,
                 seed_candidates=False, seeds_resident=False, image_seeds=None, image_seed_params=None, structopt_resident=False, compact=None, lm_room=None, keystage=None, align=None,
                 relocalize=None, reloc_params=None):
    """-> list of per-frame dicts (pose T_f_w, cov, counts).  Frame 0 is the keyframe with the true pose.  One line per flag; what a flag
    does, and its contract with the backend, is written at the step of _Run named in the last column.  With a flag off (False / None)
    every record is what it is without it.

    flag                values              needs: flags; backend method                                   the records gain                                          step
    mapping             bool                structure_optimize, update_seeds                               n_seed_converged, n_known, n_seeds, landmark_err          _Run.init_mapping
    detect              bool                mapping; detect_corners (ignored without)                      n_image_seeds, n_image_seeds_converged                    image_seeds_host
    kf_select           bool                mapping; close_keyframes, keyframe_decide (ignored without)    is_kf, n_overlap, depth_mean                              decide_keyframe_host
    map_candidates      bool                map_candidates, no frame_step                                  n_filed_pt, n_filed_seg, ref_kf_hist                      track_map_candidates
    record_candidates   bool                map_candidates                                                 candidates; insert, add, structopt (tests)                the steps that record
    cell_select         bool                map_candidates; map_select                                     n_trials, n_promoted, n_deleted                           select_cells
    kf_insert           bool                mapping, cell_select; map_insert, map_reserve                  n_joined, n_deleted_kf, remove_kf, n_seed_candidates      insert_keyframe
    seed_candidates     bool                kf_insert; map_add_candidates, map_reserve_landmarks           (rec["add"])                                              converged_seeds_join
    seeds_resident      bool                seed_candidates; seeds_stage                                   --                                                        stage_seeds
    image_seeds         "host" | "device"   seeds_resident; detect_corners | seeds_keyframe_detect         n_image_seeds, _converged, _started                       start_image_seeds
    structopt_resident  bool                mapping, cell_select; map_optimize_structure                   n_structopt_pt, n_structopt_seg                           structure_resident
    compact             "room" | "always"   seed_candidates; map_compact                                   n_compacted_pt                                            compact_tables
    keystage            "host" | "device"   kf_select, cell_select, kf_insert; keyframe_decide |           is_kf, n_overlap, depth_mean, overlap, key_pts_new,       decide_keyframe
                                            map_keyframe_decide                                            n_kp_rebuilt ("host"), key_pts (last record)
    align               "host" | "device"   map_candidates, cell_select; "device": align_build             --                                                        queue_next_align
    relocalize          "host" | "device"   align, keystage; "device": keystage="device", align_kf         stage, gate, tracking_quality, reloc_kf, reloc_tracked    relocalize_frame, gate

    known_frac, pos_noise, map_seed, kf_every: the map mapping=True starts from and the keyframe cadence without kf_select (_Run.init_mapping).
    kfselect_mindist_t / _r, max_n_kfs: the keyframe stage's options.  detect_cell_size: the detector's grid, detect and image_seeds.
    select_params: keyword arguments of capi.Context.candidates_select (default: max_fts 120, max_fts_segs 100, cells in index order).
    image_seed_params: fast_threshold, detection_threshold (20, 20.0).  reloc_params: quality_min_fts (20), quality_max_drop_fts (50); the
    clamps are the selection's max_fts / max_fts_segs.  lm_room: landmark rows reserved per kind instead of one per seed of the sequence;
    without compaction a sequence whose converged seeds outnumber it ends in PLSVO_E_CAPACITY."""
    o = types.SimpleNamespace(**locals())              # (first statement: exactly the arguments)
    o.map_stage = "cell_select" if cell_select else "map_candidates" if map_candidates else None
    _check_options(o)
    if not kf_insert:
        return _Run(o).run()
    # room for every keyframe the sequence can add (a joined candidate adds a feature, every feature an observation)
    n_fr, n_lm = len(seq["images"]), len(seq["pt_pos"]) + 2 * len(seq["seg_spos"])
    backend.map_reserve(extra_kf=n_fr, extra_kf_pt=n_fr * n_lm, extra_kf_seg=n_fr * n_lm, extra_pt_obs=n_fr * n_lm, extra_seg_obs=n_fr * n_lm)
    if seed_candidates:                                # a landmark row per seed that can converge (its observation fits the room above)
        backend.map_reserve_landmarks(extra_pt=len(seq["pt_pos"]) if lm_room is None else int(lm_room), extra_seg=0 if lm_room is None else int(lm_room))
    try:
        return _Run(o).run()
    finally:
        backend.map_reserve()                          # the tight layout again for whoever stages next on this backend
        if seed_candidates:
            backend.map_reserve_landmarks()


_MODES = (None, "host", "device")
# flag, its values (None: a switch), the flags it needs, per value what else: a backend method, "!method" (the backend must not have it) or (flag, value); the refusal
_PREREQUISITES = (
    ("relocalize", _MODES, ("align", "keystage"), {"device": (("keystage", "device"), "align_kf")}, "relocalize is None, 'host' or 'device' and needs align, keystage and, for 'device', keystage='device' (the live key-point table) and a backend with align_kf() / track_gate()"),
    ("align", _MODES, ("map_candidates", "cell_select"), {"device": ("align_build",)}, "align is None, 'host' or 'device' and needs map_candidates, cell_select and, for 'device', a backend with align_build() / align_built()"),
    ("keystage", _MODES, ("kf_select", "cell_select", "kf_insert"), {"device": ("map_keyframe_decide",), "host": ("keyframe_decide",)}, "keystage is None, 'host' or 'device' and needs kf_select, cell_select, kf_insert and a backend with keyframe_decide() / map_keyframe_decide()"),
    ("compact", (None, "room", "always"), ("seed_candidates",), {"room": ("map_compact",), "always": ("map_compact",)}, "compact is None, 'room' or 'always' and needs seed_candidates and a backend with map_compact()"),
    ("structopt_resident", None, ("mapping", "cell_select"), {True: ("map_optimize_structure",)}, "structopt_resident needs mapping, cell_select and a backend with map_optimize_structure()"),
    ("image_seeds", _MODES, ("seeds_resident",), {"device": ("seeds_keyframe_detect",), "host": ("detect_corners",)}, "image_seeds is None, 'host' or 'device', needs seeds_resident and a backend with detect_corners() / seeds_keyframe_detect()"),
    ("seeds_resident", None, ("seed_candidates",), {True: ("seeds_stage",)}, "seeds_resident needs seed_candidates and a backend with seeds_stage()"),
    ("seed_candidates", None, ("kf_insert",), {True: ("map_add_candidates",)}, "seed_candidates needs kf_insert and a backend with map_add_candidates()"),
    ("kf_insert", None, ("cell_select", "mapping"), {True: ("map_insert",)}, "kf_insert needs mapping, cell_select and a backend with map_insert()"),
    ("cell_select", None, ("map_candidates",), {True: ("map_select",)}, "cell_select needs map_candidates and a backend with map_select()"),
    ("map_stage", (None, "map_candidates", "cell_select"), (), {"map_candidates": ("!frame_step", "map_candidates"), "cell_select": ("!frame_step", "map_select")}, {"map_candidates": "map_candidates needs a per-call backend with map_candidates()", "cell_select": "cell_select needs a per-call backend with map_select()"}))


def _check_options(o):
    """the refusals of run_sequence: a value outside a flag's list, a flag without the flags it stands on, a backend without the
    method -- in the table's order.  (map_stage: steps 2 and 3 by name, the flag the two backend-shape refusals speak of)"""
    met = lambda need: getattr(o, need[0]) == need[1] if isinstance(need, tuple) else hasattr(o.backend, need.lstrip("!")) != need.startswith("!")
    for flag, values, flags, per_value, refusal in _PREREQUISITES:
        v = getattr(o, flag)
        if values is not None and v not in values or v and not (all(getattr(o, f) for f in flags) and all(met(n) for n in per_value.get(v if values else True, ()))):
            raise ValueError(refusal[v] if isinstance(refusal, dict) else refusal)


def _f3(v):
    return [float(x) for x in v]                       # plain floats for the map tables


def _rows_of(table, rows):
    return np.array([table[int(r)] for r in rows], float).reshape(-1, 3)


def _overlap_of(close):
    """the overlap list of a close_keyframes report"""
    return [int(v) for v in close["close_idx"][:close["n_overlap"]]]


class _MapTables:
    """map_candidates: the map tables the harness follows beside the device's.  cm: the tables as lists (tests/np_candidates.py reads
    them so): the keyframes' feature lists, every landmark's observation list with px / f / level, newest first.  They are restaged
    when they change without the device (dirty: a frame becomes a keyframe, a seed converges into the candidate list) and, where the
    device changes them, taken from its fetch (adopt) or kept in step from its reports.
    Point rows of the tables <-> landmarks (indices of P3 / px_new): the identity until seed_candidates appends a converged seed as a NEW
    row (its own row stays behind, empty and in no list), or image_seeds a row without a landmark (-1); segment rows are segment indices
    throughout.  The harness translates wherever the backend speaks in rows (filed and selected landmarks, moved positions)."""

    def __init__(self, seq, known):
        n_pts, n_seg = len(seq["pt_pos"]), len(seq["seg_spos"])
        # keyframe 0 with the features of the landmarks it starts with, one observation each
        self.cm = dict(kf_T=[_f3(seq["poses_true"][0])], kf_slot=[0], kf_pt=[[int(i) for i in np.nonzero(known)[0]]], kf_seg=[list(range(n_seg))],
                       pt_pos=None, pt_type=[abi.LM_UNKNOWN] * n_pts,
                       pt_obs=[[dict(kf=0, px=_f3(seq["pt_px0"][i]), f=_f3(seq["pt_f0"][i]), level=0, type=abi.FTR_CORNER, grad=[0.0, 0.0])] if known[i] else [] for i in range(n_pts)],
                       seg_spos=[_f3(v) for v in seq["seg_spos"]], seg_epos=[_f3(v) for v in seq["seg_epos"]], seg_type=[abi.LM_UNKNOWN] * n_seg,
                       seg_obs=[[dict(kf=0, spx=_f3(seq["seg_spx0"][i]), epx=_f3(seq["seg_epx0"][i]), sf=_f3(seq["seg_sf0"][i]), ef=_f3(seq["seg_ef0"][i]), level=0)]
                                for i in range(n_seg)], pt_cand=[], seg_cand=[])
        self.dirty = True                              # the device's tables are behind cm: the next frame stages
        self.seed_kf = 0                               # the row of frame 0, where every seed was started (None once kf_insert removed it)
        self.row_lm, self.lm_row = list(range(n_pts)), np.arange(n_pts, dtype=np.int64)
        self.quality = None                            # cell_select: the quality state after the last frame (None: nothing staged yet), carried over a restage
        self.so_keys = dict(pt=[], seg=[])             # structopt_resident: last_structure_optim_ per table row, followed from the reports (0: never refined)

    def stage_job(self, P3):
        """-> the abi.CandidateMapJob to (re)stage, the point rows at their landmarks' positions now; None: the device's tables are current"""
        if not self.dirty:
            return None
        self.cm["pt_pos"] = [[float(x) for x in P3[i]] for i in self.row_lm]
        self.dirty = False
        return candidate_map_job(self.cm)

    def adopt(self, tables):
        """behind an insertion or a compaction the harness's tables are the backend's fetch"""
        self.cm = candidate_map_tables(tables)

    def lm_of_rows(self, rows):
        return np.asarray(self.row_lm, np.int64)[rows]

    def row_of_lm(self, lms):
        return self.lm_row[lms]

    def append_candidate(self, pos, kf, px, f, level, grad, lm, own_row=False):
        """a converged seed becomes a candidate of the map (map_.point_candidates_, newCandidatePoint) with its one observation, in keyframe
        row kf: a NEW row behind the others, as plsvo_candidates_add / the seed commit append it on the device (lm -1: a seed from the
        image, no landmark of the harness's map) -- or, own_row, the landmark's staged row, empty until now, for the restage that follows
        (which takes the position from P3).  A seed is observed in the keyframe it was started in (frame 0); once that keyframe has left
        the table the seed's only observation is gone with it, as removeFrameCandidates would delete it, and the callers leave the
        landmark outside the map's tables.  -> the row"""
        cm, obs = self.cm, [dict(kf=kf, px=_f3(px), f=_f3(f), level=level, type=abi.FTR_CORNER, grad=grad)]
        if own_row:
            row = int(self.lm_row[lm])
            cm["pt_obs"][row], cm["pt_type"][row], self.dirty = obs, abi.LM_CANDIDATE, True
        else:
            row = len(cm["pt_pos"])
            cm["pt_pos"].append(_f3(pos)); cm["pt_type"].append(abi.LM_CANDIDATE); cm["pt_obs"].append(obs)
            self.row_lm.append(lm)
            if lm >= 0:
                self.lm_row[lm] = row
        cm["pt_cand"].append(row)
        return row

    def apply_pt_remap(self, remap):
        """a compaction's effect on the rows the harness follows: remap[old row] = the new row, or < 0 for a deleted one"""
        self.lm_row[[lm for row, lm in enumerate(self.row_lm) if lm >= 0 and remap[row] < 0]] = -1
        self.row_lm = [lm for row, lm in enumerate(self.row_lm) if remap[row] >= 0]
        for row, lm in enumerate(self.row_lm):
            if lm >= 0:
                self.lm_row[lm] = row
        self.so_keys["pt"] = [v for row, v in enumerate(self.so_keys["pt"]) if row >= len(remap) or remap[row] >= 0]

    def keyframe_removed(self, row):
        """the keyframe table closes up: frame 0's row moves, or is gone"""
        if self.seed_kf is not None:
            self.seed_kf = None if row == self.seed_kf else self.seed_kf - (row < self.seed_kf)

    def key_point_positions(self, kp_tab, tables=None):
        """getCloseKeyframes reads key_pts_[k]->feat3D->pos_ as it is NOW: kp_tab [n_kf, 5], positions in the keyframes' point-feature lists
        (-1 or out of range: none) -> ([n_kf, 5, 3] landmark positions, [n_kf, 5] validity).  Read from the harness's own tables, or from
        `tables`, a fetched record of the device's (capi.Context.candidates_fetch_map)"""
        n_kf = len(self.cm["kf_T"])
        fts, pos = self.cm["kf_pt"], self.cm["pt_pos"]
        if tables is not None:
            off, pos = tables["kf_pt_off"], tables["pt_pos"]
            fts = [tables["kf_pt_lm"][int(off[j]):int(off[j + 1])] for j in range(n_kf)]
        kpos, kval = np.zeros((n_kf, 5, 3)), np.zeros((n_kf, 5), np.uint8)
        for j, row in enumerate(kp_tab):
            for s, h in enumerate(row):
                lm = int(fts[j][int(h)]) if 0 <= h < len(fts[j]) else -1
                if lm >= 0:
                    kpos[j, s], kval[j, s] = pos[lm], 1
        return kpos, kval

    def follow_selection(self, q_after):
        """the tables follow the device behind a selection: types, candidate lists, and the keyframe features of the landmarks safeDelete* cut loose"""
        cm = self.cm
        for name in ("pt", "seg"):
            for lm in np.nonzero(q_after[name + "_event"] & abi.LM_EVENT_DELETED)[0]:
                if cm[name + "_type"][int(lm)] == abi.LM_UNKNOWN:
                    cm["kf_" + name] = [[-1 if v == lm else v for v in fts] for fts in cm["kf_" + name]]
            cm[name + "_type"] = [int(v) for v in q_after[name + "_type"]]
            cm[name + "_cand"] = [int(v) for v in q_after[name + "_cand"]]


class _SeedRows:
    """seeds_resident: the resident seed rows as the harness follows them, one (landmark, or -1: a seed from the image; keyframe row;
    feature: px / f / level of an image seed) per point row of the device's lists, through removals, starts and erasures"""

    def __init__(self):
        self.rows, self.n_image_converged = [], 0
        self.on_device = False                         # the seed lists are staged and their keyframe is still in the table
        self.last_rows = None                          # image_seeds: pt_status / pt_px_cur of the last update (the occupancy of the next keyframe)

    def lms(self):
        return np.array([r[0] for r in self.rows], np.int64)

    def n_image(self):
        return sum(1 for lm, _, _ in self.rows if lm < 0)

    def remove_keyframe(self, row):
        """removeKeyframe: the seeds of keyframe `row` leave, the rows behind it move down"""
        self.rows = [(lm, kf - (kf > row), ftr) for lm, kf, ftr in self.rows if kf != row]

    def started(self, n, new_kf, lists):
        """n image seeds started in keyframe row new_kf, at the back; their features from the fetched lists (both transports), for the
        landmark a converged one becomes"""
        first = len(self.rows)
        assert len(lists["pt_ref_kf"]) == first + n
        self.rows += [(-1, new_kf, dict(px=_f3(lists["pt_px"][j]), f=_f3(lists["pt_f"][j]), level=int(lists["pt_level"][j]))) for j in range(first, first + n)]

    def drop(self, status):
        """an update's erasures: converged, NaN and aged rows leave"""
        self.rows = [r for r, st in zip(self.rows, status) if st not in (abi.SEED_CONVERGED, abi.SEED_NAN, abi.SEED_AGED)]


class _Keyframes:
    """kf_select without keystage: the keyframe table of the synchronous keyframe stage -- per row the pose and the landmark positions of
    the five key points, snapshotted when the keyframe is added -- and seed_depth, the (depth_mean * 2.0, 0.1 * depth_min) a keyframe's
    corner seeds start from (:391), which keystage keeps here too"""

    def __init__(self, backend, o, seed_depth):
        self.backend, self.o, self.seed_depth = backend, o, seed_depth
        self.T, self.pos, self.valid = [], [], []

    def decide(self, T_new, T_last, px, pos, sp, ep, overlap):
        kf_T = np.stack(self.T) if self.T else np.zeros((0, 7))
        return self.backend.keyframe_decide(abi.KeyframeDecideJob(self.o.seq["cam"], T_new, T_last, px, pos, None, sp, ep, None, kf_T, overlap,
                                                                  (-1,) * 5, self.o.kfselect_mindist_t, self.o.kfselect_mindist_r))

    def add_keyframe(self, T, key_pts, pos):
        """the keyframe table row: the pose and the landmark positions of the five key points (key_pts index `pos`, -1 = none)"""
        self.T.append(np.asarray(T, float).copy())
        self.pos.append(np.array([pos[i] if i >= 0 else np.zeros(3) for i in key_pts]))
        self.valid.append(np.array([i >= 0 for i in key_pts], np.uint8))

    def remove(self, row):
        del self.T[row], self.pos[row], self.valid[row]

    def close_job(self, T, max_n_kfs):
        return abi.CloseKeyframesJob(self.o.seq["cam"], T, np.stack(self.T), np.stack(self.pos), np.stack(self.valid), max_n_kfs)

    def depth_from(self, dec):
        if dec["has_depth"]:
            self.seed_depth = (dec["depth_mean"] * 2.0, 0.1 * dec["depth_min"])


class _RelocState:
    """relocalize: the reference's stage machine, and align's hand-over to the next frame"""

    def __init__(self):
        self.stage, self.gate_dev = "default", None    # "default" | "reloc": STAGE_DEFAULT_FRAME / STAGE_RELOCALIZING; the gate's carried poses on the device
        self.obs_last, self.obs_resident = None, False  # num_obs_last_pt / _ls, and whether the device holds them
        self.next_align = None                         # align: the job of the frame to come -- an abi.AlignJob ("host") or True: built on the device


class _Frame:
    """what the steps of one frame hand to one another"""

    def __init__(self, reloc):
        self.reloc = reloc                             # the frame is a relocalisation attempt
        self.reloc_kf = self.reloc_tracked = self.T_reset = self.T_ref_kf = None   # its keyframe, n_tracked of the gating alignment, T_f_w_last, the keyframe's pose
        self.job = self.ar = self.T_k = self.poses_dev = None   # 1: the gathered job, the alignment's result, the aligned pose (host copy, device pointer)
        self.map_job = self.close = self.cand_rec = None        # 2-3: the stage job if the tables were staged, the close_keyframes report, the candidate stage's record fields
        self.px_new = self.level = self.pt_ok = self.seg_ok = None   # per landmark (points, segment starts, segment ends): matched px and level; found, per point / segment
        self.frame_sel = self.sel_mask = None          # cell_select: the frame's selection, and which selected points have a landmark of the harness
        self.pr = self.pt_i = self.seg_i = self.n_ties = self.gate = None   # 4: the pose optimiser's result, the landmarks of its features, align_ties; the gates' (result, tracking quality)
        self.T = self.T_last = self.pt_keep = self.seg_keep = self.kept = None   # the optimised pose, last_frame_'s, the keep masks over pt_i / seg_i, pt_i[pt_keep]
        self.rec = self.dec = self.is_kf = None        # the record, the keyframe decision
        self.bad_quality, self.kp_frame = False, 0     # TRACKING_BAD; keystage "host": key-point rows rebuilt in this frame


_IDENT = [0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]


class _Run:
    """One run_sequence call: the state that lives from frame to frame, and the steps of FrameHandlerMono::processFrame as methods, in
    the order process_frame calls them.  A step reads and writes the run's state and the frame's _Frame, nothing else."""

    def __init__(self, o):
        self.o, self.backend, self.seq, self.cam = o, o.backend, o.seq, o.seq["cam"]
        seq = o.seq
        self.chain = hasattr(o.backend, "frame_step")  # steps 1-4 are one resident call
        self.rs, self.rows = _RelocState(), _SeedRows()
        self.gate_kw = dict(dict(quality_min_fts=20, quality_max_drop_fts=50), **(o.reloc_params or {}))
        self.img_kw = dict(dict(fast_threshold=20, detection_threshold=20.0), **(o.image_seed_params or {}))
        self.kp_tab, self.kp_live = None, False        # keystage: Frame::key_pts_ per keyframe row of cm ("host": kept here; "device": fetched when a restage needs it)
        o.backend.load_frames(seq["images"])
        self.n_frames, self.n_pts, self.n_seg = len(seq["images"]), len(seq["pt_pos"]), len(seq["seg_spos"])
        self.kf_T, self.T_prev = seq["poses_true"][0], seq["poses_true"][0].copy()
        self.P3 = seq["pt_pos"].copy()                 # the map's point positions (seq["pt_pos"] stays the truth)
        self.known = np.ones(self.n_pts, bool)
        self.kf_select = self.detect = False           # the flags where the backend can serve them
        if o.mapping:
            self.init_mapping()
        k0 = np.nonzero(self.known)[0]                 # prev: features of the previous frame that still carry a landmark: index into the map + pixel position
        self.prev = dict(pt_idx=k0, pt_px=seq["pt_px0"][k0].copy(), seg_idx=np.arange(self.n_seg), seg_spx=seq["seg_spx0"].copy(), seg_epx=seq["seg_epx0"].copy())
        self.out = [dict(T=self.T_prev.copy(), cov=np.full((6, 6), 1e-9), n_align=0, n_matched_pt=int(self.known.sum()), n_matched_seg=self.n_seg)]
        if o.map_candidates:
            self.mt = _MapTables(seq, self.known)
            self.select_kw = dict(dict(max_fts=120, max_fts_segs=100, cell_order=None, seg_cell_order=None, reproj_thresh=o.reproj_thresh), **(o.select_params or {}))
            self.align_caps = (max(self.select_kw["max_fts"] + 2, 8), max(self.select_kw["max_fts_segs"] + 2, 8))   # align: the alignment batch's capacities

    def init_mapping(self):
        """mapping=True: only `known_frac` of the point landmarks start in the map (positions off by `pos_noise` x depth along their viewing
        ray), the others are depth-filter seeds that turn into landmarks when they converge; the seed update runs every frame; every
        `kf_every`-th frame plays the keyframe: its matches become observations of their landmarks (Feature3D::obs_ grows at keyframes
        only, as in the reference) and the 20 least recently refined landmarks with >= 2 observations are structure-optimised.
        detect and kf_select hold where the backend has detect_corners / keyframe_decide.  With kf_select frame 0 is a keyframe whose key
        points come from the same call as every other's (no overlap keyframes: nothing else is looked at)."""
        o, seq, kf_T, P3, n_pts = self.o, self.seq, self.kf_T, self.P3, self.n_pts
        rng = np.random.default_rng(o.map_seed + 77)
        known = self.known = rng.uniform(size=n_pts) < o.known_frac
        kf_pos = synth.se3_inv(kf_T)[4:]
        ray = P3 - kf_pos
        P3[known] = (kf_pos + ray * (1.0 + rng.uniform(-o.pos_noise, o.pos_noise, n_pts))[:, None])[known]
        depth0 = np.linalg.norm(ray, axis=1)
        dmean, dmin = float(depth0[known].mean()), 0.7 * float(depth0[known].min())
        nsd = int((~known).sum())
        self.seeds = dict(idx=np.nonzero(~known)[0], a=np.full(nsd, 10.0, np.float32), b=np.full(nsd, 10.0, np.float32), mu=np.full(nsd, 1.0 / dmean, np.float32),
                          z_range=np.full(nsd, 1.0 / dmin, np.float32), sigma2=np.full(nsd, (1.0 / dmin) ** 2 / 36.0, np.float32))
        self.obs = {int(i): [(0, seq["pt_f0"][i])] for i in range(n_pts)}     # Feature3D::obs_: (frame, unit bearing)
        self.last_optim = np.zeros(n_pts, np.int64)
        self.poses_est = [kf_T.copy()]
        self.detect = o.detect and hasattr(self.backend, "detect_corners")
        self.img_seeds, self.img_converged = None, 0
        self.w_img, self.h_img = int(self.cam[4]), int(self.cam[5])
        self.kf_select = o.kf_select and hasattr(self.backend, "keyframe_decide")
        self.kfs = _Keyframes(self.backend, o, (dmean, dmin))
        if self.kf_select:
            z3 = np.zeros((0, 3))
            self.kfs.add_keyframe(kf_T, self.kfs.decide(kf_T, kf_T, seq["pt_px0"][known], P3[known], z3, z3, ())["key_pts"], P3[known])
        if self.detect:
            self.img_seeds = self.new_image_seeds(0, seq["pt_px0"][known])

    def run(self):
        for k in range(1, self.n_frames):
            self.out.append(self.process_frame(k))
        if self.o.keystage and self.kp_live:           # Frame::key_pts_ of every keyframe at the end
            kp = self.kp_tab if self.o.keystage == "host" else self.backend.map_fetch_keypts()[:len(self.mt.cm["kf_T"])]
            self.out[-1]["key_pts"] = np.array(kp, np.int32).reshape(-1, 5)
        return self.out

    def process_frame(self, k):
        """frame k through FrameHandlerMono::processFrame (src/frame_handler_mono.cpp:266-340) and, with mapping, what stands behind it
        there and in the depth-filter thread.  -> the frame's record"""
        o = self.o
        fr = _Frame(bool(o.relocalize) and self.rs.stage == "reloc")
        failed = self.relocalize_frame(k, fr) if fr.reloc else None
        if failed:
            return failed
        self.align(k, fr)
        if self.chain:
            self.track_map_chain(k, fr)
        elif o.map_candidates:
            self.track_map_candidates(k, fr)
        else:
            self.track_map_keyframe0(k, fr)
        if not self.chain and not o.cell_select:
            self.pose_optimize_host(k, fr)
        fr.n_ties = self.backend.align_ties() if hasattr(self.backend, "align_ties") else None
        fr.T_last = fr.T_ref_kf if fr.reloc else self.T_prev     # last_frame_ of this processFrame
        failed = self.gate(k, fr) if o.relocalize else None
        if failed:
            return failed
        rec = fr.rec = self.tracked(k, fr)
        if o.mapping:
            fr.is_kf = (k % o.kf_every) == 0
            if self.kf_select and not o.keystage:
                self.decide_keyframe_host(k, fr)
            if o.structopt_resident:
                self.structure_resident(k, fr)
            if o.keystage:
                self.decide_keyframe(k, fr)
            if fr.is_kf:
                for i, brg in zip(fr.kept, _bearing(self.cam, fr.px_new[fr.kept])):
                    self.obs[int(i)].append((k, brg))
                if o.kf_insert:
                    self.insert_keyframe(k, fr)
                elif o.map_candidates:
                    self.join_keyframe_host(k, fr)
            self.structure_host(k, fr)
            self.update_seeds(k, fr)
            if self.detect:
                self.image_seeds_host(k, fr)
            rec.update(n_known=int(self.known.sum()), n_seeds=len(self.seeds["idx"]),
                       landmark_err=float(np.median(np.linalg.norm(self.P3[self.known] - self.seq["pt_pos"][self.known], axis=1))))
        self.queue_next_align(k, fr)
        return rec

    def record(self, fr, T, cov, n_align, n_matched, n_kept, gate=None, n_ties=None):
        """the per-frame record of a tracked frame, a failed gate and a failed relocalisation; gate: (result, tracking quality)"""
        rec = dict(T=T, cov=cov, n_align=n_align, n_matched_pt=n_matched[0], n_matched_seg=n_matched[1], n_kept_pt=n_kept[0], n_kept_seg=n_kept[1])
        if n_ties is not None:
            rec["align_ties"] = n_ties
        if gate is not None:
            rec.update(stage=self.rs.stage, gate=gate[0], tracking_quality=gate[1])
            if fr.reloc:
                rec.update(reloc_kf=fr.reloc_kf, reloc_tracked=fr.reloc_tracked)
        if fr.cand_rec is not None:
            rec.update(fr.cand_rec)
        if self.o.mapping:
            self.poses_est.append(T.copy())
        return rec

    def pos_all(self):
        return np.concatenate([self.P3, self.seq["seg_spos"], self.seq["seg_epos"]])

    def relocalize_frame(self, k, fr):
        """relocalize="host" | "device": the harness plays the reference's stage machine, STAGE_DEFAULT_FRAME <-> STAGE_RELOCALIZING
        (finishFrameProcessingCommon).  A frame that fails the gates (gate) is carried forward with the pose the gate
        gives and the next frame relocalises against the closest keyframe of the resident tables until a frame passes the gates again:
        relocalizeFrame (:408-436) is Map::getClosestKeyframe from the last frame's pose, a gating alignment against that keyframe from the
        identity that must track more than 30, a second alignment from the keyframe's own pose (new_frame_->T_f_w_ =
        ref_keyframe->T_f_w_, :266), and the rest of processFrame with last_frame_ = ref_keyframe, whose every failure carries the last
        frame's pose; a success returns to STAGE_DEFAULT_FRAME.  (last_frame_ is never a keyframe of the table here: self_kf -1.)
        "device" uses plsvo_candidates_align_build_kf (a backend with align_kf / track_gate); "host" does the same with the calls there
        were before -- fetched tables, close_keyframes, align_kf_job_host staged through plsvo_align_stage.  The two differ in transport
        alone and agree in every record.  One of the two host waits of "device" is here: n_tracked behind the gating alignment.
        The tables must not wait for a restage while a stream relocalises (kf_insert with seed_candidates keeps them resident).
        -> the failure's record, or None: fr holds the alignment against the keyframe (ar, T_k, poses_dev)"""
        o, backend, mt, rs = self.o, self.backend, self.mt, self.rs
        if mt.dirty:
            raise ValueError("relocalize: the resident tables wait for a restage")
        caps = (max(self.align_caps[0], max(len(l) for l in mt.cm["kf_pt"])), max(self.align_caps[1], max(len(l) for l in mt.cm["kf_seg"])))
        if o.relocalize == "device":
            ar, fr.reloc_kf, T_gate, _ = backend.align_kf(None, k, _IDENT, o.max_level, o.min_level, *caps, T_last=self.T_prev, last_dev=rs.gate_dev)
        else:
            tabs = backend.map_fetch()
            kp_now = self.kp_tab if o.keystage == "host" else backend.map_fetch_keypts()[:len(mt.cm["kf_T"])]
            kpos, kval = mt.key_point_positions(kp_now, tabs)
            cl = backend.close_keyframes(abi.CloseKeyframesJob(self.cam, self.T_prev, np.asarray(tabs["kf_T"], float).reshape(-1, 7), kpos, kval, o.max_n_kfs))
            ar, fr.reloc_kf, T_gate = None, -1, None
            if cl["n_close"] > 0:                      # Map::getClosestKeyframe: the front of the sorted list
                fr.reloc_kf = int(cl["close_idx"][0])
                ar = backend.sparse_align(align_kf_job_host(self.cam, o.max_level, o.min_level, tabs, fr.reloc_kf, _IDENT, k))
                T_gate = np.array(_se3_mul_s(ar.T, tabs["kf_T"][fr.reloc_kf]))
        fr.reloc_tracked = 0 if ar is None else int(ar.n_tracked)
        if ar is None or ar.n_tracked <= 30:
            # "No reference keyframe": new_frame_ keeps its default pose; the gating alignment (:421): the pose it wrote stays
            fail, T_fail = ("no_keyframe", np.array(_IDENT)) if ar is None else ("gating", np.asarray(T_gate, float).copy())
            rec = self.record(fr, T_fail, np.full((6, 6), 1e-9), fr.reloc_tracked, (0, 0), (0, 0), gate=(fail, abi.TRACKING_INSUFFICIENT))
            self.T_prev, rs.gate_dev, rs.obs_last, rs.obs_resident, rs.next_align = T_fail, None, (0, 0), False, None   # Frame::nObs() of a frame without features
            return rec
        fr.T_reset = self.T_prev                       # T_f_w_last
        fr.T_ref_kf = np.array(mt.cm["kf_T"][fr.reloc_kf], float)
        if o.relocalize == "device":
            fr.ar, _, fr.T_k, fr.poses_dev = backend.align_kf(fr.reloc_kf, k, None, o.max_level, o.min_level, *caps)
        else:
            fr.ar = backend.sparse_align(align_kf_job_host(self.cam, o.max_level, o.min_level, tabs, fr.reloc_kf, None, k))
            fr.T_k = np.array(_se3_mul_s(fr.ar.T, tabs["kf_T"][fr.reloc_kf]))
        rs.next_align = None
        return None

    def align(self, k, fr):
        """1. sparse image alignment, previous frame -> frame k (processFrame :266-274; T_k = T_cur_from_ref * T_prev, :92).  The job:
          - gathered here from the previous frame's kept features (f * |pos - ref_pos|, :229-230) -- every frame without align, and
            with it the first frame and a frame behind one that left the tables waiting for a restage (a keyframe without kf_insert, a
            converged seed without seed_candidates): the resident tables are then behind the harness's own; the resident chain runs
            it inside frame_step;
          - align="host": the abi.AlignJob queue_next_align left, staged through plsvo_align_stage;
          - align="device": built on the device behind the previous frame: run, compose, the pose stays on the device and reaches the
            candidate stage by device pointer (poses_dev);
          - a relocalising frame is aligned against its keyframe already (relocalize_frame)."""
        rs, backend = self.rs, self.backend
        if rs.next_align is None and not fr.reloc:
            prev, seq, scaled = self.prev, self.seq, self.scaled_bearing
            fr.job = abi.AlignJob(self.cam, self.o.max_level, self.o.min_level, 30, 1e-6, synth.se3_mul(self.T_prev, synth.se3_inv(self.T_prev)), prev["pt_px"],
                                  scaled(prev["pt_px"], self.P3[prev["pt_idx"]]), prev["seg_spx"], prev["seg_epx"],
                                  np.linalg.norm(prev["seg_epx"] - prev["seg_spx"], axis=1), scaled(prev["seg_spx"], seq["seg_spos"][prev["seg_idx"]]),
                                  scaled(prev["seg_epx"], seq["seg_epos"][prev["seg_idx"]]), ref_slot=k - 1, cur_slot=k)
        if self.chain or fr.reloc:
            return
        if rs.next_align is None:
            fr.ar = backend.sparse_align(fr.job)
            fr.T_k = synth.se3_mul(fr.ar.T, self.T_prev)
        elif self.o.align == "device":
            fr.ar, fr.T_k, fr.poses_dev = backend.align_built()
        else:
            fr.ar = backend.sparse_align(rs.next_align)
            fr.T_k = np.array(_se3_mul_s(fr.ar.T, self.T_prev))
        rs.next_align = None

    def scaled_bearing(self, px, pos):
        """f * |pos - ref_pos| of a feature of the previous frame (:229-230)"""
        return _bearing(self.cam, px) * np.linalg.norm(pos - synth.se3_inv(self.T_prev)[4:], axis=1)[:, None]

    def track_map_chain(self, k, fr):
        """1-4 as one resident call (HipChainBackend.frame_step): nothing but the final results comes back"""
        seq, n_pts, n_seg = self.seq, self.n_pts, self.n_seg
        act = np.concatenate([self.known, np.ones(2 * n_seg, bool)]).astype(np.uint8)
        ref_px_all = np.concatenate([seq["pt_px0"], seq["seg_spx0"], seq["seg_epx0"]])
        ref_f_all = np.concatenate([seq["pt_f0"], seq["seg_sf0"], seq["seg_ef0"]])
        cr = self.backend.frame_step(fr.job, self.T_prev, self.kf_T, 0, n_pts, n_seg, self.pos_all(), ref_px_all, ref_f_all, act, self.cam, self.o.n_pyr_levels, self.o.reproj_thresh)
        fr.ar, fr.pr, fr.px_new, fr.T_k = cr.align, cr.pose, cr.px, synth.se3_mul(cr.align.T, self.T_prev)
        fr.pt_i, fr.seg_i = cr.sel_pt.astype(np.int64), cr.sel_seg.astype(np.int64)
        fr.pt_ok = np.zeros(n_pts, bool); fr.pt_ok[fr.pt_i] = True
        fr.seg_ok = np.zeros(n_seg, bool); fr.seg_ok[fr.seg_i] = True

    def track_map_keyframe0(self, k, fr):
        """2. reprojection of the whole map (Reprojector::reprojectMap) and 3. direct matching against the keyframe-0 observations
        (Matcher::findMatchDirect); seeds are not in the map yet"""
        seq, n_pts, n_seg, pos_all = self.seq, self.n_pts, self.n_seg, self.pos_all()
        frame_T = np.stack([self.kf_T, fr.T_k])
        rp = self.backend.reproject(abi.ReprojectJob(self.cam, frame_T, np.ones(len(pos_all), np.int32), pos_all, cell_size=30))
        vis = rp["cell"] >= 0
        vis[:n_pts] &= self.known
        seg_vis = vis[n_pts:n_pts + n_seg] & vis[n_pts + n_seg:]
        vis[n_pts:n_pts + n_seg] = vis[n_pts + n_seg:] = seg_vis
        idx = np.nonzero(vis)[0]
        ref_px = np.concatenate([seq["pt_px0"], seq["seg_spx0"], seq["seg_epx0"]])[idx]
        ref_f = np.concatenate([seq["pt_f0"], seq["seg_sf0"], seq["seg_ef0"]])[idx]
        m = len(idx)
        mr = self.backend.match_direct(abi.MatchJob(self.cam, frame_T, np.array([0, k], np.int32), np.ones(m, np.int32), np.zeros(m, np.int32), ref_px, ref_f,
                                                    np.zeros(m, np.int32), np.zeros(m, np.uint8), np.zeros((m, 2)), pos_all[idx], rp["px"][idx], self.o.n_pyr_levels, 10))
        found = np.zeros(len(pos_all), bool)
        found[idx] = mr["found"].astype(bool)
        fr.px_new = rp["px"].copy()
        fr.px_new[idx] = mr["px_cur"]
        fr.level = np.zeros(len(pos_all), np.int32)
        fr.level[idx] = np.maximum(mr["search_level"], 0)
        fr.pt_ok, fr.seg_ok = found[:n_pts], found[n_pts:n_pts + n_seg] & found[n_pts + n_seg:]

    def overlap_keyframes(self, k, fr):
        """the frame's overlap list for the candidate stage: the one of plsvo_close_keyframes with kf_select, otherwise every keyframe in
        table order.
        keystage="host" | "device": the keyframe stage follows the reference instead of snapshotting a key point's position when its
        keyframe is inserted -- Frame::key_pts_ are positions in the keyframes' feature lists, a key point's position is its landmark's
        position in the tables NOW (Map::getCloseKeyframes, src/map.cpp:165-169), a key point whose landmark is deleted is replaced
        (Map::safeDeletePoint -> Frame::removeKeyPoint, :116-123).  "device" does it on the resident tables (plsvo_candidates_set_keypts,
        _run_close; DESIGN.md 3.19: a backend with map_set_keypts / map_keyframe_decide) and the list is decided there, inside map_select
        (-> []); "host" does the same with the calls there were before: the key-point table kept here from the tables the harness
        follows (Frame::setKeyframe: from five NULLs), then the synchronous close_keyframes on gathered arrays.  A restage drops the
        resident table: it travels with the tables."""
        o, mt = self.o, self.mt
        if o.keystage:
            n_kf = len(mt.cm["kf_T"])
            if fr.map_job is not None and o.keystage == "device" and self.kp_live:
                self.kp_tab = [[int(h) for h in r] for r in self.backend.map_fetch_keypts()[:n_kf]]
            if self.kp_tab is None and o.keystage == "host":
                self.kp_tab, _ = _key_point_upkeep(mt.cm, [[-1] * 5] * n_kf, self.cam, fresh=range(n_kf))
            self.kp_live = True
            if o.keystage == "device":
                return []
            kpos, kval = mt.key_point_positions(self.kp_tab)
            fr.close = self.backend.close_keyframes(abi.CloseKeyframesJob(self.cam, fr.T_k, np.array(mt.cm["kf_T"], float).reshape(-1, 7), kpos, kval, o.max_n_kfs))
        elif self.kf_select:
            fr.close = self.backend.close_keyframes(self.kfs.close_job(fr.T_k, o.max_n_kfs))
        else:
            return list(range(len(mt.cm["kf_T"])))
        return _overlap_of(fr.close)

    def track_map_candidates(self, k, fr):
        """2 + 3 from the map-candidate stage (plsvo_candidates_*) instead of keyframe 0: overlap keyframes' features,
        first visit wins, closest-view observation, quality order, matched on the device (reprojectMap :157-183, getCloseViewObs,
        findMatchDirect).  The harness keeps the map tables the stage needs (_MapTables), restages them when they change, and hands each
        frame its pose and its overlap list.  Without cell_select the matches reach the pose optimiser in landmark-index order, as
        without the stage.  ref_kf_hist: how many of the filed landmarks took their reference observation from each keyframe of the
        table.  record_candidates keeps the frame's stage inputs and result in rec["candidates"]; with cell_select also the selection
        and the quality state before and after the frame."""
        o, mt, n_pts, n_seg = self.o, self.mt, self.n_pts, self.n_seg
        fr.map_job = mt.stage_job(self.P3)
        overlap = self.overlap_keyframes(k, fr)
        frame_job = abi.CandidateFrameJob(fr.T_k, overlap, cur_slot=k)
        cm_before = copy.deepcopy(mt.cm) if o.record_candidates else None
        if o.cell_select:
            cr, mr, q_after = self.select_cells(k, fr, frame_job)
            overlap = _overlap_of(fr.close) if o.keystage == "device" else overlap
        else:
            cr, mr = self.backend.map_candidates(fr.map_job, frame_job, self.cam, o.n_pyr_levels)
        n_all = n_pts + 2 * n_seg
        found, fr.px_new, fr.level = np.zeros(n_all, bool), np.zeros((n_all, 2)), np.zeros(n_all, np.int32)
        lm_at = np.concatenate([mt.lm_of_rows(cr["pt_lm"]), n_pts + cr["seg_lm"], n_pts + n_seg + cr["seg_lm"]]).astype(np.int64)
        own = lm_at >= 0                               # (image_seeds: a row without a landmark of the harness's map is the device's alone)
        found[lm_at[own]] = mr["found"].astype(bool)[own]
        fr.px_new[lm_at[own]] = mr["px"][own]
        fr.level[lm_at[own]] = np.maximum(mr["search_level"], 0)[own]
        fr.pt_ok, fr.seg_ok = found[:n_pts], found[n_pts:n_pts + n_seg] & found[n_pts + n_seg:]
        hist = np.zeros(len(mt.cm["kf_T"]), np.int64)
        for name in ("pt", "seg"):
            for lm, ob in zip(cr[name + "_lm"], cr[name + "_obs"]):
                if ob >= 0:
                    hist[mt.cm[name + "_obs"][lm][ob]["kf"]] += 1
        fr.cand_rec = dict(n_filed_pt=cr["n_filed_pt"], n_filed_seg=cr["n_filed_seg"], ref_kf_hist=[int(v) for v in hist])
        if o.record_candidates:
            fr.cand_rec["candidates"] = dict(stream=cm_before, T=[float(v) for v in fr.T_k], overlap=list(overlap), out=cr, match=mr)
        if o.cell_select:
            self.follow_selection(fr, q_after)

    def select_cells(self, k, fr, frame_job):
        """cell_select: the second half of Reprojector::reprojectMap on the device as well (plsvo_candidates_select): one
        candidate per grid cell in place of every found match, the landmark quality (n_failed_reproj_ / n_succeeded_reproj_, promotions,
        deletions) kept resident from frame to frame, and the pose optimiser fed on the device in place of the per-call one.  The
        features reach the pose optimiser in selection order; a segment that won both of its cells is a feature twice.  The harness
        restages only when the map changes at a keyframe (or a seed converges), and carries the counters over a restage with
        fetch_quality / set_quality (carry=); the structure optimiser's keys do not survive a stage either and are carried like them
        (map_set_last_optim; rows appended since read 0).
        -> (the stage's result, the matcher's, the quality state after the frame); fr: the selection, the pose optimiser's result"""
        o, mt, backend = self.o, self.mt, self.backend
        staged = fr.map_job is not None
        cr, mr, fr.frame_sel, fr.pr, q_after = backend.map_select(fr.map_job, frame_job, self.cam, o.n_pyr_levels, self.select_kw, carry=mt.quality if staged else None,
                                                                 **(dict(close=o.max_n_kfs, key_pts=self.kp_tab) if o.keystage == "device" else {}),
                                                                 **(dict(poses_dev=fr.poses_dev) if fr.poses_dev else {}))
        if o.keystage == "device":
            fr.close = backend.last_close
        if o.structopt_resident and staged and (any(mt.so_keys["pt"]) or any(mt.so_keys["seg"])):
            backend.map_set_last_optim(mt.so_keys["pt"] + [0] * (len(mt.cm["pt_pos"]) - len(mt.so_keys["pt"])), mt.so_keys["seg"] + [0] * (len(mt.cm["seg_spos"]) - len(mt.so_keys["seg"])))
        if o.seeds_resident and staged and o.mapping and mt.seed_kf is not None:
            self.stage_seeds()
        return cr, mr, q_after

    def stage_seeds(self):
        """seeds_resident: the map's seeds are staged ONCE, beside the map tables that were just staged, and are updated, erased and
        handed over to the resident tables on the device (plsvo_seeds_update): no seed travels per frame and no record
        comes back, only the report and the update's rows (update_seeds).  Every seed was started in frame 0's keyframe, in one batch
        that never ages (the harness keeps its seeds until they converge).  image_seeds: room for the seeds the keyframes start."""
        o, seq, seeds = self.o, self.seq, self.seeds
        si_ = seeds["idx"]
        cells = (-(-self.w_img // o.detect_cell_size)) * (-(-self.h_img // o.detect_cell_size))
        self.backend.seeds_stage(dict(batch_counter=0, pt_ref_kf=np.full(len(si_), self.mt.seed_kf, np.int32), pt_batch_id=np.zeros(len(si_), np.int32), pt_px=seq["pt_px0"][si_],
                                      pt_f=seq["pt_f0"][si_], pt_level=np.zeros(len(si_), np.int32), pt_type=np.zeros(len(si_), np.uint8),
                                      pt_grad=np.zeros((len(si_), 2)), pt_a=seeds["a"], pt_b=seeds["b"], pt_mu=seeds["mu"], pt_z_range=seeds["z_range"],
                                      pt_sigma2=seeds["sigma2"]), self.cam, max_n_kfs=1 << 30, n_pyr_levels=o.n_pyr_levels,
                                 **(dict(room=dict(extra_pt=self.n_frames * cells)) if o.image_seeds else {}))
        self.rows.rows, self.rows.on_device = [(int(i), self.mt.seed_kf, None) for i in si_], True

    def follow_selection(self, fr, q_after):
        """behind map_select: the harness follows the types, the candidate lists and the deletions in its own tables from fetch_quality,
        keystage "host" replaces the key points of the landmarks the selection deleted (removeKeyPoint), and 4. on the device: the
        selected features in selection order with the resident pose optimiser's result, as landmarks of the harness"""
        o, mt = self.o, self.mt
        mt.follow_selection(q_after)
        ev = np.concatenate([q_after["pt_event"], q_after["seg_event"]])
        fr.cand_rec.update(n_trials=fr.frame_sel["n_trials"], n_promoted=int((ev & abi.LM_EVENT_PROMOTED).astype(bool).sum()),
                           n_deleted=int((ev & abi.LM_EVENT_DELETED).astype(bool).sum()))
        if o.record_candidates:
            fr.cand_rec["candidates"].update(select=fr.frame_sel, quality_before=mt.quality, quality=q_after, select_params=dict(self.select_kw))
        mt.quality = q_after
        if o.keystage == "host":
            self.kp_tab, fr.kp_frame = _key_point_upkeep(mt.cm, self.kp_tab, self.cam)
        pt_i, fr.seg_i = mt.lm_of_rows(fr.frame_sel["pt_lm"]), fr.frame_sel["seg_lm"].astype(np.int64)
        fr.sel_mask = pt_i >= 0
        fr.pt_i = pt_i[fr.sel_mask]
        fr.pt_ok = np.zeros(self.n_pts, bool); fr.pt_ok[fr.pt_i] = True
        fr.seg_ok = np.zeros(self.n_seg, bool); fr.seg_ok[fr.seg_i] = True

    def pose_optimize_host(self, k, fr):
        """4. motion-only pose optimisation on the matches (processFrame :327-329); a LineFeat's level is the END point's (matcher.cpp:264)"""
        seq, cam, px_new, n_pts, n_seg = self.seq, self.cam, fr.px_new, self.n_pts, self.n_seg
        pt_i, seg_i = fr.pt_i, fr.seg_i = np.nonzero(fr.pt_ok)[0], np.nonzero(fr.seg_ok)[0]
        sf, ef = _bearing(cam, px_new[n_pts + seg_i]), _bearing(cam, px_new[n_pts + n_seg + seg_i])
        line = np.cross(sf, ef)
        line = line / np.sqrt(line[:, 0:1] ** 2 + line[:, 1:2] ** 2) if len(seg_i) else np.zeros((0, 3))    # feature.cpp:103-104
        fr.pr = self.backend.pose_optimize(abi.PoseOptJob(fr.T_k, abs(cam[0]), self.o.reproj_thresh, 10, _bearing(cam, px_new[pt_i]), self.P3[pt_i], fr.level[pt_i], line,
                                                          seq["seg_spos"][seg_i], seq["seg_epos"][seg_i], fr.level[n_pts + n_seg + seg_i]))

    def gate(self, k, fr):
        """relocalize: the gates of processFrame (:315-321, :335) and setTrackingQuality stand behind every frame's pose optimisation, ahead
        of the structure optimisation: a frame that fails is not structure-optimised, decided, inserted or fed to the depth filter
        (RESULT_FAILURE: nothing behind the gate runs), its pose is the one the gate carries, and the next frame relocalises.
        TRACKING_BAD keeps a frame from becoming a keyframe.  "device": plsvo_candidates_track_gate (its record is the other host wait);
        "host": track_gate_host on the fetched counts.  -> the failure's record, or None"""
        o, rs, pr, frame_sel = self.o, self.rs, fr.pr, fr.frame_sel
        if rs.obs_last is None:
            rs.obs_last = (self.out[0]["n_matched_pt"], self.out[0]["n_matched_seg"])
        T_reset = fr.T_reset if fr.reloc else self.T_prev
        gk = dict(self.gate_kw, max_fts=self.select_kw["max_fts"], max_fts_segs=self.select_kw["max_fts_segs"])
        if o.relocalize == "device":
            grec, T_carried, rs.gate_dev = self.backend.track_gate(mode=abi.GATE_RELOC if fr.reloc else abi.GATE_TRACK, T_reset=T_reset,
                                                                   **({} if rs.obs_resident and fr.map_job is None else dict(num_obs_last=rs.obs_last)), **gk)
            fr.gate = (int(grec["result"]), int(grec["tracking_quality"]))
        else:
            g_result, g_quality, reset = track_gate_host(frame_sel["n_matches"], frame_sel["n_ls_matches"], pr.num_obs_pt, pr.num_obs_ls, *rs.obs_last,
                                                        relocalizing=fr.reloc, **gk)
            fr.gate, T_carried = (int(g_result), int(g_quality)), np.array(T_reset, float) if reset else pr.T.copy()
        rs.obs_last, rs.obs_resident = (int(frame_sel["n_matches"]), int(frame_sel["n_ls_matches"])), True
        fr.bad_quality = fr.gate[1] == abi.TRACKING_BAD
        if fr.gate[0] == abi.GATE_OK:
            return None
        rec = self.record(fr, np.asarray(T_carried, float).copy(), pr.cov.copy(), fr.ar.n_tracked, (int(fr.pt_ok.sum()), int(fr.seg_ok.sum())),
                          (int(pr.pt_keep.sum()), int(pr.seg_keep.sum())), gate=fr.gate)
        self.T_prev, rs.stage, rs.next_align = rec["T"].copy(), "reloc", None      # the next frame relocalises
        return rec

    def tracked(self, k, fr):
        """the frame is tracked: its pose and keep masks, the features the next frame is aligned from, its record"""
        pr, px_new, n_pts, n_seg = fr.pr, fr.px_new, self.n_pts, self.n_seg
        fr.T = pr.T.copy()
        fr.pt_keep, fr.seg_keep = pr.pt_keep.astype(bool), pr.seg_keep.astype(bool)
        if fr.sel_mask is not None:
            fr.pt_keep = fr.pt_keep[fr.sel_mask]
        fr.kept, skept = fr.pt_i[fr.pt_keep], fr.seg_i[fr.seg_keep]
        self.prev = dict(pt_idx=fr.kept, pt_px=px_new[fr.kept], seg_idx=skept, seg_spx=px_new[n_pts + skept], seg_epx=px_new[n_pts + n_seg + skept])
        self.T_prev = fr.T
        rec = self.record(fr, fr.T.copy(), pr.cov.copy(), fr.ar.n_tracked, (int(fr.pt_ok.sum()), int(fr.seg_ok.sum())), (int(fr.pt_keep.sum()), int(fr.seg_keep.sum())), gate=fr.gate, n_ties=fr.n_ties)
        self.rs.stage = "default"                      # "Relocalization successful."
        return rec

    def decide_keyframe_host(self, k, fr):
        """kf_select without keystage: scene depth, needNewKf against the overlap keyframes -- measured, like the reference, from the
        PREVIOUS frame's pose --, the frame's five key points (plsvo_keyframe_decide, :351-358, :396).  A frame plays the
        keyframe when needNewKf says so instead of every kf_every-th; the keyframe table (_Keyframes) grows with it.
        Without map_candidates the keyframes that overlap the aligned frame are found here (the head of reprojectMap: it runs before the
        matching, which then takes its candidates from keyframe 0 either way, so the call's place does not matter)."""
        if not self.o.map_candidates:
            fr.close = self.backend.close_keyframes(self.kfs.close_job(fr.T_k, self.o.max_n_kfs))
        skept = fr.seg_i[fr.seg_keep]
        dec = fr.dec = self.kfs.decide(fr.T, fr.T_last, fr.px_new[fr.kept], self.P3[fr.kept], self.seq["seg_spos"][skept], self.seq["seg_epos"][skept],
                                       fr.close["close_idx"][:fr.close["n_overlap"]])
        fr.is_kf = bool(dec["need_new_kf"])
        fr.rec.update(is_kf=fr.is_kf, n_overlap=fr.close["n_overlap"], depth_mean=dec["depth_mean"])
        if fr.is_kf:
            self.kfs.add_keyframe(fr.T, dec["key_pts"], self.P3[fr.kept])
            self.kfs.depth_from(dec)

    def structure_resident(self, k, fr):
        """structopt_resident: step 5 runs on the resident tables (plsvo_candidates_optimize_structure) in place of the
        gather / structure_optimize / map_set_positions of structure_host: one call on EVERY tracked frame, behind the pose optimiser
        and ahead of an insertion as in processFrame (:340 before :358), points and segments, with the resident keep masks and
        frame_id = k.  The harness takes the moved positions for its own tables from the call's report and follows the keys from it, to
        carry them over a restage.  record_candidates: rec["structopt"] holds the tables and the keys before, the selection, the masks,
        the report, and both after."""
        mt, rec = self.mt, fr.rec
        cm, so_keys = mt.cm, mt.so_keys
        for name, n_rows in (("pt", len(cm["pt_pos"])), ("seg", len(cm["seg_spos"]))):
            so_keys[name] += [0] * (n_rows - len(so_keys[name]))
        before = (copy.deepcopy(cm), copy.deepcopy(so_keys)) if self.o.record_candidates else None
        so = self.backend.map_optimize_structure(k)
        for row, p in zip(so["pt_lm"], so["pt_pos"]):
            cm["pt_pos"][int(row)] = [float(x) for x in p]
            so_keys["pt"][int(row)] = k
            if mt.row_lm[int(row)] >= 0:
                self.P3[mt.row_lm[int(row)]] = p
        for row, a, b in zip(so["seg_lm"], so["seg_spos"], so["seg_epos"]):
            cm["seg_spos"][int(row)], cm["seg_epos"][int(row)] = [float(x) for x in a], [float(x) for x in b]
            so_keys["seg"][int(row)] = k
        rec.update(n_structopt_pt=int(so["n_sel_pt"]), n_structopt_seg=int(so["n_sel_seg"]))
        if self.o.record_candidates:
            rec["structopt"] = dict(stream=before[0], keys_before=before[1], select=fr.frame_sel, pt_keep=fr.pr.pt_keep.copy(), seg_keep=fr.pr.seg_keep.copy(), frame_id=k, report=so,
                                    tables=copy.deepcopy(cm), keys=copy.deepcopy(so_keys))

    def decide_keyframe(self, k, fr):
        """keystage: the keyframe decision behind the structure optimisation (src/frame_handler_mono.cpp:340 before :351), on the
        selection with the keep masks as alive and the landmark positions as the tables hold them now; key_pts are indices in selection
        order.  "device": on the resident selection (plsvo_candidates_keyframe_decide); "host": the synchronous keyframe_decide on
        gathered arrays.  The two differ in transport alone and agree in every record.  The records gain overlap, the list itself, and a
        keyframe's record key_pts_new, the frame's key_pts_ as it becomes a keyframe.  (!needNewKf || TRACKING_BAD: no keyframe, :352)"""
        o, cm, frame_sel, close = self.o, self.mt.cm, fr.frame_sel, fr.close
        if o.keystage == "device":
            dec = self.backend.map_keyframe_decide(fr.T_last, o.kfselect_mindist_t, o.kfselect_mindist_r)
        else:
            dec = self.backend.keyframe_decide(abi.KeyframeDecideJob(self.cam, fr.T, fr.T_last, frame_sel["pt_px"], _rows_of(cm["pt_pos"], frame_sel["pt_lm"]), fr.pr.pt_keep,
                                                                     _rows_of(cm["seg_spos"], frame_sel["seg_lm"]), _rows_of(cm["seg_epos"], frame_sel["seg_lm"]), fr.pr.seg_keep,
                                                                     np.array(cm["kf_T"], float).reshape(-1, 7), close["close_idx"][:close["n_overlap"]], (-1,) * 5,
                                                                     o.kfselect_mindist_t, o.kfselect_mindist_r))
        fr.dec, fr.is_kf = dec, bool(dec["need_new_kf"]) and not fr.bad_quality
        fr.rec.update(is_kf=fr.is_kf, n_overlap=close["n_overlap"], depth_mean=dec["depth_mean"], overlap=_overlap_of(close))
        if fr.is_kf:
            fr.rec["key_pts_new"] = [int(h) for h in dec["key_pts"]]
            self.kfs.depth_from(dec)

    def insert_keyframe(self, k, fr):
        """kf_insert: a keyframe no longer restages: the frame joins the RESIDENT tables on the device (plsvo_candidates_insert_keyframe,
        DESIGN.md 3.13) with the resident pose and keep masks; when the table holds max_n_kfs keyframes the one keyframe_decide names as
        the furthest is removed in the same call (kf_select; the first row when it names none).  The harness brings its own tables up to
        date from the backend's fetch, sends structure-optimised positions with map_set_positions (structure_host), and stages only at
        the start and when a seed converges into a NEW candidate.  keystage "host": the key-point rows close up, the new keyframe's row
        is the decision's, holders lost to the removal are replaced (n_kp_rebuilt counts the rows rebuilt in the frame).  A removal is
        passed on to the resident seed lists (plsvo_seeds_keyframe); when it takes frame 0's keyframe out, the seeds that are left leave
        the device with it -- their keyframe is no longer in the table, image seeds included -- and the harness goes on following them
        on the host, outside the map.  record_candidates: rec["insert"] holds the tables and the quality before, the selection, the
        masks, the pose, and all three after."""
        o, mt, rows, rec, backend = self.o, self.mt, self.rows, fr.rec, self.backend
        remove = -1
        if self.kf_select and len(mt.cm["kf_T"]) >= o.max_n_kfs:
            remove = max(int(fr.dec["furthest_kf"]), 0)
            if not o.keystage:
                self.kfs.remove(remove)
            mt.keyframe_removed(remove)
        before = (copy.deepcopy(mt.cm), mt.quality) if o.record_candidates else None
        tables, mt.quality, ins = backend.map_insert(remove, k)
        mt.adopt(tables)
        if o.keystage == "host":
            self.kp_tab, n_rebuilt = _key_point_upkeep(mt.cm, [r for j, r in enumerate(self.kp_tab) if j != remove] + [[int(h) for h in fr.dec["key_pts"]]], self.cam)
            fr.kp_frame += n_rebuilt
        if rows.on_device and o.image_seeds and mt.seed_kf is not None:
            rec["n_image_seeds_started"] = self.start_image_seeds(k, fr, remove, ins)
        elif rows.on_device and remove >= 0:
            backend.seeds_keyframe(removed_kf=remove)
            rows.rows, rows.on_device = [], mt.seed_kf is not None
        rec.update(n_joined=ins["n_joined_pt"] + ins["n_joined_seg"], n_deleted_kf=ins["n_deleted_pt"] + ins["n_deleted_seg"], remove_kf=remove)
        if o.keystage == "host":
            rec["n_kp_rebuilt"] = int(fr.kp_frame)
        if o.align and o.compact and k + 1 < self.n_frames:
            self.rs.next_align = self.align_job_of(k, fr)    # ahead of the compaction, which renumbers the rows the selection points at
        if o.compact:
            tables = self.compact_tables(k, fr)
        if o.record_candidates:
            rec["insert"] = dict(stream=before[0], quality_before=before[1], select=fr.frame_sel, pt_keep=fr.pr.pt_keep.copy(), seg_keep=fr.pr.seg_keep.copy(), T=[float(v) for v in fr.T],
                                 slot=k, remove_kf=remove, tables=tables, quality=mt.quality, report=ins)

    def start_image_seeds(self, k, fr, remove, ins):
        """image_seeds="host" | "device": at a keyframe whose seed tables are on the device the image's corners become point seeds of the
        RESIDENT lists (DepthFilter::initializeSeeds' creating half), behind the insertion: the removal, then the corners
        of the frame's free cells, with the cells of the frame's selected features and of the last update's matches occupied.  "device"
        is plsvo_seeds_keyframe_detect with both occupancy sources; "host" does the same with the calls there were before --
        detect_corners on an occupancy built from the fetched selection and the fetched rows by the same rule, seeds_from_corners,
        seeds_keyframe(pt_..) -- so the two differ in transport alone and agree in every record and in the lists.  These seeds have no
        landmark of the synthetic map: the harness keeps, per resident row, the landmark of a map seed or -1 (_SeedRows) and follows
        removals and erasures through the rows and the reports.  -> the seeds started"""
        o, backend, rows, img_kw = self.o, self.backend, self.rows, self.img_kw
        new_kf = len(self.mt.cm["kf_T"]) - 1
        assert ins.get("new_kf", new_kf) == new_kf and self.mt.cm["kf_slot"][new_kf] == k
        ev = dict(removed_kf=remove, new_batch=True, new_kf=new_kf, depth_mean=self.kfs.seed_depth[0], depth_min=self.kfs.seed_depth[1])
        if o.image_seeds == "device":
            backend.seeds_keyframe_detect(o.detect_cell_size, o.n_pyr_levels, img_kw["detection_threshold"], fast_threshold=img_kw["fast_threshold"],
                                          occ_sources=abi.SEED_OCC_SELECTED | (abi.SEED_OCC_UPDATED if rows.last_rows is not None else 0), **ev)
            kf_rep = backend.seeds_keyframe_fetch()
            assert not kf_rep["no_room"]
            n_started = kf_rep["n_new_pt"]
        else:
            marking = np.zeros((0, 2))
            if rows.last_rows is not None:
                stl = rows.last_rows["pt_status"]
                marking = rows.last_rows["pt_px_cur"][(stl == abi.SEED_UPDATED) | (stl == abi.SEED_CONVERGED) | (stl == abi.SEED_NAN)]
            occ = _occupancy(np.concatenate([fr.frame_sel["pt_px"].reshape(-1, 2), marking]), self.w_img, self.h_img, o.detect_cell_size)
            corners = backend.detect_corners(k, occ, o.detect_cell_size, o.n_pyr_levels, img_kw["detection_threshold"], fast_threshold=img_kw["fast_threshold"])
            sdn = seeds_from_corners(corners, self.cam, *self.kfs.seed_depth)
            backend.seeds_keyframe(pt_px=sdn["px"], pt_f=sdn["f"], pt_level=sdn["level"], pt_type=sdn["type"], pt_grad=sdn["grad"], **ev)
            n_started = len(corners)
        if remove >= 0:
            rows.remove_keyframe(remove)
        if n_started:
            rows.started(n_started, new_kf, backend.seeds_fetch_lists())
        return int(n_started)

    def compact_tables(self, k, fr):
        """compact="room" | "always": behind every keyframe's insertion the resident tables close up over their deleted POINT rows on the
        device (plsvo_candidates_compact; Map::emptyTrash: the deleted rows leave, the rows behind them move down) --
        "always" at every keyframe, "room" only when fewer rows are free than seeds are alive, decided on the device.  The harness takes
        the tables from the backend's fetch and applies the remap to its row <-> landmark maps and to the keys it follows.  The segments
        have no reserve here (no segment seed exists) and are never compacted.  Stable order is kept, so every pose, covariance and
        count equals those of the run with the full reserve.  -> the fetched tables"""
        alive = len(self.seeds["idx"]) + self.rows.n_image()
        tables, self.mt.quality, cp = self.backend.map_compact("room", (1 << 30) if self.o.compact == "always" else alive, 0)
        if cp["ran_pt"]:
            self.mt.adopt(tables)
            self.mt.apply_pt_remap(cp["pt_remap"])
        fr.rec["n_compacted_pt"] = int(cp["n_pt_before"] - cp["n_pt_after"])
        return tables

    def join_keyframe_host(self, k, fr):
        """map_candidates without kf_insert: the frame joins the keyframe table of the harness's own tables, which are restaged: its
        features, and an observation at the FRONT of every landmark's list (Feature3D::addFrameRef pushes at the front,
        include/plsvo/feature3D.h:204); a candidate it matched leaves the map's candidate list for the keyframe's features (a candidate
        that joins a keyframe: TYPE_UNKNOWN)"""
        cm, cam, px_new, level, n_pts, n_seg, kept = self.mt.cm, self.cam, fr.px_new, fr.level, self.n_pts, self.n_seg, fr.kept
        skept = fr.seg_i[fr.seg_keep]
        kf_id = len(cm["kf_T"])
        cm["kf_T"].append(_f3(fr.T)); cm["kf_slot"].append(k)
        cm["kf_pt"].append([int(i) for i in kept]); cm["kf_seg"].append([int(i) for i in skept])
        for i, brg in zip(kept, _bearing(cam, px_new[kept])):
            cm["pt_obs"][int(i)].insert(0, dict(kf=kf_id, px=_f3(px_new[i]), f=_f3(brg), level=int(level[i]), type=abi.FTR_CORNER, grad=[0.0, 0.0]))
            if not self.o.cell_select or cm["pt_type"][int(i)] == abi.LM_CANDIDATE:
                cm["pt_type"][int(i)] = abi.LM_UNKNOWN
        for i, sb, eb in zip(skept, _bearing(cam, px_new[n_pts + skept]), _bearing(cam, px_new[n_pts + n_seg + skept])):
            cm["seg_obs"][int(i)].insert(0, dict(kf=kf_id, spx=_f3(px_new[n_pts + i]), epx=_f3(px_new[n_pts + n_seg + i]), sf=_f3(sb), ef=_f3(eb), level=int(level[n_pts + i])))
        matched = set(int(v) for v in kept)
        cm["pt_cand"] = [i for i in cm["pt_cand"] if i not in matched]
        self.mt.dirty = True

    def structure_host(self, k, fr):
        """5. structure optimisation at a keyframe (FrameHandlerBase::optimizeStructure: the 20 least recently refined, :202-237) of the
        kept point landmarks with >= 2 observations; the moved positions go to the resident tables (kf_insert: map_set_positions, in
        rows) or wait for the restage"""
        o, P3 = self.o, self.P3
        cand = np.array([i for i in fr.kept if len(self.obs[int(i)]) >= 2], np.int64)
        if not (len(cand) and fr.is_kf and not o.structopt_resident):
            return
        refine = cand[np.argsort(self.last_optim[cand], kind="stable")[:20]]
        off, ofr, of_ = [0], [], []
        for i in refine:
            for fr_, brg in self.obs[int(i)]:
                ofr.append(fr_)
                of_.append(brg)
            off.append(len(ofr))
        z3, zi = np.zeros((0, 3)), np.zeros(0, np.int32)
        so = self.backend.structure_optimize(abi.StructOptJob(np.stack(self.poses_est), P3[refine], off, ofr, np.array(of_), z3, z3, np.zeros(1, np.int32), zi, z3, z3, 5, 5))
        P3[refine] = so["pt_pos"]
        self.last_optim[refine] = k
        if o.kf_insert:
            self.backend.map_set_positions(self.mt.row_of_lm(refine).astype(np.int32), P3[refine])
            for i in refine:
                self.mt.cm["pt_pos"][int(self.mt.lm_row[i])] = [float(x) for x in P3[i]]
        elif o.map_candidates:
            self.mt.dirty = True

    def update_seeds(self, k, fr):
        """6. depth-filter update of the seeds with this frame (DepthFilter::updateSeeds, depth_filter.cpp:262); a converged seed turns
        into a landmark.  On the resident lists (seeds_resident) the report and the update's rows come back, no record travels; with
        image_seeds they hold seeds from the image beside the map's, which are the rows with a landmark, in the order of seeds["idx"].
        n_seed_candidates counts the converged seeds whose keyframe, frame 0's, is still in the table."""
        o, seq, rows, seeds, rec = self.o, self.seq, self.rows, self.seeds, fr.rec
        ns, si_ = len(seeds["idx"]), seeds["idx"]
        img_dev = bool(o.image_seeds) and rows.on_device
        if not (ns or (img_dev and rows.rows)):
            return
        all_rows = report = quality = None
        if rows.on_device:
            report, sr, quality = self.backend.seeds_update(k, fr.T)
            assert len(sr["pt_status"]) == (len(rows.rows) if img_dev else ns) and report["no_room"] == 0
            if img_dev:
                all_rows, is_map = sr, rows.lms() >= 0
                rows.last_rows = dict(pt_status=sr["pt_status"].copy(), pt_px_cur=sr["pt_px_cur"].copy())
                assert np.array_equal(rows.lms()[is_map], si_)
                sr = {f: v[is_map] for f, v in sr.items() if f.startswith("pt_")}
        else:
            ptd = dict(ref_frame=np.zeros(ns, np.int32), cur_frame=np.ones(ns, np.int32), px=seq["pt_px0"][si_], f=seq["pt_f0"][si_], level=np.zeros(ns, np.int32),
                       a=seeds["a"], b=seeds["b"], mu=seeds["mu"], z_range=seeds["z_range"], sigma2=seeds["sigma2"])
            sr = self.backend.update_seeds(abi.SeedsJob(self.cam, np.stack([self.kf_T, fr.T]), np.array([0, k], np.int32), ptd, None, n_pyr_levels=o.n_pyr_levels))
        stt = sr["pt_status"]
        conv = stt == abi.SEED_CONVERGED
        self.P3[si_[conv]] = sr["pt_xyz_world"][conv]
        self.known[si_[conv]] = True
        in_table = conv.any() and o.map_candidates and self.mt.seed_kf is not None
        if img_dev:
            self.converged_rows_join(fr, all_rows, report, quality)
        elif o.seed_candidates and in_table:
            self.converged_seeds_join(fr, [int(i) for i in si_[conv]], sr["pt_xyz_world"][conv], report, quality)
        elif in_table:
            for i in si_[conv]:
                self.mt.append_candidate(None, self.mt.seed_kf, seq["pt_px0"][i], seq["pt_f0"][i], 0, [0.0, 0.0], int(i), own_row=True)
        keep_s = ~(conv | (stt == abi.SEED_NAN))
        self.seeds = dict(idx=si_[keep_s], a=sr["pt_a"][keep_s], b=sr["pt_b"][keep_s], mu=sr["pt_mu"][keep_s], z_range=seeds["z_range"][keep_s], sigma2=sr["pt_sigma2"][keep_s])
        rec["n_seed_converged"] = int(conv.sum())
        if o.kf_insert:
            rec["n_seed_candidates"] = int(conv.sum()) if self.mt.seed_kf is not None else 0

    def converged_rows_join(self, fr, all_rows, report, quality):
        """image_seeds: every converged row of the resident lists, from the map or from the image, is a new landmark row of the resident
        tables, in list order; a converged image seed gets a table row of its own without a landmark (such rows are selected, optimised
        and inserted on the device like any other; the harness's own alignment and structure optimisation leave them out)"""
        seq, rows, mt = self.seq, self.rows, self.mt
        status = all_rows["pt_status"]
        for j, r in enumerate(np.nonzero(status == abi.SEED_CONVERGED)[0]):
            lm, kf, ftr = rows.rows[r]
            if lm >= 0:
                ftr = dict(px=seq["pt_px0"][lm], f=seq["pt_f0"][lm], level=0)
            else:
                rows.n_image_converged += 1
            row = mt.append_candidate(all_rows["pt_xyz_world"][r], kf, ftr["px"], ftr["f"], ftr["level"], [0.0, 0.0] if lm >= 0 else [1.0, 0.0], lm)
            assert row == report["first_pt"] + j
            mt.quality = quality
        rows.drop(status)
        fr.rec.update(n_image_seeds=rows.n_image(), n_image_seeds_converged=rows.n_image_converged)

    def converged_seeds_join(self, fr, lms, pos, seed_report, seed_quality):
        """seed_candidates: a converged seed whose keyframe is still in the table joins the RESIDENT tables on the device as a new landmark
        row with one observation and an entry at the back of the candidate list (newCandidatePoint; plsvo_candidates_add, DESIGN.md
        3.14) instead of marking the tables for a restage, so the stage is called once, at the first frame; the harness appends the same
        row to its own tables.  With seeds_resident the update's commit has appended them already: its report stands in for the add's,
        from which the harness keeps its own tables exactly as it does from an add's.  A seed that converges after frame 0's keyframe
        was removed stays outside the map's tables.  record_candidates: rec["add"] holds the tables and the quality before, the new
        records, the tables and the quality after, and the backend's report."""
        seq, mt, n = self.seq, self.mt, len(lms)
        new = dict(pt_pos=pos, pt_obs_kf=np.full(n, mt.seed_kf, np.int32), pt_obs_px=seq["pt_px0"][lms], pt_obs_f=seq["pt_f0"][lms],
                   pt_obs_level=np.zeros(n, np.int32), pt_obs_type=np.full(n, abi.FTR_CORNER, np.uint8), pt_obs_grad=np.zeros((n, 2)))
        before = (copy.deepcopy(mt.cm), mt.quality) if self.o.record_candidates else None
        if self.rows.on_device:
            report = dict(first_pt=seed_report["first_pt"], first_seg=-1, n_added_pt=n, n_added_seg=0, n_pt=seed_report["n_pt"], n_seg=seed_report["n_seg"],
                          n_pt_cand=seed_report["n_pt_cand"], n_seg_cand=seed_report["n_seg_cand"], n_pt_obs=seed_report["n_pt_obs"], n_seg_obs=seed_report["n_seg_obs"])
            mt.quality = seed_quality
        else:
            report, mt.quality = self.backend.map_add_candidates(new)
        for j, i in enumerate(lms):
            assert mt.append_candidate(self.P3[i], mt.seed_kf, seq["pt_px0"][i], seq["pt_f0"][i], 0, [0.0, 0.0], i) == report["first_pt"] + j
        if self.o.record_candidates:
            fr.rec["add"] = dict(stream=before[0], quality_before=before[1], new=new, tables=copy.deepcopy(mt.cm), quality=mt.quality, report=report)

    def new_image_seeds(self, frame, feature_px):
        """detect: the corner detector on the frame's own pyramid slot with the cells of the features it tracks marked occupied
        (DepthFilter::initializeSeeds); the corners become point seeds (seeds_from_corners)"""
        o = self.o
        corners = self.backend.detect_corners(frame, _occupancy(feature_px, self.w_img, self.h_img, o.detect_cell_size), o.detect_cell_size, o.n_pyr_levels)
        sd = seeds_from_corners(corners, self.cam, *self.kfs.seed_depth)
        sd["ref_frame"] = np.full(len(corners), frame, np.int32)
        return sd

    def image_seeds_host(self, k, fr):
        """7. detect=True: the seeds that came from the image are updated with this frame next to the map's own; every keyframe, frame 0
        included, adds those of its own free cells (new_image_seeds).  These seeds come from the image alone and are not added to the
        map, whose landmarks carry the truth."""
        ni = len(self.img_seeds["px"])
        if ni:
            sr = self.backend.update_seeds(abi.SeedsJob(self.cam, np.stack(self.poses_est), np.arange(len(self.poses_est), dtype=np.int32),
                                                        dict(self.img_seeds, cur_frame=np.full(ni, k, np.int32)), None, n_pyr_levels=self.o.n_pyr_levels))
            stt = sr["pt_status"]
            self.img_converged += int((stt == abi.SEED_CONVERGED).sum())
            keep_s = ~((stt == abi.SEED_CONVERGED) | (stt == abi.SEED_NAN))
            self.img_seeds = {key: v[keep_s] for key, v in self.img_seeds.items()}
            for key in ("a", "b", "mu", "sigma2"):
                self.img_seeds[key] = sr["pt_" + key][keep_s]
        if fr.is_kf:
            fresh = self.new_image_seeds(k, fr.px_new[fr.kept])
            self.img_seeds = {key: np.concatenate([v, fresh[key]]) for key, v in self.img_seeds.items()}
        fr.rec.update(n_image_seeds=len(self.img_seeds["px"]), n_image_seeds_converged=self.img_converged)

    def align_job_of(self, k, fr):
        """frame k + 1's alignment job from frame k's selection and the tables as they stand at this point of frame k.  "device" builds
        it there (plsvo_candidates_align_build .. _compose, DESIGN.md 3.20: no selection fetch, no pose fetch, no host arithmetic ahead
        of the alignment; -> True); "host" restates the same job here in scalar float64 (align_job_host), so the two differ in
        transport alone and agree in every record"""
        o, cm, pr = self.o, self.mt.cm, fr.pr
        if o.align == "device":
            self.backend.align_build(k, k + 1, o.max_level, o.min_level, *self.align_caps)
            return True
        return align_job_host(self.cam, o.max_level, o.min_level, fr.frame_sel, pr.pt_keep, pr.seg_keep, cm["pt_type"], cm["seg_type"], cm["pt_pos"], cm["seg_spos"], cm["seg_epos"],
                              pr.T, k, k + 1)

    def queue_next_align(self, k, fr):
        """align="host" | "device": step 1 of every frame but the first is fed by the frame before it: the features of the alignment job
        are the previous frame's SELECTION with the pose optimiser's keep masks, the landmarks' positions and types as the tables hold
        them when that frame is done -- behind the structure optimisation and an insertion, behind everything that moves a landmark in
        the frame, ahead of a compaction (insert_keyframe queues it there) --, the reference pose the optimised one.  Tables that wait
        for a restage no longer say what the harness's own do: the frame behind them is staged by the host as without the flag."""
        if self.o.align and self.rs.next_align is None and k + 1 < self.n_frames and not self.mt.dirty:
            self.rs.next_align = self.align_job_of(k, fr)


def pose_errors(result, seq):
    """(rotation error [rad], translation error [m]) per frame against the true poses"""
    return [synth.se3_log_angle_dist(r["T"], T) for r, T in zip(result, seq["poses_true"])]
