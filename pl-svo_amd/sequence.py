"""A minimal frame-to-frame harness over the widened hot path, in the order FrameHandlerMono::processFrame runs it
(src/frame_handler_mono.cpp:266-340):

    sparse image alignment (previous frame -> new frame)        plsvo_sparse_align
    reprojection of the map into the new frame                  plsvo_reproject
    direct feature matching against the keyframe observations   plsvo_match_direct
    motion-only pose optimisation on the matches                plsvo_pose_optimize
    trajectory record (TUM line of T_f_w^-1)                    plsvo_trajectory_record

on a synthetic sequence with a known map (a textured plane carrying point and line-segment landmarks, observed in
keyframe 0).  It exists to exercise the entry points chained the way the reference chains them and to emit trajectory
files in the reference harness's format; it is not a VO system: the map is given, and its maintenance (candidate
lists, keyframe removal) is not part of it.

With mapping=True two more steps run per frame, again as processFrame / the depth-filter thread order them:

    structure optimisation of the 20 least recently refined landmarks   plsvo_structure_optimize   (:340)
    depth-filter update of the seeds with the new frame                  plsvo_update_seeds         (depth_filter.cpp:262)

starting from a map that knows only part of the landmarks (with noisy positions) and holds the rest as seeds that turn
into landmarks when they converge.

With kf_select=True (and mapping) the keyframe stage of processFrame runs on the device too (:351-358, :396):

    keyframes that overlap the aligned frame, before matching           plsvo_close_keyframes      (reprojector.cpp:147-163)
    scene depth, new-keyframe test, the frame's five key points          plsvo_keyframe_decide

A frame then plays the keyframe when needNewKf says so -- measured, like the reference, from the PREVIOUS frame's pose -- instead of
every kf_every-th; the keyframe table (pose and the landmark positions of the five key points) grows with it, and the seeds of a
keyframe's corners start from depth_mean * 2.0 and 0.1 * depth_min of that call (:391).

With map_candidates=True (a per-call backend with map_candidates) steps 2 and 3 take their candidates and reference observations from the
map-candidate stage (plsvo_candidates_*) instead of keyframe 0: the harness keeps the map tables the stage needs -- the
keyframes' feature lists, every landmark's observation list with px / f / level, newest first -- restages them when they change (a frame
becomes a keyframe, a seed converges into the map's candidate list), and hands each frame its pose and its overlap list: the one of
plsvo_close_keyframes with kf_select, otherwise every keyframe in table order.  The matches reach the pose optimiser in landmark-index
order, as without it.

With cell_select=True on top of it (a backend with map_select) the second half of Reprojector::reprojectMap runs on the device as well
(plsvo_candidates_select): one candidate per grid cell in place of every found match, the landmark quality
(n_failed_reproj_ / n_succeeded_reproj_, promotions, deletions) kept resident from frame to frame, and the pose optimiser fed on the
device.  The harness follows the types, the candidate lists and the deletions in its own tables from fetch_quality, restages only when
the map changes at a keyframe (or a seed converges), and carries the counters over a restage with fetch_quality / set_quality.  With
kf_insert=True on top of that (a backend with map_insert) a keyframe no longer restages: the frame joins the resident tables on the device
(plsvo_candidates_insert_keyframe), the harness takes its own tables from the backend's fetch, moved landmarks go through
map_set_positions, and only a seed that converges into a NEW candidate stages again.  With seed_candidates=True on top of that (a
backend with map_add_candidates) that last restage goes too: the converged seed is appended to the resident tables on the device
(plsvo_candidates_add) as a new landmark row with one observation and an entry at the back of the candidate list, and the
stage is called once, at the first frame.  The
features reach the pose optimiser in selection order; a segment that won both of its cells is a feature twice.  With
structopt_resident=True (cell_select, a backend with map_optimize_structure) the structure optimisation runs on the resident tables too
(plsvo_candidates_optimize_structure): one call on every tracked frame, points and segments, ahead of an insertion; the
harness takes the moved positions and the keys from the call's report.

With align="host" | "device" (map_candidates and cell_select) step 1 of every frame but the first is fed by the frame before it: the features of the
alignment job are the previous frame's SELECTION with the pose optimiser's keep masks, the landmarks' positions and types as the tables
hold them when that frame is done -- behind the structure optimisation and an insertion, ahead of a compaction --, the reference pose the
optimised one; the first frame, and a frame behind one whose tables wait for a restage, are staged by the host as without it.  "device" builds that job on the device (plsvo_candidates_align_build .. _compose, DESIGN.md 3.20: no selection fetch, no
pose fetch, no host arithmetic ahead of the alignment) and hands the composed pose on by device pointer; "host" restates the same job here
in scalar float64 and stages it through plsvo_align_stage, so the two differ in transport alone and agree in every record.

With relocalize="host" | "device" (align and keystage) the harness plays the reference's stage machine: the gates of
processFrame stand behind every frame's pose optimisation, a frame that fails them is carried forward with the pose the gate gives and
the next frame relocalises against the closest keyframe of the resident tables (relocalizeFrame) until a frame passes the gates again.

`backend` is duck-typed: load_frames(list of level-0 images; HipBackend also takes raw frames with rectify=), sparse_align(job), reproject(job), match_direct(job),
pose_optimize(job), for mapping structure_optimize(job), update_seeds(job), and for kf_select close_keyframes(job), keyframe_decide(job).  The product backend is HipBackend (C ABI on the GPU, no fallback); tests pass an oracle-backed one
to check the whole chain end to end."""
import copy
import math

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
    """-> list of per-frame dicts (pose T_f_w, cov, counts).  Frame 0 is the keyframe with the true pose.
    mapping=True: only `known_frac` of the point landmarks start in the map (positions off by `pos_noise` x depth along
    their viewing ray), the others are depth-filter seeds; the seed update runs every frame; every `kf_every`-th frame
    plays the keyframe: its matches become observations of their landmarks (Feature3D::obs_ grows at keyframes only, as
    in the reference) and the 20 least recently refined landmarks with >= 2 observations are structure-optimised.
    detect=True (with mapping, a backend with detect_corners): every keyframe, frame 0 included, also runs the corner detector on its
    own pyramid slot with the cells of the features it tracks marked occupied (DepthFilter::initializeSeeds), and the corners become
    point seeds (seeds_from_corners) that the following frames update next to the map's own; the records gain n_image_seeds /
    n_image_seeds_converged.  These seeds come from the image alone and are not added to the map, whose landmarks carry the truth.
    kf_select=True (with mapping, a backend with close_keyframes / keyframe_decide): the keyframe stage decides which frames play the
    keyframe (module docstring); the records gain is_kf, n_overlap, depth_mean.
    map_candidates=True (a backend with map_candidates, not the resident chain): candidates and reference observations come from the
    map-candidate stage (module docstring); the records gain n_filed_pt / n_filed_seg and ref_kf_hist, how many of the filed landmarks
    took their reference observation from each keyframe of the table.  record_candidates=True also keeps each frame's stage inputs and
    result in rec["candidates"] (tests).
    cell_select=True (with map_candidates, a backend with map_select): the cell selection and the resident pose optimiser take the place
    of "every found match" and the per-call pose optimiser (module docstring); select_params: keyword arguments of
    capi.Context.candidates_select (default: max_fts 120, max_fts_segs 100, cells in index order).  The records gain n_trials and
    n_promoted / n_deleted; rec["candidates"] gains the selection and the quality state before and after the frame.
    kf_insert=True (with cell_select, a backend with map_insert): a keyframe is inserted into the resident tables on the device
    (plsvo_candidates_insert_keyframe) with the resident pose and keep masks; when the table holds max_n_kfs keyframes the
    one keyframe_decide names as the furthest is removed in the same call (kf_select; the first row when it names none).  The harness
    brings its own tables up to date from the backend's fetch, sends structure-optimised positions with map_set_positions, and stages
    only at the start and when a seed converges into a NEW candidate -- observed in frame 0's keyframe, whose row the harness follows through
    the removals; a seed that converges after that keyframe was removed stays outside the map's tables (n_seed_candidates counts the
    others).  The keyframe records gain n_joined / n_deleted_kf / remove_kf, and
    with record_candidates rec["insert"]: the tables and the quality before, the selection, the masks, the pose, and all three after.
    seed_candidates=True (with kf_insert, a backend with map_add_candidates): a converged seed whose keyframe is still in the table is
    appended to the resident tables on the device (plsvo_candidates_add) instead of marking the tables for a restage; the
    harness appends the same row to its own tables.  The seed's table row is then a NEW one behind the staged rows, no longer its landmark
    index: the harness keeps the row of every landmark and the landmark of every row, and translates wherever the backend speaks in rows
    (filed and selected landmarks, moved positions).  With record_candidates rec["add"] holds the tables and the quality before, the new
    records, the tables and the quality after, and the backend's report.
    seeds_resident=True (with seed_candidates, a backend with seeds_stage): the map's seeds are staged ONCE, beside the map tables, and are
    updated, erased and handed over to the resident tables on the device (plsvo_seeds_update): no seed travels per frame and
    no record comes back, only the report and the update's rows, from which the harness keeps its own tables exactly as it does from an
    add's report.  A removal at an insertion is passed on (plsvo_seeds_keyframe); when it takes frame 0's keyframe out, the seeds that
    are left leave the device with it -- their keyframe is no longer in the table -- and the harness goes on following them on the host,
    outside the map, as it does without this flag.  With the flag off every record is what it is without it.
    image_seeds="host" | "device" (with seeds_resident; default None: nothing changes): at a keyframe whose seed tables are on the device
    the image's corners become point seeds of the RESIDENT lists (DepthFilter::initializeSeeds' creating half), behind the
    insertion, with the cells of the frame's selected features and of the last update's matches occupied.  "device" is
    plsvo_seeds_keyframe_detect with both occupancy sources; "host" does the same with the calls there were before -- detect_corners on
    an occupancy built from the fetched selection and the fetched rows by the same rule, seeds_from_corners, seeds_keyframe(pt_..) --
    so the two differ in transport alone and agree in every record and in the lists.  These seeds have no landmark of the synthetic
    map: the harness keeps, per resident row, the landmark of a map seed or -1, follows removals and erasures through the rows and the
    reports, and gives a converged image seed a table row of its own without a landmark (such rows are selected, optimised and inserted
    on the device like any other; the harness's own alignment and structure optimisation leave them out).  The records gain
    n_image_seeds / n_image_seeds_converged / n_image_seeds_started.  image_seed_params: fast_threshold, detection_threshold (20, 20.0).
    When frame 0's keyframe leaves the table the resident lists are given up as without this flag, image seeds included.
    structopt_resident=True (with mapping and cell_select, a backend with map_optimize_structure): step 5 runs on the resident tables
    (plsvo_candidates_optimize_structure) in place of the gather / structure_optimize / map_set_positions of the harness:
    one call on EVERY tracked frame, behind the pose optimiser and ahead of an insertion as in processFrame (:340), points and segments,
    with the resident keep masks and frame_id = k.  The harness takes the moved positions for its own tables from the call's report and
    follows the keys from it, to carry them over a restage (map_set_last_optim).  The records gain n_structopt_pt / n_structopt_seg, and
    with record_candidates rec["structopt"]: the tables and the keys before, the selection, the masks, the report, and both after.
    With the flag off every record is what it is without it.
    compact="room" | "always" (with seed_candidates, a backend with map_compact; default None: nothing changes): behind every keyframe's
    insertion the resident tables close up over their deleted POINT rows on the device (plsvo_candidates_compact) --
    "always" at every keyframe, "room" only when fewer rows are free than seeds are alive, decided on the device.  The harness takes the
    tables from the backend's fetch and applies the remap to its row <-> landmark maps and to the keys it follows.  The segments have no
    reserve here (no segment seed exists) and are never compacted.  lm_room: landmark rows reserved per kind instead of one per seed of
    the sequence; without compaction a sequence whose converged seeds outnumber it ends in PLSVO_E_CAPACITY.  Stable order is kept, so
    every pose, covariance and count equals those of the run with the full reserve; the keyframe records gain n_compacted_pt.
    keystage="host" | "device" (with kf_select, cell_select and kf_insert; default None: every record is what it is without it): the
    keyframe stage follows the reference instead of snapshotting a key point's position when its keyframe is inserted -- Frame::key_pts_
    are positions in the keyframes' feature lists, a key point's position is its landmark's position in the tables NOW
    (Map::getCloseKeyframes, src/map.cpp:165-169), a key point whose landmark is deleted is replaced (Map::safeDeletePoint ->
    Frame::removeKeyPoint, :116-123), and the decision runs behind the structure optimisation (src/frame_handler_mono.cpp:340 before
    :351) on the selection with the keep masks as alive.  "device" does it on the resident tables (plsvo_candidates_set_keypts,
    _run_close, _keyframe_decide; DESIGN.md 3.19: a backend with map_set_keypts / map_keyframe_decide); "host" does the same with the
    calls there were before: the key-point table kept here from the tables the harness follows, then the synchronous
    close_keyframes / keyframe_decide on gathered arrays.  The two differ in transport alone and agree in every record; the last record
    gains key_pts, the table at the end, every record overlap, the list itself, a keyframe's record key_pts_new, the decision's key points, and in "host" the keyframe records count the rows
    rebuilt (n_kp_rebuilt).
    align="host" | "device" (with map_candidates and cell_select; default None: every record is what it is without it): from the second
    frame on the alignment job is the previous frame's selection as the device holds it when that frame is done (module docstring,
    DESIGN.md 3.20).  "device" builds it there (a backend with align_build / align_built), runs it and passes the composed pose by device
    pointer into the candidate stage; "host" restates the same job (align_job_host) and stages it as before.  The first frame's job
    is gathered from keyframe 0 as without the flag, and so is the job of a frame behind one that left the tables waiting for a restage
    (a keyframe without kf_insert, a converged seed without seed_candidates): the resident tables are then behind the harness's own.
    The two agree in every record.
    relocalize="host" | "device" (with align and keystage; default None: every record is what it is without it): the harness plays the
    reference's stage machine, STAGE_DEFAULT_FRAME <-> STAGE_RELOCALIZING (finishFrameProcessingCommon).  Behind the pose optimisation of
    every frame stand the gates of processFrame (src/frame_handler_mono.cpp:315-321, :335, setTrackingQuality): a frame that fails is not
    structure-optimised, decided, inserted or fed to the depth filter, its pose is the one the gate carries, and the next frame
    relocalises (relocalizeFrame :408-436): Map::getClosestKeyframe from the last frame's pose, a gating alignment against that keyframe
    from the identity that must track more than 30, a second alignment from the keyframe's own pose, and the rest of processFrame, whose
    every failure carries the last frame's pose; a success returns to STAGE_DEFAULT_FRAME.  TRACKING_BAD keeps a frame from becoming a
    keyframe.  "device" uses plsvo_candidates_align_build_kf and plsvo_candidates_track_gate (a backend with align_kf /
    track_gate); "host" does the same with the calls there were before -- fetched tables, close_keyframes, align_kf_job_host staged
    through plsvo_align_stage, track_gate_host on the fetched counts.  The two differ in transport alone and agree in every record.  The
    two host waits of "device": the gate's record ahead of the structure optimisation, and n_tracked behind the gating alignment.
    reloc_params: quality_min_fts (20), quality_max_drop_fts (50); the clamps are the selection's max_fts / max_fts_segs.  The records
    gain stage (the stage the frame was processed in), gate, tracking_quality and, in a relocalising frame, reloc_kf / reloc_tracked.
    The tables must not wait for a restage while a stream relocalises (kf_insert with seed_candidates keeps them resident)."""
    params = dict(locals())                            # (first statement: exactly the arguments)
    if relocalize not in (None, "host", "device") or (relocalize and not (align and keystage and (relocalize == "host" or (keystage == "device" and hasattr(backend, "align_kf"))))):
        raise ValueError("relocalize is None, 'host' or 'device' and needs align, keystage and, for 'device', keystage='device' (the live key-point table) and a backend with align_kf() / track_gate()")
    if align not in (None, "host", "device") or (align and not (map_candidates and cell_select and (align == "host" or hasattr(backend, "align_build")))):
        raise ValueError("align is None, 'host' or 'device' and needs map_candidates, cell_select and, for 'device', a backend with align_build() / align_built()")
    if keystage not in (None, "host", "device") or (keystage and not (kf_select and cell_select and kf_insert and hasattr(backend, "map_keyframe_decide" if keystage == "device" else "keyframe_decide"))):
        raise ValueError("keystage is None, 'host' or 'device' and needs kf_select, cell_select, kf_insert and a backend with keyframe_decide() / map_keyframe_decide()")
    if compact not in (None, "room", "always") or (compact and not (seed_candidates and hasattr(backend, "map_compact"))):
        raise ValueError("compact is None, 'room' or 'always' and needs seed_candidates and a backend with map_compact()")
    if structopt_resident and not (mapping and cell_select and hasattr(backend, "map_optimize_structure")):
        raise ValueError("structopt_resident needs mapping, cell_select and a backend with map_optimize_structure()")
    if image_seeds not in (None, "host", "device") or (image_seeds and not (seeds_resident and hasattr(backend, "seeds_keyframe_detect" if image_seeds == "device" else "detect_corners"))):
        raise ValueError("image_seeds is None, 'host' or 'device', needs seeds_resident and a backend with detect_corners() / seeds_keyframe_detect()")
    if seeds_resident and not (seed_candidates and hasattr(backend, "seeds_stage")):
        raise ValueError("seeds_resident needs seed_candidates and a backend with seeds_stage()")
    if seed_candidates and not (kf_insert and hasattr(backend, "map_add_candidates")):
        raise ValueError("seed_candidates needs kf_insert and a backend with map_add_candidates()")
    if kf_insert and not (cell_select and mapping and hasattr(backend, "map_insert")):
        raise ValueError("kf_insert needs mapping, cell_select and a backend with map_insert()")
    if not kf_insert:
        return _run_sequence(**params)
    # room for every keyframe the sequence can add (a joined candidate adds a feature, every feature an observation)
    n_fr, n_lm = len(seq["images"]), len(seq["pt_pos"]) + 2 * len(seq["seg_spos"])
    backend.map_reserve(extra_kf=n_fr, extra_kf_pt=n_fr * n_lm, extra_kf_seg=n_fr * n_lm, extra_pt_obs=n_fr * n_lm, extra_seg_obs=n_fr * n_lm)
    if seed_candidates:                                # a landmark row per seed that can converge (its observation fits the room above)
        backend.map_reserve_landmarks(extra_pt=len(seq["pt_pos"]) if lm_room is None else int(lm_room), extra_seg=0 if lm_room is None else int(lm_room))
    try:
        return _run_sequence(**params)
    finally:
        backend.map_reserve()                          # the tight layout again for whoever stages next on this backend
        if seed_candidates:
            backend.map_reserve_landmarks()


def _run_sequence(backend, seq, max_level, min_level, n_pyr_levels, reproj_thresh, mapping, known_frac, pos_noise, map_seed, kf_every, detect, detect_cell_size, kf_select,
                  kfselect_mindist_t, kfselect_mindist_r, max_n_kfs, map_candidates, record_candidates, cell_select, select_params, kf_insert, seed_candidates, seeds_resident,
                  image_seeds=None, image_seed_params=None, structopt_resident=False, compact=None, lm_room=None, keystage=None, align=None, relocalize=None, reloc_params=None):
    cam = seq["cam"]
    stage, gate_dev, obs_last, obs_resident = "default", None, None, False   # relocalize: the stage, the gate's carried poses on the device, num_obs_last_pt / _ls and whether the device holds them
    gate_kw = dict(quality_min_fts=20, quality_max_drop_fts=50)
    gate_kw.update(reloc_params or {})
    IDENT = [0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]
    next_align = None                                  # align: the job of the frame to come -- an abi.AlignJob ("host") or True: built on the device
    kp_tab, kp_live = None, False                      # keystage: Frame::key_pts_ per keyframe row of cm ("host": kept here; "device": fetched when a restage needs it)
    img_kw = dict(fast_threshold=20, detection_threshold=20.0)
    img_kw.update(image_seed_params or {})
    res_lm, res_kf, res_ftr, last_rows, img_conv = [], [], [], None, 0   # image_seeds: per resident point row its landmark (-1: from the image), its keyframe row, its feature
    sel_mask = None
    seeds_on_device = False                            # seeds_resident: the seed lists are staged and their keyframe is still in the table
    if cell_select and not (map_candidates and hasattr(backend, "map_select")):
        raise ValueError("cell_select needs map_candidates and a backend with map_select()")
    if map_candidates and (hasattr(backend, "frame_step") or not hasattr(backend, "map_select" if cell_select else "map_candidates")):
        raise ValueError("cell_select needs a per-call backend with map_select()" if cell_select else "map_candidates needs a per-call backend with map_candidates()")
    backend.load_frames(seq["images"])
    n_pts, n_seg = len(seq["pt_pos"]), len(seq["seg_spos"])
    T_prev = seq["poses_true"][0].copy()
    kf_T = seq["poses_true"][0]
    P3 = seq["pt_pos"].copy()                      # the map's point positions (seq["pt_pos"] stays the truth)
    known = np.ones(n_pts, bool)
    if mapping:
        rng = np.random.default_rng(map_seed + 77)
        known = rng.uniform(size=n_pts) < known_frac
        kf_pos = synth.se3_inv(kf_T)[4:]
        ray = P3 - kf_pos
        P3[known] = (kf_pos + ray * (1.0 + rng.uniform(-pos_noise, pos_noise, n_pts))[:, None])[known]
        depth0 = np.linalg.norm(ray, axis=1)
        dmean, dmin = float(depth0[known].mean()), 0.7 * float(depth0[known].min())
        nsd = int((~known).sum())
        seeds = dict(idx=np.nonzero(~known)[0], a=np.full(nsd, 10.0, np.float32), b=np.full(nsd, 10.0, np.float32), mu=np.full(nsd, 1.0 / dmean, np.float32),
                     z_range=np.full(nsd, 1.0 / dmin, np.float32), sigma2=np.full(nsd, (1.0 / dmin) ** 2 / 36.0, np.float32))
        obs = {int(i): [(0, seq["pt_f0"][i])] for i in range(n_pts)}     # Feature3D::obs_: (frame, unit bearing)
        last_optim = np.zeros(n_pts, np.int64)
        poses_est = [kf_T.copy()]
        detect = detect and hasattr(backend, "detect_corners")
        img_seeds, img_converged = None, 0
        w_img, h_img = int(cam[4]), int(cam[5])

        kf_select = kf_select and hasattr(backend, "keyframe_decide")
        z3 = np.zeros((0, 3))

        def decide(T_new, T_last, px, pos, sp, ep, overlap):
            return backend.keyframe_decide(abi.KeyframeDecideJob(cam, T_new, T_last, px, pos, None, sp, ep, None, np.stack(kfs["T"]), overlap,
                                                                 (-1,) * 5, kfselect_mindist_t, kfselect_mindist_r))

        def add_keyframe(T, key_pts, pos):
            """the keyframe table row: the pose and the landmark positions of the five key points (key_pts index `pos`, -1 = none)"""
            kfs["T"].append(np.asarray(T, float).copy())
            kfs["pos"].append(np.array([pos[i] if i >= 0 else np.zeros(3) for i in key_pts]))
            kfs["valid"].append(np.array([i >= 0 for i in key_pts], np.uint8))
        kfs = dict(T=[kf_T.copy()], pos=[], valid=[])
        seed_depth = (dmean, dmin)
        if kf_select:      # frame 0 is a keyframe: its key points come from the same call (no overlap keyframes: nothing else is looked at)
            kfs["T"] = []
            d0_ = backend.keyframe_decide(abi.KeyframeDecideJob(cam, kf_T, kf_T, seq["pt_px0"][known], P3[known], None, z3, z3, None, np.zeros((0, 7)), (),
                                                                (-1,) * 5, kfselect_mindist_t, kfselect_mindist_r))
            add_keyframe(kf_T, d0_["key_pts"], P3[known])

        def new_image_seeds(frame, feature_px):
            corners = backend.detect_corners(frame, _occupancy(feature_px, w_img, h_img, detect_cell_size), detect_cell_size, n_pyr_levels)
            sd = seeds_from_corners(corners, cam, *seed_depth)
            sd["ref_frame"] = np.full(len(corners), frame, np.int32)
            return sd
        if detect:
            img_seeds = new_image_seeds(0, seq["pt_px0"][known])
    # features of the previous frame that still carry a landmark: index into the map + pixel position
    k0 = np.nonzero(known)[0]
    prev = dict(pt_idx=k0, pt_px=seq["pt_px0"][k0].copy(), seg_idx=np.arange(n_seg), seg_spx=seq["seg_spx0"].copy(),
                seg_epx=seq["seg_epx0"].copy())
    out = [dict(T=T_prev.copy(), cov=np.full((6, 6), 1e-9), n_align=0, n_matched_pt=int(known.sum()), n_matched_seg=n_seg)]
    kf_select = mapping and kf_select
    f3 = lambda v: [float(x) for x in v]             # plain floats for the map tables below and in the keyframe branch of the loop
    if map_candidates:
        # the map tables of the stage: keyframe 0 with the features of the landmarks it starts with, one observation each (newest first later)
        cm = dict(kf_T=[f3(kf_T)], kf_slot=[0], kf_pt=[[int(i) for i in k0]], kf_seg=[list(range(n_seg))],
                  pt_pos=None, pt_type=[abi.LM_UNKNOWN] * n_pts,
                  pt_obs=[[dict(kf=0, px=f3(seq["pt_px0"][i]), f=f3(seq["pt_f0"][i]), level=0, type=abi.FTR_CORNER, grad=[0.0, 0.0])] if known[i] else [] for i in range(n_pts)],
                  seg_spos=[f3(v) for v in seq["seg_spos"]], seg_epos=[f3(v) for v in seq["seg_epos"]], seg_type=[abi.LM_UNKNOWN] * n_seg,
                  seg_obs=[[dict(kf=0, spx=f3(seq["seg_spx0"][i]), epx=f3(seq["seg_epx0"][i]), sf=f3(seq["seg_sf0"][i]), ef=f3(seq["seg_ef0"][i]), level=0)]
                           for i in range(n_seg)], pt_cand=[], seg_cand=[])
        cm_dirty = True
        seed_kf = 0                                    # the row of frame 0, where every seed was started (None once kf_insert removed it)
        # point rows of the tables <-> landmarks (indices of P3 / px_new): the identity until seed_candidates appends a converged seed as a
        # NEW row (its own row stays behind, empty and in no list); segment rows are segment indices throughout
        row_lm = list(range(n_pts))
        lm_row = np.arange(n_pts, dtype=np.int64)
        quality = None                                 # cell_select: the quality state after the last frame (None: nothing staged yet)
        so_keys = dict(pt=[], seg=[])                  # structopt_resident: last_structure_optim_ per table row, followed from the reports (0: never refined)
        select_kw = dict(max_fts=120, max_fts_segs=100, cell_order=None, seg_cell_order=None, reproj_thresh=reproj_thresh)
        select_kw.update(select_params or {})
    def align_job_of(k, sel, pr):
        """frame k + 1's alignment job from frame k's selection and the tables as they stand at this point of frame k"""
        if align == "device":
            backend.align_build(k, k + 1, max_level, min_level, max(select_kw["max_fts"] + 2, 8), max(select_kw["max_fts_segs"] + 2, 8))
            return True
        return align_job_host(cam, max_level, min_level, sel, pr.pt_keep, pr.seg_keep, cm["pt_type"], cm["seg_type"], cm["pt_pos"], cm["seg_spos"], cm["seg_epos"], pr.T, k, k + 1)

    for k in range(1, len(seq["images"])):
        reloc_try, T_reset = bool(relocalize) and stage == "reloc", None
        if reloc_try:
            # ---- relocalizeFrame (:408-436): the closest keyframe from the last frame's pose, the gating alignment from the identity,
            #      then processFrame with last_frame_ = ref_keyframe.  (last_frame_ is never a keyframe of the table here: self_kf -1)
            if cm_dirty:
                raise ValueError("relocalize: the resident tables wait for a restage")
            caps = (max(select_kw["max_fts"] + 2, 8, max(len(l) for l in cm["kf_pt"])), max(select_kw["max_fts_segs"] + 2, 8, max(len(l) for l in cm["kf_seg"])))
            fail = None
            if relocalize == "device":
                ar, ref_kf, T_gate, _ = backend.align_kf(None, k, IDENT, max_level, min_level, *caps, T_last=T_prev, last_dev=gate_dev)
            else:
                tabs = backend.map_fetch()
                kp_now = kp_tab if keystage == "host" else backend.map_fetch_keypts()[:len(cm["kf_T"])]
                n_kf_now = len(cm["kf_T"])
                kpos, kval = np.zeros((n_kf_now, 5, 3)), np.zeros((n_kf_now, 5), np.uint8)
                for j, row in enumerate(kp_now):
                    for s_, h in enumerate(row):
                        lm = int(tabs["kf_pt_lm"][int(tabs["kf_pt_off"][j]) + int(h)]) if 0 <= h < int(tabs["kf_pt_off"][j + 1]) - int(tabs["kf_pt_off"][j]) else -1
                        if lm >= 0:
                            kpos[j, s_], kval[j, s_] = tabs["pt_pos"][lm], 1
                cl = backend.close_keyframes(abi.CloseKeyframesJob(cam, T_prev, np.asarray(tabs["kf_T"], float).reshape(-1, 7), kpos, kval, max_n_kfs))
                ar, ref_kf, T_gate = None, -1, None
                if cl["n_close"] > 0:                  # Map::getClosestKeyframe: the front of the sorted list
                    ref_kf = int(cl["close_idx"][0])
                    ar = backend.sparse_align(align_kf_job_host(cam, max_level, min_level, tabs, ref_kf, IDENT, k))
                    T_gate = np.array(_se3_mul_s(ar.T, tabs["kf_T"][ref_kf]))
            if ar is None:
                fail, T_fail, n_tr = "no_keyframe", np.array(IDENT), 0           # "No reference keyframe": new_frame_ keeps its default pose
            elif ar.n_tracked <= 30:
                fail, T_fail, n_tr = "gating", np.asarray(T_gate, float).copy(), int(ar.n_tracked)   # (:421; the pose the alignment wrote stays)
            if fail:
                out.append(dict(T=T_fail, cov=np.full((6, 6), 1e-9), n_align=n_tr, n_matched_pt=0, n_matched_seg=0, n_kept_pt=0, n_kept_seg=0, stage="reloc",
                                gate=fail, tracking_quality=abi.TRACKING_INSUFFICIENT, reloc_kf=ref_kf, reloc_tracked=n_tr))
                if mapping:
                    poses_est.append(T_fail.copy())
                T_prev, gate_dev, obs_last, obs_resident, next_align = T_fail, None, (0, 0), False, None   # Frame::nObs() of a frame without features
                continue
            T_reset, reloc_kf, reloc_tracked = T_prev, ref_kf, int(ar.n_tracked)     # T_f_w_last
            T_ref_kf = np.array(cm["kf_T"][ref_kf], float)
            if relocalize == "device":                 # the second alignment: new_frame_->T_f_w_ = ref_keyframe->T_f_w_ (:266)
                ar, _, T_k, reloc_dev = backend.align_kf(ref_kf, k, None, max_level, min_level, *caps)
            else:
                ar = backend.sparse_align(align_kf_job_host(cam, max_level, min_level, tabs, ref_kf, None, k))
                T_k, reloc_dev = np.array(_se3_mul_s(ar.T, tabs["kf_T"][ref_kf])), None
            next_align = None
        # ---- 1. sparse image alignment, previous frame -> frame k (processFrame :266-274) ----
        job = None
        if next_align is None and not reloc_try:       # (align: otherwise the job was made behind the frame before this one)
            ref_pos = synth.se3_inv(T_prev)[4:]

            def scaled(px, pos):
                return _bearing(cam, px) * np.linalg.norm(pos - ref_pos, axis=1)[:, None]    # f * |pos - ref_pos| (:229-230)
            pi, si = prev["pt_idx"], prev["seg_idx"]
            job = abi.AlignJob(cam, max_level, min_level, 30, 1e-6, synth.se3_mul(T_prev, synth.se3_inv(T_prev)), prev["pt_px"],
                               scaled(prev["pt_px"], P3[pi]), prev["seg_spx"], prev["seg_epx"],
                               np.linalg.norm(prev["seg_epx"] - prev["seg_spx"], axis=1), scaled(prev["seg_spx"], seq["seg_spos"][si]),
                               scaled(prev["seg_epx"], seq["seg_epos"][si]), ref_slot=k - 1, cur_slot=k)
        pos_all = np.concatenate([P3, seq["seg_spos"], seq["seg_epos"]])
        if hasattr(backend, "frame_step"):
            # ---- 1-4 as one resident call: nothing but the final results comes back ----
            act = np.concatenate([known, np.ones(2 * n_seg, bool)]).astype(np.uint8)
            ref_px_all = np.concatenate([seq["pt_px0"], seq["seg_spx0"], seq["seg_epx0"]])
            ref_f_all = np.concatenate([seq["pt_f0"], seq["seg_sf0"], seq["seg_ef0"]])
            cr = backend.frame_step(job, T_prev, kf_T, 0, n_pts, n_seg, pos_all, ref_px_all, ref_f_all, act, cam, n_pyr_levels, reproj_thresh)
            ar, pr = cr.align, cr.pose
            px_new = cr.px
            pt_i, seg_i = cr.sel_pt.astype(np.int64), cr.sel_seg.astype(np.int64)
            pt_ok = np.zeros(n_pts, bool); pt_ok[pt_i] = True
            seg_ok = np.zeros(n_seg, bool); seg_ok[seg_i] = True
        else:
            poses_dev = None
            if reloc_try:                              # aligned against the keyframe above
                poses_dev = reloc_dev
            elif next_align is None:
                ar = backend.sparse_align(job)
                T_k = synth.se3_mul(ar.T, T_prev)                                                # :92
            elif align == "device":                    # the job was built behind the previous frame: run, compose, the pose stays on the device
                ar, T_k, poses_dev = backend.align_built()
            else:
                ar = backend.sparse_align(next_align)
                T_k = np.array(_se3_mul_s(ar.T, T_prev))
            next_align = None
            close = None
            if map_candidates:
                # ---- 2 + 3 from the map-candidate stage: overlap keyframes' features, first visit wins, closest-view observation,
                #      quality order, matched on the device (reprojectMap :157-183, getCloseViewObs, findMatchDirect) ----
                map_job = None
                if cm_dirty:
                    cm["pt_pos"] = [[float(x) for x in P3[i]] for i in row_lm]
                    map_job = candidate_map_job(cm)
                    cm_dirty = False
                kp_frame = 0
                if keystage:
                    n_kf_now = len(cm["kf_T"])
                    if map_job is not None and keystage == "device" and kp_live:
                        kp_tab = [[int(h) for h in r] for r in backend.map_fetch_keypts()[:n_kf_now]]      # a restage drops the resident table: it travels with the tables
                    if kp_tab is None and keystage == "host":
                        kp_tab, _ = _key_point_upkeep(cm, [[-1] * 5] * n_kf_now, cam, fresh=range(n_kf_now))   # Frame::setKeyframe: from five NULLs
                    kp_live = True
                    if keystage == "host":
                        # getCloseKeyframes reads key_pts_[k]->feat3D->pos_ as it is NOW
                        kpos, kval = np.zeros((n_kf_now, 5, 3)), np.zeros((n_kf_now, 5), np.uint8)
                        for j, row in enumerate(kp_tab):
                            for s_, h in enumerate(row):
                                lm = cm["kf_pt"][j][h] if h >= 0 else -1
                                if lm >= 0:
                                    kpos[j, s_], kval[j, s_] = cm["pt_pos"][lm], 1
                        close = backend.close_keyframes(abi.CloseKeyframesJob(cam, T_k, np.array(cm["kf_T"], float).reshape(-1, 7), kpos, kval, max_n_kfs))
                        overlap = [int(v) for v in close["close_idx"][:close["n_overlap"]]]
                    else:
                        overlap = []                   # decided on the device, from the resident table
                elif kf_select:
                    close = backend.close_keyframes(abi.CloseKeyframesJob(cam, T_k, np.stack(kfs["T"]), np.stack(kfs["pos"]), np.stack(kfs["valid"]), max_n_kfs))
                    overlap = [int(v) for v in close["close_idx"][:close["n_overlap"]]]
                else:
                    overlap = list(range(len(cm["kf_T"])))
                if cell_select:
                    cm_before = copy.deepcopy(cm) if record_candidates else None
                    cr, mr, sel, pr_sel, q_after = backend.map_select(map_job, abi.CandidateFrameJob(T_k, overlap, cur_slot=k), cam, n_pyr_levels, select_kw,
                                                                      carry=quality if map_job is not None else None,
                                                                      **(dict(close=max_n_kfs, key_pts=kp_tab) if keystage == "device" else {}),
                                                                      **(dict(poses_dev=poses_dev) if poses_dev else {}))
                    if keystage == "device":
                        close = backend.last_close
                        overlap = [int(v) for v in close["close_idx"][:close["n_overlap"]]]
                    if structopt_resident and map_job is not None and (any(so_keys["pt"]) or any(so_keys["seg"])):
                        # the keys do not survive a stage: carried over like the quality counters (rows appended since read 0)
                        backend.map_set_last_optim(so_keys["pt"] + [0] * (len(cm["pt_pos"]) - len(so_keys["pt"])), so_keys["seg"] + [0] * (len(cm["seg_spos"]) - len(so_keys["seg"])))
                    if seeds_resident and map_job is not None and mapping and seed_kf is not None:
                        # the seed lists join the tables that were just staged: every seed was started in frame 0's keyframe, in one batch
                        # that never ages (the harness keeps its seeds until they converge)
                        si_ = seeds["idx"]
                        backend.seeds_stage(dict(batch_counter=0, pt_ref_kf=np.full(len(si_), seed_kf, np.int32), pt_batch_id=np.zeros(len(si_), np.int32), pt_px=seq["pt_px0"][si_],
                                                 pt_f=seq["pt_f0"][si_], pt_level=np.zeros(len(si_), np.int32), pt_type=np.zeros(len(si_), np.uint8),
                                                 pt_grad=np.zeros((len(si_), 2)), pt_a=seeds["a"], pt_b=seeds["b"], pt_mu=seeds["mu"], pt_z_range=seeds["z_range"],
                                                 pt_sigma2=seeds["sigma2"]), cam, max_n_kfs=1 << 30, n_pyr_levels=n_pyr_levels,
                                            **(dict(room=dict(extra_pt=len(seq["images"]) * (-(-w_img // detect_cell_size)) * (-(-h_img // detect_cell_size)))) if image_seeds else {}))
                        seeds_on_device = True
                        res_lm, res_kf, res_ftr = [int(i) for i in si_], [seed_kf] * len(si_), [None] * len(si_)
                else:
                    cr, mr = backend.map_candidates(map_job, abi.CandidateFrameJob(T_k, overlap, cur_slot=k), cam, n_pyr_levels)
                npf, nsf = cr["n_filed_pt"], cr["n_filed_seg"]
                found = np.zeros(len(pos_all), bool)
                px_new = np.zeros((len(pos_all), 2))
                level = np.zeros(len(pos_all), np.int32)
                at = np.concatenate([np.asarray(row_lm, np.int64)[cr["pt_lm"]], n_pts + cr["seg_lm"], n_pts + n_seg + cr["seg_lm"]]).astype(np.int64)
                own = at >= 0                          # (image_seeds: a row without a landmark of the harness's map is the device's alone)
                found[at[own]] = mr["found"].astype(bool)[own]
                px_new[at[own]] = mr["px"][own]
                level[at[own]] = np.maximum(mr["search_level"], 0)[own]
                hist = np.zeros(len(cm["kf_T"]), np.int64)
                for lm, o in zip(cr["pt_lm"], cr["pt_obs"]):
                    if o >= 0:
                        hist[cm["pt_obs"][lm][o]["kf"]] += 1
                for lm, o in zip(cr["seg_lm"], cr["seg_obs"]):
                    if o >= 0:
                        hist[cm["seg_obs"][lm][o]["kf"]] += 1
                cand_rec = dict(n_filed_pt=npf, n_filed_seg=nsf, ref_kf_hist=[int(v) for v in hist])
                if record_candidates:
                    cand_rec["candidates"] = dict(stream=cm_before if cell_select else copy.deepcopy(cm), T=[float(v) for v in T_k], overlap=list(overlap), out=cr, match=mr)
                if cell_select:
                    # the tables follow the device: types, candidate lists, and the keyframe features of the landmarks safeDelete* cut loose
                    for name in ("pt", "seg"):
                        for lm in np.nonzero(q_after[name + "_event"] & abi.LM_EVENT_DELETED)[0]:
                            if cm[name + "_type"][int(lm)] == abi.LM_UNKNOWN:
                                cm["kf_" + name] = [[-1 if v == lm else v for v in fts] for fts in cm["kf_" + name]]
                        cm[name + "_type"] = [int(v) for v in q_after[name + "_type"]]
                        cm[name + "_cand"] = [int(v) for v in q_after[name + "_cand"]]
                    ev = np.concatenate([q_after["pt_event"], q_after["seg_event"]])
                    cand_rec.update(n_trials=sel["n_trials"], n_promoted=int((ev & abi.LM_EVENT_PROMOTED).astype(bool).sum()),
                                    n_deleted=int((ev & abi.LM_EVENT_DELETED).astype(bool).sum()))
                    if record_candidates:
                        cand_rec["candidates"].update(select=sel, quality_before=quality, quality=q_after, select_params=dict(select_kw))
                    quality = q_after
                    if keystage == "host":             # removeKeyPoint of the landmarks the selection deleted
                        kp_tab, kp_frame = _key_point_upkeep(cm, kp_tab, cam)
            else:
                # ---- 2. reprojection of the whole map (Reprojector::reprojectMap) ----
                rp = backend.reproject(abi.ReprojectJob(cam, np.stack([kf_T, T_k]), np.ones(len(pos_all), np.int32), pos_all, cell_size=30))
                vis = rp["cell"] >= 0
                vis[:n_pts] &= known                     # seeds are not in the map yet
                seg_vis = vis[n_pts:n_pts + n_seg] & vis[n_pts + n_seg:]
                vis[n_pts:n_pts + n_seg] = seg_vis
                vis[n_pts + n_seg:] = seg_vis
                idx = np.nonzero(vis)[0]
                # ---- 3. direct matching against the keyframe-0 observations (Matcher::findMatchDirect) ----
                ref_px = np.concatenate([seq["pt_px0"], seq["seg_spx0"], seq["seg_epx0"]])[idx]
                ref_f = np.concatenate([seq["pt_f0"], seq["seg_sf0"], seq["seg_ef0"]])[idx]
                m = len(idx)
                mj = abi.MatchJob(cam, np.stack([kf_T, T_k]), np.array([0, k], np.int32), np.ones(m, np.int32), np.zeros(m, np.int32), ref_px, ref_f,
                                  np.zeros(m, np.int32), np.zeros(m, np.uint8), np.zeros((m, 2)), pos_all[idx], rp["px"][idx], n_pyr_levels, 10)
                mr = backend.match_direct(mj)
                found = np.zeros(len(pos_all), bool)
                found[idx] = mr["found"].astype(bool)
                px_new = rp["px"].copy()
                px_new[idx] = mr["px_cur"]
                level = np.zeros(len(pos_all), np.int32)
                level[idx] = np.maximum(mr["search_level"], 0)
            pt_ok = found[:n_pts]
            seg_ok = found[n_pts:n_pts + n_seg] & found[n_pts + n_seg:]
            if cell_select:
                # ---- 4. on the device: the selected features in selection order, the resident pose optimiser's result ----
                frame_sel = sel                        # (align: the selection under a name of its own -- step 5 has a `sel` too)
                pt_i, seg_i = np.asarray(row_lm, np.int64)[sel["pt_lm"]], sel["seg_lm"].astype(np.int64)
                sel_mask = pt_i >= 0
                pt_i = pt_i[sel_mask]
                pt_ok = np.zeros(n_pts, bool); pt_ok[pt_i] = True
                seg_ok = np.zeros(n_seg, bool); seg_ok[seg_i] = True
                pr = pr_sel
        if not hasattr(backend, "frame_step") and not cell_select:
            # ---- 4. motion-only pose optimisation on the matches (processFrame :327-329) ----
            pt_i, seg_i = np.nonzero(pt_ok)[0], np.nonzero(seg_ok)[0]
            sf, ef = _bearing(cam, px_new[n_pts + seg_i]), _bearing(cam, px_new[n_pts + n_seg + seg_i])
            line = np.cross(sf, ef)
            line = line / np.sqrt(line[:, 0:1] ** 2 + line[:, 1:2] ** 2) if len(seg_i) else np.zeros((0, 3))    # feature.cpp:103-104
            pj = abi.PoseOptJob(T_k, abs(cam[0]), reproj_thresh, 10, _bearing(cam, px_new[pt_i]), P3[pt_i], level[pt_i], line,
                                seq["seg_spos"][seg_i], seq["seg_epos"][seg_i], level[n_pts + n_seg + seg_i])       # a LineFeat's level: the END point's (matcher.cpp:264)
            pr = backend.pose_optimize(pj)
        n_ties = backend.align_ties() if hasattr(backend, "align_ties") else None
        if kf_select and not map_candidates:
            # ---- the keyframes that overlap the aligned frame (the head of reprojectMap: it runs before the matching, which without
            #      map_candidates takes its candidates from keyframe 0 either way, so the call's place here does not matter) ----
            close = backend.close_keyframes(abi.CloseKeyframesJob(cam, synth.se3_mul(ar.T, T_prev), np.stack(kfs["T"]), np.stack(kfs["pos"]),
                                                                  np.stack(kfs["valid"]), max_n_kfs))
        T_last = T_ref_kf if reloc_try else T_prev       # last_frame_ of this processFrame
        bad_quality = False
        if relocalize:
            # ---- the gates of processFrame (:315-321, :335) and setTrackingQuality, ahead of the structure optimisation ----
            if obs_last is None:
                obs_last = (out[0]["n_matched_pt"], out[0]["n_matched_seg"])
            T_rs = T_reset if reloc_try else T_prev
            gk = dict(gate_kw, max_fts=select_kw["max_fts"], max_fts_segs=select_kw["max_fts_segs"])
            if relocalize == "device":
                grec, T_carried, gate_dev = backend.track_gate(mode=abi.GATE_RELOC if reloc_try else abi.GATE_TRACK, T_reset=T_rs,
                                                               **({} if obs_resident and map_job is None else dict(num_obs_last=obs_last)), **gk)
                g_result, g_quality = grec["result"], grec["tracking_quality"]
            else:
                g_result, g_quality, reset = track_gate_host(frame_sel["n_matches"], frame_sel["n_ls_matches"], pr.num_obs_pt, pr.num_obs_ls, *obs_last, relocalizing=reloc_try, **gk)
                T_carried = np.array(T_rs, float) if reset else pr.T.copy()
            obs_last, obs_resident = (int(frame_sel["n_matches"]), int(frame_sel["n_ls_matches"])), True
            if g_result != abi.GATE_OK:                # RESULT_FAILURE: nothing behind the gate runs; the next frame relocalises
                frec = dict(T=np.asarray(T_carried, float).copy(), cov=pr.cov.copy(), n_align=ar.n_tracked, n_matched_pt=int(pt_ok.sum()), n_matched_seg=int(seg_ok.sum()),
                            n_kept_pt=int(pr.pt_keep.sum()), n_kept_seg=int(pr.seg_keep.sum()), stage=stage, gate=int(g_result), tracking_quality=int(g_quality))
                if reloc_try:
                    frec.update(reloc_kf=reloc_kf, reloc_tracked=reloc_tracked)
                if map_candidates:
                    frec.update(cand_rec)
                if mapping:
                    poses_est.append(frec["T"].copy())
                out.append(frec)
                T_prev, stage, next_align = frec["T"].copy(), "reloc", None
                continue
            bad_quality = g_quality == abi.TRACKING_BAD
        T_k = pr.T.copy()
        pt_keep, seg_keep = pr.pt_keep.astype(bool), pr.seg_keep.astype(bool)
        if cell_select and sel_mask is not None:
            pt_keep = pt_keep[sel_mask]
        prev = dict(pt_idx=pt_i[pt_keep], pt_px=px_new[pt_i[pt_keep]], seg_idx=seg_i[seg_keep],
                    seg_spx=px_new[n_pts + seg_i[seg_keep]], seg_epx=px_new[n_pts + n_seg + seg_i[seg_keep]])
        T_prev = T_k
        rec = dict(T=T_k.copy(), cov=pr.cov.copy(), n_align=ar.n_tracked, n_matched_pt=int(pt_ok.sum()), n_matched_seg=int(seg_ok.sum()),
                   n_kept_pt=int(pt_keep.sum()), n_kept_seg=int(seg_keep.sum()))
        if n_ties is not None:
            rec["align_ties"] = n_ties
        if relocalize:
            rec.update(stage=stage, gate=int(g_result), tracking_quality=int(g_quality))
            if reloc_try:
                rec.update(reloc_kf=reloc_kf, reloc_tracked=reloc_tracked)
            stage = "default"                          # "Relocalization successful."
        if map_candidates:
            rec.update(cand_rec)
        if mapping:
            poses_est.append(T_k.copy())
            kept = pt_i[pt_keep]
            is_kf = (k % kf_every) == 0
            if kf_select and not keystage:
                # ---- scene depth, needNewKf against the overlap keyframes from the previous frame's pose, the frame's key points ----
                skept = seg_i[seg_keep]
                dec = decide(T_k, T_last, px_new[kept], P3[kept], seq["seg_spos"][skept], seq["seg_epos"][skept], close["close_idx"][:close["n_overlap"]])
                is_kf = bool(dec["need_new_kf"])
                rec.update(is_kf=is_kf, n_overlap=close["n_overlap"], depth_mean=dec["depth_mean"])
                if is_kf:
                    add_keyframe(T_k, dec["key_pts"], P3[kept])
                    if dec["has_depth"]:
                        seed_depth = (dec["depth_mean"] * 2.0, 0.1 * dec["depth_min"])
            if structopt_resident:
                # ---- 5. structure optimisation on the resident tables, ahead of the insertion as in processFrame (:340 before :358) ----
                for name, rows in (("pt", len(cm["pt_pos"])), ("seg", len(cm["seg_spos"]))):
                    so_keys[name] += [0] * (rows - len(so_keys[name]))
                before = (copy.deepcopy(cm), copy.deepcopy(so_keys)) if record_candidates else None
                so = backend.map_optimize_structure(k)
                for row, p in zip(so["pt_lm"], so["pt_pos"]):
                    cm["pt_pos"][int(row)] = [float(x) for x in p]
                    so_keys["pt"][int(row)] = k
                    if row_lm[int(row)] >= 0:
                        P3[row_lm[int(row)]] = p
                for row, a, b in zip(so["seg_lm"], so["seg_spos"], so["seg_epos"]):
                    cm["seg_spos"][int(row)], cm["seg_epos"][int(row)] = [float(x) for x in a], [float(x) for x in b]
                    so_keys["seg"][int(row)] = k
                rec.update(n_structopt_pt=int(so["n_sel_pt"]), n_structopt_seg=int(so["n_sel_seg"]))
                if record_candidates:
                    rec["structopt"] = dict(stream=before[0], keys_before=before[1], select=sel, pt_keep=pr.pt_keep.copy(), seg_keep=pr.seg_keep.copy(), frame_id=k, report=so,
                                            tables=copy.deepcopy(cm), keys=copy.deepcopy(so_keys))
            if keystage:
                # ---- the keyframe decision behind the structure optimisation (:340 before :351), on the selection with the keep masks as
                #      alive and the landmark positions as the tables hold them now; key_pts are indices in selection order ----
                if keystage == "device":
                    dec = backend.map_keyframe_decide(T_last, kfselect_mindist_t, kfselect_mindist_r)
                else:
                    at = lambda name, rows: np.array([cm[name][int(r)] for r in rows], float).reshape(-1, 3)
                    dec = backend.keyframe_decide(abi.KeyframeDecideJob(cam, T_k, T_last, sel["pt_px"], at("pt_pos", sel["pt_lm"]), pr.pt_keep, at("seg_spos", sel["seg_lm"]),
                                                                        at("seg_epos", sel["seg_lm"]), pr.seg_keep, np.array(cm["kf_T"], float).reshape(-1, 7),
                                                                        close["close_idx"][:close["n_overlap"]], (-1,) * 5, kfselect_mindist_t, kfselect_mindist_r))
                is_kf = bool(dec["need_new_kf"]) and not bad_quality       # (!needNewKf || TRACKING_BAD: no keyframe, :352)
                rec.update(is_kf=is_kf, n_overlap=close["n_overlap"], depth_mean=dec["depth_mean"], overlap=[int(v) for v in close["close_idx"][:close["n_overlap"]]])
                if is_kf:
                    rec["key_pts_new"] = [int(h) for h in dec["key_pts"]]      # the frame's key_pts_ as it becomes a keyframe, in selection order
                if is_kf and dec["has_depth"]:
                    seed_depth = (dec["depth_mean"] * 2.0, 0.1 * dec["depth_min"])
            if is_kf:
                for i, brg in zip(kept, _bearing(cam, px_new[kept])):
                    obs[int(i)].append((k, brg))
                if kf_insert:
                    # the frame joins the RESIDENT tables on the device; the harness's own follow the backend's fetch
                    remove = -1
                    if kf_select and len(cm["kf_T"]) >= max_n_kfs:
                        remove = max(int(dec["furthest_kf"]), 0)
                        for key in ([] if keystage else kfs):
                            del kfs[key][remove]
                        if seed_kf is not None:                       # the table closes up: frame 0's row moves, or is gone
                            seed_kf = None if remove == seed_kf else seed_kf - (remove < seed_kf)
                    before = (copy.deepcopy(cm), quality) if record_candidates else None
                    tables, quality, ins = backend.map_insert(remove, k)
                    cm = candidate_map_tables(tables)
                    if keystage == "host":             # the rows close up, the new keyframe's row is the decision's, holders lost to the removal are replaced
                        kp_tab, n_ = _key_point_upkeep(cm, [r for j, r in enumerate(kp_tab) if j != remove] + [[int(h) for h in dec["key_pts"]]], cam)
                        kp_frame += n_
                    if seeds_on_device and image_seeds and seed_kf is not None:
                        # initializeSeeds on the resident lists: the removal, then the corners of the frame's free cells
                        new_kf = len(cm["kf_T"]) - 1
                        assert ins.get("new_kf", new_kf) == new_kf and cm["kf_slot"][new_kf] == k
                        ev = dict(removed_kf=remove, new_batch=True, new_kf=new_kf, depth_mean=seed_depth[0], depth_min=seed_depth[1])
                        if image_seeds == "device":
                            backend.seeds_keyframe_detect(detect_cell_size, n_pyr_levels, img_kw["detection_threshold"], fast_threshold=img_kw["fast_threshold"],
                                                          occ_sources=abi.SEED_OCC_SELECTED | (abi.SEED_OCC_UPDATED if last_rows is not None else 0), **ev)
                            kf_rep = backend.seeds_keyframe_fetch()
                            assert not kf_rep["no_room"]
                            n_started = kf_rep["n_new_pt"]
                        else:
                            marking = np.zeros((0, 2))
                            if last_rows is not None:
                                stl = last_rows["pt_status"]
                                marking = last_rows["pt_px_cur"][(stl == abi.SEED_UPDATED) | (stl == abi.SEED_CONVERGED) | (stl == abi.SEED_NAN)]
                            occ = _occupancy(np.concatenate([sel["pt_px"].reshape(-1, 2), marking]), w_img, h_img, detect_cell_size)
                            corners = backend.detect_corners(k, occ, detect_cell_size, n_pyr_levels, img_kw["detection_threshold"], fast_threshold=img_kw["fast_threshold"])
                            sdn = seeds_from_corners(corners, cam, *seed_depth)
                            backend.seeds_keyframe(pt_px=sdn["px"], pt_f=sdn["f"], pt_level=sdn["level"], pt_type=sdn["type"], pt_grad=sdn["grad"], **ev)
                            n_started = len(corners)
                        if remove >= 0:
                            stay = [j for j, r in enumerate(res_kf) if r != remove]
                            res_lm, res_ftr = [res_lm[j] for j in stay], [res_ftr[j] for j in stay]
                            res_kf = [res_kf[j] - (res_kf[j] > remove) for j in stay]
                        if n_started:                                  # the new rows' features, for the landmark a converged one becomes (both transports: from the lists)
                            ls = backend.seeds_fetch_lists()
                            assert len(ls["pt_ref_kf"]) == len(res_lm) + n_started
                            for j in range(len(res_lm), len(res_lm) + n_started):
                                res_ftr.append(dict(px=[float(x) for x in ls["pt_px"][j]], f=[float(x) for x in ls["pt_f"][j]], level=int(ls["pt_level"][j])))
                            res_lm += [-1] * n_started; res_kf += [new_kf] * n_started
                        rec["n_image_seeds_started"] = int(n_started)
                    elif seeds_on_device and remove >= 0:              # removeKeyframe: the seeds' keyframe moves down a row, or leaves with its seeds
                        backend.seeds_keyframe(removed_kf=remove)
                        seeds_on_device = seed_kf is not None
                        res_lm, res_kf, res_ftr = [], [], []
                    rec.update(n_joined=ins["n_joined_pt"] + ins["n_joined_seg"], n_deleted_kf=ins["n_deleted_pt"] + ins["n_deleted_seg"], remove_kf=remove)
                    if keystage == "host":
                        rec["n_kp_rebuilt"] = int(kp_frame)
                    if align and compact and k + 1 < len(seq["images"]):
                        next_align = align_job_of(k, frame_sel, pr)    # ahead of the compaction, which renumbers the rows the selection points at
                    if compact:
                        # Map::emptyTrash on the resident tables: the deleted point rows leave, the rows behind them move down; the
                        # harness's rows follow the remap ("room": only when every live seed could no longer get a row)
                        alive = len(seeds["idx"]) + sum(1 for v in res_lm if v < 0)
                        tables, quality, cp = backend.map_compact("room", (1 << 30) if compact == "always" else alive, 0)
                        if cp["ran_pt"]:
                            cm = candidate_map_tables(tables)
                            remap = cp["pt_remap"]
                            lm_row[[lm for row, lm in enumerate(row_lm) if lm >= 0 and remap[row] < 0]] = -1
                            row_lm = [lm for row, lm in enumerate(row_lm) if remap[row] >= 0]
                            for row, lm in enumerate(row_lm):
                                if lm >= 0:
                                    lm_row[lm] = row
                            so_keys["pt"] = [v for row, v in enumerate(so_keys["pt"]) if row >= len(remap) or remap[row] >= 0]
                        rec["n_compacted_pt"] = int(cp["n_pt_before"] - cp["n_pt_after"])
                    if record_candidates:
                        rec["insert"] = dict(stream=before[0], quality_before=before[1], select=sel, pt_keep=pr.pt_keep.copy(), seg_keep=pr.seg_keep.copy(), T=[float(v) for v in T_k],
                                             slot=k, remove_kf=remove, tables=tables, quality=quality, report=ins)
                elif map_candidates:
                    # the frame joins the keyframe table: its features, and an observation at the FRONT of every landmark's list
                    # (Feature3D::addFrameRef pushes at the front, include/plsvo/feature3D.h:204); a candidate it matched leaves the
                    # map's candidate list for the keyframe's features
                    skept_ = seg_i[seg_keep]
                    kf_id = len(cm["kf_T"])
                    cm["kf_T"].append(f3(T_k)); cm["kf_slot"].append(k)
                    cm["kf_pt"].append([int(i) for i in kept]); cm["kf_seg"].append([int(i) for i in skept_])
                    for i, brg in zip(kept, _bearing(cam, px_new[kept])):
                        cm["pt_obs"][int(i)].insert(0, dict(kf=kf_id, px=f3(px_new[i]), f=f3(brg), level=int(level[i]), type=abi.FTR_CORNER, grad=[0.0, 0.0]))
                        if not cell_select or cm["pt_type"][int(i)] == abi.LM_CANDIDATE:      # (a candidate that joins a keyframe: TYPE_UNKNOWN)
                            cm["pt_type"][int(i)] = abi.LM_UNKNOWN
                    for i, sb, eb in zip(skept_, _bearing(cam, px_new[n_pts + skept_]), _bearing(cam, px_new[n_pts + n_seg + skept_])):
                        cm["seg_obs"][int(i)].insert(0, dict(kf=kf_id, spx=f3(px_new[n_pts + i]), epx=f3(px_new[n_pts + n_seg + i]), sf=f3(sb), ef=f3(eb),
                                                             level=int(level[n_pts + i])))
                    matched = set(int(v) for v in kept)
                    cm["pt_cand"] = [i for i in cm["pt_cand"] if i not in matched]
                    cm_dirty = True
            # ---- 5. structure optimisation (FrameHandlerBase::optimizeStructure: the 20 least recently refined, :202-237) ----
            cand = np.array([i for i in kept if len(obs[int(i)]) >= 2], np.int64)
            if len(cand) and is_kf and not structopt_resident:
                sel = cand[np.argsort(last_optim[cand], kind="stable")[:20]]
                off, ofr, of_ = [0], [], []
                for i in sel:
                    for fr_, brg in obs[int(i)]:
                        ofr.append(fr_)
                        of_.append(brg)
                    off.append(len(ofr))
                z3, zi = np.zeros((0, 3)), np.zeros(0, np.int32)
                so = backend.structure_optimize(abi.StructOptJob(np.stack(poses_est), P3[sel], off, ofr, np.array(of_), z3, z3, np.zeros(1, np.int32), zi, z3, z3, 5, 5))
                P3[sel] = so["pt_pos"]
                last_optim[sel] = k
                if kf_insert:
                    backend.map_set_positions(lm_row[sel].astype(np.int32), P3[sel])
                    for i in sel:
                        cm["pt_pos"][int(lm_row[i])] = [float(x) for x in P3[i]]
                elif map_candidates:
                    cm_dirty = True
            # ---- 6. depth-filter update of the seeds with this frame (DepthFilter::updateSeeds) ----
            ns = len(seeds["idx"])
            img_dev = bool(image_seeds) and seeds_on_device    # the resident rows hold seeds from the image beside the map's
            if ns or (img_dev and res_lm):
                si_ = seeds["idx"]
                ptd = dict(ref_frame=np.zeros(ns, np.int32), cur_frame=np.ones(ns, np.int32), px=seq["pt_px0"][si_], f=seq["pt_f0"][si_], level=np.zeros(ns, np.int32),
                           a=seeds["a"], b=seeds["b"], mu=seeds["mu"], z_range=seeds["z_range"], sigma2=seeds["sigma2"])
                if seeds_on_device:                               # on the resident lists: the report and the rows come back, no record travels
                    seed_report, sr, seed_quality = backend.seeds_update(k, T_k)
                    assert len(sr["pt_status"]) == (len(res_lm) if img_dev else ns) and seed_report["no_room"] == 0
                    if img_dev:                                   # the map's seeds are the rows with a landmark, in the order of seeds["idx"]
                        all_rows, is_map = sr, np.asarray(res_lm, np.int64) >= 0
                        last_rows = dict(pt_status=sr["pt_status"].copy(), pt_px_cur=sr["pt_px_cur"].copy())
                        assert np.array_equal(np.asarray(res_lm, np.int64)[is_map], si_)
                        sr = {f: v[is_map] for f, v in sr.items() if f.startswith("pt_")}
                else:
                    sr = backend.update_seeds(abi.SeedsJob(cam, np.stack([kf_T, T_k]), np.array([0, k], np.int32), ptd, None, n_pyr_levels=n_pyr_levels))
                stt = sr["pt_status"]
                conv = stt == abi.SEED_CONVERGED
                P3[si_[conv]] = sr["pt_xyz_world"][conv]
                known[si_[conv]] = True
                if img_dev:
                    # every converged row, from the map or from the image, is a new landmark row of the resident tables, in list order
                    st_all = all_rows["pt_status"]
                    for j, r in enumerate(np.nonzero(st_all == abi.SEED_CONVERGED)[0]):
                        row, lm = len(cm["pt_pos"]), res_lm[r]
                        assert row == seed_report["first_pt"] + j
                        if lm >= 0:
                            ftr = dict(px=[float(x) for x in seq["pt_px0"][lm]], f=[float(x) for x in seq["pt_f0"][lm]], level=0, grad=[0.0, 0.0])
                            lm_row[lm] = row
                        else:
                            ftr = dict(res_ftr[r], grad=[1.0, 0.0])
                            img_conv += 1
                        cm["pt_pos"].append([float(x) for x in all_rows["pt_xyz_world"][r]])
                        cm["pt_type"].append(abi.LM_CANDIDATE)
                        cm["pt_obs"].append([dict(kf=res_kf[r], px=ftr["px"], f=ftr["f"], level=ftr["level"], type=abi.FTR_CORNER, grad=ftr["grad"])])
                        cm["pt_cand"].append(row)
                        row_lm.append(lm)
                        quality = seed_quality
                    stay = [r for r in range(len(res_lm)) if st_all[r] not in (abi.SEED_CONVERGED, abi.SEED_NAN, abi.SEED_AGED)]
                    res_lm, res_kf, res_ftr = [res_lm[r] for r in stay], [res_kf[r] for r in stay], [res_ftr[r] for r in stay]
                    rec.update(n_image_seeds=sum(1 for v in res_lm if v < 0), n_image_seeds_converged=img_conv)
                elif seed_candidates and conv.any() and seed_kf is not None:
                    # the converged seeds join the RESIDENT tables on the device as new landmark rows (newCandidatePoint); the harness
                    # appends the same rows to its own
                    ci = [int(i) for i in si_[conv]]
                    new = dict(pt_pos=sr["pt_xyz_world"][conv], pt_obs_kf=np.full(len(ci), seed_kf, np.int32), pt_obs_px=seq["pt_px0"][ci], pt_obs_f=seq["pt_f0"][ci],
                               pt_obs_level=np.zeros(len(ci), np.int32), pt_obs_type=np.full(len(ci), abi.FTR_CORNER, np.uint8), pt_obs_grad=np.zeros((len(ci), 2)))
                    before = (copy.deepcopy(cm), quality) if record_candidates else None
                    if seeds_on_device:                           # the commit has appended them already: its report stands in for the add's
                        report = dict(first_pt=seed_report["first_pt"], first_seg=-1, n_added_pt=len(ci), n_added_seg=0, n_pt=seed_report["n_pt"], n_seg=seed_report["n_seg"],
                                      n_pt_cand=seed_report["n_pt_cand"], n_seg_cand=seed_report["n_seg_cand"], n_pt_obs=seed_report["n_pt_obs"], n_seg_obs=seed_report["n_seg_obs"])
                        quality = seed_quality
                    else:
                        report, quality = backend.map_add_candidates(new)
                    for j, i in enumerate(ci):
                        row = len(cm["pt_pos"])
                        assert row == report["first_pt"] + j
                        cm["pt_pos"].append([float(x) for x in P3[i]])
                        cm["pt_type"].append(abi.LM_CANDIDATE)
                        cm["pt_obs"].append([dict(kf=seed_kf, px=[float(x) for x in seq["pt_px0"][i]], f=[float(x) for x in seq["pt_f0"][i]], level=0,
                                                  type=abi.FTR_CORNER, grad=[0.0, 0.0])])
                        cm["pt_cand"].append(row)
                        row_lm.append(i); lm_row[i] = row
                    if record_candidates:
                        rec["add"] = dict(stream=before[0], quality_before=before[1], new=new, tables=copy.deepcopy(cm), quality=quality, report=report)
                elif map_candidates and conv.any() and seed_kf is not None:
                    # a converged seed becomes a candidate of the map (map_.point_candidates_), observed in the keyframe it was started in
                    # (frame 0; once that keyframe has left the table the seed's only observation is gone with it, as
                    # removeFrameCandidates would delete it: the landmark stays outside the map's tables)
                    for i in si_[conv]:
                        cm["pt_obs"][int(i)] = [dict(kf=seed_kf, px=[float(x) for x in seq["pt_px0"][i]], f=[float(x) for x in seq["pt_f0"][i]], level=0,
                                                     type=abi.FTR_CORNER, grad=[0.0, 0.0])]
                        cm["pt_type"][int(i)] = abi.LM_CANDIDATE
                        cm["pt_cand"].append(int(i))
                    cm_dirty = True
                keep_s = ~(conv | (stt == abi.SEED_NAN))
                seeds = dict(idx=si_[keep_s], a=sr["pt_a"][keep_s], b=sr["pt_b"][keep_s], mu=sr["pt_mu"][keep_s], z_range=seeds["z_range"][keep_s],
                             sigma2=sr["pt_sigma2"][keep_s])
                rec["n_seed_converged"] = int(conv.sum())
                if kf_insert:
                    rec["n_seed_candidates"] = int(conv.sum()) if seed_kf is not None else 0
            if detect:
                # ---- 7. the seeds that came from the image: updated with this frame; a keyframe adds those of its own free cells ----
                ni = len(img_seeds["px"])
                if ni:
                    sr = backend.update_seeds(abi.SeedsJob(cam, np.stack(poses_est), np.arange(len(poses_est), dtype=np.int32),
                                                           dict(img_seeds, cur_frame=np.full(ni, k, np.int32)), None, n_pyr_levels=n_pyr_levels))
                    stt = sr["pt_status"]
                    img_converged += int((stt == abi.SEED_CONVERGED).sum())
                    keep_s = ~((stt == abi.SEED_CONVERGED) | (stt == abi.SEED_NAN))
                    img_seeds = {key: v[keep_s] for key, v in img_seeds.items()}
                    for key in ("a", "b", "mu", "sigma2"):
                        img_seeds[key] = sr["pt_" + key][keep_s]
                if is_kf:
                    fresh = new_image_seeds(k, px_new[kept])
                    img_seeds = {key: np.concatenate([img_seeds[key], fresh[key]]) for key in img_seeds}
                rec.update(n_image_seeds=len(img_seeds["px"]), n_image_seeds_converged=img_converged)
            rec.update(n_known=int(known.sum()), n_seeds=len(seeds["idx"]),
                       landmark_err=float(np.median(np.linalg.norm(P3[known] - seq["pt_pos"][known], axis=1))))
        if align and next_align is None and k + 1 < len(seq["images"]) and not cm_dirty:
            # behind everything that moves a landmark in this frame.  Tables that wait for a restage no longer say what the harness's own do:
            # the frame behind them is staged by the host as without the flag
            next_align = align_job_of(k, frame_sel, pr)
        out.append(rec)
    if keystage and kp_live:                           # Frame::key_pts_ of every keyframe at the end
        out[-1]["key_pts"] = np.array(kp_tab if keystage == "host" else backend.map_fetch_keypts()[:len(cm["kf_T"])], np.int32).reshape(-1, 5)
    return out


def pose_errors(result, seq):
    """(rotation error [rad], translation error [m]) per frame against the true poses"""
    return [synth.se3_log_angle_dist(r["T"], T) for r, T in zip(result, seq["poses_true"])]
