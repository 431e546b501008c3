"""Relocalisation on the resident map: the alignment job from a resident keyframe (plsvo_candidates_align_build_kf,
map_align_kf_job_kernel) and the tracking gates (plsvo_candidates_track_gate, map_track_gate_kernel) against their restatement
tests/np_reloc.py on the cases of tests/reloc_cases.py.  Per job case:
  * the fetched job (feature arrays, T0, T_ref, the per-level slot codes, the launch-order key) and the report are byte for byte the
    restatement's, whose inputs are the tables as plsvo_candidates_fetch_map reports them at build time and the live key-point table;
  * plsvo_align_run + _fetch on the built batch equal plsvo_sparse_align_batch on the restated job bit for bit, and the composed pose
    equals the restated product.
The gate's inputs are what the device holds: the fetched selection's counts and the fetched pose optimisation's num_obs; its
thresholds are placed around them."""
import copy

import numpy as np
import pytest

import alignjob_cases as A
import candidates_cases as Cc
import insert_cases as Ic
import np_alignjob as NA
import np_reloc as R
import reloc_cases as Rc
import test_gpu_alignjob as TA

same_bytes = TA.same_bytes
CUR = Rc.CUR_SLOT


@pytest.fixture(scope="module")
def ctx(P):
    c = TA.make_ctx(P, A.SMALL)
    yield c
    c.close()


@pytest.fixture(scope="module")
def wide_ctx(P):
    c = TA.make_ctx(P, A.WIDE)
    yield c
    c.close()


@pytest.fixture
def own_ctx(P):
    c = TA.make_ctx(P, A.SMALL)
    yield c
    c.close()


def restate(ctx, geo, cfg, jobs, n=None, prev=None):
    """the restatement of a keyframe build on what the device holds now; jobs as candidates_align_build_kf takes them"""
    maps = ctx.candidates_fetch_map()
    keypts = ctx.candidates_fetch_keypts() if any(j is not None and j.get("ref_kf") is None for j in jobs) else [None] * len(jobs)
    align = TA.seg_align_of(ctx, len(jobs) if n is None else n)
    out = []
    for k, j in enumerate(jobs):
        if j is None:
            out.append(prev[k] if prev else NA.empty_job(cfg))
            continue
        src = R.INIT_DEV if j.get("init_dev") is not None else R.INIT_HOST if (j.get("T_init") is not None and not j.get("init_keyframe")) else R.INIT_KEYFRAME
        T_init = j.get("T_init_value", j.get("T_init", Cc.IDENT))
        out.append(R.kf_align_job(maps[k], R.CLOSEST if j.get("ref_kf") is None else j["ref_kf"], T_init, geo["cam_t"], cfg, align, init_source=src,
                                  key_pts=keypts[k], T_last=j.get("T_last_value", j.get("T_last")), self_kf=j.get("self_kf", -1)))
    return out


def slots_of(streams, wants):
    return [(s["st"]["kf_slot"][w["report"]["ref_kf"]] if w["report"].get("ref_kf", -1) >= 0 else CUR, CUR) for s, w in zip(streams, wants)]


def check(ctx, P, geo, cfg, streams, jobs, tag, run=True, n=None, prev=None):
    wants = restate(ctx, geo, cfg, jobs, n=n, prev=prev)
    TA.check_jobs(ctx, P, geo, cfg, wants, tag, n=n)
    maps = ctx.candidates_fetch_map()
    for k, (j, w) in enumerate(zip(jobs, wants)):                     # the host path's job from the same fetched tables: the two transports' jobs are equal
        if j is None or w["report"]["status"] != R.OK or j.get("init_dev") is not None:
            continue
        h = P.sequence.align_kf_job_host(geo["cam_t"], cfg["max_level"], cfg["min_level"], maps[k], w["report"]["ref_kf"],
                                         j.get("T_init") if j.get("T_init") is not None and not j.get("init_keyframe") else None, j["cur_slot"])
        for f in ("pt_px", "pt_xyz_ref", "seg_spx", "seg_epx", "seg_len", "seg_p_ref", "seg_q_ref", "seg_alive_in"):
            same_bytes(getattr(h, f), w[f], (tag, "host path", k, f))
        same_bytes(np.array(h.c.T_cur_from_ref[:]), w["T0"], (tag, "host path", k, "T0"))
    if run:
        TA.check_run(ctx, P, geo, cfg, wants, tag, slots=slots_of(streams, wants))
    return wants


def job(ref_kf, **kw):
    return dict(dict(ref_kf=ref_kf, cur_slot=CUR, T_init=Rc.T_INIT), **kw)


# ---- the job from a keyframe -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_holes_a_deleted_and_a_candidate_landmark_first_and_last_row(ctx, P):
    """keyframe 1's lists hold -1 features and a TYPE_DELETED landmark in the middle (passed over; the segment features stay, dead, with
    zeros) and TYPE_CANDIDATE landmarks (kept); the first and the last row as ref_kf"""
    streams = (Rc.holes(),)
    geo, cfg = TA.stage(ctx, streams), Rc.cfg()
    ctx.candidates_align_reserve(**cfg)
    for ref_kf, n_pts, n_seg, alive in ((1, 11, 9, 5), (0, 4, 2, 2), (2, 3, 1, 1)):
        jobs = [job(ref_kf)]
        ctx.candidates_align_build_kf(jobs)
        w = check(ctx, P, geo, cfg, streams, jobs, ("holes", ref_kf))[0]
        assert (w["n_pts"], w["n_seg"], w["report"]["n_seg_alive"], w["report"]["ref_kf"]) == (n_pts, n_seg, alive, ref_kf)
        same_bytes(w["T_ref"], streams[0]["st"]["kf_T"][ref_kf], "T_ref")
    dead = [s for s, a in enumerate(restate(ctx, geo, cfg, [job(1)])[0]["seg_alive_in"]) if not a]
    ctx.candidates_align_build_kf([job(1)])
    g = ctx.candidates_align_fetch_job(0)
    assert len(dead) == 4 and not g["seg_spx"][dead].any() and not g["seg_len"][dead].any() and not g["seg_p_ref"][dead].any()


@pytest.mark.gpu
def test_the_first_observation_in_the_keyframe_is_the_feature(ctx, P):
    """landmarks observed in both keyframes with the other keyframe's observation first; a landmark that is a feature twice; features
    without an observation in the keyframe (passed over); a second observation in the same keyframe (the first is the pairing); the
    stored bearing, not the pixel's"""
    streams = (Rc.shared(),)
    geo, cfg = TA.stage(ctx, streams), Rc.cfg()
    ctx.candidates_align_reserve(**cfg)
    jobs = [job(1)]
    ctx.candidates_align_build_kf(jobs)
    w = check(ctx, P, geo, cfg, streams, jobs, "shared")[0]
    st = streams[0]["st"]
    assert w["n_pts"] == len(st["kf_pt"][1]) - 1 and w["n_seg"] == len(st["kf_seg"][1]) and w["report"]["n_seg_alive"] == w["n_seg"] - 1
    same_bytes(w["pt_px"][2], w["pt_px"][7], "a feature twice")
    first = [o for o in st["pt_obs"][st["kf_pt"][1][0]] if o["kf"] == 1][0]
    same_bytes(w["pt_px"][0], first["px"], "first observation")
    # the stored bearing: scale an observation's f and the row follows it
    st2 = copy.deepcopy(streams[0]); lm = st2["st"]["kf_pt"][1][1]
    o = [o for o in st2["st"]["pt_obs"][lm] if o["kf"] == 1][0]
    o["f"] = [0.5 * v for v in o["f"]]
    TA.stage(ctx, (st2,))
    ctx.candidates_align_reserve(**cfg)
    ctx.candidates_align_build_kf(jobs)
    w2 = check(ctx, P, geo, cfg, (st2,), jobs, "stored bearing", run=False)[0]
    same_bytes(w2["pt_xyz_ref"][1], 0.5 * w["pt_xyz_ref"][1], "f is read from the table")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [64, 65, 70])
def test_kept_points_across_the_rounds_of_64(ctx, P, n):
    streams = (Rc.kept_points(n),)
    geo, cfg = TA.stage(ctx, streams), Rc.cfg()
    ctx.candidates_align_reserve(**cfg)
    jobs = [job(0)]
    ctx.candidates_align_build_kf(jobs)
    assert check(ctx, P, geo, cfg, streams, jobs, ("kept", n))[0]["n_pts"] == n


@pytest.mark.gpu
def test_no_points_no_segments_nothing_and_an_inactive_stream(ctx, P):
    streams = (Rc.only(0, 4), Rc.only(6, 0), Rc.only(0, 0), Rc.only(3, 2))
    geo, cfg = TA.stage(ctx, streams), Rc.cfg(cap_pts=16, cap_seg=8, slot_cap=256)
    ctx.candidates_align_reserve(**cfg)
    jobs = [job(1), job(1), job(1), None]
    ctx.candidates_align_build_kf(jobs)
    first = check(ctx, P, geo, cfg, streams, jobs, "empty 1")
    assert [(w["n_pts"], w["n_seg"], w["skip"]) for w in first] == [(0, 4, 0), (6, 0, 0), (0, 0, 1), (0, 0, 1)]
    jobs = [None, job(0), None, job(1)]
    ctx.candidates_align_build_kf(jobs)
    second = check(ctx, P, geo, cfg, streams, jobs, "empty 2", prev=first)
    assert second[0] is first[0] and (second[1]["n_pts"], second[3]["n_pts"]) == (2, 3)


@pytest.mark.gpu
def test_segments_of_64_and_65_samples_on_the_wide_camera(wide_ctx, P):
    streams = (Rc.wide_lines(),)
    geo, cfg = TA.stage(wide_ctx, streams), Rc.cfg(cap_pts=16, cap_seg=16, slot_cap=640)
    wide_ctx.candidates_align_reserve(**cfg)
    jobs = [job(0)]
    wide_ctx.candidates_align_build_kf(jobs)
    w = check(wide_ctx, P, geo, cfg, streams, jobs, "wide")[0]
    assert TA.levels_n(w, cfg, 1) == [64, 65] and w["long_mask"] == 2


@pytest.mark.gpu
def test_the_three_sources_of_the_initial_pose(ctx, P):
    """a host pose, a device pointer (the carried poses of a gate) and the keyframe's own pose, whose T0 is T_kf * T_kf^-1 and not the
    literal identity"""
    streams = (Rc.holes(), Rc.shared(), Rc.three_keyframes())
    geo, cfg = TA.stage(ctx, streams), Rc.cfg()
    ctx.candidates_align_reserve(**cfg)
    sels = TA.frame(ctx, P, streams)
    ctx.candidates_pose_optimize()
    ctx.candidates_track_gate([dict(T_reset=Rc.T_INIT, num_obs_last=(0, 0), quality_min_fts=10 ** 6)] * 3)   # every stream fails: the carried pose is T_reset
    dev = ctx.candidates_gate_poses_dev()
    assert dev
    jobs = [job(1), dict(ref_kf=0, cur_slot=CUR, init_dev=dev + 56, T_init_value=Rc.T_INIT), dict(ref_kf=2, cur_slot=CUR)]
    ctx.candidates_align_build_kf(jobs)
    wants = check(ctx, P, geo, cfg, streams, jobs, "init")
    same_bytes(wants[1]["T0"], wants[0]["T0"] * 0 + np.array(R.K.se3_mul(Rc.T_INIT, R.K.se3_inv(streams[1]["st"]["kf_T"][0]))), "T0 from the device pointer")
    kfT = streams[2]["st"]["kf_T"][2]
    same_bytes(wants[2]["T0"], R.K.se3_mul(kfT, R.K.se3_inv(kfT)), "T_kf * T_kf^-1")


@pytest.mark.gpu
def test_a_stream_beyond_a_capacity_is_dropped_and_its_neighbours_are_intact(ctx, P):
    streams = Rc.overflow_batch()
    geo, cfg = TA.stage(ctx, streams), Rc.cfg(**Rc.OVERFLOW_CFG)
    ctx.candidates_align_reserve(**cfg)
    jobs = [job(0)] * 4
    ctx.candidates_align_build_kf(jobs)
    wants = check(ctx, P, geo, cfg, streams, jobs, "overflow")
    rep = [w["report"] for w in wants]
    assert [r["status"] for r in rep] == [R.NO_ROOM, R.NO_ROOM, R.NO_ROOM, R.OK]
    assert rep[0]["n_pts"] == 21 and rep[0]["n_slots"] == 0 and rep[1]["n_seg"] == 21 and rep[2]["n_slots"] > 80 and rep[3]["n_slots"] == 70   # 64 + one segment of 1 + (200 / 16 - 1) / 2 = 6 samples
    assert [(w["skip"], w["n_pts"], w["n_seg"]) for w in wants] == [(1, 0, 0)] * 3 + [(0, 10, 1)]


@pytest.mark.gpu
def test_a_build_behind_a_compaction_and_from_an_inserted_keyframe(ctx, P):
    """the frame is tracked, inserted as a keyframe on the device and the tables are compacted: the job from the NEW keyframe row with its
    own pose as the initial one equals the restatement on the fetched tables; plsvo_candidates_align_build refuses behind the compaction,
    the keyframe build does not"""
    streams = (Ic.directed_stream(),)
    geo, cfg = TA.stage(ctx, streams, Ic.RESERVE), Rc.cfg()
    ctx.candidates_align_reserve(**cfg)
    sels = TA.frame(ctx, P, streams)
    masks = [Ic.keep_masks(streams[0], sels[0])]
    ctx.candidates_insert_keyframe([dict(remove_kf=3, kf_slot=2, T_f_w=Ic.T_NEW, pt_keep=masks[0][0], seg_keep=masks[0][1])])
    new_kf = ctx.candidates_insert_fetch()[0]["new_kf"]
    sel_jobs = [dict(ref_slot=2, cur_slot=CUR, T_f_w=Ic.T_NEW, pt_keep=masks[0][0], seg_keep=masks[0][1])]
    ctx.candidates_align_build(sel_jobs)
    from_sel = ctx.candidates_align_fetch_job(0)
    jobs = [dict(ref_kf=new_kf, cur_slot=CUR)]
    ctx.candidates_align_build_kf(jobs)
    w = check(ctx, P, geo, cfg, [dict(st=dict(kf_slot=[0] * new_kf + [2]))], jobs, "inserted")[0]
    assert w["n_pts"] > 0
    same_bytes(w["pt_px"], from_sel["pt_px"], "the kept point rows of the two builds")       # DESIGN.md 3.21 records this
    ctx.candidates_compact([dict()])
    with pytest.raises(P.capi.PlsvoError):
        ctx.candidates_align_build(sel_jobs)
    ctx.candidates_align_build_kf(jobs)
    check(ctx, P, geo, cfg, [dict(st=dict(kf_slot=[0] * new_kf + [2]))], jobs, "behind the compaction")


# ---- the closest keyframe --------------------------------------------------------------------------------------------------------------
def closest(T_last, self_kf=-1, **kw):
    return dict(dict(cur_slot=CUR, T_init=Rc.T_INIT, T_last=T_last, self_kf=self_kf), **kw)


@pytest.mark.gpu
def test_the_closest_keyframe(ctx, P):
    """keyframe centres at x = -0.06, -0.03, 0: the nearest of three; an exact distance tie (the lower row); self_kf nearest (the second);
    self_kf the only close one (none); no key point visible (NO_KEYFRAME: skip, the composed pose is T_init); a device pointer for T_last"""
    streams = (Rc.three_keyframes(),) * 5
    geo, cfg = TA.stage(ctx, streams), Rc.cfg()
    ctx.candidates_align_reserve(**cfg)
    ctx.candidates_set_keypts()
    away = [0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0]                     # looking backwards: nothing is visible
    jobs = [closest(Rc.far_T(-0.05)), closest(Rc.far_T(-0.045)), closest(Rc.far_T(-0.05), self_kf=0), closest(Rc.far_T(0.01), self_kf=2), closest(away)]
    ctx.candidates_align_build_kf(jobs)
    wants = check(ctx, P, geo, cfg, streams, jobs, "closest")
    assert [w["report"]["ref_kf"] for w in wants] == [0, 0, 1, 1, -1]
    d = R.close_list(ctx.candidates_fetch_map()[1], ctx.candidates_fetch_keypts()[1], Rc.far_T(-0.045), geo["cam_t"])
    assert d[0][1] == d[1][1], "an exact tie"
    assert wants[4]["report"]["status"] == R.NO_KEYFRAME and wants[4]["skip"] == 1
    same_bytes(wants[4]["T_ref"], Rc.T_INIT, "T_ref of no keyframe")
    # self_kf the only close keyframe: the others' landmarks are out of view for a frame that sees keyframe 2's alone
    st = copy.deepcopy(Rc.three_keyframes())
    for k in (0, 1):
        for lm in st["st"]["kf_pt"][k]:
            st["st"]["pt_pos"][lm][2] = -4.0                       # behind the camera
    TA.stage(ctx, (st, st))
    ctx.candidates_align_reserve(**cfg)
    ctx.candidates_set_keypts()
    jobs = [closest(Rc.far_T(0.0), self_kf=2), closest(Rc.far_T(0.0))]
    ctx.candidates_align_build_kf(jobs)
    wants = check(ctx, P, geo, cfg, (st, st), jobs, "only self")
    assert [w["report"]["ref_kf"] for w in wants] == [-1, 2] and wants[0]["report"]["status"] == R.NO_KEYFRAME


@pytest.mark.gpu
def test_a_keyframe_of_five_null_key_points_is_never_close(ctx, P):
    streams = (Rc.three_keyframes(),)
    geo, cfg = TA.stage(ctx, streams), Rc.cfg()
    ctx.candidates_align_reserve(**cfg)
    kp = np.array([[-1] * 5, [0, 1, -1, -1, -1], [-1] * 5], np.int32)
    ctx.candidates_set_keypts([kp])
    jobs = [closest(Rc.far_T(-0.06))]
    ctx.candidates_align_build_kf(jobs)
    assert check(ctx, P, geo, cfg, streams, jobs, "null key points")[0]["report"]["ref_kf"] == 1


# ---- mixed batches and shapes ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_tracking_and_a_relocalising_stream_in_one_run(ctx, P):
    """stream 0 built by plsvo_candidates_align_build, stream 1 by _align_build_kf, run together: each stream's job and result equals
    its own single-source restatement"""
    streams = (A.only_points(), Rc.holes())
    geo, cfg = TA.stage(ctx, streams), Rc.cfg()
    ctx.candidates_align_reserve(**cfg)
    sels = TA.frame(ctx, P, streams)
    masks = [TA.ones(s) for s in sels]
    TA.build(ctx, sels, masks, [A.T_REF, A.T_REF], active=[True, False])
    jobs = [None, job(1)]
    ctx.candidates_align_build_kf(jobs)
    from_sel = TA.restate(ctx, geo, sels, masks, [A.T_REF, A.T_REF], cfg, active=[True, False])
    wants = restate(ctx, geo, cfg, jobs, prev=from_sel)
    assert wants[0]["n_pts"] == 9 and wants[1]["n_pts"] == 11 and wants[0]["report"].get("ref_kf", -1) == -1
    TA.check_jobs(ctx, P, geo, cfg, wants, "mixed")
    TA.check_run(ctx, P, geo, cfg, wants, "mixed", slots=[(0, 1), (1, CUR)])
    # and the other way round: the keyframe build first
    ctx.candidates_align_build_kf(jobs)
    TA.build(ctx, sels, masks, [A.T_REF, A.T_REF], active=[True, False])
    TA.check_jobs(ctx, P, geo, cfg, wants, "mixed, reversed")
    TA.check_run(ctx, P, geo, cfg, wants, "mixed, reversed", slots=[(0, 1), (1, CUR)])


@pytest.mark.gpu
def test_the_directed_cases_in_a_large_batch_and_in_one_of_two(ctx, P):
    """more than cu_count / 2 streams start their segments right behind the points (seg_align 32), two streams at a multiple of 64"""
    head = (Rc.holes(), Rc.shared(), Rc.kept_points(65))
    jobs_head = [job(1), job(1), job(0)]
    for n in (TA.large_n(ctx), 2):
        streams = head[:n] + tuple(Rc.tiny(k) for k in range(max(n - len(head), 0)))
        geo, cfg = TA.stage(ctx, streams), Rc.cfg(n_iter=2)
        ctx.candidates_align_reserve(**cfg)
        jobs = (jobs_head + [job(k % 2) for k in range(n)])[:len(streams)]
        ctx.candidates_align_build_kf(jobs)
        assert TA.seg_align_of(ctx, len(streams)) == (32 if n > 2 else 64)
        wants = restate(ctx, geo, cfg, jobs)
        TA.check_jobs(ctx, P, geo, cfg, wants[:8], ("batch", n), n=len(streams))
        TA.check_run(ctx, P, geo, cfg, wants, ("batch", n), slots=slots_of(streams, wants))   # (the restated jobs in a batch of the same size: the same launch shape)


# ---- the gates -------------------------------------------------------------------------------------------------------------------------
def tracked(ctx, P, streams, outliers):
    """a tracked frame up to the pose optimisation; outliers: per stream, every seventh match lands six pixels off and the pose optimiser
    rejects it.  -> per stream (n_matches, n_ls_matches, num_obs_pt, num_obs_ls, the optimised pose)"""
    TA.stage(ctx, streams)
    ctx.candidates_run([P.abi.CandidateFrameJob(s["T"], s["overlap"], cur_slot=1) for s in streams])
    matches = [TA.Sc.match_of(s, r) for s, r in zip(streams, ctx.candidates_fetch())]
    for m, off in zip(matches, outliers):
        if off:
            m["px"][::7] += 6.0
    ctx.candidates_set_match(matches)
    ctx.candidates_select(**A.PARAMS)
    sels = ctx.candidates_select_fetch()
    ctx.candidates_pose_optimize()
    po = ctx.candidates_pose_fetch([(s["n_matches"], s["n_ls_matches"]) for s in sels])
    return [(int(s["n_matches"]), int(s["n_ls_matches"]), int(p.num_obs_pt), int(p.num_obs_ls), np.array(p.T)) for s, p in zip(sels, po)]


def check_gate(ctx, jobs, facts, last, tag):
    """jobs as candidates_track_gate takes them; last: per stream the (pt, ls) the drops are taken against.  -> the records"""
    ctx.candidates_track_gate(jobs)
    got, carried = ctx.candidates_gate_fetch(poses=True)
    assert ctx.candidates_gate_poses_dev()
    for k, (j, f) in enumerate(zip(jobs, facts)):
        if j is None:
            continue
        kw = {p: j[p] for p in ("mode", "quality_min_fts", "quality_max_drop_fts", "max_fts", "max_fts_segs") if p in j}
        rec, T, _ = R.gate(f[0], f[1], f[2], f[3], last[k][0], last[k][1], f[4], j["T_reset"], **kw)
        assert got[k] == rec, (tag, k, got[k], rec)
        same_bytes(carried[k], T, (tag, "carried", k))
    return got, carried


@pytest.mark.gpu
def test_the_gates_around_every_threshold(own_ctx, P):
    """the streams' counts: 80 + 14 matched of which 68 + 14 are edges (every seventh match of the points is an outlier); 5 + 6 matched,
    4 + 6 = 10 edges; 9 points, all edges: 9; 6 segment features and no edge at all.  The thresholds are placed around them."""
    ctx = own_ctx
    streams = (A.eighty(), A.border(), A.only_points(), A.only_segments())
    facts = tracked(ctx, P, streams, outliers=(1, 1, 0, 0))
    m, e, op = [f[0] + f[1] for f in facts], [f[2] + f[3] for f in facts], [f[2] for f in facts]
    assert m == [94, 11, 9, 6] and e[0] < m[0] and e[1:] == [10, 9, 0]
    Tr = Rc.T_INIT
    base = dict(T_reset=Tr, num_obs_last=(0, 0))
    # matched at quality_min_fts - 1 and at quality_min_fts; edges 10 and 9
    jobs = [dict(base, quality_min_fts=m[0] + 1), dict(base, quality_min_fts=m[1]), dict(base, quality_min_fts=0), dict(base, quality_min_fts=0)]
    last = [(0, 0)] * 4
    got, carried = check_gate(ctx, jobs, facts, last, "matched")
    assert [g["result"] for g in got] == [R.FAIL_MATCHES, R.GATE_OK, R.FAIL_EDGES, R.FAIL_EDGES]
    assert [g["tracking_quality"] for g in got] == [R.INSUFFICIENT, R.BAD, R.INSUFFICIENT, R.INSUFFICIENT]   # stream 1: 10 edges < quality_min_fts 11
    same_bytes(carried[0], Tr, "FAIL_MATCHES resets")
    same_bytes(carried[1], facts[1][4], "OK carries the optimised pose")
    same_bytes(carried[2], facts[2][4], "FAIL_EDGES keeps the optimised pose under GATE_TRACK")
    # the relocalising mode resets on every failure
    got, carried = check_gate(ctx, [dict(j, mode=R.GATE_RELOC) for j in jobs], facts, last, "reloc")
    same_bytes(carried[0], Tr, "FAIL_MATCHES resets under GATE_RELOC")
    same_bytes(carried[2], Tr, "FAIL_EDGES resets under GATE_RELOC")
    same_bytes(carried[1], facts[1][4], "OK carries the optimised pose under GATE_RELOC")
    # a drop above the limit and one at it; a failure is INSUFFICIENT whatever the drop; the clamps of both kinds
    q = dict(T_reset=Tr, quality_min_fts=0, quality_max_drop_fts=50)
    jobs = [dict(q, num_obs_last=(op[0] + 51, 0), max_fts=10 ** 6), dict(q, num_obs_last=(op[1] + 50, 0)), dict(q, num_obs_last=(op[2] + 51, 0)),
            dict(q, num_obs_last=(400, 500), max_fts=50, max_fts_segs=3)]
    got, _ = check_gate(ctx, jobs, facts, [j["num_obs_last"] for j in jobs], "drops")
    assert [(g["drop_pt"], g["tracking_quality"]) for g in got] == [(51, R.BAD), (50, R.GOOD), (51, R.INSUFFICIENT), (50, R.INSUFFICIENT)]
    assert got[3]["drop_ls"] == 3 - facts[3][3]
    # edges below quality_min_fts with enough matches: OK, but BAD; num_obs_last_pt above max_fts: the clamp decides on both sides of the limit
    jobs = [dict(q, quality_min_fts=e[0] + 1, num_obs_last=(0, 0)), dict(q, num_obs_last=(400, 90), max_fts=op[1] + 50, max_fts_segs=7), None, None]
    got, _ = check_gate(ctx, jobs, facts, [(0, 0), (400, 90), None, None], "clamp at the limit")
    assert (got[0]["result"], got[0]["tracking_quality"]) == (R.GATE_OK, R.BAD)
    assert (got[1]["drop_pt"], got[1]["drop_ls"], got[1]["tracking_quality"]) == (50, 7 - facts[1][3], R.GOOD)   # the segments' drop decides nothing
    jobs[1] = dict(jobs[1], max_fts=op[1] + 51, max_fts_segs=100)
    got, _ = check_gate(ctx, jobs, facts, [(0, 0), (400, 90), None, None], "clamp above the limit")
    assert (got[1]["drop_pt"], got[1]["drop_ls"], got[1]["tracking_quality"]) == (51, 90 - facts[1][3], R.BAD)


@pytest.mark.gpu
def test_resident_counts_across_two_calls_and_an_inactive_stream(own_ctx, P):
    ctx = own_ctx
    streams = (A.eighty(), A.border(), A.only_points())
    facts = tracked(ctx, P, streams, outliers=(1, 1, 1))
    base = dict(T_reset=Rc.T_INIT, quality_min_fts=1, quality_max_drop_fts=3)
    with pytest.raises(P.capi.PlsvoError):                            # no resident counts before the first gate since the stage
        ctx.candidates_track_gate([dict(base)] * 3)
    jobs = [dict(base, num_obs_last=(7, 2)), dict(base, num_obs_last=(1, 1)), None]
    got1, carried1 = check_gate(ctx, jobs, facts, [(7, 2), (1, 1), None], "host counts")
    assert got1[2] == dict.fromkeys(got1[2], 0) and not carried1[2].any(), "a stream that sat every call out reads as zeros"
    # the second call: the resident counts are the frame's n_matches / n_ls_matches (Frame::nObs()); stream 1 sits it out and keeps its rows
    jobs = [dict(base), None, dict(base, num_obs_last=(0, 0), mode=R.GATE_RELOC)]
    got2, carried2 = check_gate(ctx, jobs, facts, [(facts[0][0], facts[0][1]), None, (0, 0)], "resident counts")
    assert got2[1] == got1[1]
    same_bytes(carried2[1], carried1[1], "an inactive stream keeps its pose")
    assert got2[0]["drop_pt"] == min(facts[0][0], 100) - facts[0][2] > 3 and got2[0]["tracking_quality"] == R.BAD
    # and its resident counts survived the call it sat out
    jobs = [None, dict(base), None]
    check_gate(ctx, jobs, facts, [None, (facts[1][0], facts[1][1]), None], "kept counts")


# ---- every error return ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_reloc_error_paths(own_ctx, P):
    ctx, E = own_ctx, P.capi.PlsvoError

    def refused(code, f, *a):
        with pytest.raises(E) as e:
            f(*a)
        assert e.value.code == code, (e.value.code, str(e.value))

    INVALID, STATE = P.abi.E_INVALID, P.abi.E_STATE
    streams = (Rc.three_keyframes(), Rc.holes())
    geo = TA.stage(ctx, streams)
    refused(STATE, ctx.candidates_align_build_kf, [job(0), job(0)])                               # no reserve
    refused(STATE, ctx.candidates_track_gate, [dict(T_reset=Rc.T_INIT, num_obs_last=(0, 0))] * 2)   # no pose optimisation
    refused(STATE, ctx.candidates_gate_fetch)
    assert not ctx.candidates_gate_poses_dev()
    cfg = Rc.cfg()
    ctx.candidates_align_reserve(**cfg)
    refused(STATE, ctx.candidates_align_build_kf, [closest(Rc.far_T(0.0)), None])                 # CLOSEST without a live key-point table
    before = ctx.candidates_align_fetch()
    refused(INVALID, ctx.candidates_align_build_kf, [job(0)])                                     # another n
    refused(INVALID, ctx.candidates_align_build_kf, [job(3), None])                               # a row outside the keyframes
    refused(INVALID, ctx.candidates_align_build_kf, [job(-2), None])
    refused(INVALID, ctx.candidates_align_build_kf, [job(0, cur_slot=TA.N_SLOTS), None])          # a slot outside the pyramids
    refused(INVALID, ctx.candidates_align_build_kf, [job(0, raw=dict(init_source=3)), None])      # an unknown source
    refused(INVALID, ctx.candidates_align_build_kf, [job(0, raw=dict(init_source=P.abi.ALIGN_INIT_DEV)), None])   # no pointer
    ctx.candidates_set_keypts()
    refused(INVALID, ctx.candidates_align_build_kf, [closest(Rc.far_T(0.0), self_kf=3), None])
    refused(INVALID, ctx.candidates_align_build_kf, [closest(Rc.far_T(0.0), raw=dict(last_source=P.abi.INSERT_POSE_DEV)), None])
    refused(INVALID, ctx.candidates_align_build_kf, [closest(Rc.far_T(0.0), raw=dict(last_source=7)), None])
    assert ctx.candidates_align_fetch() == before, "nothing was enqueued"
    ctx.candidates_align_build_kf([closest(Rc.far_T(0.0)), job(1)])
    # a keyframe whose slot lies outside the pyramids
    far = copy.deepcopy(Rc.holes()); far["st"]["kf_slot"][1] = TA.N_SLOTS
    TA.stage(ctx, (far,))
    ctx.candidates_align_reserve(**cfg)
    refused(INVALID, ctx.candidates_align_build_kf, [job(1)])
    ctx.candidates_align_build_kf([job(0)])
    # the gate's arguments
    TA.stage(ctx, streams)
    TA.frame(ctx, P, streams)
    ctx.candidates_pose_optimize()
    g = dict(T_reset=Rc.T_INIT, num_obs_last=(0, 0))
    refused(INVALID, ctx.candidates_track_gate, [g])
    for bad in (dict(mode=2), dict(quality_min_fts=-1), dict(quality_max_drop_fts=-1), dict(max_fts=-1), dict(max_fts_segs=-1), dict(num_obs_last=(-1, 0))):
        refused(INVALID, ctx.candidates_track_gate, [dict(g, **bad), None])
    refused(STATE, ctx.candidates_track_gate, [dict(T_reset=Rc.T_INIT), None])                    # resident counts before the first gate
    refused(STATE, ctx.candidates_gate_fetch)
    ctx.candidates_track_gate([g, None])
    assert len(ctx.candidates_gate_fetch()) == 2
    TA.stage(ctx, streams)                                                                       # a stage drops the gate's rows
    refused(STATE, ctx.candidates_gate_fetch)
