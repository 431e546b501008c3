"""run_sequence(map_candidates=True, cell_select=True): candidates, match, cell selection and pose optimisation as one enqueue sequence on
resident tables (plsvo_candidates_select ..), chained into the harness.  Every frame's selection and the quality state it
leaves equal the restatement tests/np_select.py on the inputs the harness recorded -- the tables the harness keeps by following the
backend's event flags must BE the backend's tables -- the counters survive the restage at a keyframe, and without cell_select nothing
changes.  Run twice: on the CPU with an oracle-backed backend whose map_select is np_candidates + the oracle's matcher + np_select + the
oracle's pose optimiser, and under `gpu` with HipBackend."""
import copy
import importlib

import numpy as np
import pytest

import np_candidates as N
import np_select as S
from test_sequence import OracleBackend

SEL_FIELDS = ("pt_lm", "pt_px", "pt_level", "pt_type", "pt_grad", "seg_lm", "seg_px", "seg_level")
CAND_FIELDS = ("pt_lm", "pt_px", "pt_cell", "pt_obs", "pt_has_view", "pt_active", "seg_lm", "seg_px", "seg_cell", "seg_obs", "seg_has_view", "seg_active", "kf_count",
               "pt_cand_failed", "seg_cand_failed")


def same_bytes(got, want, tag):
    g = np.asarray(got)
    w = np.asarray(want, dtype=g.dtype).reshape(g.shape if g.size else (-1,) + g.shape[1:])
    assert g.shape == w.shape and g.tobytes() == w.tobytes(), (tag, g, w)


def stream_of(job):
    """an abi.CandidateMapJob's CSR arrays back as the dict of lists tests/np_candidates.py reads"""
    t = job.t
    cut = lambda v, off: [[x for x in v[off[k]:off[k + 1]]] for k in range(len(off) - 1)]
    po, so = t["pt_obs_off"], t["seg_obs_off"]
    pt_obs = [[dict(kf=int(t["pt_obs_kf"][o]), px=[float(x) for x in t["pt_obs_px"][o]], f=[float(x) for x in t["pt_obs_f"][o]], level=int(t["pt_obs_level"][o]),
                    type=int(t["pt_obs_type"][o]), grad=[float(x) for x in t["pt_obs_grad"][o]]) for o in range(po[k], po[k + 1])] for k in range(len(po) - 1)]
    seg_obs = [[dict(kf=int(t["seg_obs_kf"][o]), spx=[float(x) for x in t["seg_obs_spx"][o]], epx=[float(x) for x in t["seg_obs_epx"][o]],
                     sf=[float(x) for x in t["seg_obs_sf"][o]], ef=[float(x) for x in t["seg_obs_ef"][o]], level=int(t["seg_obs_level"][o])) for o in range(so[k], so[k + 1])]
               for k in range(len(so) - 1)]
    f3 = lambda a: [[float(x) for x in v] for v in a]
    return dict(kf_T=f3(t["kf_T"]), kf_slot=[int(v) for v in t["kf_slot"]], kf_pt=[[int(x) for x in l] for l in cut(t["kf_pt_lm"], t["kf_pt_off"])],
                kf_seg=[[int(x) for x in l] for l in cut(t["kf_seg_lm"], t["kf_seg_off"])], pt_pos=f3(t["pt_pos"]), pt_type=[int(v) for v in t["pt_type"]], pt_obs=pt_obs,
                seg_spos=f3(t["seg_spos"]), seg_epos=f3(t["seg_epos"]), seg_type=[int(v) for v in t["seg_type"]], seg_obs=seg_obs,
                pt_cand=[int(v) for v in t["pt_cand"]], seg_cand=[int(v) for v in t["seg_cand"]])


class OracleSelectBackend(OracleBackend):
    """test infrastructure: OracleBackend with the map part of a frame in the restatements' and the oracle's hands -- np_candidates, the
    oracle's direct matcher on the entries the stage marks active, np_select on the backend's OWN copy of the tables (which it mutates, as
    the device mutates the resident ones), the oracle's pose optimiser on the selection.  Returns what HipBackend.map_select returns."""

    def __init__(self, ob, P, n_levels=4):
        OracleBackend.__init__(self, ob, n_levels)
        self.abi, self.st, self.restages = P.abi, None, 0

    def map_select(self, map_job, frame_job, cam, n_pyr_levels, select, carry=None, cell_size=30, seg_cell_size=30):
        A = self.abi
        if map_job is not None:
            self.st = S.quality(stream_of(map_job))                                   # counters zero after a stage ...
            self.restages += 1
            if carry is not None:                                                     # ... unless the caller puts them back
                for name in ("pt", "seg"):
                    self.st[name + "_nfail"] = [int(v) for v in carry[name + "_n_failed"]]
                    self.st[name + "_nsucc"] = [int(v) for v in carry[name + "_n_succeeded"]]
        st, cam = self.st, tuple(cam)
        T, overlap, cur_slot = [float(v) for v in frame_job.c.T_f_w], [int(v) for v in frame_job.overlap_idx], int(frame_job.c.cur_slot)
        r = N.candidates(st, T, overlap, cam, cell_size, seg_cell_size, 8)
        n_pt, n_seg, n_kf = r["n_filed_pt"], r["n_filed_seg"], len(st["kf_T"])
        rows = []                                                                     # (active, reference observation, position, projection)
        for i, (lm, o) in enumerate(zip(r["pt_lm"], r["pt_obs"])):
            ob_ = st["pt_obs"][lm][o] if o >= 0 else None
            rows.append((r["pt_active"][i], ob_ and (ob_["kf"], ob_["px"], ob_["f"], ob_["level"], ob_["type"], ob_["grad"]), st["pt_pos"][lm], r["pt_px"][i]))
        for e, (pk, fk, posk) in enumerate((("spx", "sf", "seg_spos"), ("epx", "ef", "seg_epos"))):
            for i, (lm, o) in enumerate(zip(r["seg_lm"], r["seg_obs"])):
                ob_ = st["seg_obs"][lm][o] if o >= 0 else None
                rows.append((r["seg_active"][i], ob_ and (ob_["kf"], ob_[pk], ob_[fk], ob_["level"], 0, (0.0, 0.0)), st[posk][lm], r["seg_px"][i][2 * e:2 * e + 2]))
        k = len(rows)
        mr = dict(found=np.zeros(k, np.uint8), px=np.array([row[3] for row in rows], float).reshape(-1, 2), search_level=np.full(k, -1, np.int32))
        act = [i for i, row in enumerate(rows) if row[0]]
        if act:
            job = A.MatchJob(cam, list(st["kf_T"]) + [T], list(st["kf_slot"]) + [cur_slot], [n_kf] * len(act), [rows[i][1][0] for i in act],
                             [rows[i][1][1] for i in act], [rows[i][1][2] for i in act], [rows[i][1][3] for i in act], [rows[i][1][4] for i in act],
                             [rows[i][1][5] for i in act], [rows[i][2] for i in act], [rows[i][3] for i in act], n_pyr_levels=n_pyr_levels, align_max_iter=10)
            m = self.match_direct(job)
            mr["found"][act], mr["px"][act], mr["search_level"][act] = m["found"], m["px_cur"], m["search_level"]
        before = copy.deepcopy(st["pt_type"]), copy.deepcopy(st["seg_type"])
        w = S.select(st, r, mr, cam, cell_size, seg_cell_size, select["max_fts"], select["max_fts_segs"], select["cell_order"], select["seg_cell_order"])
        sel = dict(n_matches=w["n_matches"], n_ls_matches=w["n_ls_matches"], n_trials=w["n_trials"],
                   pt_lm=np.array(w["pt_lm"], np.int32), pt_px=np.array(w["pt_px"], float).reshape(-1, 2), pt_level=np.array(w["pt_level"], np.int32),
                   pt_type=np.array(w["pt_type"], np.uint8), pt_grad=np.array(w["pt_grad"], float).reshape(-1, 2), seg_lm=np.array(w["seg_lm"], np.int32),
                   seg_px=np.array(w["seg_px"], float).reshape(-1, 4), seg_level=np.array(w["seg_level"], np.int32))

        def bearing(px):
            x, y = (px[:, 0] - cam[2]) / cam[0], (px[:, 1] - cam[3]) / cam[1]
            n = np.sqrt((x * x + y * y) + 1.0)
            return np.stack([x / n, y / n, 1.0 / n], -1)
        sf, ef = bearing(sel["seg_px"][:, 0:2]), bearing(sel["seg_px"][:, 2:4])
        l = np.stack([sf[:, 1] * ef[:, 2] - sf[:, 2] * ef[:, 1], sf[:, 2] * ef[:, 0] - sf[:, 0] * ef[:, 2], sf[:, 0] * ef[:, 1] - sf[:, 1] * ef[:, 0]], -1)
        line = l / np.sqrt(l[:, 0] * l[:, 0] + l[:, 1] * l[:, 1])[:, None] if len(l) else np.zeros((0, 3))
        pr = self.pose_optimize(A.PoseOptJob(T, abs(cam[0]), select.get("reproj_thresh", 2.0), select.get("poseopt_n_iter", 10), bearing(sel["pt_px"]),
                                             np.array(st["pt_pos"]).reshape(-1, 3)[sel["pt_lm"]], np.maximum(sel["pt_level"], 0), line,
                                             np.array(st["seg_spos"]).reshape(-1, 3)[sel["seg_lm"]], np.array(st["seg_epos"]).reshape(-1, 3)[sel["seg_lm"]],
                                             np.maximum(sel["seg_level"], 0)))
        cr = dict(n_filed_pt=n_pt, n_filed_seg=n_seg)
        for f, dt, shape in (("pt_lm", np.int32, (-1,)), ("pt_px", float, (-1, 2)), ("pt_cell", np.int32, (-1,)), ("pt_obs", np.int32, (-1,)), ("pt_has_view", np.uint8, (-1,)),
                             ("pt_active", np.uint8, (-1,)), ("seg_lm", np.int32, (-1,)), ("seg_px", float, (-1, 4)), ("seg_cell", np.int32, (-1, 2)), ("seg_obs", np.int32, (-1,)),
                             ("seg_has_view", np.uint8, (-1,)), ("seg_active", np.uint8, (-1,)), ("kf_count", np.int32, (-1,)), ("pt_cand_failed", np.uint8, (-1,)),
                             ("seg_cand_failed", np.uint8, (-1,))):
            cr[f] = np.array(r[f], dt).reshape(shape)
        q = dict(pt_n_failed=np.array(st["pt_nfail"], np.int32), pt_n_succeeded=np.array(st["pt_nsucc"], np.int32), pt_type=np.array(st["pt_type"], np.int32),
                 pt_event=np.array(w["pt_event"], np.uint8), seg_n_failed=np.array(st["seg_nfail"], np.int32), seg_n_succeeded=np.array(st["seg_nsucc"], np.int32),
                 seg_type=np.array(st["seg_type"], np.int32), seg_event=np.array(w["seg_event"], np.uint8), pt_cand=np.array(st["pt_cand"], np.int32),
                 seg_cand=np.array(st["seg_cand"], np.int32))
        return cr, mr, sel, pr, q


@pytest.fixture(scope="module")
def seqm():
    return importlib.import_module("pl-svo_amd.sequence")


def check_frames(seq, res):
    """every recorded frame against the restatement on the tables the HARNESS held before it"""
    cam = tuple(seq["cam"])
    n_trials = n_events = 0
    for k, r in enumerate(res[1:], 1):
        c = r["candidates"]
        st = copy.deepcopy(c["stream"])
        before = c["quality_before"]
        for name in ("pt", "seg"):
            n = len(st[name + "_type"])
            st[name + "_nfail"] = [0] * n if before is None else [int(v) for v in before[name + "_n_failed"]]
            st[name + "_nsucc"] = [0] * n if before is None else [int(v) for v in before[name + "_n_succeeded"]]
        cand = N.candidates(st, c["T"], c["overlap"], cam, 30, 30, 8)
        assert (c["out"]["n_filed_pt"], c["out"]["n_filed_seg"]) == (cand["n_filed_pt"], cand["n_filed_seg"]), k
        for f in CAND_FIELDS:
            same_bytes(c["out"][f][:len(cand[f])], cand[f], (k, f))                 # (a candidate list may have closed up since it was staged)
        p = c["select_params"]
        w = S.select(st, cand, c["match"], cam, 30, 30, p["max_fts"], p["max_fts_segs"], p["cell_order"], p["seg_cell_order"])
        g, q = c["select"], c["quality"]
        assert (g["n_matches"], g["n_ls_matches"], g["n_trials"]) == (w["n_matches"], w["n_ls_matches"], w["n_trials"]), k
        for f in SEL_FIELDS:
            same_bytes(g[f], w[f], (k, f))
        for f, key in (("pt_n_failed", "pt_nfail"), ("pt_n_succeeded", "pt_nsucc"), ("pt_type", "pt_type"), ("seg_n_failed", "seg_nfail"), ("seg_n_succeeded", "seg_nsucc"),
                       ("seg_type", "seg_type"), ("pt_cand", "pt_cand"), ("seg_cand", "seg_cand")):
            same_bytes(q[f], st[key], (k, f))
        same_bytes(q["pt_event"], w["pt_event"], (k, "pt_event")); same_bytes(q["seg_event"], w["seg_event"], (k, "seg_event"))
        assert r["n_matched_pt"] == g["n_matches"] and r["n_trials"] == g["n_trials"] and r["n_kept_pt"] <= g["n_matches"]
        n_trials += g["n_trials"]; n_events += r["n_promoted"] + r["n_deleted"]
    assert n_trials > 40 * (len(res) - 1) and all(np.isfinite(r["T"]).all() for r in res)
    assert n_events > 0                                     # eleven successes promote a landmark: the types do change between keyframes


def check_carry(res):
    """a frame after a keyframe starts from the counters the frame before it left, although the tables were staged anew in between"""
    restaged = [k for k in range(2, len(res)) if len(res[k]["candidates"]["stream"]["kf_T"]) > len(res[k - 1]["candidates"]["stream"]["kf_T"])]
    assert restaged, "no keyframe was added"
    for k in restaged:
        before, q = res[k]["candidates"]["quality_before"], res[k]["candidates"]["quality"]
        assert before["pt_n_succeeded"].sum() > 0
        moved = (q["pt_n_succeeded"] - before["pt_n_succeeded"]) + (q["pt_n_failed"] - before["pt_n_failed"])
        assert (moved >= 0).all() and moved.sum() > 0 and (q["pt_n_succeeded"] >= before["pt_n_succeeded"]).all()
        for f in ("pt_n_failed", "pt_n_succeeded", "seg_n_failed", "seg_n_succeeded"):
            same_bytes(before[f], res[k - 1]["candidates"]["quality"][f], (k, f))
    return restaged


# ---- on the CPU: the oracle-backed backend ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def run_cpu(P, ob, seqm):
    """14 frames, every fourth a keyframe (the oracle-backed backend has no keyframe stage): a landmark tracked from frame 1 on is promoted
    at its eleventh success, after two restages"""
    seq = seqm.make_sequence(11, n_frames=14, W=320, H=240, n_pts=100, n_seg=20, step_scale=0.5)
    backend = OracleSelectBackend(ob, P)
    res = seqm.run_sequence(backend, seq, mapping=True, kf_every=4, map_candidates=True, cell_select=True, record_candidates=True)
    return seq, res, backend


def test_cpu_every_frame_equals_the_restatement_on_the_recorded_inputs(run_cpu):
    seq, res, backend = run_cpu
    check_frames(seq, res)


def test_cpu_counters_carry_over_a_keyframe_restage(run_cpu):
    seq, res, backend = run_cpu
    restaged = check_carry(res)
    assert backend.restages >= 1 + len(restaged)
    # the harness restages only when the map's structure changes: not on the frames where only types, counters or lists moved
    assert backend.restages < len(res) - 1


def test_cpu_a_promoted_landmark_keeps_its_type_over_a_keyframe(run_cpu):
    """the keyframe branch turns a matched TYPE_CANDIDATE into TYPE_UNKNOWN and nothing else: a landmark promoted to TYPE_GOOD before a
    keyframe is still TYPE_GOOD in the tables staged after it"""
    seq, res, backend = run_cpu
    A = backend.abi
    seen = 0
    for k in range(2, len(res)):
        prev_q, st = res[k - 1]["candidates"]["quality"], res[k]["candidates"]["stream"]
        good = np.nonzero(prev_q["pt_type"] == A.LM_GOOD)[0]
        assert all(st["pt_type"][int(i)] == A.LM_GOOD for i in good), k
        if len(st["kf_T"]) > len(res[k - 1]["candidates"]["stream"]["kf_T"]):
            seen += len(good)
    assert seen > 0


def test_cpu_cell_select_needs_map_candidates_and_a_backend_with_map_select(P, ob, seqm):
    seq = seqm.make_sequence(11, n_frames=3, W=320, H=240, n_pts=60, n_seg=10, step_scale=0.5)
    with pytest.raises(ValueError):
        seqm.run_sequence(OracleSelectBackend(ob, P), seq, cell_select=True)
    with pytest.raises(ValueError):
        seqm.run_sequence(OracleBackend(ob), seq, map_candidates=True, cell_select=True)


# ---- on the device ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def run(gpu_ctx, seqm):
    seq = seqm.make_sequence(11, n_frames=12, W=320, H=240, n_pts=100, n_seg=20, step_scale=0.5)
    res = seqm.run_sequence(seqm.HipBackend(gpu_ctx), seq, mapping=True, kf_select=True, map_candidates=True, cell_select=True, record_candidates=True)
    return seq, res


@pytest.mark.gpu
def test_every_frame_equals_the_restatement_on_the_recorded_inputs(run):
    seq, res = run
    check_frames(seq, res)


@pytest.mark.gpu
def test_counters_carry_over_a_keyframe_restage(run):
    seq, res = run
    check_carry(res)


@pytest.mark.gpu
def test_without_cell_select_the_records_are_what_they_were(gpu_ctx, seqm):
    seq = seqm.make_sequence(11, n_frames=5, W=320, H=240, n_pts=100, n_seg=20, step_scale=0.5)
    plain = seqm.run_sequence(seqm.HipBackend(gpu_ctx), seq, map_candidates=True)
    off = seqm.run_sequence(seqm.HipBackend(gpu_ctx), seq, map_candidates=True, cell_select=False)
    assert len(plain) == len(off)
    for a, b in zip(plain, off):
        assert set(a) == set(b) and "n_trials" not in a
        for f in a:
            assert np.asarray(a[f]).tobytes() == np.asarray(b[f]).tobytes(), f
    with pytest.raises(ValueError):
        seqm.run_sequence(seqm.HipBackend(gpu_ctx), seq, cell_select=True)
