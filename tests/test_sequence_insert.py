"""run_sequence(map_candidates=True, cell_select=True, kf_insert=True): a keyframe is inserted into the resident tables on the device
(plsvo_candidates_insert_keyframe ..) instead of being staged anew.  Every keyframe's tables equal the restatement
tests/np_insert.py run on the tables the harness recorded before it; the stage is called only at the start and when a seed converges;
with max_n_kfs the table stays that small.  Run twice: on the CPU with an oracle-backed backend whose map_insert is np_insert, and under
`gpu` with HipBackend."""
import copy
import importlib

import numpy as np
import pytest

import candidates_cases as Cc
import np_insert as I
import np_keyframe as K
import np_select as S
from test_sequence_select import OracleSelectBackend, same_bytes

QUALITY = (("pt_n_failed", "pt_nfail"), ("pt_n_succeeded", "pt_nsucc"), ("pt_type", "pt_type"), ("seg_n_failed", "seg_nfail"), ("seg_n_succeeded", "seg_nsucc"),
           ("seg_type", "seg_type"), ("pt_cand", "pt_cand"), ("seg_cand", "seg_cand"))


class OracleInsertBackend(OracleSelectBackend):
    """test infrastructure: OracleSelectBackend whose tables stay resident over a keyframe -- map_insert is np_insert on the backend's
    OWN tables with the last selection and the last pose optimisation, as the device uses its resident ones; the keyframe stage is the
    restatement tests/np_keyframe.py"""

    def __init__(self, ob, P, n_levels=4):
        OracleSelectBackend.__init__(self, ob, P, n_levels)
        self.staged_at, self.last, self.reserve = [], None, None

    def close_keyframes(self, job):
        return K.close(job)

    def keyframe_decide(self, job):
        return K.decide(job)

    def map_reserve(self, **room):
        self.reserve = room

    def map_select(self, map_job, frame_job, cam, n_pyr_levels, select, carry=None, cell_size=30, seg_cell_size=30):
        if map_job is not None:
            self.staged_at.append(int(frame_job.c.cur_slot))
        out = OracleSelectBackend.map_select(self, map_job, frame_job, cam, n_pyr_levels, select, carry, cell_size, seg_cell_size)
        self.last = dict(sel=out[2], pose=out[3], events=(out[4]["pt_event"], out[4]["seg_event"]), cam=tuple(cam))
        return out

    def map_insert(self, remove_kf, kf_slot):
        st, L = self.st, self.last
        out = I.insert(st, L["sel"], L["pose"].pt_keep, L["pose"].seg_keep, [float(v) for v in L["pose"].T], kf_slot, remove_kf, L["cam"])
        q = dict(pt_n_failed=np.array(st["pt_nfail"], np.int32), pt_n_succeeded=np.array(st["pt_nsucc"], np.int32), pt_type=np.array(st["pt_type"], np.int32),
                 pt_event=L["events"][0] | np.array(out["pt_event"], np.uint8), seg_n_failed=np.array(st["seg_nfail"], np.int32), seg_n_succeeded=np.array(st["seg_nsucc"], np.int32),
                 seg_type=np.array(st["seg_type"], np.int32), seg_event=L["events"][1] | np.array(out["seg_event"], np.uint8), pt_cand=np.array(st["pt_cand"], np.int32),
                 seg_cand=np.array(st["seg_cand"], np.int32))
        rep = dict(n_kf=len(st["kf_T"]), new_kf=out["new_kf"], n_joined_pt=out["n_joined_pt"], n_joined_seg=out["n_joined_seg"], n_deleted_pt=out["n_deleted_pt"],
                   n_deleted_seg=out["n_deleted_seg"])
        return Cc.to_job(st).t, q, rep

    def map_set_positions(self, pt_idx, pt_pos):
        for i, p in zip(pt_idx, pt_pos):
            self.st["pt_pos"][int(i)] = [float(v) for v in p]


@pytest.fixture(scope="module")
def seqm():
    return importlib.import_module("pl-svo_amd.sequence")


def check_insertions(seq, res, seqm):
    """every keyframe's tables against the restatement on the tables the HARNESS held before it; -> the keyframes' frame numbers"""
    cam = tuple(seq["cam"])
    kfs = [k for k, r in enumerate(res) if "insert" in r]
    n_joined = 0
    for k in kfs:
        c = res[k]["insert"]
        st = copy.deepcopy(c["stream"])
        for name in ("pt", "seg"):
            st[name + "_nfail"] = [int(v) for v in c["quality_before"][name + "_n_failed"]]
            st[name + "_nsucc"] = [int(v) for v in c["quality_before"][name + "_n_succeeded"]]
        out = I.insert(st, c["select"], c["pt_keep"], c["seg_keep"], c["T"], c["slot"], c["remove_kf"], cam)
        want = Cc.to_job(st).t
        for f in Cc.abi._CAND_MAP_ORDER:
            same_bytes(c["tables"][f], want[f], (k, f))
        for f, key in QUALITY:
            same_bytes(c["quality"][f], st[key], (k, f))
        for name in ("pt", "seg"):
            same_bytes(c["quality"][name + "_event"] & (I.EVENT_JOINED | I.EVENT_DELETED) | np.array(out[name + "_event"], np.uint8),
                       c["quality"][name + "_event"] & (I.EVENT_JOINED | I.EVENT_DELETED), (k, name, "events hold the insertion's"))
        assert c["report"]["new_kf"] == out["new_kf"] == len(st["kf_T"]) - 1 and c["report"]["n_joined_pt"] == out["n_joined_pt"], k
        assert res[k]["n_joined"] == out["n_joined_pt"] + out["n_joined_seg"] and res[k]["remove_kf"] == c["remove_kf"]
        if k + 1 < len(res):                                           # the next frame ran on these tables: the harness's own are the fetched ones
            nxt = res[k + 1]["candidates"]["stream"]
            assert nxt["kf_T"] == st["kf_T"] and nxt["kf_pt"] == st["kf_pt"] and nxt["kf_seg"] == st["kf_seg"] and nxt["pt_obs"] == st["pt_obs"] and nxt["seg_obs"] == st["seg_obs"]
        n_joined += out["n_joined_pt"]
    return kfs, n_joined


def check_stage_calls(res, staged_at):
    """the stage is called at the first frame and on the frame after a seed converged, and nowhere else: at no keyframe"""
    want = [1] + [k + 1 for k in range(1, len(res) - 1) if res[k].get("n_seed_candidates", 0) > 0]       # (a seed whose keyframe has left adds nothing)
    assert staged_at == want, (staged_at, want)
    kfs = [k for k, r in enumerate(res) if "insert" in r]
    assert any(k + 1 not in staged_at for k in kfs if k + 1 < len(res)), "every keyframe was followed by a stage"


def check_table_size(res, max_n_kfs):
    sizes = []
    for r in res[1:]:
        st = r["candidates"]["stream"]
        n_kf = len(st["kf_T"])
        sizes.append(n_kf)
        assert n_kf <= max_n_kfs and all(0 <= o["kf"] < n_kf for name in ("pt_obs", "seg_obs") for l in st[name] for o in l)
        assert all(0 <= v < n_kf for v in r["candidates"]["overlap"])
    assert max(sizes) == max_n_kfs and any(r.get("remove_kf", -1) >= 0 for r in res)
    # a seed that converges is observed in frame 0's keyframe, wherever the removals have moved that row, and nowhere once it is gone
    row = 0
    for k, r in enumerate(res[1:-1], 1):
        if r.get("remove_kf", -1) >= 0 and row is not None:
            row = None if r["remove_kf"] == row else row - (r["remove_kf"] < row)
        if r.get("n_seed_converged", 0) > 0:
            assert (r["n_seed_candidates"] > 0) == (row is not None), k
            if row is not None:
                nxt = res[k + 1]["candidates"]["stream"]
                assert nxt["kf_slot"][row] == 0 and all(nxt["pt_obs"][lm][-1]["kf"] == row for lm in nxt["pt_cand"][-r["n_seed_candidates"]:]), k


# ---- on the CPU: the oracle-backed backend ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def run_cpu(P, ob, seqm):
    seq = seqm.make_sequence(11, n_frames=14, W=320, H=240, n_pts=100, n_seg=20, step_scale=0.5)
    backend = OracleInsertBackend(ob, P)
    res = seqm.run_sequence(backend, seq, mapping=True, kf_every=4, map_candidates=True, cell_select=True, record_candidates=True, kf_insert=True)
    return seq, res, backend


def test_cpu_every_keyframe_equals_the_restatement_on_the_recorded_tables(run_cpu, seqm):
    seq, res, backend = run_cpu
    kfs, n_joined = check_insertions(seq, res, seqm)
    assert kfs == [4, 8, 12] and backend.reserve == {}                # (the harness gives the room back when it is done)


def test_cpu_the_stage_is_called_at_the_start_and_when_a_seed_converges(run_cpu):
    seq, res, backend = run_cpu
    check_stage_calls(res, backend.staged_at)


def test_cpu_the_table_never_exceeds_max_n_kfs(P, ob, seqm):
    seq = seqm.make_sequence(11, n_frames=12, W=320, H=240, n_pts=100, n_seg=20, step_scale=0.5)
    backend = OracleInsertBackend(ob, P)
    res = seqm.run_sequence(backend, seq, mapping=True, kf_select=True, kfselect_mindist_t=0.03, max_n_kfs=3, map_candidates=True, cell_select=True, record_candidates=True,
                            kf_insert=True)
    check_insertions(seq, res, seqm)
    check_table_size(res, 3)
    check_stage_calls(res, backend.staged_at)


def test_cpu_without_kf_insert_the_records_are_what_they_were(P, ob, seqm):
    seq = seqm.make_sequence(11, n_frames=6, W=320, H=240, n_pts=100, n_seg=20, step_scale=0.5)
    plain = seqm.run_sequence(OracleSelectBackend(ob, P), seq, mapping=True, kf_every=2, map_candidates=True, cell_select=True)
    off = seqm.run_sequence(OracleInsertBackend(ob, P), seq, mapping=True, kf_every=2, map_candidates=True, cell_select=True, kf_insert=False)
    assert len(plain) == len(off)
    for a, b in zip(plain, off):
        assert set(a) == set(b) and "n_joined" not in a
        for f in a:
            assert np.asarray(a[f]).tobytes() == np.asarray(b[f]).tobytes(), f
    with pytest.raises(ValueError):
        seqm.run_sequence(OracleSelectBackend(ob, P), seq, mapping=True, map_candidates=True, cell_select=True, kf_insert=True)     # no map_insert
    with pytest.raises(ValueError):
        seqm.run_sequence(OracleInsertBackend(ob, P), seq, mapping=True, map_candidates=True, kf_insert=True)                      # no cell_select


# ---- on the device ------------------------------------------------------------------------------------------------------------------------
def counting_backend(seqm, ctx):
    class Counting(seqm.HipBackend):
        def map_select(self, map_job, frame_job, *a, **kw):
            if map_job is not None:
                self.staged_at.append(int(frame_job.c.cur_slot))
            return seqm.HipBackend.map_select(self, map_job, frame_job, *a, **kw)
    b = Counting(ctx)
    b.staged_at = []
    return b


@pytest.mark.gpu
def test_every_keyframe_equals_the_restatement_and_no_keyframe_stages(gpu_ctx, seqm):
    seq = seqm.make_sequence(11, n_frames=12, W=320, H=240, n_pts=100, n_seg=20, step_scale=0.5)
    backend = counting_backend(seqm, gpu_ctx)
    res = seqm.run_sequence(backend, seq, mapping=True, kf_select=True, map_candidates=True, cell_select=True, record_candidates=True, kf_insert=True)
    kfs, _ = check_insertions(seq, res, seqm)
    assert len(kfs) >= 2
    check_stage_calls(res, backend.staged_at)


@pytest.mark.gpu
def test_the_table_never_exceeds_max_n_kfs(gpu_ctx, seqm):
    seq = seqm.make_sequence(11, n_frames=12, W=320, H=240, n_pts=100, n_seg=20, step_scale=0.5)
    backend = counting_backend(seqm, gpu_ctx)
    res = seqm.run_sequence(backend, seq, mapping=True, kf_select=True, kfselect_mindist_t=0.03, max_n_kfs=3, map_candidates=True, cell_select=True, record_candidates=True,
                            kf_insert=True)
    check_insertions(seq, res, seqm)
    check_table_size(res, 3)
    check_stage_calls(res, backend.staged_at)


@pytest.mark.gpu
def test_without_kf_insert_the_records_are_what_they_were(gpu_ctx, seqm):
    seq = seqm.make_sequence(11, n_frames=6, W=320, H=240, n_pts=100, n_seg=20, step_scale=0.5)
    plain = seqm.run_sequence(seqm.HipBackend(gpu_ctx), seq, mapping=True, kf_select=True, map_candidates=True, cell_select=True)
    off = seqm.run_sequence(seqm.HipBackend(gpu_ctx), seq, mapping=True, kf_select=True, map_candidates=True, cell_select=True, kf_insert=False)
    assert len(plain) == len(off)
    for a, b in zip(plain, off):
        assert set(a) == set(b) and "n_joined" not in a
        for f in a:
            assert np.asarray(a[f]).tobytes() == np.asarray(b[f]).tobytes(), f
