"""run_sequence(.., kf_insert=True, seed_candidates=True): a depth-filter seed that converges is appended to the resident map tables on the
device (plsvo_candidates_add ..) instead of staging them anew.  The stage is called at frame 1 and nowhere else, over a
sequence in which seeds converge on several frames and keyframes are inserted and removed; every add's tables equal the restatement
tests/np_newcand.py on the tables the harness recorded before it; and the per-frame records equal those of the same sequence with
seed_candidates=False, which restages -- no result depends on a landmark's row index.  Run twice: on the CPU with an oracle-backed backend
whose map_add_candidates is np_newcand, and under `gpu` with HipBackend."""
import copy
import importlib

import numpy as np
import pytest

import candidates_cases as Cc
import np_newcand as NC
from test_sequence_insert import QUALITY, OracleInsertBackend, check_insertions, check_stage_calls, counting_backend
from test_sequence_select import same_bytes

BULKY = ("candidates", "insert", "add")                               # the recorded tables; everything else is a per-frame result
RUN = dict(mapping=True, kf_select=True, kfselect_mindist_t=0.4, max_n_kfs=3, map_candidates=True, cell_select=True, record_candidates=True, kf_insert=True)


def records_of(new):
    """the arrays HipBackend.map_add_candidates takes, as the records np_newcand reads"""
    k = len(new["pt_pos"])
    return dict(pt=[dict(pos=new["pt_pos"][j], obs=dict(kf=new["pt_obs_kf"][j], px=new["pt_obs_px"][j], f=new["pt_obs_f"][j], level=new["pt_obs_level"][j],
                                                        type=new["pt_obs_type"][j], grad=new["pt_obs_grad"][j])) for j in range(k)], seg=[])


def quality_of(st, pt_event, seg_event):
    return dict(pt_n_failed=np.array(st["pt_nfail"], np.int32), pt_n_succeeded=np.array(st["pt_nsucc"], np.int32), pt_type=np.array(st["pt_type"], np.int32),
                pt_event=np.array(pt_event, np.uint8), seg_n_failed=np.array(st["seg_nfail"], np.int32), seg_n_succeeded=np.array(st["seg_nsucc"], np.int32),
                seg_type=np.array(st["seg_type"], np.int32), seg_event=np.array(seg_event, np.uint8), pt_cand=np.array(st["pt_cand"], np.int32),
                seg_cand=np.array(st["seg_cand"], np.int32))


class OracleNewcandBackend(OracleInsertBackend):
    """test infrastructure: OracleInsertBackend whose tables stay resident when a seed converges -- map_add_candidates is np_newcand on the
    backend's OWN tables (the event bytes it reports are the add's alone)"""

    def __init__(self, ob, P, n_levels=4):
        OracleInsertBackend.__init__(self, ob, P, n_levels)
        self.lm_reserve, self.n_adds = None, 0

    def map_reserve_landmarks(self, **room):
        self.lm_reserve = room

    def map_add_candidates(self, new):
        st = self.st
        assert len(st["pt_pos"]) + len(new["pt_pos"]) <= self.rows_staged + self.lm_reserve["extra_pt"]
        out = NC.add(st, records_of(new))
        self.n_adds += 1
        rep = dict(first_pt=out["first_pt"], first_seg=out["first_seg"], n_added_pt=out["n_added_pt"], n_added_seg=out["n_added_seg"], n_pt=len(st["pt_pos"]),
                   n_seg=len(st["seg_spos"]), n_pt_cand=len(st["pt_cand"]), n_seg_cand=len(st["seg_cand"]), n_pt_obs=sum(len(l) for l in st["pt_obs"]),
                   n_seg_obs=sum(len(l) for l in st["seg_obs"]))
        return rep, quality_of(st, out["pt_event"], out["seg_event"])

    def map_select(self, map_job, frame_job, *a, **kw):
        if map_job is not None:
            self.rows_staged = map_job.n_pt
        return OracleInsertBackend.map_select(self, map_job, frame_job, *a, **kw)


@pytest.fixture(scope="module")
def seqm():
    return importlib.import_module("pl-svo_amd.sequence")


def make_seq(seqm):
    """steps large enough for the seeds to converge (frames 6 to 9) before the third keyframe pushes frame 0's out of a table of three"""
    return seqm.make_sequence(11, n_frames=13, W=320, H=240, n_pts=100, n_seg=20, step_scale=3.0)


def check_adds(seq, res, device_tables=None):
    """every add's tables against the restatement on the tables the HARNESS held before it; -> the frames that added"""
    n_pts = len(seq["pt_pos"])
    adds = [k for k, r in enumerate(res) if "add" in r]
    for n, k in enumerate(adds):
        c = res[k]["add"]
        st = copy.deepcopy(c["stream"])
        for name in ("pt", "seg"):
            st[name + "_nfail"] = [int(v) for v in c["quality_before"][name + "_n_failed"]]
            st[name + "_nsucc"] = [int(v) for v in c["quality_before"][name + "_n_succeeded"]]
        out = NC.add(st, records_of(c["new"]))
        want, got = Cc.to_job(st).t, Cc.to_job(c["tables"]).t
        for f in Cc.abi._CAND_MAP_ORDER:
            same_bytes(got[f], want[f], (k, f))
            if device_tables is not None:                              # what the device holds behind the add
                same_bytes(device_tables[n][f], want[f], (k, "device", f))
        for f, key in QUALITY:
            same_bytes(c["quality"][f], st[key], (k, f))
        for name in ("pt", "seg"):
            new_bits = np.asarray(c["quality"][name + "_event"]) & NC.EVENT_NEW
            same_bytes(new_bits, out[name + "_event"], (k, name, "the new rows, and only they, carry PLSVO_LM_EVENT_NEW"))
        rep = c["report"]
        assert rep["n_added_pt"] == res[k]["n_seed_candidates"] == out["n_added_pt"] > 0 and rep["first_pt"] == out["first_pt"] >= n_pts and rep["n_added_seg"] == 0, k
        assert (rep["n_pt"], rep["n_pt_cand"], rep["n_pt_obs"]) == (len(st["pt_pos"]), len(st["pt_cand"]), sum(len(l) for l in st["pt_obs"])), k
        if k + 1 < len(res):                                           # the next frame ran on these tables
            nxt = res[k + 1]["candidates"]["stream"]
            assert nxt["pt_obs"] == st["pt_obs"] and nxt["pt_cand"] == st["pt_cand"] and nxt["pt_type"] == st["pt_type"] and nxt["pt_pos"] == st["pt_pos"], k
    return adds


def check_insertions_too(seq, res, seqm):
    """tests/test_sequence_insert.py's check of every keyframe, which expects the tables an insertion left at the head of the NEXT frame:
    where an add followed on the same frame those are the tables recorded BEFORE the add"""
    shown = list(res)
    for k, r in enumerate(res[:-1]):
        if "insert" in r and "add" in r:
            shown[k + 1] = dict(res[k + 1], candidates=dict(res[k + 1]["candidates"], stream=r["add"]["stream"]))
    return check_insertions(seq, shown, seqm)


def check_seed_rows(seq, res):
    """a converged seed is a candidate in a NEW row, observed at the row the removals have moved frame 0's keyframe to, and is absent once
    that keyframe is gone"""
    n_pts = len(seq["pt_pos"])
    row, rows_seen = 0, set()
    assert any(r.get("remove_kf", -1) >= 0 for r in res)
    for k, r in enumerate(res[1:-1], 1):
        if r.get("remove_kf", -1) >= 0 and row is not None:
            row = None if r["remove_kf"] == row else row - (r["remove_kf"] < row)
        if r.get("n_seed_converged", 0) > 0:
            assert (r["n_seed_candidates"] > 0) == (row is not None) == ("add" in r), k
            if row is not None:
                nxt = res[k + 1]["candidates"]["stream"]
                new_rows = nxt["pt_cand"][-r["n_seed_candidates"]:]
                assert nxt["kf_slot"][row] == 0 and all(lm >= n_pts and nxt["pt_obs"][lm][-1]["kf"] == row and len(nxt["pt_obs"][lm]) == 1 for lm in new_rows), k
                rows_seen.add(row)
    return row, rows_seen


def check_same_records(res, restaged):
    """T, cov and every count of every frame equal those of the run that restages"""
    assert len(res) == len(restaged)
    for k, (a, b) in enumerate(zip(res, restaged)):
        assert set(a) - set(BULKY) == set(b) - set(BULKY), k
        for f in set(a) - set(BULKY):
            assert np.asarray(a[f]).tobytes() == np.asarray(b[f]).tobytes(), (k, f, a[f], b[f])


# ---- on the CPU: the oracle-backed backend ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def run_cpu(P, ob, seqm):
    seq = make_seq(seqm)
    backend = OracleNewcandBackend(ob, P)
    res = seqm.run_sequence(backend, seq, seed_candidates=True, **RUN)
    return seq, res, backend


def test_cpu_the_stage_is_called_at_frame_1_and_nowhere_else(run_cpu):
    seq, res, backend = run_cpu
    assert backend.staged_at == [1]
    adds = [k for k, r in enumerate(res) if "add" in r]
    kfs = [k for k, r in enumerate(res) if "insert" in r]
    assert len(adds) >= 3 and backend.n_adds == len(adds) and len(kfs) >= 3 and any(res[k]["remove_kf"] >= 0 for k in kfs)   # seeds converge on several frames, keyframes come and go
    assert any(k in kfs for k in adds) and any(k not in kfs for k in adds)                                                # behind an insertion on the same run, and without one
    assert backend.reserve == {} and backend.lm_reserve == {}          # (the harness gives both rooms back when it is done)


def test_cpu_every_add_equals_the_restatement_on_the_recorded_tables(run_cpu, seqm):
    seq, res, backend = run_cpu
    check_adds(seq, res)
    check_insertions_too(seq, res, seqm)                               # the insertions behind them run on the grown tables


def test_cpu_a_converged_seed_is_a_candidate_at_frame_0s_row_while_that_keyframe_lasts(run_cpu):
    seq, res, backend = run_cpu
    check_seed_rows(seq, res)


def test_cpu_the_records_equal_those_of_the_run_that_restages(run_cpu, P, ob, seqm):
    seq, res, backend = run_cpu
    other = OracleNewcandBackend(ob, P)
    restaged = seqm.run_sequence(other, seq, seed_candidates=False, **RUN)
    assert len(other.staged_at) > 1 and other.n_adds == 0
    check_stage_calls(restaged, other.staged_at)
    check_same_records(res, restaged)


def test_cpu_seed_candidates_needs_kf_insert_and_a_backend_that_adds(P, ob, seqm):
    seq = seqm.make_sequence(11, n_frames=3, W=320, H=240, n_pts=100, n_seg=20, step_scale=0.5)
    with pytest.raises(ValueError):
        seqm.run_sequence(OracleInsertBackend(ob, P), seq, mapping=True, map_candidates=True, cell_select=True, kf_insert=True, seed_candidates=True)    # no map_add_candidates
    with pytest.raises(ValueError):
        seqm.run_sequence(OracleNewcandBackend(ob, P), seq, mapping=True, map_candidates=True, cell_select=True, seed_candidates=True)                   # no kf_insert


# ---- on the device ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_seeds_join_the_resident_tables_and_only_frame_1_stages(gpu_ctx, seqm):
    seq = make_seq(seqm)
    backend = counting_backend(seqm, gpu_ctx)
    tables = []
    plain_add = backend.map_add_candidates

    def add_and_keep(new):
        out = plain_add(new)
        tables.append(gpu_ctx.candidates_fetch_map()[0])
        return out
    backend.map_add_candidates = add_and_keep
    res = seqm.run_sequence(backend, seq, seed_candidates=True, **RUN)
    assert backend.staged_at == [1]
    adds = check_adds(seq, res, tables)
    assert len(adds) >= 3 and len(tables) == len(adds)
    check_insertions_too(seq, res, seqm)
    check_seed_rows(seq, res)
    other = counting_backend(seqm, gpu_ctx)
    restaged = seqm.run_sequence(other, seq, seed_candidates=False, **RUN)
    assert len(other.staged_at) > 1
    check_same_records(res, restaged)
