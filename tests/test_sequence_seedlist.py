"""run_sequence(.., seed_candidates=True, seeds_resident=True): the map's seeds are staged once beside the resident map tables and are
updated, erased and handed over on the device (plsvo_seeds_*).  T, cov and every count of every frame equal those of the
same sequence with seeds_resident=False, whose seeds travel every frame; after each update the lists the backend holds equal the restatement
tests/np_seedlist.py on the lists before it; the seed stage is called once.  Run twice: on the CPU with an oracle-backed backend of its own,
whose seed calls are np_seedlist around the oracle's per-seed body, and under `gpu` with HipBackend."""
import copy
import importlib

import numpy as np
import pytest

import np_seedlist as SL
from test_sequence_insert import counting_backend
from test_sequence_newcand import RUN, OracleNewcandBackend, check_same_records, make_seq, quality_of
from test_sequence_select import same_bytes

LIST_OF = dict(SL.PT_LIST)


def seeds_of(lists):
    """the arrays HipBackend.seeds_stage takes (points only: the harness has no line seeds) as np_seedlist's lists"""
    n = len(lists["pt_ref_kf"])
    cell = lambda f, j: (lists[f][j].tolist() if np.ndim(lists[f][j]) else lists[f][j])
    return dict(pt=[{key: (np.float32(cell(f, j)) if key in ("a", "b", "mu", "z_range", "sigma2") else int(cell(f, j)) if key in ("ref_kf", "batch_id", "level", "type") else cell(f, j))
                     for f, key in SL.PT_LIST} for j in range(n)], seg=[], batch_counter=int(lists["batch_counter"]))


def check_lists(got, seeds, tag):
    want = SL.lists_of(seeds)
    assert got["batch_counter"] == want["batch_counter"], tag
    for f, _ in SL.PT_LIST + SL.SEG_LIST:
        same_bytes(got[f], want[f], (tag, f))


class OracleSeedlistBackend(OracleNewcandBackend):
    """test infrastructure: OracleNewcandBackend whose seed lists stay with the backend -- the seed calls are np_seedlist on the backend's OWN
    lists and tables, the per-seed body is the oracle's plsvo_update_seeds on one seed's frames"""

    def __init__(self, ob, P, n_levels=4):
        OracleNewcandBackend.__init__(self, ob, P, n_levels)
        self.seeds, self.seed_stages, self.seed_updates, self.seed_events = None, 0, 0, []

    def seeds_stage(self, lists, cam, room=None, max_n_kfs=3, n_pyr_levels=3):
        self.seeds, self.seed_cam, self.seed_max_n_kfs, self.seed_levels = seeds_of(lists), cam, max_n_kfs, n_pyr_levels
        self.seed_stages += 1

    def seeds_update(self, cur_slot, T_f_w=None):
        st, sd = self.st, self.seeds
        n = len(sd["pt"])
        col = lambda k: np.array([x[k] for x in sd["pt"]])
        T_ref = np.array([st["kf_T"][x["ref_kf"]] for x in sd["pt"]]).reshape(n, 7)
        slots = [st["kf_slot"][x["ref_kf"]] for x in sd["pt"]]
        px_cur, depth = np.zeros((n, 2)), np.zeros(n)
        res = None
        if n:
            # one job: frame 2j is seed j's reference keyframe (pose and slot from the backend's table as it stands), the last one the new frame
            pt = dict(ref_frame=np.arange(n, dtype=np.int32), cur_frame=np.full(n, n, np.int32), **{k: col(k) for k in ("px", "f", "level", "type", "grad", "a", "b", "mu", "z_range", "sigma2")})
            res = self.update_seeds(self.abi.SeedsJob(self.seed_cam, np.concatenate([T_ref, np.asarray(T_f_w, float)[None]]), np.array(slots + [cur_slot], np.int32), pt, None,
                                                   n_pyr_levels=self.seed_levels))
        at = {id(x): j for j, x in enumerate(sd["pt"])}

        def body(kind, seed):
            j = at[id(seed)]
            return {key: (int(res[f][j]) if key == "status" else res[f][j].tolist() if key.startswith("xyz") else res[f][j]) for f, key in SL.PT_ROWS}
        before = copy.deepcopy(sd)
        rep, ev, rows = SL.update(sd, st, body, self.seed_max_n_kfs)
        self.seed_updates += 1
        out = {f: np.array([r[key] for r in rows["pt"]], dtype=np.int32 if key == "status" else np.float64 if key == "xyz" else np.float32).reshape((-1, 3) if key == "xyz" else -1)
               for f, key in SL.PT_ROWS}
        self.seed_events.append(dict(before=before, rows=rows, after=copy.deepcopy(sd), report=rep))
        ev = (ev[0] if ev[0] is not None else [0] * len(st["pt_pos"]), ev[1] if ev[1] is not None else [0] * len(st["seg_spos"]))
        return rep, out, quality_of(st, *ev)

    def seeds_keyframe(self, **event):
        SL.keyframe(self.seeds, **event)

    def seeds_fetch_lists(self):
        return SL.lists_of(self.seeds)


@pytest.fixture(scope="module")
def seqm():
    return importlib.import_module("pl-svo_amd.sequence")


def check_run(seq, res, plain):
    check_same_records(res, plain)
    adds = [k for k, r in enumerate(res) if "add" in r]
    assert len(adds) >= 3 and any("insert" in res[k] for k in adds) and any(r.get("remove_kf", -1) >= 0 for r in res)
    return adds


# ---- on the CPU: the oracle-backed backend ----------------------------------------------------------------------------------------------
def test_cpu_resident_seeds_give_the_records_of_the_run_whose_seeds_travel(P, ob, seqm):
    seq = make_seq(seqm)
    backend = OracleSeedlistBackend(ob, P)
    res = seqm.run_sequence(backend, seq, seed_candidates=True, seeds_resident=True, **RUN)
    other = OracleSeedlistBackend(ob, P)
    plain = seqm.run_sequence(other, seq, seed_candidates=True, seeds_resident=False, **RUN)
    adds = check_run(seq, res, plain)
    assert backend.seed_stages == 1 and backend.staged_at == [1] and other.seed_stages == 0 and other.n_adds == len(adds)
    assert backend.n_adds == 0 and backend.seed_updates >= max(adds)                  # no record travelled: the commit appended every candidate
    assert sum(e["report"]["pt"][SL.CONVERGED] for e in backend.seed_events) == sum(res[k]["n_seed_candidates"] for k in adds)


def test_cpu_seeds_resident_needs_seed_candidates_and_a_backend_with_seed_lists(P, ob, seqm):
    seq = seqm.make_sequence(11, n_frames=3, W=320, H=240, n_pts=100, n_seg=20, step_scale=0.5)
    with pytest.raises(ValueError):
        seqm.run_sequence(OracleNewcandBackend(ob, P), seq, seed_candidates=True, seeds_resident=True, **RUN)          # no seeds_stage
    with pytest.raises(ValueError):
        seqm.run_sequence(OracleSeedlistBackend(ob, P), seq, seeds_resident=True, **RUN)                               # no seed_candidates


# ---- on the device ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_resident_seeds_on_the_device_equal_the_run_whose_seeds_travel_and_the_restatement(gpu_ctx, seqm):
    seq = make_seq(seqm)
    backend = counting_backend(seqm, gpu_ctx)
    calls = dict(stage=0, lists=[])
    plain_stage, plain_update, plain_kf = backend.seeds_stage, backend.seeds_update, backend.seeds_keyframe

    def stage(lists, *a, **kw):
        calls["stage"] += 1
        calls["seeds"] = seeds_of(lists)
        plain_stage(lists, *a, **kw)
        check_lists(backend.seeds_fetch_lists(), calls["seeds"], "staged")

    def update(cur_slot, T_f_w=None):
        rep, rows, quality = plain_update(cur_slot, T_f_w)
        sd = calls["seeds"]
        it = iter(range(len(sd["pt"])))

        def body(kind, seed):
            j = next(it)
            return {key: (int(rows[f][j]) if key == "status" else rows[f][j].tolist() if key.startswith("xyz") else rows[f][j]) for f, key in SL.PT_ROWS}
        n_conv = int((rows["pt_status"] == SL.CONVERGED).sum())
        st = dict(pt_pos=[None] * (rep["n_pt"] - n_conv), pt_obs=[[]] * (rep["n_pt"] - n_conv), pt_type=[], pt_cand=[], pt_nfail=[], pt_nsucc=[], seg_spos=[], seg_epos=[], seg_obs=[], seg_type=[],
                  seg_cand=[], seg_nfail=[], seg_nsucc=[])
        want, _, _ = SL.update(sd, st, body, 1 << 30)                   # the list handling around the device's own rows
        assert (rep["pt"], rep["n_pt_seeds"], rep["first_pt"], rep["no_room"]) == (want["pt"], want["n_pt_seeds"], want["first_pt"], 0), cur_slot
        check_lists(backend.seeds_fetch_lists(), sd, ("update", cur_slot))
        calls["lists"].append(cur_slot)
        return rep, rows, quality

    def keyframe(**event):
        plain_kf(**event)
        SL.keyframe(calls["seeds"], **event)
        check_lists(backend.seeds_fetch_lists(), calls["seeds"], ("keyframe event", event))
    backend.seeds_stage, backend.seeds_update, backend.seeds_keyframe = stage, update, keyframe
    res = seqm.run_sequence(backend, seq, seed_candidates=True, seeds_resident=True, **RUN)
    assert calls["stage"] == 1 and backend.staged_at == [1] and len(calls["lists"]) >= 5
    other = counting_backend(seqm, gpu_ctx)
    plain = seqm.run_sequence(other, seq, seed_candidates=True, seeds_resident=False, **RUN)
    check_run(seq, res, plain)
