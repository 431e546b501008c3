"""run_sequence(.., structopt_resident=True): FrameHandlerBase::optimizeStructure runs on the resident map tables
(plsvo_candidates_optimize_structure ..) on every tracked frame, in place of the harness's gather / structure_optimize /
map_set_positions.  On every frame the tables and the keys after the call equal the restatement tests/np_structsel.py on the tables the
harness recorded before it; structure_optimize and map_set_positions are never called; the stage is still called once.  Run twice: on the
CPU with an oracle-backed backend whose map_optimize_structure is np_structsel on its own tables, and under `gpu` with HipBackend."""
import copy
import importlib

import numpy as np
import pytest

import candidates_cases as Cc
import np_structsel as NS
from test_sequence_insert import OracleInsertBackend, counting_backend
from test_sequence_newcand import RUN, make_seq
from test_sequence_seedstart import OracleSeedstartBackend
from test_sequence_select import same_bytes

FETCH = ("pt_lm", "pt_iters", "pt_pos", "seg_lm", "seg_iters", "seg_spos", "seg_epos")


class OracleStructselBackend(OracleSeedstartBackend):
    """test infrastructure: the newest oracle-backed backend whose map_optimize_structure is np_structsel on the backend's OWN tables with the
    last selection and the last pose optimisation's masks, as the device uses its resident ones; the keys live beside the tables and a
    stage zeroes them"""

    def __init__(self, ob, P, n_levels=4):
        OracleSeedstartBackend.__init__(self, ob, P, n_levels)
        self.n_structopt, self.n_host_structopt, self.n_set_positions = 0, 0, 0

    def map_select(self, map_job, *a, **kw):
        out = OracleSeedstartBackend.map_select(self, map_job, *a, **kw)
        if map_job is not None:
            self.st.pop("pt_last_optim", None); self.st.pop("seg_last_optim", None)
        return out

    def map_optimize_structure(self, frame_id, **params):
        L = self.last
        out = NS.optimize_structure(self.st, L["sel"], L["pose"].pt_keep, L["pose"].seg_keep, frame_id, **params)
        self.n_structopt += 1
        return dict(out, n_sel_pt=len(out["pt_lm"]), n_sel_seg=len(out["seg_lm"]))

    def map_set_last_optim(self, pt_last_optim, seg_last_optim):
        self.st["pt_last_optim"], self.st["seg_last_optim"] = [int(v) for v in pt_last_optim], [int(v) for v in seg_last_optim]

    def structure_optimize(self, job):
        self.n_host_structopt += 1
        return OracleSeedstartBackend.structure_optimize(self, job)

    def map_set_positions(self, pt_idx, pt_pos):
        self.n_set_positions += 1
        return OracleSeedstartBackend.map_set_positions(self, pt_idx, pt_pos)


@pytest.fixture(scope="module")
def seqm():
    return importlib.import_module("pl-svo_amd.sequence")


def check_structopt(res, device=None):
    """every frame's call against the restatement on the tables and keys the HARNESS held before it; -> the frames that refined something"""
    busy = []
    for k, r in enumerate(res[1:], 1):
        c = r["structopt"]
        st = copy.deepcopy(c["stream"])
        st["pt_last_optim"], st["seg_last_optim"] = list(c["keys_before"]["pt"]), list(c["keys_before"]["seg"])
        want = NS.optimize_structure(st, c["select"], c["pt_keep"], c["seg_keep"], c["frame_id"])
        assert c["frame_id"] == k and (r["n_structopt_pt"], r["n_structopt_seg"]) == (len(want["pt_lm"]), len(want["seg_lm"])), k
        for f in FETCH:
            same_bytes(c["report"][f], want[f], (k, "report", f))
        w, g = Cc.to_job(st).t, Cc.to_job(c["tables"]).t
        for f in Cc.abi._CAND_MAP_ORDER:
            same_bytes(g[f], w[f], (k, f))
            if device is not None:                                      # what the device holds behind the call
                same_bytes(device[k - 1][0][f], w[f], (k, "device", f))
        assert c["keys"]["pt"] == st["pt_last_optim"] and c["keys"]["seg"] == st["seg_last_optim"], k
        if device is not None:
            same_bytes(device[k - 1][1]["pt_last_optim"], np.array(st["pt_last_optim"], np.int32), (k, "device keys", "pt"))
            same_bytes(device[k - 1][1]["seg_last_optim"], np.array(st["seg_last_optim"], np.int32), (k, "device keys", "seg"))
        if len(want["pt_lm"]) + len(want["seg_lm"]):
            busy.append(k)
        if k + 1 < len(res) and "insert" not in r and not r.get("n_seed_converged"):   # the next frame ran on the moved positions (a converged seed brings a position of its own)
            nxt = res[k + 1]["candidates"]["stream"]
            assert nxt["pt_pos"] == st["pt_pos"] and nxt["seg_spos"] == st["seg_spos"] and nxt["seg_epos"] == st["seg_epos"], k
    return busy


def check_rotation(res):
    """what frame k refined is not refined at k + 1 while landmarks that were never refined are among the kept features"""
    for k in range(1, len(res) - 1):
        a, b = res[k]["structopt"], res[k + 1]["structopt"]
        if len(a["report"]["pt_lm"]) == 20 and len(b["report"]["pt_lm"]) == 20:
            kept_b = [int(lm) for lm, keep in zip(b["select"]["pt_lm"], b["pt_keep"]) if keep]
            if sum(1 for lm in kept_b if b["keys_before"]["pt"][lm] < k) >= 20:
                assert not set(int(v) for v in a["report"]["pt_lm"]) & set(int(v) for v in b["report"]["pt_lm"]), k


# ---- on the CPU: the oracle-backed backend ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def run_cpu(P, ob, seqm):
    seq = make_seq(seqm)
    backend = OracleStructselBackend(ob, P)
    res = seqm.run_sequence(backend, seq, seed_candidates=True, structopt_resident=True, **RUN)
    return seq, res, backend


def test_cpu_every_frame_equals_the_restatement_on_the_recorded_tables(run_cpu):
    seq, res, backend = run_cpu
    busy = check_structopt(res)
    assert len(busy) >= len(res) - 2 and any("insert" in res[k] for k in busy) and any("insert" not in res[k] for k in busy)   # every tracked frame, keyframe or not
    assert any(r["n_structopt_seg"] > 0 for r in res[1:]) and max(r["n_structopt_pt"] for r in res[1:]) == 20
    check_rotation(res)


def test_cpu_one_call_per_frame_and_nothing_host_fed(run_cpu):
    seq, res, backend = run_cpu
    assert backend.n_structopt == len(res) - 1 and backend.n_host_structopt == 0 and backend.n_set_positions == 0
    assert backend.staged_at == [1]                                    # the stage is still called once


def test_cpu_structopt_resident_needs_cell_select_and_the_hook(P, ob, seqm):
    seq = seqm.make_sequence(11, n_frames=3, W=320, H=240, n_pts=100, n_seg=20, step_scale=0.5)
    with pytest.raises(ValueError):
        seqm.run_sequence(OracleInsertBackend(ob, P), seq, mapping=True, map_candidates=True, cell_select=True, structopt_resident=True)      # no map_optimize_structure
    with pytest.raises(ValueError):
        seqm.run_sequence(OracleStructselBackend(ob, P), seq, mapping=True, map_candidates=True, structopt_resident=True)                    # no cell_select


def test_cpu_the_keys_are_carried_over_a_restage(P, ob, seqm):
    """without kf_insert a keyframe stages the tables anew: the harness hands the keys it followed to the fresh tables, and every frame
    still equals the restatement on the recorded keys"""
    seq = make_seq(seqm)
    backend = OracleStructselBackend(ob, P)
    res = seqm.run_sequence(backend, seq, structopt_resident=True, **dict(RUN, kf_insert=False))
    assert len(backend.staged_at) > 1 and backend.n_host_structopt == 0
    check_structopt(res)
    later = [k for k in backend.staged_at if k > 1]
    assert any(any(res[k]["structopt"]["keys_before"]["pt"]) for k in later)


# ---- on the device ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_structure_is_optimised_on_the_resident_tables_every_frame(gpu_ctx, seqm):
    seq = make_seq(seqm)
    backend = counting_backend(seqm, gpu_ctx)
    device, calls = [], dict(host=0, set_positions=0)
    plain = backend.map_optimize_structure

    def optimise_and_keep(frame_id, **params):
        out = plain(frame_id, **params)
        device.append((gpu_ctx.candidates_fetch_map()[0], gpu_ctx.candidates_fetch_last_optim()[0]))
        return out

    def count(name, fn):
        def counted(*a, **kw):
            calls[name] += 1
            return fn(*a, **kw)
        return counted
    backend.map_optimize_structure = optimise_and_keep
    backend.structure_optimize = count("host", backend.structure_optimize)
    backend.map_set_positions = count("set_positions", backend.map_set_positions)
    res = seqm.run_sequence(backend, seq, seed_candidates=True, structopt_resident=True, **RUN)
    assert backend.staged_at == [1] and calls == dict(host=0, set_positions=0) and len(device) == len(res) - 1
    busy = check_structopt(res, device)
    assert len(busy) >= len(res) - 2
    check_rotation(res)
