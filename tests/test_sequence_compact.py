"""run_sequence(.., seed_candidates=True, compact="room" | "always", lm_room=N): behind every keyframe the resident map tables close up over
their deleted point rows on the device (plsvo_candidates_compact ..), so a sequence whose converged seeds outnumber the
landmark reserve completes without a restage.  The sequence is chosen so that the run WITHOUT compaction runs out of rows (asserted on the
oracle backend, so nothing here passes vacuously); with compaction every pose, covariance and count of every frame equals those of the
run with the full reserve.  Run twice: on the CPU with an oracle-backed backend whose map_compact is np_compact, and under `gpu` with
HipBackend."""
import importlib

import numpy as np
import pytest

import candidates_cases as Cc
import np_compact as NK
from test_sequence_insert import counting_backend
from test_sequence_newcand import RUN as RUN_NEWCAND, OracleNewcandBackend, quality_of

# on the oracle backend seventeen seeds converge: fifteen on frames 6 and 7, which the next keyframes match and join (they leave the
# candidate list), one each on frames 12 and 13; the keyframe removals at frames 11 and 12 delete four point landmarks.  The reserve is
# one row less than the seeds that converge ON THE BACKEND UNDER TEST (the depth filter's last bits differ between backends, and with them
# a seed's frame of convergence): without compaction the last seed finds no free row
SEQ = dict(seed=67, n_frames=16, W=320, H=240, n_pts=100, n_seg=20, step_scale=3.0)
RUN = dict(RUN_NEWCAND, max_n_kfs=4, record_candidates=False)


class OutOfRows(Exception):
    pass


class OracleCompactBackend(OracleNewcandBackend):
    """test infrastructure: OracleNewcandBackend whose tables are compacted where the device's are -- map_compact is np_compact on the
    backend's OWN tables; an add beyond the rows of the layout is refused as plsvo_candidates_add refuses it"""

    def __init__(self, ob, P, n_levels=4):
        OracleNewcandBackend.__init__(self, ob, P, n_levels)
        self.compactions = []

    def map_add_candidates(self, new):
        if len(self.st["pt_pos"]) + len(new["pt_pos"]) > self.rows_staged + self.lm_reserve["extra_pt"]:
            raise OutOfRows()
        assert len(self.st["pt_cand"]) + len(new["pt_pos"]) <= self.lm_reserve["extra_pt"]                   # (the candidate list's rows: staged empty, plus the reserve)
        return OracleNewcandBackend.map_add_candidates(self, new)

    def map_compact(self, mode="always", min_room_pt=0, min_room_seg=0):
        st = self.st
        rep = NK.compact(st, dict(always=NK.ALWAYS, room=NK.ROOM)[mode], min_room_pt, min_room_seg, self.rows_staged + self.lm_reserve["extra_pt"],
                         len(st["seg_spos"]) + self.lm_reserve["extra_seg"])
        self.compactions.append(rep)
        return Cc.to_job(st).t, quality_of(st, [0] * len(st["pt_pos"]), [0] * len(st["seg_spos"])), rep


@pytest.fixture(scope="module")
def seqm():
    return importlib.import_module("pl-svo_amd.sequence")


def make_seq(seqm):
    return seqm.make_sequence(SEQ["seed"], **{k: v for k, v in SEQ.items() if k != "seed"})


def check_same_records(res, full):
    """T, cov and every count of every frame equal those of the run with the full reserve (which has no compaction's count)"""
    assert len(res) == len(full)
    for k, (a, b) in enumerate(zip(res, full)):
        assert set(a) - {"n_compacted_pt"} == set(b), k
        for f in b:
            assert np.asarray(a[f]).tobytes() == np.asarray(b[f]).tobytes(), (k, f, a[f], b[f])


def check_sequence(seqm, make_backend, refused, must_run_out=True):
    seq = make_seq(seqm)
    full = seqm.run_sequence(make_backend(), seq, seed_candidates=True, **RUN)
    total = sum(r.get("n_seed_candidates", 0) for r in full)
    last = max(k for k, r in enumerate(full) if r.get("n_seed_candidates", 0))
    runs_out = sum(r.get("n_deleted_kf", 0) for r in full[:last]) >= 1                                    # rows are deleted before the last seed converges
    assert total >= 10 and (runs_out or not must_run_out)
    lm_room = total - 1 if runs_out else total
    if runs_out:
        with pytest.raises(refused):                                  # the reserve alone does not carry the sequence
            seqm.run_sequence(make_backend(), seq, seed_candidates=True, lm_room=lm_room, **RUN)
    for mode in ("room", "always"):
        backend = make_backend()
        res = seqm.run_sequence(backend, seq, seed_candidates=True, compact=mode, lm_room=lm_room, **RUN)
        check_same_records(res, full)
        done = [r["n_compacted_pt"] for r in res if "n_compacted_pt" in r]
        assert len(done) == sum(1 for r in res if "n_joined" in r) and sum(done) >= 1, (mode, done)       # one call behind every keyframe; rows came free
        yield mode, backend, res


def test_cpu_the_sequence_runs_out_of_rows_without_compaction_and_completes_with_it(P, ob, seqm):
    seen = {}
    for mode, backend, res in check_sequence(seqm, lambda: OracleCompactBackend(ob, P), OutOfRows):
        seen[mode] = [(r["ran_pt"], r["ran_seg"]) for r in backend.compactions]
        assert backend.staged_at == [1]                               # no restage anywhere
    assert all(p == 1 and s == 0 for p, s in seen["always"]) and any(p == 0 for p, _ in seen["room"]) and any(p == 1 for p, _ in seen["room"])


def test_cpu_compact_needs_seed_candidates_and_a_backend_that_compacts(P, ob, seqm):
    seq = seqm.make_sequence(11, n_frames=3, W=320, H=240, n_pts=100, n_seg=20, step_scale=0.5)
    with pytest.raises(ValueError):
        seqm.run_sequence(OracleNewcandBackend(ob, P), seq, seed_candidates=True, compact="room", **RUN)     # no map_compact
    with pytest.raises(ValueError):
        seqm.run_sequence(OracleCompactBackend(ob, P), seq, compact="always", **RUN)                         # no seed_candidates
    with pytest.raises(ValueError):
        seqm.run_sequence(OracleCompactBackend(ob, P), seq, seed_candidates=True, compact="sometimes", **RUN)


# ---- on the device ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_sequence_completes_on_the_device_with_compaction_and_equals_the_full_reserve(P, gpu_ctx, seqm):
    """the same sequence on the device.  The depth filter's last bits differ from the oracle's and can move a seed's frame of convergence
    in front of the first deletion; then the reserve holds every seed and the refusal is not asserted here (the CPU test asserts it) --
    the compactions, the remap of the harness's rows and the equality of every record are checked either way"""
    for mode, backend, res in check_sequence(seqm, lambda: counting_backend(seqm, gpu_ctx), P.capi.PlsvoError, must_run_out=False):
        assert backend.staged_at == [1]
