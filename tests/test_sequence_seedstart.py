"""run_sequence(.., seeds_resident=True, image_seeds="host" | "device"): at a keyframe whose seed tables are on the device the image's corners
become point seeds of the resident lists, in the pipeline's own order -- selection, pose optimisation, insertion of the
frame into the resident tables (which rewrites the keyframe table, the slots and the host's mirrors), then the seed event on the row just
inserted with both occupancy sources.  "device" is plsvo_seeds_keyframe_detect, "host" the calls there were before it; they differ in
transport alone, so every T, cov and count of every frame and the lists at the end agree byte for byte.  Run twice: on the CPU with an
oracle-backed backend whose device event is the restatement tests/np_seedstart.py, and under `gpu` with HipBackend."""
import importlib

import numpy as np
import pytest

import np_fast as F
import np_seedlist as SL
import np_seedstart as SS
from test_sequence_insert import counting_backend
from test_sequence_newcand import RUN, check_same_records, make_seq
from test_sequence_seedlist import OracleSeedlistBackend
from test_sequence_select import same_bytes

DET = dict(fast_threshold=7, detection_threshold=2.0)       # the rendered plane is soft: the reference's thresholds find no corner in it


class OracleSeedstartBackend(OracleSeedlistBackend):
    """test infrastructure: OracleSeedlistBackend with the detector (np_fast on the backend's own pyramids) and the device's keyframe
    event, which is np_seedstart on the backend's own lists, selection and rows"""

    def __init__(self, ob, P, n_levels=4):
        OracleSeedlistBackend.__init__(self, ob, P, n_levels)
        self.last_sel, self.last_rows, self.last_res, self.kf_report, self.events = None, None, None, None, []

    def map_select(self, *a, **kw):
        out = OracleSeedlistBackend.map_select(self, *a, **kw)
        self.last_sel = out[2]
        return out

    def update_seeds(self, job):
        self.last_res = OracleSeedlistBackend.update_seeds(self, job)
        return self.last_res

    def seeds_update(self, cur_slot, T_f_w=None):
        n = len(self.seeds["pt"])
        rep, out, q = OracleSeedlistBackend.seeds_update(self, cur_slot, T_f_w)
        out["pt_px_cur"] = self.last_res["pt_px_cur"].reshape(-1, 2).copy() if n else np.zeros((0, 2))
        assert len(out["pt_px_cur"]) == len(out["pt_status"])          # (no seed ages in the harness: the rows are the body's, in list order)
        self.last_rows = (out["pt_status"].copy(), out["pt_px_cur"].copy())
        return rep, out, q

    def detect_corners(self, slot, occupancy=None, cell_size=25, n_levels=3, detection_threshold=20.0, fast_threshold=20):
        return F.detect(self.pyr[slot][:n_levels], cell_size, fast_threshold, detection_threshold, occupancy)

    def seeds_keyframe_detect(self, cell_size=25, n_levels=3, detection_threshold=20.0, fast_threshold=20, occ_sources=3, **event):
        slot = self.st["kf_slot"][event["new_kf"]]
        self.kf_report = SS.keyframe_detect(self.seeds, self.pyr[slot][:n_levels], self.seed_cam, cell_size, selected_px=self.last_sel["pt_px"] if occ_sources & SS.OCC_SELECTED else None,
                                            update_rows=self.last_rows if occ_sources & SS.OCC_UPDATED else None, fast_threshold=fast_threshold, detection_threshold=detection_threshold,
                                            **event)
        self.events.append(dict(slot=slot, occ_sources=occ_sources, report=self.kf_report))

    def seeds_keyframe(self, pt_px=None, pt_f=None, pt_level=None, pt_type=None, pt_grad=None, **event):
        """HipBackend.seeds_keyframe's arrays as np_seedlist's features (the host transport's upload)"""
        n = 0 if pt_px is None else len(pt_px)
        new_pt = [dict(px=[float(v) for v in pt_px[j]], f=[float(v) for v in pt_f[j]], level=int(pt_level[j]), type=int(pt_type[j]), grad=[float(v) for v in pt_grad[j]]) for j in range(n)]
        SL.keyframe(self.seeds, new_pt=new_pt, **event)

    def seeds_keyframe_fetch(self):
        return self.kf_report


@pytest.fixture(scope="module")
def seqm():
    return importlib.import_module("pl-svo_amd.sequence")


def check_pair(dev, host, lists_dev, lists_host):
    check_same_records(dev, host)
    started = [r["n_image_seeds_started"] for r in dev if "n_image_seeds_started" in r]
    assert len(started) >= 1 and sum(started) > 20, started          # keyframes behind an insertion started seeds from their images
    assert max(r.get("n_image_seeds", 0) for r in dev) > 20          # ... and the following frames updated them on the resident rows
    assert any(r.get("remove_kf", -1) >= 0 for r in dev)
    assert lists_dev["batch_counter"] == lists_host["batch_counter"]
    for f, _ in SL.PT_LIST + SL.SEG_LIST:
        same_bytes(lists_dev[f], lists_host[f], ("lists at the end", f))


# ---- on the CPU: the oracle-backed backend ----------------------------------------------------------------------------------------------
def test_cpu_device_transport_equals_host_transport(P, ob, seqm):
    seq = make_seq(seqm)
    b_dev, b_host = OracleSeedstartBackend(ob, P), OracleSeedstartBackend(ob, P)
    dev = seqm.run_sequence(b_dev, seq, seed_candidates=True, seeds_resident=True, image_seeds="device", image_seed_params=DET, **RUN)
    host = seqm.run_sequence(b_host, seq, seed_candidates=True, seeds_resident=True, image_seeds="host", image_seed_params=DET, **RUN)
    check_pair(dev, host, b_dev.seeds_fetch_lists(), b_host.seeds_fetch_lists())
    assert b_dev.events and not b_host.events and all(e["occ_sources"] & SS.OCC_SELECTED for e in b_dev.events) and any(e["occ_sources"] & SS.OCC_UPDATED for e in b_dev.events)
    assert all(e["report"]["n_occupied"] > 0 for e in b_dev.events)
    # without the flag nothing changes: the records are those of the run without image seeds, less the new counts
    plain = seqm.run_sequence(OracleSeedstartBackend(ob, P), seq, seed_candidates=True, seeds_resident=True, **RUN)
    assert not any(f.startswith("n_image_seeds") for r in plain for f in r)


def test_cpu_image_seeds_needs_resident_seed_lists(P, ob, seqm):
    seq = seqm.make_sequence(11, n_frames=3, W=320, H=240, n_pts=100, n_seg=20, step_scale=0.5)
    with pytest.raises(ValueError):
        seqm.run_sequence(OracleSeedstartBackend(ob, P), seq, seed_candidates=True, image_seeds="device", **RUN)
    with pytest.raises(ValueError):
        seqm.run_sequence(OracleSeedstartBackend(ob, P), seq, seed_candidates=True, seeds_resident=True, image_seeds="both", **RUN)
    with pytest.raises(ValueError):
        seqm.run_sequence(OracleSeedlistBackend(ob, P), seq, seed_candidates=True, seeds_resident=True, image_seeds="device", **RUN)


# ---- on the device ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_device_transport_equals_host_transport_behind_real_insertions(gpu_ctx, seqm):
    seq = make_seq(seqm)
    b_dev = counting_backend(seqm, gpu_ctx)
    dev = seqm.run_sequence(b_dev, seq, seed_candidates=True, seeds_resident=True, image_seeds="device", image_seed_params=DET, **RUN)
    lists_dev = b_dev.seeds_fetch_lists()
    b_host = counting_backend(seqm, gpu_ctx)
    host = seqm.run_sequence(b_host, seq, seed_candidates=True, seeds_resident=True, image_seeds="host", image_seed_params=DET, **RUN)
    check_pair(dev, host, lists_dev, b_host.seeds_fetch_lists())
    assert b_dev.staged_at == [1] and b_host.staged_at == [1]
