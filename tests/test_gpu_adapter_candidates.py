"""The C++ drop-in of the map-candidate stage (pl-svo_amd/host/plsvo/hip_adapter.hpp: reprojector::mapCandidates) on the GPU, through
pl-svo_amd/host/candidates_driver: the driver builds a map of mini types from a dump of a test stream, runs the adapter and a host loop
written in the reference's form, and fails when they disagree (candidates, chosen Feature*, overlap_kfs[r].second,
last_projected_kf_id_); its printed result equals the restatement tests/np_candidates.py.  The driver links the product library, so the
emulated run leaves this file out by name (tests/test_emu_parity.py)."""
import os
import subprocess

import numpy as np
import pytest

import candidates_cases as Cc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "pl-svo_amd", "host", "candidates_driver")
FRAME_ID = 4711


def dump(st, T, ov):
    v = [Cc.CAM_T[4], Cc.CAM_T[5], *Cc.CAM_T[:4], Cc.CELL, Cc.SEG_CELL, FRAME_ID, len(st["kf_T"]), len(st["pt_pos"]), len(st["seg_spos"]), len(st["pt_cand"]),
         len(st["seg_cand"]), len(ov), *T, *ov]
    for pos, typ, obs in zip(st["pt_pos"], st["pt_type"], st["pt_obs"]):
        v += [*pos, typ, len(obs)]
        for o in obs:
            v += [o["kf"], *o["px"], *o["f"], o["level"], o["type"], *o["grad"]]
    for s, e, typ, obs in zip(st["seg_spos"], st["seg_epos"], st["seg_type"], st["seg_obs"]):
        v += [*s, *e, typ, len(obs)]
        for o in obs:
            v += [o["kf"], *o["spx"], *o["epx"], *o["sf"], *o["ef"], o["level"]]
    for Tk, pf, sf in zip(st["kf_T"], st["kf_pt"], st["kf_seg"]):
        v += [*Tk, len(pf), len(sf), *pf, *sf]
    return np.array(v + list(st["pt_cand"]) + list(st["seg_cand"]), np.float64)


def cases():
    e, s = Cc.edge_case(), Cc.sizes_case()
    return {"edge": (e["streams"][0], e["T"][0], e["overlap"][0]), "random": (s["streams"][4], s["T"][4], s["overlap"][4])}


@pytest.mark.parametrize("name", ["edge", "random"])
def test_adapter_agrees_with_the_reference_form_and_the_restatement(name, tmp_path):
    assert os.path.exists(DRIVER), "build it with __graft_entry__.build()"
    st, T, ov = cases()[name]
    dump(st, T, ov).tofile(tmp_path / "in.bin")
    out = subprocess.run([DRIVER, str(tmp_path / "in.bin"), str(tmp_path / "out.txt")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    got = {}
    for line in open(tmp_path / "out.txt").read().splitlines():
        tag, *v = line.split()
        got.setdefault(tag, []).append([float(x) for x in v])
    assert got["agree"] == [[1.0]]
    want = Cc.restate(dict(streams=[st], T=[T], overlap=[ov]))[0]
    obs_kf = lambda obs_lists, lm, o: -1 if o < 0 else obs_lists[lm][o]["kf"]
    rows = [[lm, *px, cell, obs_kf(st["pt_obs"], lm, o), hv, ac] for lm, px, cell, o, hv, ac in
            zip(want["pt_lm"], want["pt_px"], want["pt_cell"], want["pt_obs"], want["pt_has_view"], want["pt_active"])]
    assert got.get("pt", []) == [[float(x) for x in r] for r in rows]
    rows = [[lm, *px, *cell, obs_kf(st["seg_obs"], lm, o), hv, ac] for lm, px, cell, o, hv, ac in
            zip(want["seg_lm"], want["seg_px"], want["seg_cell"], want["seg_obs"], want["seg_has_view"], want["seg_active"])]
    assert got.get("seg", []) == [[float(x) for x in r] for r in rows]
    assert got["count"] == [[float(x) for x in want["kf_count"]]]
    assert got["pfail"] == [[float(x) for x in want["pt_cand_failed"]]] and got["sfail"] == [[float(x) for x in want["seg_cand_failed"]]]
    visited = {lm for k in ov for lm in st["kf_pt"][k] if lm >= 0}
    assert got["marks"] == [[float(FRAME_ID if lm in visited else -1) for lm in range(len(st["pt_pos"]))]]
    assert len(want["pt_lm"]) > 5 and len(want["seg_lm"]) >= 2
