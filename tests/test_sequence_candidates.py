"""run_sequence(map_candidates=True): the map-candidate stage (plsvo_candidates_*) chained into the harness through the C ABI, per-call
backend.  With one keyframe and landmarks of one type it must change nothing; with the keyframe stage selecting keyframes, every frame's
stage result equals the restatement tests/np_candidates.py on the inputs the harness recorded, and reference observations move to the
newer keyframes."""
import importlib

import numpy as np
import pytest

import np_candidates as N
from test_gpu_candidates import check_against_restatement


@pytest.fixture(scope="module")
def seqm():
    return importlib.import_module("pl-svo_amd.sequence")


@pytest.mark.gpu
def test_one_keyframe_and_one_type_change_nothing(gpu_ctx, seqm):
    """every landmark is seen by keyframe 0 only and has type UNKNOWN: the stage files the visible landmarks in landmark order with
    their keyframe-0 observation, which is what the default path matches -- same matches, same poses, bit for bit"""
    seq = seqm.make_sequence(11, n_frames=5, W=320, H=240, n_pts=100, n_seg=20, step_scale=0.5)
    plain = seqm.run_sequence(seqm.HipBackend(gpu_ctx), seq)
    cand = seqm.run_sequence(seqm.HipBackend(gpu_ctx), seq, map_candidates=True)
    for k, (a, b) in enumerate(zip(plain, cand)):
        assert np.asarray(a["T"]).tobytes() == np.asarray(b["T"]).tobytes() and np.asarray(a["cov"]).tobytes() == np.asarray(b["cov"]).tobytes(), k
        for f in ("n_matched_pt", "n_matched_seg", "n_kept_pt", "n_kept_seg"):
            assert a.get(f) == b.get(f), (k, f)
    assert all("n_filed_pt" not in r for r in plain)
    assert all(r["n_filed_pt"] >= r["n_matched_pt"] > 50 and r["ref_kf_hist"] == [r["n_filed_pt"] + r["n_filed_seg"]] for r in cand[1:])


@pytest.mark.gpu
def test_with_keyframe_selection_every_frame_equals_the_restatement(gpu_ctx, seqm):
    """a sequence that moves far enough for needNewKf to add keyframes: the overlap list comes from plsvo_close_keyframes, the tables
    are restaged at keyframes, and once a second keyframe exists some landmarks take their reference observation from it"""
    seq = seqm.make_sequence(11, n_frames=12, W=320, H=240, n_pts=100, n_seg=20, step_scale=0.5)
    res = seqm.run_sequence(seqm.HipBackend(gpu_ctx), seq, mapping=True, kf_select=True, map_candidates=True, record_candidates=True)
    cam = tuple(seq["cam"])
    n_kf_seen, outside0 = 1, 0
    for k, r in enumerate(res[1:], 1):
        c = r["candidates"]
        want = N.candidates(c["stream"], c["T"], c["overlap"], cam, 30, 30, 8)
        check_against_restatement(c["out"], want, ("frame", k))
        assert len(c["overlap"]) == r["n_overlap"] and len(r["ref_kf_hist"]) == len(c["stream"]["kf_T"])
        if len(c["stream"]["kf_T"]) >= 2:
            n_kf_seen = max(n_kf_seen, len(c["stream"]["kf_T"]))
            outside0 += sum(r["ref_kf_hist"][1:])
    assert n_kf_seen >= 2 and outside0 > 0, (n_kf_seen, outside0)
    # (no bound on the pose error here: references that move to estimated keyframes drift, which keyframe 0's true observations do not)
    kf_frames = [k for k, r in enumerate(res) if r.get("is_kf")]
    assert len(kf_frames) >= 1 and all(np.isfinite(r["T"]).all() for r in res)
