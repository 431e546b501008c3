"""run_sequence(.., kf_select=True, cell_select=True, kf_insert=True, keystage="host" | "device"): the keyframe stage with LIVE key points
 chained into the mapping harness -- Frame::key_pts_ as positions in the keyframes' feature lists, replaced when their
landmark is deleted, their positions read from the tables when the close keyframes are looked for, the decision behind the structure
optimisation.  "device" is plsvo_candidates_set_keypts / _run_close / _keyframe_decide on the resident tables, "host" the synchronous calls
there were before on arrays gathered from the tables the harness follows; they differ in transport alone, so every record and the key-point
table at the end agree byte for byte.  max_n_kfs = 3 on twelve frames of 320 x 240: keyframes are removed.

The seed is chosen on the CPU (test_cpu_the_sequence_exercises_the_stage, an oracle-backed backend in "host" mode): the sequence holds at
least one key-point rebuild and at least one overlap list that is not "every keyframe in table order" -- seeds 11 to 13 all do; 12 has two
rebuilds.  The `gpu` test asserts both again on its own records."""
import numpy as np
import pytest

import np_keystage as NK
from test_sequence_insert import OracleInsertBackend

SEED = 12
RUN = dict(mapping=True, kf_select=True, kfselect_mindist_t=0.03, max_n_kfs=3, map_candidates=True, cell_select=True, kf_insert=True)
FIELDS = ("T", "cov", "n_align", "n_matched_pt", "n_matched_seg", "n_kept_pt", "n_kept_seg", "is_kf", "n_overlap", "overlap", "depth_mean")


@pytest.fixture(scope="module")
def seqm(P):
    return P.sequence


def make_seq(seqm):
    return seqm.make_sequence(SEED, n_frames=12, W=320, H=240, n_pts=100, n_seg=20, step_scale=0.5)


def exercises_the_stage(res):
    """at least one rebuild, one removal, and one overlap list that is not the table in order"""
    rebuilt = sum(r.get("n_kp_rebuilt", 0) for r in res)
    removed = [r["remove_kf"] for r in res if r.get("remove_kf", -1) >= 0]
    unordered = [r["overlap"] for r in res[1:] if r["overlap"] != list(range(len(r["overlap"])))]
    assert rebuilt >= 1 and removed and unordered, (rebuilt, removed, unordered)
    return rebuilt


def replay(res, cam):
    """the key-point table of the sequence from the recorded tables alone, EVENT BY EVENT with tests/np_keystage.py: setKeyPoints from five
    NULLs on the first tables, safeDeletePoint by safeDeletePoint through every selection and every insertion.  -> (the table, keyframes
    rebuilt per frame)"""
    tab, rebuilt = None, []
    for k in range(1, len(res)):
        before = res[k]["candidates"]["stream"]
        tab = NK.fresh(before, cam) if tab is None else tab
        after = res[k]["insert"]["stream"] if "insert" in res[k] else res[k + 1]["candidates"]["stream"] if k + 1 < len(res) else None
        n = 0
        if after is not None:
            tab, ev = NK.sequential_upkeep(before, tab, cam, NK.deleted_landmarks(before, after))
            n += len(ev)
        if "insert" in res[k]:
            ins = res[k]["insert"]
            tab, ev = NK.sequential_insert_upkeep(ins["stream"], ins["select"], ins["pt_keep"], tab, cam, ins["remove_kf"], decided=res[k]["key_pts_new"])
            n += len(ev)
        rebuilt.append(n)
    return tab, rebuilt


def test_cpu_the_sequence_exercises_the_stage(P, ob, seqm):
    seq = make_seq(seqm)
    res = seqm.run_sequence(OracleInsertBackend(ob, P), seq, keystage="host", record_candidates=True, **RUN)
    assert exercises_the_stage(res) >= 2
    # the restatement, from the recorded tables: the same table at the end, and ITS count of rebuilds chooses the seed
    tab, rebuilt = replay(res, tuple(seq["cam"]))
    assert np.array_equal(tab, res[-1]["key_pts"]), (tab, res[-1]["key_pts"])
    assert sum(rebuilt) >= 2, rebuilt
    tab = res[-1]["key_pts"]
    assert tab.shape == (3, 5) and (tab[:, 0] >= 0).all()              # three keyframes at the end, each with a centre key point
    assert all("n_kp_rebuilt" in r for r in res if r.get("is_kf")) and all(r["n_overlap"] == len(r["overlap"]) <= 3 for r in res[1:])
    with pytest.raises(ValueError):
        seqm.run_sequence(OracleInsertBackend(ob, P), make_seq(seqm), keystage="device", **RUN)          # no map_keyframe_decide
    with pytest.raises(ValueError):
        seqm.run_sequence(OracleInsertBackend(ob, P), make_seq(seqm), keystage="host", **dict(RUN, kf_insert=False))


@pytest.mark.gpu
def test_device_and_host_transport_agree_in_every_record(gpu_ctx, seqm):
    seq = make_seq(seqm)
    host = seqm.run_sequence(seqm.HipBackend(gpu_ctx), seq, keystage="host", **RUN)
    dev = seqm.run_sequence(seqm.HipBackend(gpu_ctx), seq, keystage="device", **RUN)
    exercises_the_stage(host)
    assert len(host) == len(dev) == 12
    for k, (a, b) in enumerate(zip(host, dev)):
        assert set(a) - {"n_kp_rebuilt"} == set(b), (k, set(a) ^ set(b))
        for f in b:
            assert np.asarray(a[f]).tobytes() == np.asarray(b[f]).tobytes(), (k, f, a[f], b[f])
    for k, (a, b) in enumerate(zip(host[1:], dev[1:])):
        assert all(f in b for f in FIELDS), k
    kfs = [k for k, r in enumerate(dev) if r.get("is_kf")]
    assert len(kfs) >= 4 and all("remove_kf" in dev[k] for k in kfs) and dev[-1]["key_pts"].shape == (3, 5)
    assert np.array_equal(host[-1]["key_pts"], dev[-1]["key_pts"])
