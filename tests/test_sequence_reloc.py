"""run_sequence(.., relocalize="host" | "device"): the reference's stage machine STAGE_DEFAULT_FRAME <-> STAGE_RELOCALIZING around the
tracking gates and relocalizeFrame.  "device" uses plsvo_candidates_track_gate and plsvo_candidates_align_build_kf,
"host" the calls there were before; the two agree in every record and in the final tables.

The sequence: frame 0 stands at the world's origin (relocalizeFrame's first alignment starts from the default-constructed pose, the
identity, so a stream can only find itself again near it) and the camera moves a few per cent of the scene depth per frame; the images
of three frames in the middle are replaced by a flat grey, in which no feature is matched: tracking is lost there and found again behind
them.  The gpu test runs on the device; tests/test_emu_reloc.py runs it on the host emulation build inside the CPU suite."""
import importlib

import numpy as np
import pytest

from test_sequence_alignjob import check_same
from test_sequence_insert import counting_backend

SEQ = dict(seed=11, n_frames=12, W=320, H=240, n_pts=100, n_seg=20, step_scale=0.5)
LOST = (4, 5, 6)                                       # the frames whose image shows nothing
RUN = dict(mapping=True, kf_select=True, kfselect_mindist_t=0.03, max_n_kfs=3, map_candidates=True, cell_select=True, kf_insert=True, seed_candidates=True,
           structopt_resident=True)
OK, FAIL_MATCHES = 0, 1


@pytest.fixture(scope="module")
def seqm():
    return importlib.import_module("pl-svo_amd.sequence")


def sequence_at_the_origin(P, seqm, lost=LOST):
    """make_sequence with the world re-based on frame 0 (T_f_w of frame 0 is the identity; the images do not change) and the lost frames blanked"""
    seq = seqm.make_sequence(SEQ["seed"], **{k: v for k, v in SEQ.items() if k != "seed"})
    T0 = seq["poses_true"][0]
    T0_inv = P.synth.se3_inv(T0)
    act = lambda pts: np.array([seqm._se3_mul_s(T0, [0.0, 0.0, 0.0, 1.0] + [float(v) for v in p])[4:] for p in pts])
    seq = dict(seq, poses_true=np.stack([P.synth.se3_mul(T, T0_inv) for T in seq["poses_true"]]), pt_pos=act(seq["pt_pos"]), seg_spos=act(seq["seg_spos"]),
               seg_epos=act(seq["seg_epos"]), images=[np.full_like(img, 128) if k in lost else img for k, img in enumerate(seq["images"])])
    seq.pop("stream")
    return seq


def run(seqm, ctx, seq, mode, **kw):
    backend = counting_backend(seqm, ctx)
    # (the alignment job and the keyframe stage on the device in both runs: their own two transports are compared in tests of their own, and
    #  keystage="host" adds a field to the keyframe records.  relocalize="host" then reads the key-point table from a fetch.)
    res = seqm.run_sequence(backend, seq, align="device", keystage="device", relocalize=kw.pop("relocalize", mode), **dict(RUN, **kw))
    return res, ctx.candidates_fetch_map()[0], ctx.candidates_fetch_quality()[0], backend.staged_at


@pytest.mark.gpu
def test_tracking_is_lost_and_found_and_the_two_transports_agree(P, gpu_ctx, seqm):
    seq = sequence_at_the_origin(P, seqm)
    host, dev = run(seqm, gpu_ctx, seq, "host"), run(seqm, gpu_ctx, seq, "device")
    check_same(dev[0], host[0], ("records",))
    check_same(dev[1], host[1], ("tables",))
    check_same(dev[2], host[2], ("quality",))
    assert dev[3] == host[3] == [1]                                   # staged once: the tables stay resident through the loss
    res = host[0]
    stages, gates = [r["stage"] for r in res[1:]], [r["gate"] for r in res[1:]]
    print("stages", stages, "gates", gates, "tracked", [r.get("reloc_tracked") for r in res[1:]], "n_align", [r["n_align"] for r in res[1:]])
    lost_at = [k for k, r in enumerate(res) if k and r["stage"] == "default" and r["gate"] == FAIL_MATCHES]
    assert lost_at == [LOST[0]], "tracking is lost at the first frame that shows nothing"
    failed = [k for k, r in enumerate(res) if k and r["stage"] == "reloc" and r["gate"] != OK]
    assert failed and failed[0] == LOST[1], "a relocalisation attempt that fails"
    found = [k for k, r in enumerate(res) if k and r["stage"] == "reloc" and r["gate"] == OK]
    assert len(found) == 1 and found[0] == LOST[-1] + 1 and res[found[0]]["reloc_tracked"] > 30 and res[found[0]]["reloc_kf"] >= 0, "the stream finds itself at the first frame that shows the scene"
    behind = res[found[0] + 1:]
    assert len(behind) >= 3 and all(r["stage"] == "default" and r["gate"] == OK for r in behind), "tracked frames behind the recovery"
    # found: every frame from the recovery on lies nearer the truth than the pose the stream was stuck at while it was lost
    err = [e[1] for e in seqm.pose_errors(res, seq)]
    assert err[LOST[0]] < err[LOST[1]] < err[LOST[-1]] and max(err[found[0]:]) < err[LOST[-1]] and max(err[:LOST[0]]) < err[LOST[0]]
    # the carried pose of a lost frame is the last tracked frame's
    assert np.array_equal(res[LOST[0]]["T"], res[LOST[0] - 1]["T"])


@pytest.mark.gpu
def test_without_the_flag_every_record_is_what_it_is_today(P, gpu_ctx, seqm):
    """a sequence that stays tracked: relocalize=None gives today's records, and with the flag the same frames are tracked with the same
    poses (the gates pass everywhere; the records only gain their fields)"""
    seq = sequence_at_the_origin(P, seqm, lost=())
    plain = seqm.run_sequence(counting_backend(seqm, gpu_ctx), seq, align="device", keystage="device", **RUN)
    none = run(seqm, gpu_ctx, seq, "device", relocalize=None)[0]
    check_same(none, plain, ("records",))
    assert all("stage" not in r for r in none)
    with_flag = run(seqm, gpu_ctx, seq, "device")[0]
    assert all(r["stage"] == "default" and r["gate"] == OK for r in with_flag[1:])
    for a, b in zip(with_flag[1:], plain[1:]):
        assert np.array_equal(a["T"], b["T"]) and a["n_align"] == b["n_align"]


def test_relocalize_needs_align_and_keystage(P, seqm):
    seq = dict(images=[np.zeros((8, 8), np.uint8)] * 2)

    class NoBuild:
        pass
    full = dict(mapping=True, kf_select=True, map_candidates=True, cell_select=True, kf_insert=True)
    for kw in (dict(full, relocalize="device", align="host", keystage="host"), dict(full, relocalize="host", align="host"), dict(full, relocalize="host", keystage="host"),
               dict(full, relocalize="sometimes", align="host", keystage="host")):
        with pytest.raises(ValueError):
            seqm.run_sequence(NoBuild(), seq, **kw)
