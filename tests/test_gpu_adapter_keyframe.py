"""The C++ drop-ins of the keyframe stage (pl-svo_amd/host/plsvo/hip_adapter.hpp: frame_utils::getSceneDepth,
keyframe::getCloseKeyframes / needNewKf / setKeyPoints) on the GPU, through pl-svo_amd/host/keyframe_driver: a 160 x 120 frame with three
keyframes gives the C ABI's results, and setKeyPoints mutates key_pts_ as the indices say.  The driver links the product library, so the
emulated run leaves this file out by name (tests/test_emu_parity.py)."""
import os
import subprocess

import numpy as np
import pytest

import keyframe_cases as Kc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "pl-svo_amd", "host", "keyframe_driver")


@pytest.fixture(scope="module")
def run(P, tmp_path_factory):
    assert os.path.exists(DRIVER), "build it with __graft_entry__.build()"
    rng = np.random.default_rng(31)
    base = Kc.rand_decide_job(rng, 40, 9, 0, dead=0.2, prev=(3, 7, -1, 12, 5))
    T_new, T_last = np.array(base.c.T_new_w), np.array(base.c.T_last_w)
    # three keyframes: the first blocks (close to the last frame), the second does not, the third has no visible key point
    kf_T = np.stack([Kc.kf_near(rng, T_last, True), Kc.kf_near(rng, T_last, False), Kc.kf_near(rng, T_last, False)])
    kp = np.zeros((3, 5, 3))
    kp[0], kp[1] = Kc.points_in_view(rng, T_new, Kc.CAM, 5)[0], Kc.points_in_view(rng, T_new, Kc.CAM, 5)[0]
    kp[2] = Kc.points_in_view(rng, T_new, Kc.CAM, 5, -5.0, -1.0)[0]
    kv = np.array([[1, 0, 1, 1, 1], [0, 0, 1, 0, 1], [1, 1, 1, 1, 1]], np.uint8)
    ctx = P.capi.Context(0)
    try:
        close = ctx.close_keyframes([P.abi.CloseKeyframesJob(Kc.CAM, T_new, kf_T, kp, kv)])[0]
        job = P.abi.KeyframeDecideJob(Kc.CAM, T_new, T_last, base.pt_px, base.pt_pos, base.pt_alive, base.seg_spos, base.seg_epos, base.seg_alive,
                                      kf_T, close["close_idx"], list(base.c.key_pts_prev), Kc.MIN_T, Kc.MIN_R)
        want = ctx.keyframe_decide([job])[0]
    finally:
        ctx.close()
    d = tmp_path_factory.mktemp("keyframe_driver")
    path, out = d / "in.bin", d / "out.txt"
    with open(path, "wb") as f:
        np.array([160, 120, base.n_pt, base.n_seg, 3, Kc.MIN_T, Kc.MIN_R], np.float64).tofile(f)
        np.array([Kc.CAM.fx, Kc.CAM.fy, Kc.CAM.cx, Kc.CAM.cy], np.float64).tofile(f)
        T_new.tofile(f)
        T_last.tofile(f)
        np.column_stack([base.pt_px, base.pt_alive.astype(np.float64), base.pt_pos]).tofile(f)
        np.column_stack([base.seg_alive.astype(np.float64), base.seg_spos, base.seg_epos]).tofile(f)
        for i in range(3):
            kf_T[i].tofile(f)
            np.column_stack([kv[i].astype(np.float64), kp[i]]).tofile(f)
        np.array(list(base.c.key_pts_prev), np.float64).tofile(f)
    subprocess.run([DRIVER, str(path), str(out)], check=True, timeout=120)
    got = {}
    for line in open(out).read().splitlines():
        tag, *v = line.split()
        got.setdefault(tag, []).append([float(x) for x in v])
    return got, want, close, base


def test_adapter_functions_give_the_c_abi_results(run):
    got, want, close, _ = run
    assert want["has_depth"] == 1 and got["depth"] == [[1.0, want["depth_mean"], want["depth_min"]]]
    assert list(close["close_idx"]) in ([0, 1], [1, 0]) and close["n_close"] == 2               # the third keyframe sees nothing
    assert [int(r[0]) for r in got["close"]] == list(close["close_idx"]) and [r[1] for r in got["close"]] == list(close["close_dist"])
    assert want["need_new_kf"] == 0 and got["need"] == [[0.0]] and got["need_empty"] == [[1.0]]


def test_set_key_points_mutates_key_pts_as_the_indices_say(run):
    got, want, _, base = run
    assert [int(v) for v in got["keypts"][0]] == list(want["key_pts"])
    prev = list(base.c.key_pts_prev)
    assert list(want["key_pts"]) != prev and all(k < 0 or base.pt_alive[k] for k in want["key_pts"])
