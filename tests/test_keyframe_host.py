"""Host checks of the keyframe stage that need no device: known answers of the restatement tests/np_keyframe.py, its logarithm against
the exponential, the quirks of the reference it reproduces, the constructed cases of tests/keyframe_cases.py, and the ctypes layouts."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import keyframe_cases as Kc
import np_keyframe as K

IDENT = [0, 0, 0, 1, 0, 0, 0]


def test_log_inverts_exp(P):
    """log(exp(xi)) = xi for GN-sized, moderate and large rotations (theta < pi), through the package's se3_exp.  The exponential's
    closed forms (1 - cos theta) / theta^2 and the logarithm's 1 - theta / (2 tan(theta / 2)) cancel to an absolute error of about
    eps / theta^2 each; they multiply theta * |upsilon|, hence the eps / theta term of the bound."""
    rng = np.random.default_rng(1)
    for scale in (1e-6, 1e-2, 0.5, 2.5):
        for _ in range(20):
            xi = np.concatenate([rng.normal(0, 1, 3), rng.normal(0, 1, 3)])
            xi[3:] *= scale / max(np.linalg.norm(xi[3:]), 1e-300) * rng.uniform(0.2, 1.0)
            back = np.array(K.se3_log(P.synth.se3_exp(xi)))
            theta, eps = np.linalg.norm(xi[3:]), np.finfo(float).eps
            assert np.allclose(back, xi, rtol=0, atol=(1e-12 + 8 * eps / theta) * max(1.0, np.abs(xi).max())), (scale, xi, back)


def test_log_small_angle_branch_and_w_near_zero():
    # n < 1e-10: omega = (2 / w) * q.vec to first order, upsilon = V^-1 t with c = 1/12
    xi = K.se3_log([1e-12, -2e-12, 5e-13, 1.0, 0.3, -0.2, 0.1])
    assert np.allclose(xi[3:], [2e-12, -4e-12, 1e-12], rtol=1e-12, atol=0) and np.allclose(xi[:3], [0.3, -0.2, 0.1], rtol=0, atol=1e-11)
    assert K.se3_log(IDENT) == [0.0] * 6
    # |w| < 1e-10: a half turn, theta = +-pi by the sign of w
    for w, sign in ((1e-12, 1.0), (-1e-12, -1.0), (0.0, -1.0)):
        xi = K.se3_log([0.0, 1.0, 0.0, w, 0.0, 0.0, 0.0])
        assert xi[4] == sign * math.pi and xi[3] == 0.0 and xi[5] == 0.0
    # a rotation about z by 90 degrees: omega = (0, 0, pi / 2); V^-1 t for t along x
    s = math.sqrt(0.5)
    xi = K.se3_log([0, 0, s, s, 1.0, 0.0, 0.0])
    th = math.pi / 2
    c = (1 - th / (2 * math.tan(th / 2))) / th ** 2
    assert np.allclose(xi[3:], [0, 0, th], atol=1e-15) and np.allclose(xi[:3], [1 - c * th * th, -0.5 * th, 0], atol=1e-15)
    # w < 0 (the same rotation, other sign of the quaternion): theta is negative and takes the 1/12 branch, as upstream
    xm = K.se3_log([0, 0, -s, -s, 1.0, 0.0, 0.0])
    assert np.allclose(xm[3:], [0, 0, th], atol=1e-15) and np.allclose(xm[:3], [1 - th * th / 12, -0.5 * th, 0], atol=1e-15)


def test_need_new_kf_known_answers():
    at = lambda x: [[0, 0, 0, 1, x, 0, 0]]
    r = K.need_new_kf(IDENT, at(0.06))
    assert r["delta_t"][0] == 0.06 and r["delta_r"][0] == 0.0 and (r["need_new_kf"], r["blocking"]) == (1, -1)      # strict <
    r = K.need_new_kf(IDENT, at(np.nextafter(0.06, 0)))
    assert (r["need_new_kf"], r["blocking"]) == (0, 0)
    assert K.need_new_kf(IDENT, np.zeros((0, 7))) == dict(need_new_kf=1, blocking=-1, delta_t=pytest.approx([]), delta_r=pytest.approx([]))
    # 3 degrees of 3.1416: a rotation of 3 * 3.1416 / 180 rad about x sits on the threshold to rounding; 2.9 degrees blocks, 3.1 does not
    for deg, blocks in ((2.9, True), (3.1, False)):
        a = deg * 3.1416 / 180.0
        r = K.need_new_kf(IDENT, [[math.sin(a / 2), 0, 0, math.cos(a / 2), 0.01, 0, 0]])
        assert abs(r["delta_r"][0] - deg) < 1e-12 and (r["blocking"] == 0) == blocks
    # the first blocking keyframe decides; the previous frame's pose is what the deltas are measured from
    T_last = [0, 0, 0, 1, 1.0, 0, 0]
    r = K.need_new_kf(T_last, [[0, 0, 0, 1, 2.0, 0, 0], [0, 0, 0, 1, 1.01, 0, 0], [0, 0, 0, 1, 1.0, 0, 0]])
    assert r["blocking"] == 1 and np.allclose(r["delta_t"], [1.0, 0.01, 0.0], atol=1e-15)


def test_scene_depth_known_answers():
    z = [3.0, 1.0, 2.0, 5.0]
    pos = [[0, 0, v] for v in z]
    r = K.scene_depth(IDENT, pos, None, [], [], None)
    assert r == dict(has_depth=1, n_depth=4, depth_mean=3.0, depth_min=1.0)                    # rank 4 // 2 = 2: the upper median
    r = K.scene_depth(IDENT, pos, [1, 0, 1, 1], [[0, 0, 0.5]], [[0, 0, 9.0]], [1])
    assert r == dict(has_depth=1, n_depth=5, depth_mean=3.0, depth_min=0.5)
    r = K.scene_depth(IDENT, pos, [0, 0, 0, 0], [[0, 0, 0.5]], [[0, 0, 9.0]], [0])
    assert r == dict(has_depth=0, n_depth=0, depth_mean=0.0, depth_min=float(np.finfo(np.float64).max))
    r = K.scene_depth([0, 0, 0, 1, 0, 0, -4.0], pos, None, [], [], None)                       # depths -1, -3, -2, 1
    assert (r["depth_mean"], r["depth_min"]) == (-1.0, -3.0)


def test_key_points_quirk_and_order():
    # 160 x 120: cu = 80, cv = 60.  Slots 3 and 4 test x < cv: a point at x = 70 is left of the centre but enters no quadrant slot
    kp = K.set_key_points(160, 120, [[70, 30], [70, 90]], None, [-1] * 5)
    assert list(kp) == [0, -1, -1, -1, -1]
    kp = K.set_key_points(160, 120, [[70, 30], [70, 90], [59, 30], [59, 90]], None, [-1] * 5)
    assert list(kp[3:]) == [2, 3]
    # first in list wins a tie, a surviving holder wins it against everybody, a dead holder is dropped
    px = [[85, 60], [80, 65], [75, 60]]
    assert K.set_key_points(160, 120, px, None, [-1] * 5)[0] == 0
    assert K.set_key_points(160, 120, px, None, [2, -1, -1, -1, -1])[0] == 2
    assert K.set_key_points(160, 120, px, [1, 1, 0], [2, -1, -1, -1, -1])[0] == 0
    assert list(K.set_key_points(160, 120, px, [0, 0, 0], [0, 1, 2, 0, 1])) == [-1] * 5
    # a holder is not tested against its quadrant again
    assert K.set_key_points(160, 120, [[5, 5], [90, 70]], None, [-1, 0, -1, -1, -1])[1] == 0


def test_close_and_furthest_known_answers():
    cam = Kc.CAM_T
    kf_T = [[0, 0, 0, 1, 3.0, 0, 0], [0, 0, 0, 1, 0, -1.0, 0], [0, 0, 0, 1, 0, 0, 2.0], [0, 0, 0, 1, 0, 1.0, 0]]
    kp = np.zeros((4, 5, 3)); kp[:, :, 2] = 2.0          # on the optical axis, 2 in front: visible
    kp[2, :, 2] = -2.0                                     # behind the camera
    kv = np.ones((4, 5), np.uint8)
    r = K.close_keyframes(IDENT, cam, kf_T, kp, kv, 2)
    assert list(r["close_idx"]) == [1, 3, 0] and list(r["close_dist"]) == [1.0, 1.0, 3.0] and (r["n_close"], r["n_overlap"]) == (3, 2)
    assert K.furthest_keyframe(IDENT, kf_T) == 0 and K.furthest_keyframe(IDENT, [IDENT, IDENT]) == -1
    assert K.furthest_keyframe(IDENT, [kf_T[1], kf_T[3]]) == 0                                     # strict >: the first of equals
    # pos() is the camera centre -R^T t, not the translation: a keyframe turned by a half turn about y has its centre at +t_x
    assert K.furthest_keyframe([0, 0, 0, 1, -1.0, 0, 0], [[0, 1.0, 0, 0, 1.0, 0, 0], [0, 0, 0, 1, 0.5, 0, 0]]) == 1


def test_constructed_cases_hold_on_the_restatement():
    """the generators assert their own edges (counts, ties, borders, the 1e-9 margin of the random decisions)"""
    b = Kc.decide_batches()
    assert all(len(v) == 9 for v in b.values()) and len(Kc.close_batch()) == 9
    sizes = {(j.n_pt, j.n_seg) for v in b.values() for j in v}
    assert len(sizes) > 15


def test_ctypes_mirrors_have_the_c_layouts(P, tmp_path):
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "plsvo_hip.h")
    structs = {"plsvo_close_kf_in": P.abi.CloseKfIn, "plsvo_close_kf_out": P.abi.CloseKfOut, "plsvo_kf_decide_in": P.abi.KfDecideIn,
               "plsvo_kf_decide_out": P.abi.KfDecideOut}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{header}"', "int main(void){"]
    for cname, ct in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in ct._fields_]
    lines.append("return 0;}")
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")], check=True)
    got = dict(l.split() for l in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, ct in structs.items():
        assert int(got[cname]) == C.sizeof(ct), cname
        for f, _ in ct._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(ct, f).offset, (cname, f)
    assert {"plsvo_close_keyframes", "plsvo_keyframe_decide"} <= set(P.capi.SYMBOLS)
