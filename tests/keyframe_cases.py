"""Cases of the keyframe stage (plsvo_close_keyframes / plsvo_keyframe_decide), shared by tests/test_gpu_keyframe.py and the host tests:
batches of nine streams of unequal size -- more than two workgroups of four waves, the last one partial.  Built once (seeded), never
changed.  Every constructed edge is asserted on the restatement here, so a case cannot silently miss what it is named for."""
import functools
import importlib

import numpy as np

import np_keyframe as K

P = importlib.import_module("pl-svo_amd")
abi, synth = P.abi, P.synth

CAM = abi.Pinhole(128.0, 128.0, 80.0, 60.0, 160, 120)          # non-square; fx a power of two: px.x == 0 and == width are exact
CAM_T = (128.0, 128.0, 80.0, 60.0, 160, 120)
CAM_BIG = abi.Pinhole(315.5, 315.5, 376.0, 240.0, 752, 480)
IDENT = np.array([0, 0, 0, 1, 0, 0, 0], float)
MIN_T, MIN_R = 0.06, 3.0


def rand_pose(rng, rot=0.3, trans=0.5):
    return synth.se3_exp(np.concatenate([rng.uniform(-trans, trans, 3), rng.uniform(-rot, rot, 3)]))


def points_in_view(rng, T_f_w, cam, n, zlo=1.0, zhi=6.0):
    """n world points that project into the image of pose T_f_w, and their pixels"""
    px = np.stack([rng.uniform(0, cam.width, n), rng.uniform(0, cam.height, n)], 1)
    z = rng.uniform(zlo, zhi, n)
    f = np.stack([(px[:, 0] - cam.cx) / cam.fx * z, (px[:, 1] - cam.cy) / cam.fy * z, z], 1)
    Ti = synth.se3_inv(np.asarray(T_f_w, float))
    return np.array([synth.se3_act(Ti, p) for p in f]).reshape(-1, 3), px


def kf_near(rng, T_last, blocking):
    """a keyframe pose closer than both thresholds to T_last (blocking) or further than at least one, with a margin"""
    if blocking:
        xi = np.concatenate([rng.uniform(-0.02, 0.02, 3), rng.uniform(-0.015, 0.015, 3)])
    elif rng.random() < 0.5:
        xi = np.concatenate([rng.uniform(0.08, 0.5, 3) * rng.choice([-1, 1], 3), rng.uniform(-0.01, 0.01, 3)])
    else:
        xi = np.concatenate([rng.uniform(-0.01, 0.01, 3), rng.uniform(0.08, 0.6, 3) * rng.choice([-1, 1], 3)])
    return synth.se3_mul(np.asarray(T_last, float), synth.se3_exp(xi))


def rand_decide_job(rng, n_pt, n_seg, n_kf=0, blocking_at=None, n_ov=None, dead=0.0, cam=CAM, prev=None, T_new=None):
    """a stream with random features; the overlap list is the first n_ov keyframes, of which only blocking_at (if any) blocks"""
    T_new = rand_pose(rng) if T_new is None else np.asarray(T_new, float)
    T_last = synth.se3_mul(synth.se3_exp(rng.uniform(-0.02, 0.02, 6)), T_new)
    pos, px = points_in_view(rng, T_new, cam, n_pt)
    px = px + rng.normal(0, 0.5, px.shape)
    sp, _ = points_in_view(rng, T_new, cam, n_seg)
    ep, _ = points_in_view(rng, T_new, cam, n_seg)
    pa = (rng.random(n_pt) >= dead).astype(np.uint8) if dead > 0 else None
    sa = (rng.random(n_seg) >= dead).astype(np.uint8) if dead > 0 else None
    n_ov = n_kf if n_ov is None else n_ov
    order = rng.permutation(n_kf)[:n_ov]
    kf_T = np.zeros((n_kf, 7))
    for i in range(n_kf):
        kf_T[i] = kf_near(rng, T_last, False)
    if blocking_at is not None:
        kf_T[order[blocking_at]] = kf_near(rng, T_last, True)
    if prev is None:
        prev = [int(rng.integers(-1, n_pt)) if n_pt else -1 for _ in range(5)]
    return abi.KeyframeDecideJob(cam, T_new, T_last, px, pos, pa, sp, ep, sa, kf_T, order, prev, MIN_T, MIN_R)


def _flat_job(z_pts, z_segs=(), alive=None, seg_alive=None, T_new=IDENT, prev=(-1,) * 5):
    """identity rotation: the depth of a feature is its z coordinate (plus T_new's t_z), bit for bit"""
    z_pts = np.asarray(z_pts, float)
    n = len(z_pts)
    pos = np.stack([np.linspace(-0.3, 0.3, n) if n else np.zeros(0), np.zeros(n), z_pts], 1)
    px = np.stack([80 + np.arange(n) % 50, 60 + np.arange(n) % 40], 1).astype(float)
    zs = np.asarray(z_segs, float).reshape(-1, 2)
    sp = np.stack([np.zeros(len(zs)), np.zeros(len(zs)), zs[:, 0]], 1)
    ep = np.stack([np.ones(len(zs)), np.zeros(len(zs)), zs[:, 1]], 1)
    return abi.KeyframeDecideJob(CAM, T_new, IDENT, px, pos, alive, sp, ep, seg_alive, (), (), prev, MIN_T, MIN_R)


@functools.lru_cache(maxsize=None)
def depth_count_batch():
    """m = 0, 1, 2, 63, 64, 65, 321, 900 depths, and a row of equal depths; dead features interleaved in the 321 row"""
    rng = np.random.default_rng(9001)
    jobs = [rand_decide_job(rng, 3, 2, 2, dead=2.0),                       # every feature dead: m = 0
            rand_decide_job(rng, 1, 0, 1),                                  # 1
            rand_decide_job(rng, 0, 1, 0),                                  # 2: one segment
            rand_decide_job(rng, 21, 21, 3, blocking_at=1),                 # 63
            rand_decide_job(rng, 64, 0, 11, blocking_at=0),                 # 64
            rand_decide_job(rng, 1, 32, 4, blocking_at=3)]                  # 65
    while True:                                                             # 321 alive depths out of 260 + 2 * 90 with dead ones between
        j = rand_decide_job(rng, 260, 90, 5, dead=0.27)
        if K.decide(j)["n_depth"] == 321:
            break
    jobs.append(j)
    jobs.append(rand_decide_job(rng, 500, 200, 12, blocking_at=11))         # 900: above any register cap
    jobs.append(_flat_job(np.full(70, 2.5)))                                # all depths equal
    want = [0, 1, 2, 63, 64, 65, 321, 900, 70]
    assert [K.decide(j)["n_depth"] for j in jobs] == want
    return tuple(jobs)


def _minus_zero_pose_and_point():
    """a pose and a point whose depth is -0.0 in the arithmetic of T * p (searched over the signs of zero and of w)"""
    import itertools
    for s in itertools.product([0.0, -0.0], repeat=4):
        for w, v0, v1 in itertools.product((1.0, -1.0), (0.3, -0.3), (0.2, -0.2)):
            T = [s[0], s[1], s[2], w, 0.0, 0.0, s[3]]
            z = K.se3_act(T, [v0, v1, -0.0])[2]
            if z == 0.0 and np.signbit(z):
                return np.array(T), np.array([v0, v1, -0.0])
    raise AssertionError("no -0.0 depth found")


@functools.lru_cache(maxsize=None)
def depth_pattern_batch():
    """more than 64 copies of the median; negative and positive depths with zeros; dead features interleaved; duplicates in clusters"""
    rng = np.random.default_rng(9002)
    z = np.concatenate([np.full(100, 3.25), rng.uniform(1, 3, 50), rng.uniform(3.5, 6, 50)])
    rng.shuffle(z)
    many = _flat_job(z)
    assert K.decide(many)["depth_mean"] == 3.25
    zz = np.concatenate([rng.uniform(-4, -0.1, 40), rng.uniform(0.1, 4, 37), [0.0, -0.0]])
    rng.shuffle(zz)
    signed = _flat_job(zz, rng.uniform(-2, 2, (10, 2)))
    r = K.decide(signed)
    assert r["depth_min"] < 0 and r["n_depth"] == 99
    Tz, pz = _minus_zero_pose_and_point()
    jobs = [many, signed]
    # a depth of -0.0 out of the pose arithmetic itself, between negative and positive ones: once the median, once the minimum
    for others in ([[0, 0, -1.0], [0, 0, 2.0]], [[0, 0, 1.0], [0, 0, 2.0]]):
        j = abi.KeyframeDecideJob(CAM, Tz, IDENT, [[80, 60]] * 3, [pz] + others, None, (), (), None, (), (), (-1,) * 5)
        r = K.decide(j)
        zero = r["depth_mean"] if others[0][2] < 0 else r["depth_min"]
        assert np.signbit(zero) and zero == 0.0
        jobs.append(j)
    alive = (np.arange(150) % 3 != 1).astype(np.uint8)
    jobs.append(_flat_job(rng.uniform(0.5, 9, 150), rng.uniform(0.5, 9, (40, 2)), alive, (np.arange(40) % 2).astype(np.uint8)))
    zc = np.concatenate([np.full(70, 2.0), np.full(70, np.nextafter(2.0, 3)), np.full(70, np.nextafter(2.0, 1))])   # three crowded neighbours
    rng.shuffle(zc)
    jobs.append(_flat_job(zc))
    jobs.append(_flat_job(-rng.uniform(1, 2, 130), -rng.uniform(1, 2, (33, 2))))   # all negative
    jobs.append(_flat_job(np.concatenate([np.full(65, 1.0), np.full(64, 2.0)])))  # the median one past a run of 65 equal values
    jobs.append(rand_decide_job(rng, 200, 80, 10, blocking_at=4, dead=0.1))
    assert len(jobs) == 9
    return tuple(jobs)


def _px_job(px, alive=None, prev=(-1,) * 5, cam=CAM):
    px = np.asarray(px, float).reshape(-1, 2)
    pos = np.stack([np.zeros(len(px)), np.zeros(len(px)), np.full(len(px), 2.0)], 1)
    return abi.KeyframeDecideJob(cam, IDENT, IDENT, px, pos, alive, (), (), None, (), (), prev, MIN_T, MIN_R)


@functools.lru_cache(maxsize=None)
def key_point_batch():
    """ties (first in list wins), holders alive / dead / outside their quadrant, the cv quirk, a non-square image, no alive point"""
    rng = np.random.default_rng(9003)
    jobs = []
    # ties: slot 0 between points 1 and 3 (both at distance 5), quadrant 1 product between points 2 and 4 (6 * 2 == 12 * 1)
    jobs.append(_px_job([[100, 20], [85, 60], [86, 62], [80, 65], [92, 61], [10, 10]]))
    assert list(K.decide(jobs[-1])["key_pts"][:2]) == [1, 2]
    # holders alive: a holder keeps its slot against an equal challenger that comes earlier in the list
    jobs.append(_px_job([[86, 62], [92, 61], [85, 60], [80, 65]], prev=(3, 1, -1, -1, -1)))
    assert list(K.decide(jobs[-1])["key_pts"][:2]) == [3, 1]
    # dead holders are dropped first
    jobs.append(_px_job([[86, 62], [83, 64], [85, 60], [80, 65], [20, 20]], alive=[1, 0, 1, 0, 1], prev=(3, 1, 4, 4, 1)))
    # a holder outside its quadrant stays until a point of the quadrant beats its product: slot 1 holds a point of the top-left corner,
    # whose product is large and positive
    jobs.append(_px_job([[5, 5], [150, 110], [90, 70]], prev=(-1, 0, -1, -1, -1)))
    assert K.decide(jobs[-1])["key_pts"][1] == 0
    jobs.append(_px_job([[70, 30], [70, 90], [50, 30], [50, 90], [100, 30], [100, 90]]))      # x = 70 is left of cu = 80 but not of cv = 60
    kp = K.decide(jobs[-1])["key_pts"]
    assert list(kp[3:]) == [2, 3] and 0 not in kp[1:] and 1 not in kp[1:]
    jobs.append(_px_job(np.stack([rng.uniform(0, 160, 40), rng.uniform(0, 120, 40)], 1), alive=np.zeros(40, np.uint8), prev=(3, 4, 5, 6, 7)))
    assert list(K.decide(jobs[-1])["key_pts"]) == [-1] * 5                                     # no alive point
    jobs.append(_px_job(np.stack([rng.uniform(0, 752, 300), rng.uniform(0, 480, 300)], 1), alive=rng.random(300) > 0.3,
                        prev=(7, 8, 9, 10, 11), cam=CAM_BIG))
    jobs.append(_px_job(np.round(np.stack([rng.uniform(0, 160, 130), rng.uniform(0, 120, 130)], 1) / 8) * 8))   # a coarse lattice: many ties
    jobs.append(_px_job(np.zeros((0, 2))))
    return tuple(jobs)


@functools.lru_cache(maxsize=None)
def need_new_kf_batch():
    """empty overlap list; first, last and no keyframe blocking; the strict < at delta_t == min_t; 70 overlap keyframes (two rounds)"""
    rng = np.random.default_rng(9004)
    at = lambda x: np.array([[0, 0, 0, 1, x, 0, 0]], float)
    eq = abi.KeyframeDecideJob(CAM, IDENT, IDENT, [[80, 60]], [[0, 0, 2]], None, (), (), None, at(0.06), [0], (-1,) * 5, MIN_T, MIN_R)
    below = abi.KeyframeDecideJob(CAM, IDENT, IDENT, [[80, 60]], [[0, 0, 2]], None, (), (), None, at(np.nextafter(0.06, 0)), [0], (-1,) * 5, MIN_T, MIN_R)
    r = K.decide(eq)
    assert r["delta_t"][0] == 0.06 and r["need_new_kf"] == 1 and K.decide(below)["blocking"] == 0
    jobs = [rand_decide_job(rng, 30, 5, 6, n_ov=0),
            rand_decide_job(rng, 30, 5, 6, blocking_at=0),
            rand_decide_job(rng, 30, 5, 10, blocking_at=9),
            rand_decide_job(rng, 30, 5, 10),
            eq, below,
            rand_decide_job(rng, 10, 0, 70, blocking_at=66),
            rand_decide_job(rng, 10, 0, 70),
            rand_decide_job(rng, 40, 10, 12, blocking_at=5, n_ov=8)]
    constructed = (4, 5)
    for k, j in enumerate(jobs):     # no decision of a random case hangs on the last bits of atan / tan
        if k in constructed:
            continue
        r = K.decide(j)
        assert np.all(np.abs(r["delta_t"] / MIN_T - 1) > 1e-9) and np.all(np.abs(r["delta_r"] / MIN_R - 1) > 1e-9)
    assert [K.decide(j)["blocking"] for j in jobs] == [-1, 0, 9, -1, -1, 0, 66, -1, 5]
    return tuple(jobs)


def decide_batches():
    return dict(depth_counts=depth_count_batch(), depth_patterns=depth_pattern_batch(), key_points=key_point_batch(), need_new_kf=need_new_kf_batch())


def _table(rng, T_f_w, n_kf, cam=CAM, p_valid=0.8, p_visible=0.6, p_kf=0.7):
    """a keyframe table around the frame: each keyframe has key points in the frame's view (close) or behind it"""
    kf_T = np.array([synth.se3_mul(rand_pose(rng, 0.2, 1.0), np.asarray(T_f_w, float)) for _ in range(n_kf)]).reshape(-1, 7)
    kp = np.zeros((n_kf, 5, 3))
    for i in range(n_kf):
        vis, _ = points_in_view(rng, T_f_w, cam, 5)
        hid, _ = points_in_view(rng, T_f_w, cam, 5, -6.0, -1.0)
        kp[i] = np.where(rng.random((5, 1)) < (p_visible if rng.random() < p_kf else 0.0), vis, hid)
    return kf_T, kp, (rng.random((n_kf, 5)) < p_valid).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def close_batch():
    """n_kf = 0, 1, 10, 11, 70; equal distances; all key points invalid; a key point on px.x == 0 and on px.x == width; z just below 0 and at 0"""
    rng = np.random.default_rng(9005)
    jobs = []
    for n_kf in (0, 1, 10, 11, 70):
        T = rand_pose(rng)
        jobs.append(abi.CloseKeyframesJob(CAM, T, *_table(rng, T, n_kf, p_visible=0.9 if n_kf <= 11 else 0.6), max_n_kfs=10))
    assert K.close(jobs[3])["n_close"] >= 1 and K.close(jobs[4])["n_close"] > 10
    # equal distances: 12 keyframes on four distances from the frame's translation, every key point visible
    T = rand_pose(rng)
    kf_T, kp, kv = _table(rng, T, 12, p_visible=1.0, p_valid=1.0)
    kp[:] = points_in_view(rng, T, CAM, 60)[0].reshape(12, 5, 3)
    for i in range(12):
        kf_T[i, 4:] = T[4:] + np.array([[0.5, 0, 0], [-0.5, 0, 0], [0, 0.25, 0], [0, 0, -0.25]][i % 4])
    jobs.append(abi.CloseKeyframesJob(CAM, T, kf_T, kp, kv))
    r = K.close(jobs[-1])
    assert r["n_close"] == 12 and len(set(r["close_dist"])) < 12 and r["n_overlap"] == 10
    # keyframes whose key points are all invalid (every second one)
    T = rand_pose(rng)
    kf_T, kp, kv = _table(rng, T, 9, p_visible=1.0, p_valid=1.0, p_kf=1.0)
    kv[::2] = 0
    jobs.append(abi.CloseKeyframesJob(CAM, T, kf_T, kp, kv))
    assert set(K.close(jobs[-1])["close_idx"]) == {1, 3, 5, 7}
    # image border and z = 0, identity pose, one valid key point per keyframe:
    #   0: px.x == 0 (visible)   1: px.x == width (not)   2: px.y == height (not)   3: z just below 0 (not)   4: z == 0, x != 0: px = inf (not)
    #   5: z == 0 and x == y == 0: px = NaN (not)   6: the smallest positive z on the axis (visible)   7: z == -0.0 on the axis: not < 0, px = NaN (not)
    edge = np.array([[-0.625, 0, 1.0], [0.625, 0, 1.0], [0, 0.46875, 1.0], [0, 0, -1e-300], [0.1, 0.1, 0.0], [0, 0, 0.0], [0, 0, 5e-324], [0, 0, -0.0]])
    kp = np.zeros((8, 5, 3)); kp[:, 2] = edge
    kv = np.zeros((8, 5), np.uint8); kv[:, 2] = 1
    kf_T = np.array([synth.se3_exp(np.concatenate([[0.1 * (8 - i), 0, 0], np.zeros(3)])) for i in range(8)])
    jobs.append(abi.CloseKeyframesJob(CAM, IDENT, kf_T, kp, kv))
    assert K.w2c(CAM_T, edge[0])[0] == 0.0 and K.w2c(CAM_T, edge[1])[0] == 160.0 and K.w2c(CAM_T, edge[2])[1] == 120.0
    assert list(K.close(jobs[-1])["close_idx"]) == [6, 0]
    # max_n_kfs = 0 and a large table in which nothing is close
    T = rand_pose(rng)
    kf_T, kp, kv = _table(rng, T, 66, p_visible=0.0)
    jobs.append(abi.CloseKeyframesJob(CAM, T, kf_T, kp, kv, max_n_kfs=0))
    assert len(jobs) == 9
    return tuple(jobs)
