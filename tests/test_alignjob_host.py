"""The restatement tests/np_alignjob.py on the CPU: its layout -- a plain first-fit loop written on its own -- against
plsvo_align_slot_layout (host-only) on random segment sets and on the directed sizes, its sample counts against the library's, and the
properties the alignment kernel relies on."""
import numpy as np
import pytest

import alignjob_cases as A
import np_alignjob as NA
import np_keyframe as K
import select_cases as Sc

P = Sc.P
CAM = (256.0, 256.0, 1088.0, 48.0, 2176, 96)


def random_segments(rng, n, cam):
    w, h = cam[4], cam[5]
    segs = []
    for _ in range(n):
        kind = rng.integers(0, 4)
        x0, y0 = rng.uniform(0, w), rng.uniform(0, h)
        if kind == 0:                                                  # along an axis, lengths around the thresholds of 64 samples
            length = float(rng.choice([16 * 127, 16 * 128 + 8, 16 * 129 + 3, 16 * 65, 16 * 33, 900.0, 40.0]))
            x0 = rng.uniform(24, max(25.0, w - length - 30))
            segs.append([x0, y0, x0 + length, y0])
        elif kind == 1:
            segs.append([x0, y0, x0 + rng.uniform(-30, 30), y0 + rng.uniform(-30, 30)])
        else:
            segs.append([x0, y0, rng.uniform(0, w), rng.uniform(0, h)])
    return segs


def host_layout(cam, n_pts, segs, alive, level):
    segs = np.asarray(segs, float).reshape(-1, 4)
    n = len(segs)
    job = P.abi.AlignJob(cam, 3, 0, 30, 1e-6, [0, 0, 0, 1, 0, 0, 0], np.zeros((n_pts, 2)), np.zeros((n_pts, 3)), segs[:, :2], segs[:, 2:],
                         [NA.seg_len([float(v) for v in s]) for s in segs], np.zeros((n, 3)), np.zeros((n, 3)), np.asarray(alive, np.uint8))
    first, N, n_slots, long_lines, n_patches = P.capi.align_slot_layout(job, level)
    return [int((c << 20) | f) if f >= 0 else -1 for f, c in zip(first, N)], n_slots, long_lines, n_patches


@pytest.mark.parametrize("seed", range(6))
def test_the_restated_layout_equals_the_host_helper(seed):
    rng = np.random.default_rng(7400 + seed)
    for n_pts in (0, 5, 63, 64, 65, 130):
        n_seg = int(rng.integers(0, 60))
        segs = random_segments(rng, n_seg, CAM)
        alive = rng.random(n_seg) < 0.85
        for level in range(4):
            want = host_layout(CAM, n_pts, segs, alive, level)
            got = NA.layout_level(n_pts, segs, list(alive), level, CAM, 32)
            assert got is not None and (got[0], got[1], got[2], got[3]) == want, (seed, n_pts, level)
            # with the segments at a multiple of 64: the same layout behind that many points
            got64 = NA.layout_level(n_pts, segs, list(alive), level, CAM, 64)
            pad = (n_pts + 63) // 64 * 64 if n_seg else n_pts
            want64 = host_layout(CAM, pad, segs, alive, level)
            assert got64[0] == want64[0] and got64[2] == want64[2] and got64[3] == want64[3] - (pad - n_pts), (seed, n_pts, level)
            assert got64[1] == (want64[1] if any(c >= 0 for c in got64[0]) else n_pts)


def test_a_short_segment_never_straddles_a_round_and_no_two_overlap():
    rng = np.random.default_rng(7410)
    segs = random_segments(rng, 80, CAM)
    for align in (32, 64):
        codes, used, _, _ = NA.layout_level(37, segs, [True] * 80, 1, CAM, align)
        taken = np.zeros(used, int)
        for c in codes:
            if c < 0:
                continue
            first, n = c & 0xfffff, c >> 20
            assert first >= (64 if align == 64 else 37) and (n > 64 or first // 64 == (first + n - 1) // 64)
            taken[first:first + n] += 1
        assert taken.max() == 1


def test_the_directed_lengths_hit_their_sample_counts():
    ns = lambda length, level: NA.num_samples([40.0, 40.0, 40.0 + length, 40.0], float(length), level)
    assert [ns(2040, l) for l in (1, 2, 3)] == [64, 32, 16] and [ns(2072, l) for l in (1, 2, 3)] == [65, 33, 17]
    assert ns(200, 1) == 6 and ns(10, 3) == 1 and ns(0.0, 0) == 1
    assert NA.in_border([20.0, 100.5, 250.0, 110.5], 2, Sc.CAM_T) and not NA.in_border([20.0, 100.5, 250.0, 110.5], 3, Sc.CAM_T)


def test_the_initial_model_is_the_product_not_the_identity():
    T0 = K.se3_mul(A.T_REF, K.se3_inv(A.T_REF))
    assert T0 != [0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0] and np.allclose(T0, [0, 0, 0, 1, 0, 0, 0], atol=1e-12)
    sel = dict(pt_lm=[0], pt_px=[[100.0, 90.0]], seg_lm=[], seg_px=np.zeros((0, 4)))
    j = NA.align_job(sel, [1], [], [3], [], [[0.1, 0.2, 4.0]], [], [], A.T_REF, Sc.CAM_T, A.cfg(), 64)
    assert j["T0"].tolist() == T0 and j["n_pts"] == 1 and j["skip"] == 0 and j["n_patches"] == 3
    dropped = NA.align_job(sel, [1], [], [NA.TYPE_DELETED], [], [[0.1, 0.2, 4.0]], [], [], A.T_REF, Sc.CAM_T, A.cfg(), 64)
    assert dropped["n_pts"] == 0 and dropped["skip"] == 1 and dropped["report"]["status"] == NA.OK
