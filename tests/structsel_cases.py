"""Cases of the structure optimisation on the resident map tables (plsvo_candidates_optimize_structure), shared by
tests/test_gpu_structsel.py and the CPU test of the restatement.  Streams are built with tests/insert_cases.Builder (the 326 x 246 camera,
cells of 30 / 25 pixels): every landmark sits in a cell of its own and is found, so it becomes a feature of the new frame; positions are
then moved off their observations so that the optimiser has work to do.  Keys are given PER FEATURE POSITION (the selection's order is
known once the frame has run) and scattered to the landmarks by keys_by_feature().  Built once (seeded), never changed."""
import functools

import numpy as np

import insert_cases as Ic
import np_structsel as NS

G, C_ = Ic.G, Ic.C_
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def stream(n_pt, n_seg, n_kf=3, seed=0, obs=None, double_seg=(), depth0=None, noise=0.02):
    """n_pt point and n_seg segment landmarks, each a feature of the new frame.  obs: {point: number of observing keyframes} (default: two
    or three); double_seg: segments that span two cells and win both; depth0: a point that gets one more observation in a keyframe
    (appended as the last row) in whose frame it lies at depth 0"""
    rng = np.random.default_rng(7100 + seed)
    b = Ic.Builder(n_kf)
    obs = obs or {}
    for k in range(n_pt):
        n_obs = obs.get(k, 2 + k % 2)
        b.pt(*Ic.pc(k + 11), G, 1, kfs=tuple((k + j) % n_kf for j in range(min(n_obs, n_kf))))
    cells = iter(c for c in range(16, 126, 2) if 2 <= c % 14 <= 10)    # (even cells away from the image border: the moved positions stay inside it)
    for k in range(n_seg):
        if k in double_seg:
            c = next(cells)
            while c % 14 > 8:
                c = next(cells)
            next(cells)
            b.seg(Ic.sc(c), Ic.sc(c + 2), G, kfs=(k % n_kf, (k + 1) % n_kf))
        else:
            p = Ic.sc(next(cells))
            b.seg((p[0] - 4, p[1]), (p[0] + 4, p[1] + 2), G, kfs=tuple((k + j) % n_kf for j in range(2 + k % 2)))
    s = b.done(remove_kf=-1)
    st = s["st"]
    if depth0 is not None:                                             # a keyframe whose centre has the landmark's z: p_in_f[2] == 0 -> dp is NaN
        z = st["pt_pos"][depth0][2]
        st["kf_T"].append([float(v) for v in Ic.Cc.kf_at((0.5, -0.4, z))]); st["kf_slot"].append(len(st["kf_T"]) - 1)
        st["kf_pt"].append([]); st["kf_seg"].append([])
        st["pt_obs"][depth0].append(dict(kf=len(st["kf_T"]) - 1, px=[100.0, 90.0], f=[0.6, 0.0, 0.8], level=0, type=0, grad=[1.0, 0.0]))
        s["depth0"] = depth0
    for name in ("pt_pos", "seg_spos", "seg_epos"):                    # (with a depth-0 landmark every z stays exact)
        moved = []
        for p in st[name]:
            e = rng.uniform(-noise, noise, 3)
            moved.append([float(p[0] + e[0]), float(p[1] + e[1]), float(p[2] + (0.0 if depth0 is not None else e[2]))])
        st[name] = moved
    NS.keys(st)
    return s


def keys_by_feature(st, sel, pt_keys=None, seg_keys=None, default=0):
    """per-landmark key arrays with keys[i] on the landmark of feature i (a later feature of the same landmark wins), `default` elsewhere"""
    out = {}
    for name, keys in (("pt", pt_keys), ("seg", seg_keys)):
        v = [int(default)] * len(st[name + "_pos" if name == "pt" else name + "_spos"])
        if keys is not None:
            for lm, k in zip(sel[name + "_lm"], keys):
                v[int(lm)] = int(k)
        out[name + "_last_optim"] = v
    return out


def tie_keys(n, low, ties, low_key=1, tie_key=5, high_key=9):
    """n feature keys: positions `low` hold low_key, positions `ties` tie_key, the rest high_key"""
    k = [high_key] * n
    for i in low:
        k[i] = low_key
    for i in ties:
        k[i] = tie_key
    return k


@functools.lru_cache(maxsize=None)
def seventy():
    """70 point features (more than a round of 64) and 12 segments, two of them doubly won"""
    return stream(70, 12, seed=1, double_seg=(3, 8))


@functools.lru_cache(maxsize=None)
def fifty():
    return stream(50, 10, seed=2)


@functools.lru_cache(maxsize=None)
def observations():
    """a landmark with one observation (rank-2 system), one with twelve, one at depth 0 in a keyframe"""
    return stream(24, 6, n_kf=12, seed=3, obs={0: 1, 1: 12, 5: 1, 6: 12}, depth0=2)


@functools.lru_cache(maxsize=None)
def batch():
    """four streams with different counts; the third has no feature at all"""
    return (stream(30, 8, seed=4, double_seg=(1,)), stream(21, 0, seed=5), Ic.many_features_stream(found=0), stream(5, 25, seed=6, double_seg=(0, 4)))
