"""Cases of the new map candidates (plsvo_candidates_add), shared by tests/test_newcand_host.py and tests/test_gpu_newcand.py.  Streams are
those of tests/insert_cases.py (the insertion's preconditions hold: a candidate has exactly one observation and no feature), on the
326 x 246 camera with cells of 30 / 25 pixels of tests/select_cases.py; matches and keep masks are inputs.  On top of a stream a case
carries `new`: the records of the landmarks that converged, in the form tests/np_newcand.py reads, and the matcher's verdict on them for
the frames behind the add (found_pt / found_seg gain the new indices).  Built once (seeded), never changed."""
import copy
import functools

import numpy as np

import candidates_cases as Cc
import insert_cases as Ic
import np_keyframe as K
import np_newcand as NC
import select_cases as Sc

CAM_T, CAM, CELL, SEG_CELL, BOUNDARY, PARAMS = Ic.CAM_T, Ic.CAM, Ic.CELL, Ic.SEG_CELL, Ic.BOUNDARY, Ic.PARAMS
# per kind: both sides of the 64-lane round.  (points, segments) per stream; (0, 0) stands by
COUNTS = ((1, 130), (0, 0), (63, 64), (64, 0), (0, 63), (0, 0), (65, 1), (130, 65), (0, 0), (5, 3), (0, 0), (2, 2), (3, 0))
LM_RESERVE = dict(extra_pt=280, extra_seg=280)                       # two adds of any stream here
RESERVE = {k: v + 280 for k, v in Ic.RESERVE.items() if k != "extra_kf"}
RESERVE["extra_kf"] = Ic.RESERVE["extra_kf"]
HIGH_LEVEL = 2                                                        # above every staged observation's (the builders give 0 and 1)


def world(T, px, py, z):
    """the world position the pose T sees at pixel (px, py) and depth z"""
    return [float(v) for v in K.se3_act(K.se3_inv(T), Sc.pos_at(px, py, z))]


def make_new(rng, s, st, n_pt, n_seg, high_level=False, edgelets=True):
    """n_pt points and n_seg segments in view of the stream's frame, each observed in one keyframe of the table as it stands: the first, the
    last, then in turn.  Every third point observation is an edgelet where the matcher's border test accepts it.
    Returns (new, found_pt, found_seg): the records and the matcher's verdict per new landmark index"""
    n_kf = len(st["kf_T"])
    assert n_kf > 0 or n_pt + n_seg == 0
    w, h = CAM_T[4], CAM_T[5]
    kf_of = lambda j: (0, n_kf - 1)[j] if j < 2 else int(rng.integers(0, n_kf))
    new = dict(pt=[], seg=[])
    found_pt, found_seg = {}, {}
    for j in range(n_pt):
        pos = world(s["T"], rng.uniform(20, w - 20), rng.uniform(20, h - 20), rng.uniform(2.0, 6.0))
        kf = kf_of(j)
        level = HIGH_LEVEL if high_level and j % 2 == 0 else j % 2
        o = Sc.observe(kf, st["kf_T"][kf], pos, level=level, ftype=0, grad=(1.0, 0.0))
        if edgelets and j % 3 == 0 and 30 <= o["px"][0] < w - 30 and 30 <= o["px"][1] < h - 30:
            o["type"], o["grad"] = 1, [0.6, 0.8]
        new["pt"].append(dict(pos=pos, obs=o))
        found_pt[len(st["pt_pos"]) + j] = int(j % 4 != 3)
    for j in range(n_seg):
        x, y = rng.uniform(40, w - 40), rng.uniform(40, h - 40)
        z = rng.uniform(2.0, 6.0)
        sp, ep = world(s["T"], x, y, z), world(s["T"], x + rng.uniform(-30, 30), y + rng.uniform(-30, 30), z + rng.uniform(-0.3, 0.3))
        kf = kf_of(j)
        a, b = Sc.observe(kf, st["kf_T"][kf], sp), Sc.observe(kf, st["kf_T"][kf], ep)
        new["seg"].append(dict(spos=sp, epos=ep, obs=dict(kf=kf, spx=a["px"], epx=b["px"], sf=a["f"], ef=b["f"], level=HIGH_LEVEL if high_level and j == 0 else j % 2)))
        found_seg[len(st["seg_spos"]) + j] = (int(j % 5 != 4), int(j % 7 != 6))
    return new, found_pt, found_seg


def with_new(s, new, found_pt, found_seg):
    """the case: the stream (its tables shared, never changed) with the records and the found flags of the new landmarks"""
    return dict(s, new=new, found_pt={**s["found_pt"], **found_pt}, found_seg={**s["found_seg"], **found_seg})


def segments_only_stream():
    """no point landmark at all before the add"""
    b = Ic.Builder(2)
    cs = iter(range(16, 60, 2))
    for k in range(8):
        p = Ic.sc(next(cs))
        b.seg((p[0] - 4, p[1]), (p[0] + 4, p[1] + 2), (Ic.C_ if k % 4 == 0 else Ic.G), kfs=(k % 2,), cand=k % 4 == 0)
    return b.done(remove_kf=0)


def no_candidates_stream():
    """both candidate lists empty before the add"""
    b = Ic.Builder(3)
    for k in range(20):
        b.pt(*Ic.pc(k + 12), (Ic.U, Ic.G)[k % 2], k % 3 != 0, kfs=(k % 3, (k + 1) % 3))
    cs = iter(range(16, 60, 2))
    for k in range(6):
        p = Ic.sc(next(cs))
        b.seg((p[0] - 4, p[1]), (p[0] + 4, p[1] + 2), Ic.G, kfs=(k % 3,))
    return b.done(remove_kf=2)


@functools.lru_cache(maxsize=None)
def batch():
    """thirteen unequal streams (four workgroups of four waves, the last one partial) and what each of them adds (COUNTS)"""
    rng = np.random.default_rng(7101)
    R = Ic.random_stream
    base = (R(rng, 4, 60, 30, 5, 4, remove_kf=1),
            R(rng, 3, 40, 20, 4, 3, remove_kf=-1, is_kf=False),
            Ic.candidates_stream(),                                   # no segment landmark before the add, 70 point candidates
            R(rng, 5, 90, 40, 9, 7, remove_kf=0),                     # adds points only
            R(rng, 6, 70, 30, 6, 5, remove_kf=5),                     # adds segments only
            Ic.directed_stream(),
            segments_only_stream(),
            R(rng, 4, 70, 30, 8, 6, remove_kf=-1),
            Ic.many_features_stream(),
            no_candidates_stream(),
            Ic.first_keyframe_stream(),                               # no keyframe: nothing can be observed, nothing is added
            R(rng, 2, 30, 10, 2, 2, remove_kf=0),
            R(rng, 3, 25, 12, 0, 3, remove_kf=-1, is_kf=False))
    assert len(base) == len(COUNTS)
    return tuple(with_new(s, *make_new(rng, s, s["st"], n_pt, n_seg, high_level=k == 9)) for k, (s, (n_pt, n_seg)) in enumerate(zip(base, COUNTS)))


def second_new(cases, sts):
    """a second add on the tables as they stand: indices continue behind the first.  -> cases with the new records"""
    rng = np.random.default_rng(7102)
    counts = [(0, 0) if not st["kf_T"] else ((k * 7) % 11, (k * 5) % 9) for k, st in enumerate(sts)]
    return [with_new(s, *make_new(rng, s, st, n_pt, n_seg)) for s, st, (n_pt, n_seg) in zip(cases, sts, counts)]


def records(new):
    """the records as capi.Context.candidates_add takes them: arrays named like plsvo_cand_new's, or None for a stream that stands by"""
    if not new["pt"] and not new["seg"]:
        return None
    col = lambda rows, f: [r["obs"][f] for r in rows]
    d = {}
    if new["pt"]:
        p = new["pt"]
        d.update(pt_pos=[r["pos"] for r in p], pt_obs_kf=col(p, "kf"), pt_obs_px=col(p, "px"), pt_obs_f=col(p, "f"), pt_obs_level=col(p, "level"), pt_obs_type=col(p, "type"),
                 pt_obs_grad=col(p, "grad"))
    if new["seg"]:
        q = new["seg"]
        d.update(seg_spos=[r["spos"] for r in q], seg_epos=[r["epos"] for r in q], seg_obs_kf=col(q, "kf"), seg_obs_spx=col(q, "spx"), seg_obs_epx=col(q, "epx"),
                 seg_obs_sf=col(q, "sf"), seg_obs_ef=col(q, "ef"), seg_obs_level=col(q, "level"))
    return d


def add(s, st):
    """the restatement's add of the case's records on `st` (mutated)"""
    return NC.add(st, s["new"])


def removal_of(s, st):
    """the keyframe an insertion behind the add removes: the stream's own choice, else the first row of a table of two or more"""
    return s["remove_kf"] if s["remove_kf"] >= 0 else (0 if len(st["kf_T"]) >= 2 else -1)
