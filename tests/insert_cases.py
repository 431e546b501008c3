"""Cases of the keyframe insertion into the resident map tables (plsvo_candidates_insert_keyframe), shared by tests/test_insert_host.py
and tests/test_gpu_insert.py.  Streams are the dicts of tests/candidates_cases.py with the counters of np_select.quality(); unlike the
random streams of the earlier stages they keep the insertion's preconditions: every keyframe feature that holds a landmark has an
observation of that landmark in that keyframe, a landmark in a candidate list has exactly one observation and no feature.  On top of a
stream a case carries the matcher's results as inputs (select_cases.match_of), the landmarks whose features the pose optimiser rejects
(`culled_*`: the keep masks are inputs too), and the insertion's arguments.  The 326 x 246 camera with cells of 30 / 25 pixels of
tests/select_cases.py.  Built once (seeded), never changed."""
import copy
import functools

import numpy as np

import candidates_cases as Cc
import np_candidates as N
import np_insert as I
import np_select as S
import select_cases as Sc

CAM_T, CAM, CELL, SEG_CELL, BOUNDARY = Sc.CAM_T, Sc.CAM, Sc.CELL, Sc.SEG_CELL, Sc.BOUNDARY
D, C_, U, G = Sc.D, Sc.C_, Sc.U, Sc.G
PARAMS = dict(max_fts=120, max_fts_segs=100, cell_order=None, seg_cell_order=None)
RESERVE = dict(extra_kf=2, extra_kf_pt=260, extra_kf_seg=120, extra_pt_obs=260, extra_seg_obs=120)   # room for two insertions of any stream here
T_NEW = [0.001, -0.002, 0.0005, 1.0, 0.01, -0.02, 0.005]     # the optimised pose handed to the insertion (copied, never normalised)


def kf_centre(k):
    return (0.03 * (k % 5) - 0.06, 0.02 * (k // 5) - 0.01, 0.0)


class Builder:
    """one stream whose new frame sits at the origin without rotation (a landmark's pixel is chosen directly) and whose keyframes stand
    next to it, so that every observation gives has_view 1"""

    def __init__(self, n_kf):
        self.kf_T = [Cc.kf_at(kf_centre(k)) for k in range(n_kf)]
        self.st = S.quality(Cc.empty_stream(self.kf_T))
        self.found_pt, self.found_seg, self.names, self.culled_pt, self.culled_seg = {}, {}, {}, set(), set()

    def pt(self, px, py, typ, found, kfs=(0,), cand=False, culled=False, edgelet=False, nfail=0, nsucc=0, name=None, z=4.0):
        """kfs: the keyframes that observe it, in the order of its observation list; each holds it as a feature unless it is a candidate"""
        pos = Sc.pos_at(px, py, z)
        lm = Cc.add_pt(self.st, pos, typ, [Sc.observe(k, self.kf_T[k], pos, level=(len(self.st["pt_pos"]) + k) % 2, ftype=int(edgelet), grad=(0.6, 0.8)) for k in kfs])
        self.st["pt_nfail"].append(nfail); self.st["pt_nsucc"].append(nsucc)
        if cand:
            self.st["pt_cand"].append(lm)
        elif typ != D:
            for k in kfs:
                self.st["kf_pt"][k].append(lm)
        self.found_pt[lm] = int(found)
        if culled:
            self.culled_pt.add(lm)
        if name:
            self.names[name] = lm
        return lm

    def seg(self, s, e, typ, found=(1, 1), kfs=(0,), cand=False, culled=False, nfail=0, nsucc=0, name=None):
        sp, ep = Sc.pos_at(*s), Sc.pos_at(*e)
        obs = []
        for k in kfs:
            a, b = Sc.observe(k, self.kf_T[k], sp), Sc.observe(k, self.kf_T[k], ep)
            obs.append(dict(kf=k, spx=a["px"], epx=b["px"], sf=a["f"], ef=b["f"], level=(len(self.st["seg_spos"]) + k) % 2))
        lm = Cc.add_seg(self.st, sp, ep, typ, obs)
        self.st["seg_nfail"].append(nfail); self.st["seg_nsucc"].append(nsucc)
        if cand:
            self.st["seg_cand"].append(lm)
        elif typ != D:
            for k in kfs:
                self.st["kf_seg"][k].append(lm)
        self.found_seg[lm] = (int(found[0]), int(found[1]))
        if culled:
            self.culled_seg.add(lm)
        if name:
            self.names[name] = lm
        return lm

    def pad(self, kf, n_pt, n_seg):
        """features without a landmark until the keyframe's lists have the given lengths"""
        for name, n in (("kf_pt", n_pt), ("kf_seg", n_seg)):
            fts = self.st[name][kf]
            assert len(fts) <= n, (name, kf, len(fts), n)
            fts += [-1] * (n - len(fts))

    def done(self, remove_kf=-1, is_kf=True, overlap=None, kf_slot=1):
        n_kf = len(self.kf_T)
        return dict(st=self.st, T=list(Cc.IDENT), overlap=tuple(range(n_kf)) if overlap is None else tuple(overlap), found_pt=self.found_pt, found_seg=self.found_seg,
                    names=self.names, culled_pt=frozenset(self.culled_pt), culled_seg=frozenset(self.culled_seg), remove_kf=remove_kf, is_kf=is_kf, kf_slot=kf_slot,
                    T_new=list(T_NEW))


pc = Sc.centre
sc = lambda cell, dx=0.5, dy=0.5: Sc.centre(cell, SEG_CELL, Sc.SEG_COLS, dx, dy)


# ---- constructed streams ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def directed_stream():
    """eight keyframes, keyframe 3 is removed.  Every landmark sits in a cell of its own, so that `found` decides whether it is a feature."""
    b = Builder(8)
    R = 3
    cells = iter(range(12, 88))
    nxt = lambda: pc(next(cells))
    # observation lists of 1, 2, 3 and 7 entries that include the removed keyframe, with and without a new observation
    for n_obs, kfs in ((1, (R,)), (2, (0, R)), (3, (R, 1, 5)), (7, (0, 1, 2, R, 4, 5, 6))):
        for found in (0, 1):
            b.pt(*nxt(), G, found, kfs=kfs, name="obs%d_found%d" % (n_obs, found))
    b.pt(*nxt(), G, 1, kfs=(0, R), culled=True, name="culled_in_removed")      # matched, rejected by the pose optimiser: no new observation, list of 2 -> deleted
    b.pt(*nxt(), G, 1, kfs=(0, 1, 2), name="untouched")
    b.pt(*pc(48), G, 1, kfs=(5, 7), edgelet=True, name="edgelet")             # (well inside the frame: the matcher's border test)
    b.pt(*nxt(), D, 1, kfs=(R, 4, R + 2), name="deleted_earlier")              # no feature holds it; its list loses the removed row
    b.pt(*nxt(), U, 0, kfs=(6, 7), nfail=15, name="deleted_by_selection")      # safeDeletePoint in this frame's selection
    # candidates
    b.pt(*nxt(), C_, 1, kfs=(R,), cand=True, name="cand_joins_removed")        # joins keyframe 3, list of 2 -> deleted, the new frame's feature loses it
    b.pt(*nxt(), C_, 0, kfs=(R,), cand=True, name="cand_unmatched_removed")    # removeFrameCandidates
    b.pt(*nxt(), C_, 0, kfs=(2,), cand=True, name="cand_unmatched_stays")
    b.pt(*nxt(), C_, 1, kfs=(2,), cand=True, culled=True, name="cand_culled")  # matched but culled: stays a candidate
    a, c = nxt(), nxt()                                                        # two candidates join keyframe 6: listed second-then-first of the visit order
    b.names["cand_pair"] = [b.pt(*c, C_, 1, kfs=(6,), cand=True), b.pt(*a, C_, 1, kfs=(6,), cand=True)]
    # segments
    cs = iter(range(16, 98, 2))                                                 # (even cells: never the last, partial column)
    one = lambda typ, found=(1, 1), **kw: (lambda p: b.seg((p[0] - 4, p[1]), (p[0] + 4, p[1] + 2), typ, found, **kw))(sc(next(cs)))
    one(G, kfs=(R, R), name="seg_twice_in_removed")                            # list of 3 after the push: erased once, then deleted
    b.seg(sc(100), sc(102), G, kfs=(0, 1), name="seg_wins_both")               # a feature twice: two observations, the later feature's in front
    b.seg(sc(104), sc(106), G, kfs=(R, 2, 4), name="seg_wins_both_removed")    # 3 + 2, one erased
    one(G, found=(1, 0), kfs=(R, 1), name="seg_unmatched_removed")             # list of 2 -> deleted
    one(G, kfs=(1, 2, 4), name="seg_untouched")
    one(C_, kfs=(5,), cand=True, name="seg_cand_joins")
    one(C_, found=(0, 1), kfs=(R,), cand=True, name="seg_cand_unmatched_removed")   # the pinned case
    one(C_, found=(0, 0), kfs=(0,), cand=True, name="seg_cand_stays")
    one(C_, kfs=(R,), cand=True, name="seg_cand_joins_removed")
    return b.done(remove_kf=R)


@functools.lru_cache(maxsize=None)
def sizes_stream():
    """keyframes of 0, 1, 63, 64, 65 and 130 point features (130, 65, 0, 1, 63, 64 segment features); the one of 64 / 1 is removed"""
    rng = np.random.default_rng(6101)
    b = Builder(6)
    sizes = ((0, 130), (1, 65), (63, 0), (64, 1), (65, 63), (130, 64))
    b.pt(*pc(12), G, 1, kfs=(1, 3, 5), name="only_feature_of_kf1")
    b.seg(sc(17), sc(17, 6, 3), G, kfs=(3, 0), name="only_segment_of_kf3")
    for k, cell in enumerate(range(13, 60)):
        kfs = [int(v) for v in rng.permutation([2, 3, 4, 5])[:rng.integers(1, 5)]]
        b.pt(*pc(cell), (U, G)[k % 2], int(rng.random() < 0.7), kfs=kfs, culled=rng.random() < 0.15)
    for k, cell in enumerate(range(30, 120, 4)):                               # (even cells: never the last, partial column)
        kfs = [int(v) for v in rng.permutation([0, 1, 4, 5])[:rng.integers(1, 5)]]
        p = sc(cell)
        b.seg((p[0] - 4, p[1]), (p[0] + 4, p[1] + 2), (U, G)[k % 2], (int(rng.random() < 0.8), 1), kfs=kfs, culled=rng.random() < 0.15)
    for k, (n_pt, n_seg) in enumerate(sizes):
        b.pad(k, n_pt, n_seg)
        rng.shuffle(b.st["kf_pt"][k]); rng.shuffle(b.st["kf_seg"][k])
    return b.done(remove_kf=3, overlap=(5, 0, 4, 2, 3))


@functools.lru_cache(maxsize=None)
def many_features_stream(culled=False, found=1):
    """70 point features in 70 cells (more than a round of 64) and 12 segments, four of them candidates; no keyframe is removed.
    culled: the pose optimiser rejects every feature; found = 0: the new frame has no feature at all"""
    b = Builder(2)
    for k in range(70):
        b.pt(*pc(k + 11), G, found, kfs=(k % 2,), culled=culled)
    cs = iter(range(16, 126, 2))
    for k in range(12):
        p = sc(next(cs))
        b.seg((p[0] - 4, p[1]), (p[0] + 4, p[1] + 2), (C_ if k % 3 == 0 else G), (found, found), kfs=(k % 2,), cand=k % 3 == 0, culled=culled)
    return b.done(remove_kf=-1)


@functools.lru_cache(maxsize=None)
def candidates_stream():
    """70 candidates in cells of their own, 66 of them matched: they join keyframes 0 .. 2 in list order; keyframe 2 (the last) is removed"""
    b = Builder(3)
    for k in range(70):
        b.pt(*pc(k + 11), C_, int(k % 17 != 3), kfs=(k % 3,), cand=True, nfail=k % 5)
    b.pt(*pc(82), G, 1, kfs=(0, 1, 2))
    return b.done(remove_kf=2)


def first_keyframe_stream():
    """a map without keyframes: the new frame becomes its first one"""
    return Builder(0).done(remove_kf=-1)


def random_stream(rng, n_kf, n_pt, n_seg, n_ptc, n_segc, remove_kf, is_kf=True, p_found=0.6):
    """a random stream under the insertion's preconditions, counters near the selection's thresholds"""
    b = Builder(n_kf)
    somewhere = lambda: (rng.uniform(-40, 360), rng.uniform(-30, 270))
    counters = lambda: dict(nfail=int(rng.choice([0, 3, 14, 15, 16, 28, 29, 30, 31])), nsucc=int(rng.choice([0, 5, 9, 10, 11])))
    kfs_of = lambda: [int(v) for v in rng.permutation(n_kf)[:rng.integers(1, min(n_kf, 5) + 1)]]
    for _ in range(n_pt):
        b.pt(*somewhere(), int(rng.choice([D, U, G], p=[0.08, 0.42, 0.5])), int(rng.random() < p_found), kfs=kfs_of(), culled=rng.random() < 0.15, z=rng.uniform(2.0, 6.0), **counters())
    for _ in range(n_seg):
        s = somewhere()
        kfs = kfs_of()
        if rng.random() < 0.1:
            kfs.append(kfs[0])                                                 # was a feature twice when that keyframe was new
        b.seg(s, (s[0] + rng.uniform(-50, 50), s[1] + rng.uniform(-50, 50)), int(rng.choice([D, U, G], p=[0.08, 0.42, 0.5])), (int(rng.random() < 0.85), int(rng.random() < 0.85)),
              kfs=kfs, culled=rng.random() < 0.15, **counters())
    for _ in range(n_ptc):
        b.pt(*somewhere(), C_, int(rng.random() < p_found), kfs=(int(rng.integers(0, n_kf)),), cand=True, culled=rng.random() < 0.15, **counters())
    for _ in range(n_segc):
        s = somewhere()
        b.seg(s, (s[0] + rng.uniform(-50, 50), s[1] + rng.uniform(-50, 50)), C_, (int(rng.random() < 0.85), int(rng.random() < 0.85)), kfs=(int(rng.integers(0, n_kf)),), cand=True,
              **counters())
    for k in range(n_kf):
        for name in ("kf_pt", "kf_seg"):
            fts = b.st[name][k]
            fts += [-1] * int(rng.integers(0, 6))
            rng.shuffle(fts)
    s = b.done(remove_kf=remove_kf, is_kf=is_kf, overlap=[int(v) for v in rng.permutation(n_kf)[:max(n_kf - 1, 1)]])
    s["T"] = Cc.rand_pose(rng, 0.05, 0.1)
    return s


@functools.lru_cache(maxsize=None)
def batch():
    """thirteen unequal streams: four workgroups of four waves, the last one partial; streams 1, 3 and 8 do not insert"""
    rng = np.random.default_rng(6102)
    return (sizes_stream(),
            random_stream(rng, 4, 60, 30, 5, 4, remove_kf=1, is_kf=False),
            directed_stream(),
            random_stream(rng, 3, 40, 20, 4, 3, remove_kf=-1, is_kf=False),
            random_stream(rng, 5, 120, 60, 9, 7, remove_kf=0),                 # the first row leaves
            random_stream(rng, 6, 90, 40, 6, 5, remove_kf=5),                  # the last one
            random_stream(rng, 4, 70, 30, 8, 6, remove_kf=-1),                 # none
            many_features_stream(found=0),                                     # a new frame without features
            random_stream(rng, 2, 30, 10, 2, 2, remove_kf=0, is_kf=False),
            many_features_stream(culled=True),                                 # every feature rejected
            many_features_stream(),                                            # 70 point features
            candidates_stream(),
            first_keyframe_stream())


# ---- the restatement of a frame and of the insertion behind it ----------------------------------------------------------------------------
def frame(s, st, A=None, T=None, overlap=None):
    """candidates -> constructed match -> selection of one frame on `st` (mutated).  Returns (candidates, match, selection)."""
    s2 = dict(s, T=s["T"] if T is None else T, overlap=s["overlap"] if overlap is None else overlap)
    r = Sc.restate_candidates(s2, st)
    m = Sc.match_of(s2, r)
    sel = S.select(st, r, m, CAM_T, CELL, SEG_CELL, PARAMS["max_fts"], PARAMS["max_fts_segs"], PARAMS["cell_order"], PARAMS["seg_cell_order"], A=Sc.synthetic_A(r) if A is None else A)
    return r, m, sel


def keep_masks(s, sel):
    return (np.array([0 if lm in s["culled_pt"] else 1 for lm in sel["pt_lm"]], np.uint8), np.array([0 if lm in s["culled_seg"] else 1 for lm in sel["seg_lm"]], np.uint8))


def insert(s, st, sel, remove_kf=None, slot=None):
    pk, sk = keep_masks(s, sel)
    return I.insert(st, sel, pk, sk, s["T_new"], s["kf_slot"] if slot is None else slot, s["remove_kf"] if remove_kf is None else remove_kf, CAM_T)


def tables(st):
    """the stream's tables as plsvo_candidates_fetch_map reports them: arrays named like the plsvo_cand_map fields"""
    return Cc.to_job(st).t


def sizes(st):
    return dict(n_kf=len(st["kf_T"]), n_kf_pt=sum(len(l) for l in st["kf_pt"]), n_kf_seg=sum(len(l) for l in st["kf_seg"]), n_pt_obs=sum(len(l) for l in st["pt_obs"]),
                n_seg_obs=sum(len(l) for l in st["seg_obs"]), n_pt_cand=len(st["pt_cand"]), n_seg_cand=len(st["seg_cand"]))


def second_frame_of(s, st, k):
    """pose and overlap list of a frame on the inserted tables: every keyframe of the new table, the new one first"""
    rng = np.random.default_rng(6200 + k)
    n_kf = len(st["kf_T"])
    T = [float(v) for v in Cc.synth.se3_exp(np.concatenate([rng.uniform(-0.02, 0.02, 3), rng.uniform(-0.01, 0.01, 3)]))]
    return T, tuple(range(n_kf - 1, -1, -1))
