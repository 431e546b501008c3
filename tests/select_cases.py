"""Cases of the cell selection of the map candidates (plsvo_candidates_select), shared by tests/test_select_host.py and
tests/test_gpu_select.py.  Streams are the dicts of tests/candidates_cases.py; on top of them a case carries the matcher's results as
INPUTS (found per landmark -- the projection shifted by a fixed amount stands in for the refined pixel, a level derived from the landmark
index for the search level), the landmarks' counters, and the selection's parameters.  Small frames, 326 x 246 with cells of 30 and
25 pixels: both grids end in a partial column and row.  Built once (seeded), never changed."""
import copy
import functools

import numpy as np

import candidates_cases as Cc
import np_candidates as N
import np_keyframe as K
import np_select as S

P = Cc.P
abi = Cc.abi

CAM_T = (256.0, 256.0, 163.0, 123.0, 326, 246)
CAM = abi.Pinhole(*CAM_T)
CELL, SEG_CELL, BOUNDARY = 30, 25, 8
COLS, SEG_COLS = 11, 14
N_CELLS, SEG_N_CELLS = S.n_cells(CAM_T, CELL), S.n_cells(CAM_T, SEG_CELL)          # 11 x 9, 14 x 10
D, C_, U, G = N.TYPE_DELETED, N.TYPE_CANDIDATE, N.TYPE_UNKNOWN, N.TYPE_GOOD


def pos_at(px, py, z=4.0):
    return [(px - CAM_T[2]) / CAM_T[0] * z, (py - CAM_T[3]) / CAM_T[1] * z, float(z)]


def observe(kf, T_kf, pos, level=0, ftype=0, grad=(1.0, 0.0)):
    c = K.se3_act(T_kf, pos)
    n = K.norm3(*c)
    return dict(kf=kf, px=[CAM_T[0] * c[0] / c[2] + CAM_T[2], CAM_T[1] * c[1] / c[2] + CAM_T[3]], f=[c[0] / n, c[1] / n, c[2] / n], level=level, type=ftype, grad=list(grad))


def cell_of(px, py, size=CELL, cols=COLS):
    return int(py / size) * cols + int(px / size)


class Builder:
    """one stream whose new frame sits at the origin without rotation: a landmark's pixel is chosen directly.  Keyframe 0 and 1 see
    every landmark from next to the new frame (has_view 1), keyframe 2 from far to the side (has_view 0)."""

    def __init__(self):
        self.kf_T = [Cc.kf_at((0.05, 0.0, 0.0)), Cc.kf_at((-0.05, 0.02, 0.0)), Cc.kf_at((6.0, 0.0, 3.0))]
        self.st = S.quality(Cc.empty_stream(self.kf_T))
        self.found_pt, self.found_seg, self.names = {}, {}, {}

    def pt(self, px, py, typ, found, nfail=0, nsucc=0, cand=False, view=True, edgelet=False, kf_list=0, name=None):
        pos = pos_at(px, py)
        k = 0 if view else 2
        lm = Cc.add_pt(self.st, pos, typ, [observe(k, self.kf_T[k], pos, level=len(self.st["pt_pos"]) % 2, ftype=int(edgelet), grad=(0.6, 0.8))])
        self.st["pt_nfail"].append(nfail); self.st["pt_nsucc"].append(nsucc)
        (self.st["pt_cand"] if cand else self.st["kf_pt"][kf_list]).append(lm)
        self.found_pt[lm] = int(found)
        if name:
            self.names[name] = lm
        return lm

    def seg(self, s, e, typ, found=(1, 1), nfail=0, nsucc=0, cand=False, view=True, kf_list=0, name=None):
        sp, ep = pos_at(*s), pos_at(*e)
        k = 0 if view else 2
        a, b = observe(k, self.kf_T[k], sp), observe(k, self.kf_T[k], ep)
        lm = Cc.add_seg(self.st, sp, ep, typ, [dict(kf=k, spx=a["px"], epx=b["px"], sf=a["f"], ef=b["f"], level=len(self.st["seg_spos"]) % 2)])
        self.st["seg_nfail"].append(nfail); self.st["seg_nsucc"].append(nsucc)
        (self.st["seg_cand"] if cand else self.st["kf_seg"][kf_list]).append(lm)
        self.found_seg[lm] = (int(found[0]), int(found[1]))
        if name:
            self.names[name] = lm
        return lm

    def done(self, overlap=(0, 1)):
        return dict(st=self.st, T=list(Cc.IDENT), overlap=tuple(overlap), found_pt=self.found_pt, found_seg=self.found_seg, names=self.names)


def centre(cell, size=CELL, cols=COLS, dx=0.5, dy=0.5):
    """a pixel inside a cell (and inside the 8-pixel border for the cells used here)"""
    return (cell % cols) * size + size // 2 + dx, (cell // cols) * size + size // 2 + dy


# ---- constructed streams ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cells_stream():
    """cell contents: one entry; first fails, second wins; four types out of order; more than 64 entries; every other cell empty"""
    b = Builder()
    b.pt(*centre(13), G, 1, name="single")
    x, y = centre(15)
    b.pt(x, y, G, 0, name="first_fails"); b.pt(x + 3, y + 2, G, 1, name="second_wins"); b.pt(x + 6, y + 4, G, 1, name="third_untried")
    x, y = centre(39)
    b.names["four_types"] = [b.pt(x - 10 + 3 * k, y - 8 + 2 * k, t, f) for k, (t, f) in enumerate(((C_, 1), (D, 1), (G, 0), (U, 1), (G, 0), (C_, 1)))]
    x, y = centre(50, dx=-14.0, dy=-14.0)
    b.names["crowd"] = [b.pt(x + 0.4 * k, y + 0.35 * k, (U, G, C_)[k % 3], int(k == 65), kf_list=k % 2) for k in range(70)]
    return b.done()


@functools.lru_cache(maxsize=None)
def stop_stream():
    """six cells with a winner each (12, 14, 16, 36, 60, 75) and one without (40): with max_fts = 3 the fourth winner ends the visit"""
    b = Builder()
    for cell in (12, 14, 16, 36, 60, 75):
        x, y = centre(cell)
        b.pt(x, y, U, 0); b.pt(x + 2, y + 2, U, 1)
    b.pt(*centre(40), G, 0)
    for cell in (20, 48, 90, 101):                                    # segments' grid: both ends in one cell, each a winner
        x, y = centre(cell, SEG_CELL, SEG_COLS)
        b.seg((x - 5, y), (x + 5, y + 3), G)
    return b.done()


@functools.lru_cache(maxsize=None)
def segments_stream():
    b = Builder()
    c = lambda cell, dx=0.5, dy=0.5: centre(cell, SEG_CELL, SEG_COLS, dx, dy)
    b.seg(c(16, -4), c(16, 5, 4), G, name="one_cell")                                     # both ends in one cell: twice in its list
    b.seg(c(16, -6, -6), c(16, 7, -5), G, name="one_cell_later")                          # never tried: the cell returns at the first success
    b.seg(c(18), c(20), G, name="wins_both")                                              # emitted twice
    # promotion: Q is filed before P; P's first success (cell 45) makes it GOOD, so in cell 47 it sorts ahead of Q and wins there too
    b.seg(c(47, -5, -5), c(47, 6, -3), U, name="Q")
    b.seg(c(45), c(47, 3, 5), U, nsucc=10, name="P")
    # deletion: the first failure (cell 73) deletes it; met again in cell 76: a trial, no increment
    b.seg(c(73), c(76), U, found=(1, 0), nfail=15, name="deleted_then_met")
    b.seg(c(76, 4, 4), c(104), G, found=(0, 0), name="after_deleted")
    b.seg(c(106), c(108), G, view=False, name="seg_no_view")
    b.seg(c(110, -3), c(110, 4), D, name="seg_pre_deleted")
    return b.done()


def _threshold_rows(b, add, kind):
    cells = iter(range(14, 120, 2))
    nxt = lambda: centre(next(cells), SEG_CELL, SEG_COLS) if kind == "seg" else centre(next(cells))
    one = lambda typ, found, **kw: (add(nxt(), typ, found, **kw) if kind == "pt" else
                                    (lambda p: b.seg((p[0] - 4, p[1]), (p[0] + 4, p[1] + 2), typ, (found, found), **kw))(nxt()))
    names = {}
    for nsucc in (9, 10):
        names["succ%d" % nsucc] = one(U, 1, nsucc=nsucc)
    for nfail in (14, 15):
        names["fail%d" % nfail] = one(U, 0, nfail=nfail)
    for nfail in (29, 30):
        names["cand%d" % nfail] = one(C_, 0, nfail=nfail, cand=True)
    names["cand_unlisted30"] = one(C_, 0, nfail=30)                   # TYPE_CANDIDATE outside the list: deleteCandidate* finds nothing
    names["good_fail40"] = one(G, 0, nfail=40)                        # a GOOD landmark is never deleted here
    return names


@functools.lru_cache(maxsize=None)
def thresholds_pt_stream():
    b = Builder()
    b.names.update(_threshold_rows(b, lambda p, typ, found, **kw: b.pt(p[0], p[1], typ, found, **kw), "pt"))
    return b.done()


@functools.lru_cache(maxsize=None)
def thresholds_seg_stream():
    b = Builder()
    b.names.update(_threshold_rows(b, None, "seg"))
    return b.done()


@functools.lru_cache(maxsize=None)
def thresholds_seg_two_cells_stream():
    """segments one below and at each failure threshold whose two ends lie in two cells, the second behind the stop of PARAMS["untried"]
    (max_fts_segs = 1: the winners in cells 30 and 32 end the visit): ONE increment each, so 14 -> 15 and 29 -> 30 stay alive"""
    b = Builder()
    c = lambda cell: centre(cell, SEG_CELL, SEG_COLS)
    for k, (typ, nfail, cand) in enumerate(((U, 14, False), (U, 15, False), (C_, 29, True), (C_, 30, True))):
        b.seg(c(14 + 2 * k), c(98 + 2 * k), typ, found=(0, 1), nfail=nfail, cand=cand, name="two%d" % nfail)
    for cell in (30, 32):
        x, y = c(cell)
        b.seg((x - 5, y), (x + 5, y + 3), G)
    return b.done()


@functools.lru_cache(maxsize=None)
def other_stream():
    """a pre-deleted landmark, has_view = 0, failing map candidates at 27, 28 and 31 failures, an edgelet observation"""
    b = Builder()
    b.pt(*centre(12), D, 1, name="pre_deleted")
    b.pt(*centre(14), G, 1, view=False, name="no_view")
    b.pt(*centre(16), G, 1, edgelet=True, name="edgelet")
    b.pt(*centre(18), G, 0, edgelet=True, name="edgelet_lost")
    for nfail in (27, 28, 31):
        b.pt(400.5 + nfail, 100.5, C_, 1, nfail=nfail, cand=True, name="cand_fail%d" % nfail)          # out of frame
        b.seg((100.5, 300.5 + nfail), (120.5, 300.5), C_, nfail=nfail, cand=True, name="seg_cand_fail%d" % nfail)
    b.pt(*centre(20), C_, 1, cand=True, name="cand_ok")
    b.seg(centre(30, SEG_CELL, SEG_COLS), centre(32, SEG_CELL, SEG_COLS), C_, cand=True, name="seg_cand_ok")
    return b.done()


def empty_stream():
    return Builder().done(overlap=())


def random_stream(rng, feats, n_pt, n_seg, n_pt_cand, n_seg_cand, p_found=0.6):
    """a random stream of candidates_cases brought under the selection's preconditions (a candidate is listed once and belongs to no
    keyframe; an edgelet observation lies where the matcher's border test accepts it), random counters near the thresholds"""
    st = Cc.rand_stream(rng, feats, n_pt, n_seg, 0, 0)
    for name, n, n_cand in (("pt", n_pt, n_pt_cand), ("seg", n_seg, n_seg_cand)):
        cand = [int(v) for v in rng.permutation(n)[:n_cand]] if n else []
        st[name + "_cand"] = cand
        for fts in st["kf_" + name]:
            for k, v in enumerate(fts):
                if v in cand:
                    fts[k] = -1
        for lm in cand:
            if st[name + "_type"][lm] != D:
                st[name + "_type"][lm] = C_
        st[name + "_nfail"] = [int(v) for v in rng.choice([0, 3, 14, 15, 16, 28, 29, 30, 31], n)]
        st[name + "_nsucc"] = [int(v) for v in rng.choice([0, 5, 9, 10, 11], n)]
    for obs in st["pt_obs"]:
        for o in obs:
            if not (30 <= o["px"][0] < CAM_T[4] - 30 and 30 <= o["px"][1] < CAM_T[5] - 30):
                o["type"] = 0
    return dict(st=st, T=Cc.rand_pose(rng, 0.1, 0.3), overlap=tuple(int(v) for v in rng.permutation(len(feats))[:max(len(feats) - 1, 0)]),
                found_pt={lm: int(rng.random() < p_found) for lm in range(n_pt)},
                found_seg={lm: (int(rng.random() < 0.8), int(rng.random() < 0.8)) for lm in range(n_seg)}, names={})


@functools.lru_cache(maxsize=None)
def batch():
    """ten unequal streams: more than two workgroups of four waves, the last one partial"""
    rng = np.random.default_rng(5201)
    return (cells_stream(), random_stream(rng, [(40, 20)] * 3, 90, 40, 5, 4), stop_stream(), segments_stream(), empty_stream(), thresholds_pt_stream(),
            random_stream(rng, [(150, 90), (130, 70)], 260, 150, 9, 7), thresholds_seg_stream(), other_stream(), thresholds_seg_two_cells_stream())


def _order(seed, n, last=None):
    o = [int(v) for v in np.random.default_rng(seed).permutation(n)]
    if last is not None:
        o.remove(last); o.append(last)
    return o


# the parameter sets every stream is run under
PARAMS = dict(
    default=dict(max_fts=120, max_fts_segs=100, cell_order=None, seg_cell_order=None),
    zero=dict(max_fts=0, max_fts_segs=0, cell_order=None, seg_cell_order=None),
    untried=dict(max_fts=3, max_fts_segs=1, cell_order=None, seg_cell_order=None),             # stop_stream: cells 60, 75 hold matches that are never tried
    last_cell=dict(max_fts=5, max_fts_segs=3, cell_order=tuple(_order(7, N_CELLS, last=36)),   # stop_stream: the sixth winner sits in the LAST cell visited
                   seg_cell_order=tuple(_order(8, SEG_N_CELLS, last=48))),
    shuffled=dict(max_fts=8, max_fts_segs=4, cell_order=tuple(_order(9, N_CELLS)), seg_cell_order=tuple(_order(10, SEG_N_CELLS))),
)


def restate_candidates(s, st=None):
    return N.candidates(s["st"] if st is None else st, s["T"], s["overlap"], CAM_T, CELL, SEG_CELL, BOUNDARY)


def match_of(s, r):
    """the synthetic matcher output for the candidates r of stream s, in the layout of plsvo_cand_match_out"""
    n_pt, n_seg = r["n_filed_pt"], r["n_filed_seg"]
    k = n_pt + 2 * n_seg
    found, px, level = np.zeros(k, np.uint8), np.zeros((k, 2)), np.zeros(k, np.int32)
    for i, lm in enumerate(r["pt_lm"]):
        found[i] = s["found_pt"][lm]; px[i] = [r["pt_px"][i][0] + 0.25, r["pt_px"][i][1] - 0.125]; level[i] = lm % 3
    for i, lm in enumerate(r["seg_lm"]):
        for e in range(2):
            m = n_pt + e * n_seg + i
            found[m] = s["found_seg"][lm][e]; px[m] = [r["seg_px"][i][2 * e] - 0.5, r["seg_px"][i][2 * e + 1] + 0.375]; level[m] = (lm + 2 * e) % 3
    return dict(found=found, px=px, search_level=level)


def synthetic_A(r):
    """a stand-in for Matcher::A_cur_ref_ per point entry (the host tests need no device)"""
    return {i: [1.0 + 0.01 * (lm % 7), 0.125 * (lm % 3), -0.0625 * (lm % 5), 0.9 + 0.02 * (lm % 4)] for i, lm in enumerate(r["pt_lm"])}


def restate(s, params, A=None, st=None, promote=True):
    """(candidates, match, selection) of one frame on a COPY of the stream (or on `st`, which is mutated); the copy is returned too"""
    st = copy.deepcopy(s["st"]) if st is None else st
    r = restate_candidates(s, st)
    m = match_of(s, r)
    sel = S.select(st, r, m, CAM_T, CELL, SEG_CELL, params["max_fts"], params["max_fts_segs"], params["cell_order"], params["seg_cell_order"],
                   A=synthetic_A(r) if A is None else A(r), promote=promote)
    return r, m, sel, st
