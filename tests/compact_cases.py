"""Cases of the compaction of the resident map tables (plsvo_candidates_compact), shared by tests/test_compact_host.py and
tests/test_gpu_compact.py.  Streams are built with the helpers of tests/insert_cases.py on the 326 x 246 camera of
tests/select_cases.py; a deleted landmark is a row of TYPE_DELETED that no keyframe feature and no candidate entry names (DESIGN.md 3.12,
3.13) -- except in the two streams that break that precondition on purpose (pin 7).  A case carries the stream, the call's record
(`mode`: mode, min_room_pt, min_room_seg) and the last_structure_optim_ keys it is staged with.  Built once (seeded), never changed."""
import functools

import numpy as np

import insert_cases as Ic
import np_compact as NK

CAM_T, CAM, CELL, SEG_CELL, BOUNDARY = Ic.CAM_T, Ic.CAM, Ic.CELL, Ic.SEG_CELL, Ic.BOUNDARY
D, C_, U, G = Ic.D, Ic.C_, Ic.U, Ic.G
LM_RESERVE = dict(extra_pt=40, extra_seg=24)
RESERVE = dict(Ic.RESERVE, extra_pt_obs=Ic.RESERVE["extra_pt_obs"] + 40, extra_seg_obs=Ic.RESERVE["extra_seg_obs"] + 24)
SIZES = (0, 1, 63, 64, 65, 130)


def dead_rows(pattern, n):
    """the deleted rows among n of a kind"""
    return {"none": set(), "all": set(range(n)), "first": {0} & set(range(n)), "last": {n - 1} & set(range(n)), "alternating": set(range(0, n, 2)),
            "run64": set(range(33, 97)) & set(range(n)),              # 64 deleted rows in a row, across the boundary of two rounds
            "behind129": set(range(min(129, n)))}[pattern]


def pattern_stream(seed, n_pt, n_seg, pat_pt, pat_seg, n_kf=3, n_ptc=0, n_segc=0):
    """n_pt + n_ptc point rows and n_seg + n_segc segment rows; the first n of a kind are keyframe features or deleted (pattern), the rest
    candidates.  Every second deleted row keeps a leftover observation list, the others' lists are emptied; candidates sit between and
    behind them in the candidate list's own (shuffled) order"""
    rng = np.random.default_rng(seed)
    b = Ic.Builder(n_kf)
    w, h = CAM_T[4], CAM_T[5]
    somewhere = lambda: (rng.uniform(20, w - 20), rng.uniform(20, h - 20))
    kfs_of = lambda: [int(v) for v in rng.permutation(n_kf)[:rng.integers(1, min(n_kf, 4) + 1)]] if n_kf else []
    counters = lambda: dict(nfail=int(rng.integers(0, 31)), nsucc=int(rng.integers(0, 12)))
    dp, ds = dead_rows(pat_pt, n_pt), dead_rows(pat_seg, n_seg)
    for i in range(n_pt):
        b.pt(*somewhere(), D if i in dp else int(rng.choice([U, G])), int(rng.random() < 0.6), kfs=kfs_of(), z=rng.uniform(2.0, 6.0), **counters())
    for i in range(n_seg):
        s = somewhere()
        b.seg(s, (s[0] + rng.uniform(-30, 30), s[1] + rng.uniform(-30, 30)), D if i in ds else int(rng.choice([U, G])), (1, int(rng.random() < 0.8)), kfs=kfs_of(), **counters())
    if n_kf:
        for _ in range(n_ptc):
            b.pt(*somewhere(), C_, int(rng.random() < 0.6), kfs=(int(rng.integers(0, n_kf)),), cand=True, **counters())
        for _ in range(n_segc):
            s = somewhere()
            b.seg(s, (s[0] + rng.uniform(-30, 30), s[1] + rng.uniform(-30, 30)), C_, (1, 1), kfs=(int(rng.integers(0, n_kf)),), cand=True, **counters())
    st = b.st
    for name, dead in (("pt", dp), ("seg", ds)):
        for k, lm in enumerate(sorted(dead)):
            if k % 2 == 0:
                st[name + "_obs"][lm].clear()                         # deleted by safeDelete*: the list was emptied
        rng.shuffle(st[name + "_cand"])
        for fts in st["kf_" + name]:
            fts += [-1] * int(rng.integers(0, 4))
            rng.shuffle(fts)
    return b.done(remove_kf=-1)


def long_list_stream():
    """a live point with 70 observations (more than a round of entries) behind deleted rows with leftover lists, and a segment that is a
    feature twice in one keyframe"""
    b = Ic.Builder(72)
    b.pt(40.0, 40.0, D, 0, kfs=(0, 1, 2))
    b.pt(60.0, 50.0, G, 1, kfs=(3,), name="short")
    b.pt(80.0, 60.0, D, 0, kfs=tuple(range(5, 45)))                   # 40 leftover entries leave
    b.pt(100.0, 70.0, G, 1, kfs=tuple(range(70)), name="long")
    b.pt(120.0, 80.0, D, 0, kfs=(7,))
    b.pt(140.0, 90.0, U, 1, kfs=(8, 9), name="behind")
    b.seg((50.0, 100.0), (70.0, 110.0), D, kfs=(1, 2))
    b.seg((90.0, 120.0), (120.0, 130.0), G, kfs=(1, 1), name="twice")
    b.seg((150.0, 140.0), (180.0, 150.0), D, kfs=())
    b.seg((200.0, 160.0), (230.0, 170.0), G, kfs=tuple(range(2, 72)), name="long_seg")
    return b.done(remove_kf=-1)


def broken_stream():
    """pin 7: keyframe features and candidate entries that name a deleted row (the tables' precondition does not hold)"""
    s = pattern_stream(8107, 20, 12, "none", "none", n_kf=3, n_ptc=6, n_segc=5)
    st = s["st"]
    for name in ("pt", "seg"):
        held = [lm for fts in st["kf_" + name] for lm in fts if lm >= 0]
        for lm in (held[0], held[len(held) // 2]):
            st[name + "_type"][lm] = D                                # still a feature (of every keyframe that observes it)
        for lm in (st[name + "_cand"][0], st[name + "_cand"][-1], st[name + "_cand"][2]):
            st[name + "_type"][lm] = D                                # still in the candidate list
    return s


def no_keyframes_stream():
    b = Ic.Builder(0)
    for k in range(5):
        b.pt(30.0 + 20 * k, 40.0, D if k in (1, 3) else G, 0, kfs=())
    for k in range(3):
        b.seg((40.0, 60.0 + 10 * k), (80.0, 70.0 + 10 * k), D if k == 0 else U, kfs=())
    return b.done(remove_kf=-1)


def case(s, mode=(NK.ALWAYS, 0, 0), seed=0):
    rng = np.random.default_rng(8200 + seed)
    st = s["st"]
    keys = dict(pt=[int(v) for v in rng.integers(1, 900, len(st["pt_pos"]))], seg=[int(v) for v in rng.integers(1, 900, len(st["seg_spos"]))])
    return dict(s, mode=mode, keys=keys)


@functools.lru_cache(maxsize=None)
def batch():
    """twenty-six unequal streams: seven workgroups of four waves, the last one partial"""
    P = pattern_stream
    room_pt, room_seg = LM_RESERVE["extra_pt"], LM_RESERVE["extra_seg"]
    streams = [
        (P(8101, 130, 65, "alternating", "first", n_ptc=70, n_segc=0), (NK.ALWAYS, 0, 0)),       # 70 candidates / none
        (P(8102, 64, 130, "all", "run64", n_ptc=0, n_segc=70), (NK.ALWAYS, 0, 0)),
        (P(8103, 130, 63, "behind129", "last", n_ptc=3, n_segc=2), (NK.ALWAYS, 0, 0)),           # a live row behind 129 deleted ones
        (P(8104, 65, 64, "last", "alternating", n_ptc=5, n_segc=5), (NK.STANDBY, 0, 0)),         # stands by
        (P(8105, 63, 1, "first", "all", n_ptc=2, n_segc=0), (NK.ALWAYS, 0, 0)),
        (P(8106, 1, 0, "all", "none"), (NK.ALWAYS, 0, 0)),                                       # one row, deleted; no segment at all
        (P(8107, 0, 64, "none", "first", n_segc=3), (NK.ALWAYS, 0, 0)),                          # segments only
        (P(8108, 64, 0, "alternating", "none", n_ptc=4), (NK.ALWAYS, 0, 0)),                     # points only
        (P(8109, 130, 130, "run64", "behind129", n_ptc=9, n_segc=7), (NK.ALWAYS, 0, 0)),
        (P(8110, 65, 65, "none", "none", n_ptc=6, n_segc=6), (NK.ALWAYS, 0, 0)),                 # nothing deleted: every byte stays
        (long_list_stream(), (NK.ALWAYS, 0, 0)),
        (broken_stream(), (NK.ALWAYS, 0, 0)),
        (no_keyframes_stream(), (NK.ALWAYS, 0, 0)),
        (P(8111, 0, 0, "none", "none"), (NK.ALWAYS, 0, 0)),                                      # an empty map
        (P(8112, 40, 20, "alternating", "alternating", n_ptc=4, n_segc=3), (NK.STANDBY, 7, 7)),
        # mode 2: the room is the landmark reserve; a threshold one above it compacts, the reserve itself does not -- per kind
        (P(8113, 40, 20, "alternating", "alternating", n_ptc=4, n_segc=3), (NK.ROOM, room_pt + 1, room_seg)),
        (P(8113, 40, 20, "alternating", "alternating", n_ptc=4, n_segc=3), (NK.ROOM, room_pt, room_seg + 1)),
        (P(8113, 40, 20, "alternating", "alternating", n_ptc=4, n_segc=3), (NK.ROOM, room_pt + 1, room_seg + 1)),
        (P(8113, 40, 20, "alternating", "alternating", n_ptc=4, n_segc=3), (NK.ROOM, room_pt, room_seg)),
        (P(8114, 1, 1, "none", "all"), (NK.ALWAYS, 0, 0)),
        (P(8115, 63, 63, "all", "alternating", n_kf=1), (NK.ALWAYS, 0, 0)),
        (P(8116, 64, 65, "first", "last", n_ptc=1, n_segc=1), (NK.ALWAYS, 0, 0)),
        (P(8117, 65, 130, "run64", "all", n_ptc=70, n_segc=70), (NK.ALWAYS, 0, 0)),
        (P(8118, 130, 64, "last", "run64"), (NK.ALWAYS, 0, 0)),
        (P(8119, 130, 1, "all", "none", n_ptc=2), (NK.ALWAYS, 0, 0)),
        (P(8120, 63, 65, "alternating", "behind129", n_ptc=3, n_segc=3), (NK.ALWAYS, 0, 0)),
    ]
    return tuple(case(s, mode, k) for k, (s, mode) in enumerate(streams))


def rows_of(st, lm_reserve=LM_RESERVE):
    """the landmark rows a stream staged as `st` is laid out with"""
    return len(st["pt_pos"]) + lm_reserve["extra_pt"], len(st["seg_spos"]) + lm_reserve["extra_seg"]


def compact(s, st, rows, events=None, keys=None):
    """the restatement's compaction of `st` (mutated) under the case's record"""
    mode, mp, ms = s["mode"]
    return NK.compact(st, mode, mp, ms, rows[0], rows[1], events=events, keys=keys)


def remapped(s, rep):
    """the case's per-landmark inputs (the matcher's verdicts, the culled sets) under the new row numbers"""
    out = dict(s)
    for name in ("pt", "seg"):
        r = rep[name + "_remap"]
        out["found_" + name] = {(r[lm] if lm < len(r) else lm): v for lm, v in s["found_" + name].items() if lm >= len(r) or r[lm] >= 0}
        out["culled_" + name] = frozenset(r[lm] for lm in s["culled_" + name] if lm < len(r) and r[lm] >= 0)
    return out
