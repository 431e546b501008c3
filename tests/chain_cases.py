"""Directed batches for the resident frame step (plsvo_chain_stage / _run / _fetch, plsvo_frame_step_batch), shared by the CPU conditions
of tests/test_chain_host.py and the device tests of tests/test_gpu_chain.py.

A case is a dict: W, H, cam, n_pyr_levels, images (one level-0 image per pyramid slot), streams (one dict per stream of the batch, the
arguments of abi.AlignJob and abi.ChainJob by name) and whatever the case is named for.  Sizes are the smallest that still reach the path:

  many_cell   one stream, 300 points + 40 segments; point cells of 20 px (192 cells = three 64-entry chunks of the selection's
              compaction) and of 10 px (768 cells: twelve chunks, three trips of the kernel's 256-stride loops), segment cells of 30 px
              (88 cells); shuffled visit orders; a mask that drops one candidate in ten.  The limits are taken from the case's own
              winners (stop_limits): the stop falls at the first winner, on the last winner of chunk 0, on the first of chunk 1, inside
              the last chunk, on the last winner overall, beyond the winners.
  border      candidates whose projection into the new frame lies up to 16 px on either side of the 8-pixel border, on all four sides;
              segments with only the start, only the end, both ends outside; segments in frame with one end masked; candidates behind
              the camera (the reference has no depth test: they are filed where they project).
  zoom        three slots, keyframe != previous frame: the keyframe stands back from the scene by 0.45 of its depth, so search levels 1
              and 2 occur; ref_level 0..3, a share of edgelets; ref_type / ref_grad are read for the points only, so the end points'
              entries are set to "edgelet, with a gradient" and must change nothing.
  mixed       six streams of different sizes in one batch with a segment grid: full, no points, no segments, no candidates, all
              masked, more than 256 points.
  lds_edge    640 x 480, point cells of 5 px (12288 cells) + segment cells of 11 px (2596 cells): 59536 B of the selection kernel's
              60000 B of dynamic LDS; the next finer grids must be refused."""
import importlib

import numpy as np

import np_chain

ALIGN = dict(max_level=3, min_level=1, n_iter=30, eps=1e-6)
IDENTITY = [0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]
N_PYR_SLOT_LEVELS = 4


def _seqm():
    return importlib.import_module("pl-svo_amd.sequence")


def _project(cam, T, pos):
    P = importlib.import_module("pl-svo_amd")
    pc = P.synth.se3_act(np.asarray(T, float), np.asarray(pos, float).reshape(-1, 3))
    with np.errstate(all="ignore"):
        return np.stack([cam[0] * pc[:, 0] / pc[:, 2] + cam[2], cam[1] * pc[:, 1] / pc[:, 2] + cam[3]], axis=1), pc[:, 2]


def _align_args(P, cam, T_prev_w, pt_px, pt_pos, seg_spx, seg_epx, seg_spos, seg_epos, ref_slot, cur_slot, **over):
    """the previous frame's features as processFrame hands them to the alignment: f * |pos - ref_pos| (frame_handler_mono.cpp:229-230)"""
    seqm = _seqm()
    ref_pos = P.synth.se3_inv(T_prev_w)[4:]
    scaled = lambda px, pos: seqm._bearing(cam, px) * np.linalg.norm(pos - ref_pos, axis=1)[:, None] if len(px) else np.zeros((0, 3))
    a = dict(ALIGN, cam=cam, T_cur_from_ref=IDENTITY, pt_px=pt_px, pt_xyz_ref=scaled(pt_px, pt_pos), seg_spx=seg_spx, seg_epx=seg_epx,
             seg_len=np.linalg.norm(np.asarray(seg_epx) - np.asarray(seg_spx), axis=1) if len(seg_spx) else np.zeros(0),
             seg_p_ref=scaled(seg_spx, seg_spos), seg_q_ref=scaled(seg_epx, seg_epos), ref_slot=ref_slot, cur_slot=cur_slot)
    a.update(over)
    return a


def seq_stream(P, seq, slot0, pts=None, segs=None, active=None):
    """One stream on a sequence.make_sequence scene: frame 0 (slot0) is keyframe and previous frame, frame 1 (slot0 + 1) the new one.
    pts / segs: which of the scene's landmarks are candidates (None: all)."""
    cam, T0 = seq["cam"], seq["poses_true"][0]
    pts = np.arange(len(seq["pt_pos"])) if pts is None else np.asarray(pts, np.int64)
    segs = np.arange(len(seq["seg_spos"])) if segs is None else np.asarray(segs, np.int64)
    align = _align_args(P, cam, T0, seq["pt_px0"], seq["pt_pos"], seq["seg_spx0"], seq["seg_epx0"], seq["seg_spos"], seq["seg_epos"], slot0, slot0 + 1)
    return dict(align=align, T_prev_w=T0, T_kf_w=T0, kf_slot=slot0, cur_slot=slot0 + 1, n_pt=len(pts), n_seg=len(segs),
                pos=np.concatenate([seq["pt_pos"][pts], seq["seg_spos"][segs], seq["seg_epos"][segs]]).reshape(-1, 3),
                ref_px=np.concatenate([seq["pt_px0"][pts], seq["seg_spx0"][segs], seq["seg_epx0"][segs]]).reshape(-1, 2),
                ref_f=np.concatenate([seq["pt_f0"][pts], seq["seg_sf0"][segs], seq["seg_ef0"][segs]]).reshape(-1, 3),
                ref_level=None, ref_type=None, ref_grad=None, active=active)


def _case(seq_or_cam, images, streams, n_pyr_levels=3, **extra):
    cam = seq_or_cam["cam"] if isinstance(seq_or_cam, dict) else seq_or_cam
    return dict(W=int(cam[4]), H=int(cam[5]), cam=cam, n_pyr_levels=n_pyr_levels, images=images, streams=streams, **extra)


def grid(case, cell_size, seg_cell_size=0, order_seed=None):
    """the two grids of a run: sizes, cell counts, and (order_seed given) shuffled visit orders"""
    W, H = case["W"], case["H"]
    g = dict(cell_size=cell_size, n_cols=-(-W // cell_size), seg_cell_size=seg_cell_size, seg_n_cols=0, seg_n_cells=0, cell_order=None, seg_cell_order=None)
    g["n_cells"] = g["n_cols"] * -(-H // cell_size)
    if seg_cell_size > 0:
        g["seg_n_cols"] = -(-W // seg_cell_size)
        g["seg_n_cells"] = g["seg_n_cols"] * -(-H // seg_cell_size)
    if order_seed is not None:
        rng = np.random.default_rng(order_seed)
        g["cell_order"] = rng.permutation(g["n_cells"]).astype(np.int32)
        if seg_cell_size > 0:
            g["seg_cell_order"] = rng.permutation(g["seg_n_cells"]).astype(np.int32)
    return g


def rule_kwargs(g, max_fts, max_fts_segs):
    """the grid as plsvo_chain_params (capi.Context.chain_stage keywords), cell_rule on"""
    return dict(cell_size=g["cell_size"], cell_rule=True, max_fts=int(max_fts), cell_order=g["cell_order"], seg_cell_size=g["seg_cell_size"],
                max_fts_segs=int(max_fts_segs), seg_cell_order=g["seg_cell_order"])


# ---- the cases -------------------------------------------------------------------------------------------------------------------------

_cache = {}


def _cached(name, make):
    if name not in _cache:
        _cache[name] = make()
    return _cache[name]


MANY_CELL_SEED = 8


def many_cell(P):
    def make():
        seq = _seqm().make_sequence(MANY_CELL_SEED, n_frames=2, W=320, H=240, n_pts=300, n_seg=40)
        active = (np.random.default_rng(801).uniform(size=300 + 80) >= 0.1).astype(np.uint8)
        return _case(seq, seq["images"], [seq_stream(P, seq, 0, active=active)])
    return _cached("many_cell", make)


def _lift_from_cur(P, seq, px):
    """world positions of the scene points that the TRUE pose of frame 1 sees at `px`"""
    syn, st = P.synth, seq["stream"]
    T_cur_ref = syn.se3_mul(seq["poses_true"][1], syn.se3_inv(seq["poses_true"][0]))
    T_ref_cur = syn.se3_inv(T_cur_ref)
    _, rays = syn._bearing(seq["cam"], np.asarray(px, float).reshape(-1, 2))
    o = T_ref_cur[4:]
    d = rays @ syn.quat_to_R(T_ref_cur[:4]).T
    t = (st.plane_d - o @ st.plane_n) / (d @ st.plane_n)
    X_ref = o + d * t[:, None]
    return syn.se3_act(syn.se3_inv(seq["poses_true"][0]), X_ref), X_ref


def _kf_obs(P, seq, X_ref):
    cam = seq["cam"]
    px = np.stack([cam[0] * X_ref[:, 0] / X_ref[:, 2] + cam[2], cam[1] * X_ref[:, 1] / X_ref[:, 2] + cam[3]], axis=1)
    return px, X_ref / np.linalg.norm(X_ref, axis=1, keepdims=True)


BORDER_SEED = 31
N_BORDER_PTS = 16


def border(P):
    """extra candidates of a sequence stream, placed in the new frame: `kinds` names their indices (points: into the point candidates,
    segments: into the segment candidates)"""
    def make():
        seq = _seqm().make_sequence(BORDER_SEED, n_frames=2, W=320, H=240, n_pts=80, n_seg=10)
        W, H = 320, 240
        rng = np.random.default_rng(BORDER_SEED + 5000)
        inside = lambda n: np.stack([rng.uniform(40, W - 40, n), rng.uniform(40, H - 40, n)], axis=1)

        def at_border(side, off):
            """a pixel `off` px inside (+) or outside (-) the 8-pixel border on `side` (0 left, 1 right, 2 top, 3 bottom)"""
            along = rng.uniform(30, (H if side < 2 else W) - 30)
            return [(8 + off, along), (W - 8 - off, along), (along, 8 + off), (along, H - 8 - off)][side]
        # points: four per side, 0 .. 16 px on either side of the border
        bpx = np.array([at_border(k % 4, rng.uniform(-16, 16)) for k in range(N_BORDER_PTS)])
        # segments: (start, end) pixel pairs
        out = lambda side: at_border(side, -rng.uniform(3, 16))
        spx = [out(k) for k in range(4)] + list(inside(4)) + [out(0), out(3)] + list(inside(4))
        epx = list(inside(4)) + [out(k) for k in range(4)] + [out(1), out(2)] + [p + rng.uniform(12, 30, 2) for p in spx[10:]]
        spx, epx = np.array(spx), np.array(epx)
        # behind the camera: the mirror image of a visible scene point projects to the same pixel
        hpx = inside(4)
        cam_pos = P.synth.se3_inv(seq["poses_true"][1])[4:]
        mirror = lambda pos: 2.0 * cam_pos - pos
        (bpos, bX), (spos, sX), (epos, eX), (hpos, hX) = (_lift_from_cur(P, seq, v) for v in (bpx, spx, epx, hpx))
        n_pt0, n_seg0 = 80, 10
        st = seq_stream(P, seq, 0)
        hpos_m = mirror(hpos)
        # three mirrored points, and one segment with a mirrored end
        pos_s, pos_e = np.concatenate([spos, hpos[3:4]]), np.concatenate([epos, hpos_m[3:4]])
        X_s, X_e = np.concatenate([sX, hX[3:4]]), np.concatenate([eX, hX[3:4]])
        kf = lambda X: _kf_obs(P, seq, X)
        base = dict(pos=st["pos"], ref_px=st["ref_px"], ref_f=st["ref_f"])
        ext = dict(pos=(np.concatenate([bpos, hpos_m[:3]]), pos_s, pos_e), ref_px=(np.concatenate([kf(bX)[0], kf(hX[:3])[0]]), kf(X_s)[0], kf(X_e)[0]),
                   ref_f=(np.concatenate([kf(bX)[1], kf(hX[:3])[1]]), kf(X_s)[1], kf(X_e)[1]))
        for k in ("pos", "ref_px", "ref_f"):
            p_, s_, e_ = ext[k]
            a = base[k]
            st[k] = np.concatenate([a[:n_pt0], p_, a[n_pt0:n_pt0 + n_seg0], s_, a[n_pt0 + n_seg0:], e_])
        n_pt, n_seg = n_pt0 + N_BORDER_PTS + 3, n_seg0 + 15
        st["n_pt"], st["n_seg"] = n_pt, n_seg
        s0 = n_seg0
        kinds = dict(border_pts=np.arange(n_pt0, n_pt0 + N_BORDER_PTS), behind_pts=np.arange(n_pt0 + N_BORDER_PTS, n_pt), seg_start_out=np.arange(s0, s0 + 4),
                     seg_end_out=np.arange(s0 + 4, s0 + 8), seg_both_out=np.arange(s0 + 8, s0 + 10), seg_start_masked=np.arange(s0 + 10, s0 + 12),
                     seg_end_masked=np.arange(s0 + 12, s0 + 14), behind_seg=np.arange(s0 + 14, s0 + 15))
        active = np.ones(n_pt + 2 * n_seg, np.uint8)
        active[n_pt + kinds["seg_start_masked"]] = 0
        active[n_pt + n_seg + kinds["seg_end_masked"]] = 0
        st["active"] = active
        return _case(seq, seq["images"], [st], kinds=kinds)
    return _cached("border", make)


ZOOM_SEED, ZOOM, ZOOM_W, ZOOM_H, ZOOM_PTS, ZOOM_SEG = 28, 0.45, 326, 246, 96, 24


def zoom(P, seed=ZOOM_SEED):
    """slot 0 the keyframe, slot 1 the previous frame, slot 2 the new frame.  The candidates are synth.make_match_batch's (the warp
    cases' scene: ref_level 0..3, one point in four an edgelet); a segment's two end points carry one level, as one LineFeat does."""
    def make():
        syn = P.synth
        st, d = syn.make_match_batch(seed, ZOOM_W, ZOOM_H, ZOOM_PTS, ZOOM_SEG)
        rng = np.random.default_rng(seed + 720000)
        d0 = st.plane_d / st.plane_n[2]
        T_cur_ref = syn.se3_exp(np.concatenate([rng.uniform(-0.02, 0.02, 2) * d0, [-ZOOM * d0], rng.uniform(-0.01, 0.01, 3)]))
        T_cur_prev = syn.se3_exp(np.concatenate([rng.uniform(-0.012, 0.012, 3) * d0, rng.uniform(-0.008, 0.008, 3)]))
        T_prev_ref = syn.se3_mul(syn.se3_inv(T_cur_prev), T_cur_ref)
        T_kf_w = st.T_ref_w
        T_prev_w, T_cur_w = syn.se3_mul(T_prev_ref, T_kf_w), syn.se3_mul(T_cur_ref, T_kf_w)
        images = [syn.render_views([st], [T], noise_tag=k).numpy()[0] for k, T in enumerate((None, T_prev_ref, T_cur_ref))]
        n_pt, n_seg = ZOOM_PTS, ZOOM_SEG
        ref_level = d["ref_level"].copy()
        ref_level[n_pt + n_seg:] = ref_level[n_pt:n_pt + n_seg]
        # the previous frame's features: the landmarks it sees, away from the border by the coarsest level's patch
        cam = st.cam
        px_prev, z_prev = _project(cam, T_prev_w, d["pos"])
        m = 4.0 * (1 << 2)
        ok = (z_prev > 0) & (px_prev[:, 0] >= m) & (px_prev[:, 0] < ZOOM_W - m) & (px_prev[:, 1] >= m) & (px_prev[:, 1] < ZOOM_H - m)
        pi = np.nonzero(ok[:n_pt])[0]
        si = np.nonzero(ok[n_pt:n_pt + n_seg] & ok[n_pt + n_seg:])[0]
        align = _align_args(P, cam, T_prev_w, px_prev[pi], d["pos"][pi], px_prev[n_pt + si], px_prev[n_pt + n_seg + si], d["pos"][n_pt + si],
                            d["pos"][n_pt + n_seg + si], 1, 2, max_level=2)
        # ref_type / ref_grad are read for the points only: the end points' entries say "edgelet" with a gradient, and must not be looked at
        ref_type = d["ref_type"].copy()
        ref_type[n_pt:] = 1
        stream = dict(align=align, T_prev_w=T_prev_w, T_kf_w=T_kf_w, kf_slot=0, cur_slot=2, n_pt=n_pt, n_seg=n_seg, pos=d["pos"], ref_px=d["ref_px"],
                      ref_f=d["ref_f"], ref_level=ref_level, ref_type=ref_type, ref_grad=d["ref_grad"].copy(), active=None)
        return _case(cam, images, [stream], T_cur_w_true=T_cur_w)
    return _cached(("zoom", seed), make)


MIXED_SEEDS = (41, 42)


def mixed(P):
    def make():
        seqm = _seqm()
        a = seqm.make_sequence(MIXED_SEEDS[0], n_frames=2, W=320, H=240, n_pts=60, n_seg=12)
        b = seqm.make_sequence(MIXED_SEEDS[1], n_frames=2, W=320, H=240, n_pts=300, n_seg=8)
        none = np.zeros(0, np.int64)
        rng = np.random.default_rng(4100)
        streams = [seq_stream(P, a, 0, active=(rng.uniform(size=60 + 24) >= 0.15).astype(np.uint8)),      # full, a mask of its own
                   seq_stream(P, a, 0, pts=none),                                                         # no points
                   seq_stream(P, a, 0, segs=none),                                                        # no segments
                   seq_stream(P, a, 0, pts=none, segs=none),                                              # no candidates at all
                   seq_stream(P, a, 0, pts=np.arange(0, 60, 2), segs=np.arange(5), active=np.zeros(30 + 10, np.uint8)),   # all masked out
                   seq_stream(P, b, 2)]                                                                   # more than 256 points
        names = ("full", "no_points", "no_segments", "no_candidates", "all_masked", "many_points")
        return _case(a, a["images"] + b["images"], streams, names=names)
    return _cached("mixed", make)


LDS_SEED = 52
LDS_GRID, LDS_REFUSED = (5, 11), ((4, 0), (5, 10), (4, 11))      # (cell_size, seg_cell_size): 59536 B; 76800, 61440, 87184 B


def lds_edge(P):
    def make():
        seq = _seqm().make_sequence(LDS_SEED, n_frames=2, W=640, H=480, n_pts=120, n_seg=20)
        return _case(seq, seq["images"], [seq_stream(P, seq, 0)])
    return _cached("lds_edge", make)


# ---- running a case ----------------------------------------------------------------------------------------------------------------------

def chain_jobs(P, case):
    abi = P.abi
    jobs = []
    for s in case["streams"]:
        a = s["align"]
        aj = abi.AlignJob(a["cam"], a["max_level"], a["min_level"], a["n_iter"], a["eps"], a["T_cur_from_ref"], a["pt_px"], a["pt_xyz_ref"], a["seg_spx"], a["seg_epx"],
                          a["seg_len"], a["seg_p_ref"], a["seg_q_ref"], ref_slot=a["ref_slot"], cur_slot=a["cur_slot"])
        jobs.append(abi.ChainJob(aj, s["T_prev_w"], s["T_kf_w"], s["kf_slot"], s["n_pt"], s["n_seg"], s["pos"], s["ref_px"], s["ref_f"], ref_level=s["ref_level"],
                                 ref_type=s["ref_type"], ref_grad=s["ref_grad"], active=s["active"]))
    return jobs


def load_frames(ctx, case):
    ctx.config_pyramids(len(case["images"]), case["W"], case["H"], N_PYR_SLOT_LEVELS)
    for k, img in enumerate(case["images"]):
        ctx.build_pyramid(k, img, 0)


class OracleCalls:
    """the three per-call entry points a case is replayed with, on the CPU oracle (reproject / match_direct as the device context has them)"""

    def __init__(self, ob, case):
        self.ob = ob
        self.pyr = [ob.build_pyramid(im, N_PYR_SLOT_LEVELS) for im in case["images"]]

    def sparse_align(self, job):
        return self.ob.sparse_align(job, self.pyr[job.c.ref_slot], self.pyr[job.c.cur_slot])[0]

    def reproject(self, job):
        return self.ob.reproject(job)

    def match_direct(self, job):
        return self.ob.match_direct(job, [self.pyr[s] for s in job.frame_slot])


def full_types(stream):
    """ref_type / ref_grad as the frame step must understand them: the caller's entries for the points, and whatever the arrays hold
    beyond them, end points are corners without a gradient"""
    n_pt, nc = stream["n_pt"], stream["n_pt"] + 2 * stream["n_seg"]
    ty, gr = np.zeros(nc, np.uint8), np.zeros((nc, 2))
    if stream["ref_type"] is not None:
        ty[:n_pt] = stream["ref_type"][:n_pt]
    if stream["ref_grad"] is not None:
        gr[:n_pt] = stream["ref_grad"][:n_pt]
    return ty, gr


def per_call(P, calls, case, s, T_k, cell_size, align_max_iter=10):
    """Reprojection and direct matching of stream s's candidates one entry point at a time, with frame table [T_kf_w, T_k]: the
    projections, the cells, the NumPy active rule on them, and the match of EVERY candidate (the rule is applied by the caller)."""
    abi, st, cam = P.abi, case["streams"][s], case["cam"]
    nc = st["n_pt"] + 2 * st["n_seg"]
    out = dict(px=np.zeros((0, 2)), cell=np.zeros(0, np.int32), found=np.zeros(0, bool), px_cur=np.zeros((0, 2)), search_level=np.zeros(0, np.int32))
    if nc:
        frame_T = np.stack([np.asarray(st["T_kf_w"], float), np.asarray(T_k, float)])
        rp = calls.reproject(abi.ReprojectJob(cam, frame_T, np.ones(nc, np.int32), st["pos"], cell_size=cell_size))
        ty, gr = full_types(st)
        level = np.zeros(nc, np.int32) if st["ref_level"] is None else st["ref_level"]
        mj = abi.MatchJob(cam, frame_T, np.array([st["kf_slot"], st["cur_slot"]], np.int32), np.ones(nc, np.int32), np.zeros(nc, np.int32), st["ref_px"], st["ref_f"],
                          level, ty, gr, st["pos"], rp["px"], case["n_pyr_levels"], align_max_iter)
        mr = calls.match_direct(mj)
        out = dict(px=rp["px"], cell=rp["cell"], found=mr["found"].astype(bool), px_cur=mr["px_cur"], search_level=mr["search_level"])
    out["active"] = np_chain.active_rule(st["active"], out["cell"], st["n_pt"], st["n_seg"])
    return out


def oracle_step(P, ob, case, s, cell_size):
    """stream s on the oracle alone: alignment -> composed pose -> per_call"""
    calls = OracleCalls(ob, case)
    job = chain_jobs(P, case)[s]
    ar = calls.sparse_align(job.align_job)
    T_k = P.synth.se3_mul(ar.T, np.asarray(case["streams"][s]["T_prev_w"], float))
    pc = per_call(P, calls, case, s, T_k, cell_size)
    pc["T_k"] = T_k
    return pc


def winning_positions(pc, stream, g, segments=False):
    """visit positions (ascending) of the cells that have a winner, points' grid or segments'"""
    n_pt, n_seg = stream["n_pt"], stream["n_seg"]
    ok = pc["found"] & pc["active"]
    if not segments:
        has = np.zeros(g["n_cells"], bool)
        has[pc["cell"][:n_pt][ok[:n_pt]]] = True
        order = g["cell_order"]
    else:
        both = ok[n_pt:n_pt + n_seg] & ok[n_pt + n_seg:]
        sk, ek = np_chain.segment_cells(pc["px"], n_pt, n_seg, g["seg_cell_size"], g["seg_n_cols"])
        has = np.zeros(g["seg_n_cells"], bool)
        has[sk[both]] = True
        has[ek[both]] = True
        order = g["seg_cell_order"]
    return np.nonzero(has[np.arange(len(has)) if order is None else order])[0]


STOP_KINDS = ("first_winner", "chunk0_last", "chunk1_first", "last_chunk_inside", "last_winner", "beyond")


def stop_limits(positions, n_cells):
    """max_fts values (kind -> limit) that put the stop -- the winner whose match makes the count exceed the limit, winner number
    `limit` counting from 0 -- at each place of the 64-entry chunks the compaction walks; and the chunk that winner is in (None: no stop)"""
    chunk = np.asarray(positions) // 64
    last = (n_cells - 1) // 64
    n, n0, n_last = len(positions), int((chunk == 0).sum()), int((chunk == last).sum())
    lim = dict(first_winner=0, chunk0_last=n0 - 1, chunk1_first=n0, last_chunk_inside=n - n_last + (n_last - 1) // 2, last_winner=n - 1, beyond=n + 7)
    where = {k: (int(chunk[v]) if 0 <= v < n else None) for k, v in lim.items()}
    return lim, where
