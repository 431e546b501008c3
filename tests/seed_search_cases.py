"""Directed inputs for the depth filter's epipolar search (pl-svo_amd/csrc/seeds_kernels.hip: update_seeds_kernel), shared by the CPU
tests of tests/test_seed_search.py and the GPU tests of tests/test_gpu_seed_search.py.

synth.make_seeds on sequence.make_sequence only makes level-0 seeds on 320 / 640 wide images with three pyramid levels.  The cases here
stand on the scene of tests/match_warp_cases.py -- 326 x 246 (level widths 326, 163, 81, 40: the byte phase of a scored patch changes
from row to row), four stored levels, two slots, reference levels 0..3, an edgelet share -- with the current camera set by an explicit
twist: a lateral motion (large enough that the seeds WALK their epipolar segment also without a zoom), the warp cases' (zoom, roll) list
with n_pyr_levels 3 and 4, a pure rotation (parallel rays: the triangulation fails), a translation of 3e-4 of the scene depth (the
same after a walk) and a pure sideways motion whose current frame is edited so that scores tie.  Seeds start from the uninformed prior
of DepthFilter::initializeSeeds; directed seeds are planted at fixed rows (PT_ROWS, SEG_ROWS) where the case's geometry allows."""
import math

import numpy as np

import match_warp_cases as mc

W, H = mc.W, mc.H
N_PTS, N_SEG = 96, 16            # 112 lanes: two workgroups; the point / line boundary in the middle of the second wave
SEED0 = 4300

# (lateral x, lateral y [fractions of the scene depth d0], zoom, roll [rad], n_pyr_levels, kind)
CASES = [(0.25, 0.10, 0.0, 0.0, 3, "walk"), (0.02, -0.02, 0.45, 0.0, 3, "walk"), (0.20, 0.05, -0.12, 0.0, 3, "walk"), (-0.15, 0.20, -0.7, 0.0, 3, "walk"),
         (0.10, -0.25, -0.85, 0.0, 3, "walk"), (-0.30, 0.10, -0.4, 0.3, 3, "walk"), (0.20, 0.20, -1.0, 0.8, 3, "walk"),
         (0.10, 0.25, 0.0, math.pi / 2, 3, "walk"), (0.02, 0.02, 0.45, 0.8, 3, "walk"), (-0.20, -0.15, -0.4, 3.0, 3, "walk"),
         (0.05, 0.03, 0.88, 0.3, 4, "walk"), (-0.25, 0.05, 0.0, 0.0, 4, "walk"), (0.02, 0.02, 0.45, 0.8, 4, "walk"),
         (0.0, 0.0, 0.0, 0.0, 3, "rotation"),      # the reference pose turned by (0.03, -0.04, 0.05) rad, no translation
         (0.0003, 0.0001, 0.0, 0.02, 3, "tiny"),   # a baseline of 3e-4 d0: a parallax below the triangulation's 1e-3 rad
         (0.25, 0.0, 0.0, 0.0, 3, "tie"),          # sideways only: horizontal epipolar lines; the current frame is edited (below)
         # beyond the warp cases' list, for the (reference level, search level) pairs it cannot reach: det(A) ~ 4^level / (1 - zoom)^2 and
         # one search level per factor 4 above 3, so level 0 -> 2 needs a zoom in 0.71 .. 0.85 (with three levels), level 2 -> 0 and
         # 3 -> 1 a zoom below -1.31, level 3 -> 0 one below -3.6
         (0.03, 0.02, 0.75, 0.2, 3, "walk"), (0.30, -0.20, -1.5, 0.4, 3, "walk"), (0.50, 0.40, -3.8, 0.0, 3, "walk")]
N_CASES = len(CASES)
TIE_CASE, ROTATION_CASE, TINY_CASE = 15, 13, 14
UNIFORM_LEVELS = (10, 11, 12, 16, 17, 18)    # reference levels 0..3 in equal shares (the others: 50 / 30 / 15 / 5 %, like the warp cases)
# the runs with other settings (GPU test 2 and the CPU tests): (case, option overrides)
VARIANTS = [(0, dict(max_epi_search_steps=5)), (10, dict(max_epi_search_steps=5)), (0, dict(edgelet_filtering=False)), (5, dict(edgelet_filtering=False)),
            (1, dict(align_max_iter=3))]

# fixed rows of every case
PT_ROWS = dict(behind=0, outside=1, tight=2, nan=3, far=4, cross=(5, 6, 7, 8), all_out=(9, 10, 11, 12), wide=tuple(range(13, 37)))
SEG_ROWS = dict(nan_s=0, nan_e=1, tight=(2, 4, 5), one_tight=3, wide=(6, 7, 10, 11, 12, 13, 14, 15), all_out=(8, 9))
CENTRAL_PT0, CENTRAL_SEG0 = 17, 10           # a strong zoom-in: the odd point rows from here and the line rows from here are re-drawn (make_case)


def _twist(P, k, d0):
    lx, ly, zoom, roll, _, kind = CASES[k]
    if kind == "rotation":
        return P.synth.se3_exp(np.array([0.0, 0.0, 0.0, 0.03, -0.04, 0.05]))
    return P.synth.se3_exp(np.array([lx * d0, ly * d0, -zoom * d0, 0.0, 0.0, roll]))   # cur_from_ref (a negative zoom moves away)


def _from_cur_px(P, st, q):
    """the scene point seen at pixel q of the CURRENT frame -> (reference pixel, bearing, depth along the bearing)"""
    syn = P.synth
    fx, fy, cx, cy = st.cam[:4]
    T_ref_cur = syn.se3_inv(st.T_true)
    r = np.array([(q[0] - cx) / fx, (q[1] - cy) / fy, 1.0])
    o, dr = T_ref_cur[4:], syn.se3_act(T_ref_cur, r) - T_ref_cur[4:]          # the ray in the reference camera frame
    s = (st.plane_d - st.plane_n @ o) / (st.plane_n @ dr)
    X = o + s * dr
    depth = np.linalg.norm(X)
    return np.array([fx * X[0] / X[2] + cx, fy * X[1] / X[2] + cy]), X / depth, depth


def _segment_px(P, st, f, mu, sigma2):
    """the two ends of a seed's epipolar segment in current level-0 pixels (double is enough: only used to place edits)"""
    fx, fy, cx, cy = st.cam[:4]
    sg = math.sqrt(sigma2)
    out = []
    for zi in (mu + sg, max(mu - sg, 1e-8)):
        p = P.synth.se3_act(st.T_true, f / zi)
        out.append([fx * p[0] / p[2] + cx, fy * p[1] / p[2] + cy])
    return np.array(out)


def make_case(P, k):
    """case k -> dict(st, pt, seg, truth, n_pyr_levels, frame_T, edits): the field dicts of abi.SeedsJob; render with synth.render_streams"""
    syn = P.synth
    lx, ly, zoom, roll, n_pyr, kind = CASES[k]
    st, d = syn.make_match_batch(SEED0 + k, W, H, N_PTS, N_SEG, **(dict(level_p=(0.25, 0.25, 0.25, 0.25)) if k in UNIFORM_LEVELS else {}))
    rng = np.random.default_rng(SEED0 + k + 90000)
    d0 = st.plane_d / st.plane_n[2]
    st.T_true = _twist(P, k, d0)
    T_cur_w = syn.se3_mul(st.T_true, st.T_ref_w)
    fx, fy, cx, cy = st.cam[:4]
    ref_pos = syn.se3_inv(st.T_ref_w)[4:]
    depth = np.linalg.norm(st.pt_pos_w - ref_pos, axis=1)
    sdepth, edepth = np.linalg.norm(st.seg_spos_w - ref_pos, axis=1), np.linalg.norm(st.seg_epos_w - ref_pos, axis=1)
    all_d = np.concatenate([depth, sdepth, edepth])
    dmean, dmin = float(all_d.mean()), 0.8 * float(all_d.min())
    mu0, zr0 = 1.0 / dmean, 1.0 / dmin
    n, ns = N_PTS, N_SEG
    pt = dict(ref_frame=np.zeros(n, np.int32), cur_frame=np.ones(n, np.int32), px=st.pt_px.copy(), f=st.pt_f.copy(), level=d["ref_level"][:n].copy(),
              type=d["ref_type"][:n].copy(), grad=d["ref_grad"][:n].copy(), a=np.full(n, 10.0), b=np.full(n, 10.0), mu=np.full(n, mu0),
              z_range=np.full(n, zr0), sigma2=np.full(n, zr0 ** 2 / 36.0))
    mid = 0.5 * (st.seg_spx + st.seg_epx)                                      # LineFeat's Feature::px is the segment centre
    fm, _ = syn._bearing(st.cam, mid)
    seg = dict(ref_frame=np.zeros(ns, np.int32), cur_frame=np.ones(ns, np.int32), px=mid, f=fm, sf=st.seg_sf.copy(), ef=st.seg_ef.copy(),
               level=d["ref_level"][n:n + ns].copy(), a=np.full(ns, 10.0), b=np.full(ns, 10.0), mu_s=np.full(ns, mu0), mu_e=np.full(ns, mu0),
               z_range_s=np.full(ns, zr0), z_range_e=np.full(ns, zr0), sigma2_s=np.full(ns, zr0 ** 2 / 36.0), sigma2_e=np.full(ns, zr0 ** 2 / 36.0))
    cdepth = np.linalg.norm(syn._on_plane(st.plane_n, st.plane_d, syn._bearing(st.cam, mid)[1]), axis=1)
    if zoom >= 0.7:
        # the current camera sees the middle 1 - zoom of the keyframe: the odd point rows and the last line rows are re-drawn from what
        # it sees, the lines 10 px long.  Their prior stays the uninformed one -- whose near bound lies BEHIND a camera that has come
        # this close: segments of thousands of steps -- except for every other re-drawn point: true depth +1 %, sigma = 3 % of mu.
        for row in range(CENTRAL_PT0, n, 2):
            q = np.array([rng.uniform(0.2, 0.8) * W, rng.uniform(0.2, 0.8) * H])
            pt["px"][row], pt["f"][row], depth[row] = _from_cur_px(P, st, q)
            if row % 4 == 1:
                pt["mu"][row] = 1.01 / depth[row]
                pt["sigma2"][row] = (0.03 * pt["mu"][row]) ** 2
        for row in range(CENTRAL_SEG0, ns):
            q, a = np.array([rng.uniform(0.25, 0.75) * W, rng.uniform(0.25, 0.75) * H]), rng.uniform(0.0, math.pi)
            h = 5.0 * np.array([math.cos(a), math.sin(a)])
            (ps, seg["sf"][row], sdepth[row]), (pe, seg["ef"][row], edepth[row]) = _from_cur_px(P, st, q - h), _from_cur_px(P, st, q + h)
            seg["px"][row] = 0.5 * (ps + pe)
            seg["f"][row] = syn._bearing(st.cam, seg["px"][row][None])[0][0]
            cdepth[row] = np.linalg.norm(syn._on_plane(st.plane_n, st.plane_d, syn._bearing(st.cam, seg["px"][row][None])[1]), axis=1)[0]

    # ---- planted point seeds
    R = PT_ROWS
    pt["f"][R["behind"]] = [0.0, 0.0, -1.0]                                    # behind the current camera
    off = np.array([6.0, 0.5, 1.0])
    pt["f"][R["outside"]] = off / np.linalg.norm(off)                           # in front of it, far outside the image
    pt["sigma2"][R["tight"]], pt["mu"][R["tight"]] = 1e-8, 1.0 / depth[R["tight"]]
    pt["type"][R["tight"]], pt["level"][R["tight"]] = 0, min(int(pt["level"][R["tight"]]), 1)
    pt["sigma2"][R["nan"]] = np.nan
    pt["mu"][R["far"]], pt["sigma2"][R["far"]] = 1e-3, 1e-10                    # a kilometre away: a segment below 2 px
    pt["type"][[R["nan"], R["far"]]] = 0                                        # (corners: the edgelet filter would come first)
    if kind in ("walk", "tie") and zoom == 0.0:
        # the epipolar lines of a sideways motion all run along its image direction.  A seed whose hypothesis is the scene point seen m
        # pixels inside the border that this direction crosses walks over the patch margin (8 px at its search level = its reference
        # level here); one whose hypothesis lies 2 px inside a border PARALLEL to the direction never leaves the margin.
        t = st.T_true[4:]
        horizontal = abs(t[0]) >= abs(t[1])
        for j, (row_c, row_o) in enumerate(zip(R["cross"], R["all_out"])):
            lv = j // 2
            m_in, m_out = (8 << lv) + 2.0, 2.0 * (1 << lv)
            far_side = j % 2
            along = rng.uniform(0.35, 0.65)
            if horizontal:
                qc = [W - 1 - m_in if far_side else m_in, along * H]
                qo = [along * W, H - 1 - m_out if far_side else m_out]
            else:
                qc = [along * W, H - 1 - m_in if far_side else m_in]
                qo = [W - 1 - m_out if far_side else m_out, along * H]
            for row, q in ((row_c, qc), (row_o, qo)):
                px, f, dep = _from_cur_px(P, st, q)
                pt["px"][row], pt["f"][row], pt["mu"][row], pt["level"][row], pt["type"][row] = px, f, 1.0 / dep, lv, 0
                depth[row] = dep
                if j < 2 and row == row_o:
                    # a line seed beside it: 8 px long, along the border, both ends at the true depth of their own bearings
                    srow = SEG_ROWS["all_out"][j]
                    e = np.array([4.0, 0.0]) if horizontal else np.array([0.0, 4.0])
                    (ps, seg["sf"][srow], sdepth[srow]), (pe, seg["ef"][srow], edepth[srow]) = _from_cur_px(P, st, q - e), _from_cur_px(P, st, q + e)
                    seg["px"][srow], seg["f"][srow], cdepth[srow], seg["level"][srow] = px, f, dep, lv
                    seg["mu_s"][srow], seg["mu_e"][srow] = 1.0 / sdepth[srow], 1.0 / edepth[srow]
    if kind in ("rotation", "tiny"):
        # an inverse-depth interval of +-20: with a baseline of 3e-4 d0 the segment is a few pixels long, the seed walks, finds its match
        # and fails the triangulation (the rays stay parallel to 1e-3 rad); without any baseline the segment is a point
        for row in R["wide"]:
            pt["sigma2"][row], pt["mu"][row], pt["type"][row], pt["level"][row] = 400.0, 1.0 / depth[row], 0, 0

    # ---- planted line seeds
    S = SEG_ROWS
    seg["sigma2_s"][S["nan_s"]] = np.nan
    seg["sigma2_e"][S["nan_e"]] = np.nan
    for row in S["tight"]:
        seg["sigma2_s"][row] = seg["sigma2_e"][row] = 1e-8
        seg["mu_s"][row], seg["mu_e"][row] = 1.0 / sdepth[row], 1.0 / edepth[row]
    seg["sigma2_s"][S["one_tight"]], seg["mu_s"][S["one_tight"]] = 1e-8, 1.0 / sdepth[S["one_tight"]]
    seg["mu_e"][S["one_tight"]] = 1.0 / edepth[S["one_tight"]]
    if kind in ("rotation", "tiny"):
        for row in S["wide"]:
            seg["sigma2_s"][row] = seg["sigma2_e"][row] = 400.0
            seg["mu_s"][row] = seg["mu_e"][row] = 1.0 / cdepth[row]
            seg["level"][row] = 0
    return dict(st=st, pt=pt, seg=seg, n_pyr_levels=n_pyr, frame_T=np.stack([st.T_ref_w, T_cur_w]), kind=kind,
                truth=dict(pt_depth=depth, seg_sdepth=sdepth, seg_edepth=edepth, seg_cdepth=cdepth))


N_FLAT, N_REPEAT = 3, 6          # seeds of the tie case whose scores are made to tie: by a flat rectangle / by a repeated texture


def edit_tie_frame(P, c, cur):
    """The tie case's current frame.  Its epipolar lines are image rows, its seeds' search levels their reference levels.  For level-0
    corner seeds that are not planted and whose segments do not meet:
      * `flat` (N_FLAT seeds): the rectangle around the whole segment + 12 px is overwritten with one grey value: every scored position
        has the same ZMSSD (sumAA - sumA^2/64 of the reference patch, below the threshold for these low-contrast patches);
      * `repeat` (N_REPEAT seeds): the 10 x 16 block around the true match is copied 10 px further along the segment: the best score
        occurs at two textured positions, and a walk that kept the LAST best instead of the first would align to the other one.
    Returns (edited image, dict(flat=[rows], repeat=[rows]))."""
    st, pt = c["st"], c["pt"]
    fx, fy, cx, cy = st.cam[:4]
    out = cur.copy()
    planted = set(v for val in PT_ROWS.values() for v in (val if isinstance(val, tuple) else (val,)))
    boxes, rows = [], dict(flat=[], repeat=[])
    for i in range(N_PTS):
        if i in planted or pt["level"][i] != 0 or pt["type"][i] != 0:
            continue
        kind = "flat" if len(rows["flat"]) < N_FLAT else "repeat"
        if kind == "repeat" and len(rows["repeat"]) >= N_REPEAT:
            break
        sp = _segment_px(P, st, pt["f"][i], pt["mu"][i], pt["sigma2"][i])
        x0, x1 = math.floor(sp[:, 0].min()) - 12, math.ceil(sp[:, 0].max()) + 13
        y0, y1 = math.floor(sp[:, 1].min()) - 12, math.ceil(sp[:, 1].max()) + 13
        if x0 < 10 or y0 < 10 or x1 > W - 10 or y1 > H - 10 or any(x0 < b[1] and b[0] < x1 and y0 < b[3] and b[2] < y1 for b in boxes):
            continue
        if kind == "flat":
            out[y0:y1, x0:x1] = 128
        else:
            p = P.synth.se3_act(st.T_true, pt["f"][i] * c["truth"]["pt_depth"][i])
            x, y = int(round(fx * p[0] / p[2] + cx)), int(round(fy * p[1] / p[2] + cy))
            sgn = 1 if x + 10 + 5 <= sp[:, 0].max() else (-1 if x - 10 - 5 >= sp[:, 0].min() else 0)
            if sgn == 0:
                continue
            out[y - 8:y + 8, x - 5 + 10 * sgn:x + 5 + 10 * sgn] = cur[y - 8:y + 8, x - 5:x + 5]
        boxes.append((x0, x1, y0, y1))
        rows[kind].append(i)
    return out, rows


_cache = {}


def options(c, **over):
    return dict(dict(n_pyr_levels=c["n_pyr_levels"]), **over)


def job_of(P, c, **over):
    return P.abi.SeedsJob(c["st"].cam, c["frame_T"], np.array([0, 1]), c["pt"], c["seg"], **options(c, **over))


def case(P, ob, k):
    """case k with its pyramids, its job and the oracle's answer, computed once per process and shared (read only)"""
    if k not in _cache:
        c = make_case(P, k)
        imgs = P.synth.render_streams([c["st"]]).numpy()[0]
        cur = imgs[1]
        if c["kind"] == "tie":
            cur, c["edits"] = edit_tie_frame(P, c, cur)
        c["frames"] = [ob.build_pyramid(imgs[0], 4), ob.build_pyramid(cur, 4)]
        c["job"] = job_of(P, c)
        c["oracle"] = ob.update_seeds(c["job"], c["frames"])
        _cache[k] = c
    return _cache[k]


_np_cache = {}


def restated(P, ob, k, **over):
    """tests/np_seeds.update_seeds on case k (with option overrides) -> (result, point records, line records), once per process"""
    import np_seeds
    key = (k, tuple(sorted(over.items())))
    if key not in _np_cache:
        c = case(P, ob, k)
        j = job_of(P, c, **over)          # the job's own buffers: the values the C ABI reads (float32 seed state)
        _np_cache[key] = np_seeds.update_seeds(c["st"].cam, c["frame_T"], c["frames"], j.pt, j.seg, **options(c, **over))
    return _np_cache[key]


def load_frames(ctx, frames_of_slots):
    ctx.config_pyramids(len(frames_of_slots), W, H, 4)
    for s, fr in enumerate(frames_of_slots):
        ctx.build_pyramid(s, fr[0], 0)


def select(c, pt_rows, seg_rows):
    """the field dicts of a case restricted to (and ordered by) the given rows"""
    return {k: v[pt_rows] for k, v in c["pt"].items()}, {k: v[seg_rows] for k, v in c["seg"].items()}


def concat(P, cases):
    """the seeds of several cases (same settings) as ONE job: case j's frames become frames / slots 2j, 2j + 1"""
    pt = {k: np.concatenate([c["pt"][k] + (2 * j if k.endswith("_frame") else 0) for j, c in enumerate(cases)]) for k in cases[0]["pt"]}
    seg = {k: np.concatenate([c["seg"][k] + (2 * j if k.endswith("_frame") else 0) for j, c in enumerate(cases)]) for k in cases[0]["seg"]}
    frame_T = np.concatenate([c["frame_T"] for c in cases])
    job = P.abi.SeedsJob(cases[0]["st"].cam, frame_T, np.arange(2 * len(cases)), pt, seg, n_pyr_levels=cases[0]["n_pyr_levels"])
    return job, [fr for c in cases for fr in c["frames"]]
