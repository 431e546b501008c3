"""Directed inputs for the matcher's affine warp (pl-svo_amd/csrc/match_device.hpp::warp_affine_lds), shared by the CPU and the GPU
tests of tests/test_match_warp.py.

synth.make_match_batch rolls the camera by at most 0.01 rad and only zooms towards the scene: every group of every candidate it makes
takes the warp's STAGED path (the group's source box fits the LDS window).  The batches here are built on the same stream of landmarks,
levels, feature types and noise, but the current camera is set by an explicit twist -- a small lateral motion, z = -zoom * d0 (a
negative zoom moves AWAY from the scene: the patch covers more of the keyframe) and a roll about the optical axis -- and the first 32
candidates sit 6.0 .. 6.0 + spread pixels (at their level) from one of the four image borders.  That reaches the other two paths, LARGE
(box too big: taps read from the image) and BORDER (a corner outside the level: per-pixel test, zero fill), and candidates that mix them.

np_staging_rule is the documented rule itself, in NumPy float32: which path each group of two patch rows takes, and its box."""
import math

import numpy as np

f32 = np.float32
W, H = 326, 246          # level widths 326, 163, 81, 40: every residue mod 4
N_PTS, N_SEG = 96, 16    # 128 candidates per case: two workgroups
N_BORDER = 32

# (zoom, roll [rad], spread [px])
CASES = [(0.0, 0.0, 1.5), (0.45, 0.0, 1.5), (-0.12, 0.0, 0.4), (-0.7, 0.0, 1.5), (-0.85, 0.0, 1.5), (-0.4, 0.3, 1.5), (-1.0, 0.8, 1.5),
         (0.0, math.pi / 2, 1.5), (0.45, 0.8, 1.5), (-0.4, 3.0, 1.5)]
# n_pyr_levels = 4, so that search level 3 (a 40 x 30 image) is reached: det(A) > 48, which a level-0 reference needs the camera at ~1/8 of
# the scene depth for, a level-2 one a zoom of 0.45 and a level-3 one (1 candidate in 20) no zoom at all
CASES_4_LEVELS = [(0.88, 0.3, 1.5), (0.0, 0.0, 1.5), (0.45, 0.8, 1.5)]
N_CASES = len(CASES) + len(CASES_4_LEVELS)
SEED0 = 11

STAGED, LARGE, BORDER, NONE = 0, 1, 2, -1


def make_batch(P, k):
    """case k -> (stream, dict of plsvo_match_in arrays, n_pyr_levels); render the image pair with synth.render_streams([stream])"""
    syn = P.synth
    zoom, roll, spread = CASES[k] if k < len(CASES) else CASES_4_LEVELS[k - len(CASES)]
    n_pyr_levels = 3 if k < len(CASES) else 4
    st, d = syn.make_match_batch(SEED0 + k, W, H, N_PTS, N_SEG)
    noise = d["px_cur"] - d["px_true"]                      # the generator's own displacement of the initial estimates
    rng = np.random.default_rng(SEED0 + k + 710000)
    d0 = st.plane_d / st.plane_n[2]
    st.T_true = syn.se3_exp(np.concatenate([rng.uniform(-0.02, 0.02, 2) * d0, [-zoom * d0], [0.0, 0.0, roll]]))   # cur_from_ref
    T_cur_w = syn.se3_mul(st.T_true, st.T_ref_w)
    d["frame_T"] = np.stack([st.T_ref_w, T_cur_w])
    # border candidates: 6.0 .. 6.0 + spread pixels of their own level from the left, right, top, bottom border in turn
    fx, fy, cx, cy = st.cam[:4]
    lv = d["ref_level"][:N_BORDER]
    wl, hl = (W >> lv).astype(float), (H >> lv).astype(float)
    dist = 6.0 + rng.uniform(0.0, spread, N_BORDER)
    side = np.arange(N_BORDER) % 4
    t = rng.uniform(0.0, 1.0, N_BORDER)                     # position along the border
    x = np.where(side == 0, dist, np.where(side == 1, wl - dist, 8.0 + t * (wl - 16.0)))
    y = np.where(side == 2, dist, np.where(side == 3, hl - dist, 8.0 + t * (hl - 16.0)))
    px = np.stack([x, y], axis=1) * (1 << lv)[:, None]
    f, rays = syn._bearing(st.cam, px)
    X = syn._on_plane(st.plane_n, st.plane_d, rays)         # where the ray meets the scene plane, reference camera frame
    d["ref_px"][:N_BORDER] = px
    d["ref_f"][:N_BORDER] = f
    d["pos"][:N_BORDER] = syn.se3_act(syn.se3_inv(st.T_ref_w), X)
    p_cur = syn.se3_act(T_cur_w, d["pos"])
    d["px_true"] = np.stack([fx * p_cur[:, 0] / p_cur[:, 2] + cx, fy * p_cur[:, 1] / p_cur[:, 2] + cy], axis=1)
    d["px_cur"] = d["px_true"] + noise
    return st, d, n_pyr_levels


_cache = {}


def case(P, ob, k):
    """case k with its pyramids and the oracle's answers, computed once per process and shared (read only)"""
    if k not in _cache:
        st, d, n_pyr = make_batch(P, k)
        imgs = P.synth.render_streams([st]).numpy()[0]
        frames = [ob.build_pyramid(imgs[0], 4), ob.build_pyramid(imgs[1], 4)]
        job = P.match_job_from_batch(d, n_pyr)
        ow = ob.match_warp_patches(job, frames)
        om = ob.match_direct(job, frames)
        rule = np_staging_rule(ow["A"], W, H, d["ref_px"], d["ref_level"], ow["search_level"])
        _cache[k] = dict(st=st, d=d, n_pyr_levels=n_pyr, frames=frames, job=job, oracle_warp=ow, oracle_match=om, rule=rule)
    return _cache[k]


def load_frames(ctx, frames_of_slots):
    """frames_of_slots: list of pyramids, slot k = entry k (the device builds levels 1.. itself, like the oracle's half-sampler)"""
    ctx.config_pyramids(len(frames_of_slots), W, H, 4)
    for s, fr in enumerate(frames_of_slots):
        ctx.build_pyramid(s, fr[0], 0)


def concat(P, cases):
    """the candidates of several cases (same n_pyr_levels) as ONE batch: case k's frames become frames 2k, 2k + 1 in slots 2k, 2k + 1.
    Returns (job, list of pyramids per slot)."""
    d = {}
    for key in ("cur_frame", "ref_frame"):
        d[key] = np.concatenate([c["d"][key] + 2 * k for k, c in enumerate(cases)])
    for key in ("frame_T", "ref_px", "ref_f", "ref_level", "ref_type", "ref_grad", "pos", "px_cur"):
        d[key] = np.concatenate([c["d"][key] for c in cases])
    d["cam"] = cases[0]["d"]["cam"]
    d["frame_slot"] = np.arange(2 * len(cases), dtype=np.int32)
    return P.match_job_from_batch(d, cases[0]["n_pyr_levels"]), [fr for c in cases for fr in c["frames"]]


def _inverse_f32(A):
    A = np.asarray(A, np.float64).reshape(-1, 4)
    with np.errstate(all="ignore"):
        det = A[:, 0] * A[:, 3] - A[:, 2] * A[:, 1]
        invdet = 1.0 / det
        return ((A[:, 3] * invdet).astype(f32), (-A[:, 1] * invdet).astype(f32), (-A[:, 2] * invdet).astype(f32), (A[:, 0] * invdet).astype(f32))


def _warp_px(a, ppx, ppy, rx, ry):
    """(a00 * ppx + a01 * ppy) + rx and its row twin: float32 products, sums and rounding one at a time (nothing fused)"""
    a00, a01, a10, a11 = a
    with np.errstate(all="ignore"):
        return (a00 * ppx + a01 * ppy) + rx, (a10 * ppx + a11 * ppy) + ry


def np_staging_rule(A, W, H, ref_px, level, search_level):
    """The rule documented above warp_affine_lds, for n candidates: A [n, 4] (double, row-major), ref_px [n, 2], level [n],
    search_level [n] (-1: rejected before the warp).  For each of the five groups of two patch rows: the four corners of the group's
    10 x 2 grid with the pixel loop's own float32 expressions; BORDER when a corner is outside [0, cols - 1) x [0, rows - 1) of the
    keyframe level; else the box cmin = floor(min x), cmax = floor(max x) + 1, rmin, rmax alike, cbase = cmin & ~3, and STAGED when
    cmax - cbase <= 19 and rmax - rmin <= 5, LARGE otherwise.  Returns a dict: cls [n, 5] (NONE for a candidate that is not warped),
    cmin, cmax, cbase, rmin, rmax [n, 5] (valid where cls is STAGED or LARGE), cols, rows [n], and mask [n] uint8 (bit g: group g STAGED)."""
    A = np.asarray(A, np.float64).reshape(-1, 4)
    n = A.shape[0]
    level = np.asarray(level).astype(np.int64)
    sl = np.asarray(search_level).astype(np.int64)
    ref_px = np.asarray(ref_px, np.float64).reshape(-1, 2)
    a = _inverse_f32(A)
    warped = (sl >= 0) & ~np.isnan(a[0])
    cols, rows = (W >> level), (H >> level)
    rx = ref_px[:, 0].astype(f32) / (1 << level).astype(f32)
    ry = ref_px[:, 1].astype(f32) / (1 << level).astype(f32)
    fscale = (1 << np.maximum(sl, 0)).astype(f32)
    out = {k: np.zeros((n, 5), np.int64) for k in ("cmin", "cmax", "cbase", "rmin", "rmax")}
    cls = np.full((n, 5), NONE, np.int8)
    for g in range(5):
        y0 = 2 * g
        xs, ys = [], []
        inside = warped.copy()
        for k in range(4):
            ppx = f32(4 if (k & 1) else -5) * fscale
            ppy = f32((y0 + 1 if (k & 2) else y0) - 5) * fscale
            px0, px1 = _warp_px(a, ppx, ppy, rx, ry)
            with np.errstate(invalid="ignore"):
                inside &= ~((px0 < 0) | (px1 < 0) | (px0 >= (cols - 1).astype(f32)) | (px1 >= (rows - 1).astype(f32))) & ~np.isnan(px0) & ~np.isnan(px1)
            xs.append(px0)
            ys.append(px1)
        xs, ys = np.where(inside, np.stack(xs), f32(0)), np.where(inside, np.stack(ys), f32(0))
        cmin, cmax = np.floor(xs.min(0)).astype(np.int64), np.floor(xs.max(0)).astype(np.int64) + 1
        rmin, rmax = np.floor(ys.min(0)).astype(np.int64), np.floor(ys.max(0)).astype(np.int64) + 1
        cbase = cmin & ~3
        staged = inside & (cmax - cbase <= 19) & (rmax - rmin <= 5)
        cls[:, g] = np.where(~warped, NONE, np.where(~inside, BORDER, np.where(staged, STAGED, LARGE)))
        for k, v in (("cmin", cmin), ("cmax", cmax), ("cbase", cbase), ("rmin", rmin), ("rmax", rmax)):
            out[k][:, g] = v
    out.update(cls=cls, cols=cols, rows=rows, mask=((cls == STAGED) << np.arange(5)).sum(1).astype(np.uint8))
    return out


def np_zero_filled(A, W, H, ref_px, level, search_level):
    """[n, 10, 10] bool: the patch pixels warpAffine leaves at 0 because their source position is outside the keyframe level"""
    A = np.asarray(A, np.float64).reshape(-1, 4)
    level = np.asarray(level).astype(np.int64)
    sl = np.asarray(search_level).astype(np.int64)
    ref_px = np.asarray(ref_px, np.float64).reshape(-1, 2)
    a = tuple(v[:, None, None] for v in _inverse_f32(A))
    cols, rows = (W >> level)[:, None, None], (H >> level)[:, None, None]
    rx = (ref_px[:, 0].astype(f32) / (1 << level).astype(f32))[:, None, None]
    ry = (ref_px[:, 1].astype(f32) / (1 << level).astype(f32))[:, None, None]
    fscale = (1 << np.maximum(sl, 0)).astype(f32)[:, None, None]
    ppx = (np.arange(10, dtype=f32) - f32(5))[None, None, :] * fscale
    ppy = (np.arange(10, dtype=f32) - f32(5))[None, :, None] * fscale
    px0, px1 = _warp_px(a, ppx, ppy, rx, ry)
    with np.errstate(invalid="ignore"):
        outside = (px0 < 0) | (px1 < 0) | (px0 >= (cols - 1).astype(f32)) | (px1 >= (rows - 1).astype(f32))
    return outside & ((sl >= 0) & ~np.isnan(a[0][:, 0, 0]))[:, None, None]
