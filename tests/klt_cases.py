"""Shared case builders of the KLT bootstrap tests (tests/test_klt_host.py, tests/test_gpu_klt.py): textures, shifted views and the
inputs that make tests/np_klt.py take every exit of the tracker.  Everything here is deterministic; the expensive references are cached
per process."""
import functools
import importlib

import numpy as np
import scipy.ndimage as ndi

import np_klt as K

P = importlib.import_module("pl-svo_amd")
abi = P.abi
PAD = 64


@functools.lru_cache(maxsize=None)
def _field(w, h, seed, sigma):
    g = ndi.gaussian_filter(np.random.default_rng(seed).random((h + 2 * PAD, w + 2 * PAD)), sigma)
    return (g - g.min()) / (g.max() - g.min())


def texture(w, h, seed=3, sigma=3.0, shift=(0.0, 0.0)):
    """Gaussian-smoothed noise seen through a window shifted by `shift` pixels: view(x, y) = field(x - sx, y - sy) (cubic spline), uint8"""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    v = ndi.map_coordinates(_field(w, h, seed, sigma), [yy + PAD - shift[1], xx + PAD - shift[0]], order=3)
    return np.clip(np.rint(v * 255.0), 0, 255).astype(np.uint8)


def interior_points(w, h, n, seed, margin=60):
    r = np.random.default_rng(seed)
    return np.stack([r.uniform(margin, w - margin, n), r.uniform(margin, h - margin, n)], axis=1).astype(np.float32)


def period4(w, h, shift=0):
    """a separable pattern of period 4: textured for the Scharr derivatives at level 0, of period 2 -- zero central differences -- at
    level 1 and constant from level 2 on (the binomial filter removes the Nyquist frequency exactly)"""
    p = np.array([40, 200, 200, 40], dtype=np.int64)
    x, y = (np.arange(w) + shift) % 4, np.arange(h) % 4
    return ((p[x][None, :] + p[y][:, None]) // 2).astype(np.uint8)


def with_flat_patch(img, x0, y0, size, value=128):
    out = img.copy()
    out[y0:y0 + size, x0:x0 + size] = value
    return out


def cam_for(w, h):
    return (0.9 * w, 0.9 * w, 0.5 * w - 0.5, 0.5 * h - 0.5)


def pinhole(w, h):
    fx, fy, cx, cy = cam_for(w, h)
    return abi.Pinhole(fx, fy, cx, cy, int(w), int(h))


def border_points(w, h):
    """window positions over each border and each corner of the level-0 image, and well inside"""
    xs, ys = (2.0, w / 2.0 + 0.3, w - 3.0), (2.5, h / 2.0 - 0.2, h - 2.0)
    return np.array([(x, y) for y in ys for x in xs], dtype=np.float32)


# ---- exits: (name, ref image, cur image, prev, next, cfg overrides, level, exit np_klt must take there, extra condition) ----
@functools.lru_cache(maxsize=None)
def exit_cases():
    w, h = 320, 240
    ref = texture(w, h)
    near = texture(w, h, shift=(3.3, -2.1))
    far = texture(w, h, shift=(25.0, -18.5))
    flat0 = with_flat_patch(ref, 130, 90, 70)
    p4 = period4(w, h)
    c = []
    mid = np.array([[160.2, 120.7]], dtype=np.float32)
    c.append(("eps_or_osc", ref, near, interior_points(w, h, 6, 11), None, {}, None, None))
    c.append(("max_iter", ref, far, interior_points(w, h, 4, 12), None, {}, None, None))
    c.append(("offset_flow", ref, near, interior_points(w, h, 4, 13), np.array([2.0, -1.5], dtype=np.float32), {}, None, None))
    c.append(("prev_oor_level0", ref, near, np.array([[w + 20.0, 100.0], [100.0, -16.0], [50.0, h + 15.0]], dtype=np.float32), None, {}, 0, K.EXIT_PREV_OOR))
    c.append(("prev_oor_all", ref, near, np.array([[w + 200.0, 100.0], [-300.0, 50.0]], dtype=np.float32), None, {}, 2, K.EXIT_PREV_OOR))
    c.append(("flat_level0", flat0, flat0, np.array([[165.0, 125.0]], dtype=np.float32), None, {}, 0, K.EXIT_FLAT))
    c.append(("flat_coarse", p4, period4(w, h, 1), mid, None, {}, 2, K.EXIT_FLAT))
    c.append(("borders", ref, near, border_points(w, h), None, {}, None, None))
    # a walk out of the image in mid-iteration, at level 0 (after 1 and after 22 iterations) and at level 1: starts at the right edge
    c.append(("walk_out", ref, texture(w, h, shift=(8.0, 0.0)), np.array([[w + 6.0, 140.0], [w + 6.0, 215.0], [w + 12.0, 95.0]], dtype=np.float32), None, {},
              None, None))
    # the range test behind level 0: the last of three iterations carries the window out
    c.append(("final_check", ref, texture(w, h, shift=(24.0, 0.0)), np.array([[w + 12.0, 155.0], [w + 12.0, 170.0]], dtype=np.float32), None, dict(max_iter=3),
              None, None))
    out = []
    for name, a, b, prev, off, cfg, level, code in c:
        nxt = prev.copy() if off is None else (prev + off).astype(np.float32)
        out.append(dict(name=name, ref=a, cur=b, prev=prev, next=nxt, cfg=cfg, level=level, code=code))
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """np_klt's result of an exit case, computed once"""
    case = next(c for c in exit_cases() if c["name"] == name)
    return K.track(case["ref"], case["cur"], case["prev"], case["next"], **case["cfg"])
