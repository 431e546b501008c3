"""The bootstrap's KLT track on the device (plsvo_klt_*, klt_device.hpp) bit for bit against tests/np_klt.py: per point
next / status / exit / iteration count per level, the KLT pyramid levels, the lists, bearings, disparities, the median and the reports.
tests/test_emu_klt.py runs this file on the host emulation build inside the CPU suite."""
import ctypes as C
import functools

import numpy as np
import pytest

import klt_cases as Kc
import np_klt as K

pytestmark = pytest.mark.gpu
A = Kc.abi
E_INVALID, E_STATE = A.E_INVALID, A.E_STATE


@pytest.fixture(scope="module")
def ctx():
    c = Kc.P.capi.Context(0)
    yield c
    c.close()


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _load(ctx, imgs):
    h, w = imgs[0].shape
    ctx.config_pyramids(len(imgs), w, h, 1)
    for i, im in enumerate(imgs):
        ctx.build_pyramid(i, im)


def _same_track(d, r):
    return all(_same(d[k], r[k]) for k in ("next", "status", "exit", "iters"))


def _same_lists(d, r, second=True):
    keys = ("px_ref", "px_cur", "f_ref") + (("f_cur", "disparity") if second else ())
    return all(len(d[k]) == len(r[k]) and _same(d[k].ravel(), np.asarray(r[k], dtype=d[k].dtype).ravel()) for k in keys)


def _same_report(d, r):
    return all(d[k] == r[k] for k in ("result", "n_before", "n_after", "n_calls")) and np.float64(d["median_disparity"]).tobytes() == np.float64(r["median_disparity"]).tobytes()


def _grid_points(w, h, n, margin):
    """n points on a lattice inside the margin (a host list for a first frame)"""
    k = int(np.ceil(np.sqrt(n)))
    xs, ys = np.linspace(margin, w - margin, k), np.linspace(margin, h - margin, k)
    return np.array([(x, y) for y in ys for x in xs], dtype=np.float32)[:n]


# ---- sizes: level counts, odd sizes, the maxLevel cap --------------------------------------------------------------------------------------
SIZES = [(320, 240, 4, 3), (97, 71, 4, 2), (61, 45, 4, 1), (320, 240, 1, 2)]


@pytest.mark.parametrize("w,h,max_level,n_lv", SIZES)
def test_sizes_levels_and_points(ctx, w, h, max_level, n_lv):
    ref, cur = Kc.texture(w, h, seed=5), Kc.texture(w, h, seed=5, shift=(1.7, -1.2))
    _load(ctx, [ref, cur])
    margin = 50 if w > 100 else 22
    inner = Kc.interior_points(w, h, 8, 41, margin=margin)
    prev = np.concatenate([inner, inner[:4], Kc.border_points(w, h)])
    nxt = prev.copy()
    nxt[8:12] += np.array([1.5, -1.0], dtype=np.float32)                 # an offset initial flow
    want = K.track(ref, cur, prev, nxt, max_level=max_level)
    assert want["status"][:12].all() and np.all(want["exit"][:, n_lv:] == K.EXIT_NONE) and np.all(want["exit"][:, :n_lv] != K.EXIT_NONE)
    assert _same_track(ctx.klt_track_points(0, 1, prev, nxt, max_level=max_level), want)
    # the resident path on the same two frames: pyramid levels, lists, report
    px = _grid_points(w, h, 100, margin - 6)
    cam = Kc.cam_for(w, h)
    ctx.klt_reserve(1, 128, max_level=max_level)
    ctx.klt_first_frame([dict(slot=0, cam=Kc.pinhole(w, h), px=px)])
    ctx.klt_second_frame([1], 40, 1.0)
    rep = ctx.klt_fetch()[0]
    lists0, rep0 = K.first_frame(cam, px)
    lists1, rep1, _ = K.second_frame(lists0, cam, ref, cur, 0, 40, 1.0, max_level=max_level)
    assert rep["levels"] == n_lv and _same_report(rep, rep1) and rep1["n_after"] >= 40
    assert _same_lists(ctx.klt_fetch_tracks(0), lists1)
    for which, img in ((0, ref), (1, cur)):
        pyr = K.build_pyramid(img, max_level=max_level)
        assert len(pyr) == n_lv
        for l in range(1, n_lv):
            assert _same(ctx.klt_download_level(0, which, l), pyr[l]), (which, l)
    for bad in (0, n_lv):
        with pytest.raises(Kc.P.capi.PlsvoError) as e:
            ctx.klt_download_level(0, 0, bad)
        assert e.value.code == E_INVALID


# ---- every exit -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in Kc.exit_cases()])
def test_exit_cases(ctx, name):
    """Inputs chosen so that np_klt takes each exit (tests/test_klt_host.py::test_exit_cases_take_their_exits asserts the whole table).
    `prev out of range at a coarse level only` cannot occur: floor(prev / 2^l - 14.5) >= W_l means prev >= 2^l W_l + 14.5 * 2^l >=
    W + 14.5, and prev / 2^l - 14.5 < -30 means prev < -15.5 * 2^l <= -15.5, so a window that is out at level l is out at level 0;
    the cases are out at level 0 alone and out at every level."""
    c = next(c for c in Kc.exit_cases() if c["name"] == name)
    want = Kc.reference(name)
    if c["code"] is not None:
        assert np.all(want["exit"][:, c["level"]] == c["code"])
    if name == "walk_out":
        assert want["exit"][0, 0] == want["exit"][2, 1] == K.EXIT_ITER_OOR and want["iters"][1, 0] > 1 and want["iters"][2, 1] > 1
    if name == "final_check":
        assert np.all(want["exit"][:, 0] == K.EXIT_MAX_ITER) and not want["status"].any()
    if name == "eps_or_osc":
        assert {K.EXIT_EPS, K.EXIT_OSC} <= set(want["exit"][:, :3].ravel().tolist())
    if name == "max_iter":
        assert K.EXIT_MAX_ITER in want["exit"][:, :3]
    _load(ctx, [c["ref"], c["cur"]])
    assert _same_track(ctx.klt_track_points(0, 1, c["prev"], c["next"], **c["cfg"]), want)


# ---- batches and lists --------------------------------------------------------------------------------------------------------------------
W, H = 160, 120
CAM = Kc.cam_for(W, H)
BAD = (-500.0, 10.0)                                                      # out of range at every level: lost, and costs nothing


@functools.lru_cache(maxsize=None)
def _views():
    return Kc.texture(W, H, seed=7), Kc.texture(W, H, seed=7, shift=(2.2, -1.3)), Kc.texture(W, H, seed=7, shift=(4.1, -2.9))


@functools.lru_cache(maxsize=None)
def _kind_px(kind):
    """a first frame's host list of 100 or more entries: 'g' a trackable interior point, 'b' a lost one"""
    good = Kc.interior_points(W, H, 70, 31, margin=35)
    pat = {"front_mid_back": "bb" + "g" * 20 + "bbb" + "g" * 25 + "b" * 48 + "gg" + "b", "all_lost": "b" * 100, "k0": "b" * 100, "k1": "b" * 57 + "g" + "b" * 42,
           "k3": "g" + "b" * 98 + "gg", "k39": "gb" * 39 + "b" * 22, "k40": "gb" * 40 + "b" * 20, "k64": "g" * 64 + "b" * 40, "k65": "b" * 36 + "g" * 65,
           "short": "g" * 60 + "b" * 39, "long": "g" * 70 + "b" * 59}[kind]
    gi = iter(good)
    return np.array([next(gi) if ch == "g" else BAD for ch in pat], dtype=np.float32)


@functools.lru_cache(maxsize=None)
def _kind_ref(kind, curs, min_tracked, min_disparity, cap):
    """np_klt's lists and reports of a stream kind behind its first frame and every second frame of `curs` (indices into _views())"""
    lists, rep = K.first_frame(CAM, _kind_px(kind), cap_pts=cap)
    out = [(lists, rep)]
    for ci in curs:
        if out[0][1]["result"] != K.FIRST:                                 # no first frame holds: a second frame does nothing
            out.append((lists, dict(result=K.INACTIVE, n_before=0, n_after=0, median_disparity=0.0, n_calls=0)))
            continue
        lists, rep, _ = K.second_frame(lists, CAM, _views()[0], _views()[ci], rep["n_calls"], min_tracked, min_disparity)
        out.append((lists, rep))
    return out


def _run_batch(ctx, kinds, calls, min_tracked=40, min_disparity=1000.0, cap=128):
    """kinds: per stream a kind or None (inactive); calls: per second frame a list of per-stream view indices (None = sits the call out)"""
    _load(ctx, list(_views()))
    n = len(kinds)
    ctx.klt_reserve(n, cap)
    ctx.klt_first_frame([None if k is None else dict(slot=0, cam=Kc.pinhole(W, H), px=_kind_px(k)) for k in kinds])
    taken = [() for _ in kinds]
    inactive = dict(result=K.INACTIVE, n_before=0, n_after=0, median_disparity=0.0, n_calls=0)

    def check(second):
        reps = ctx.klt_fetch()
        for s, k in enumerate(kinds):
            if k is None:
                assert _same_report(reps[s], inactive), s
                continue
            lists, rep = _kind_ref(k, taken[s], min_tracked, min_disparity, cap)[len(taken[s])]
            assert _same_report(reps[s], rep), (s, k, reps[s], rep)
            assert _same_lists(ctx.klt_fetch_tracks(s), lists, second=len(taken[s]) > 0 and rep["result"] != K.INACTIVE), (s, k)
        return reps

    check(False)
    for call in calls:
        ctx.klt_second_frame(call, min_tracked, min_disparity)
        taken = [t + ((c,) if c is not None else ()) for t, c, k in zip(taken, call, kinds)]
        reps = check(True)
    return reps


def test_list_lengths_losses_and_a_second_call(ctx):
    """0, 1, 64 and 65 entries, an inactive stream, losses at the front, in the middle and at the back, everything lost; the second call
    starts from the kept px_cur (NO_KEYFRAME leaves the lists compacted) and a stream may sit it out"""
    kinds = ["front_mid_back", "k0", "k1", None, "k64", "k65", "all_lost", "k3"]
    reps = _run_batch(ctx, kinds, [[1] * 8, [2, 2, 2, 2, None, 2, 2, 2]])
    assert [r["result"] for r in reps] == [K.NO_KEYFRAME, K.FAILURE, K.FAILURE, K.INACTIVE, K.NO_KEYFRAME, K.NO_KEYFRAME, K.FAILURE, K.FAILURE]
    assert [r["n_after"] for r in reps] == [47, 0, 1, 0, 64, 65, 0, 3] and [r["n_calls"] for r in reps] == [2, 2, 2, 0, 1, 2, 2, 2]
    assert reps[0]["median_disparity"] > 4.0                               # the second view's shift, tracked from the first view's result


def test_gates(ctx):
    """39 against 40 tracked; a median just below and at the threshold"""
    reps = _run_batch(ctx, ["k39", "k40"], [[1, 1]], min_tracked=40, min_disparity=0.5)
    assert [r["result"] for r in reps] == [K.FAILURE, K.TRACKED] and [r["n_after"] for r in reps] == [39, 40]
    m = reps[1]["median_disparity"]
    assert 2.0 < m < 3.0
    assert _run_batch(ctx, ["k40"], [[1]], min_disparity=m)[0]["result"] == K.TRACKED            # median < threshold is false at the threshold
    assert _run_batch(ctx, ["k40"], [[1]], min_disparity=float(np.nextafter(m, np.inf)))[0]["result"] == K.NO_KEYFRAME


def test_batch_sizes_and_capacity(ctx):
    """cu_count / 2 + 1 streams and two; cap_pts exceeded by one stream"""
    n = ctx.device_info()[1] // 2 + 1
    cycle = ["k1", "k0", "k3", None, "all_lost"]
    kinds = [cycle[i % len(cycle)] for i in range(n)]
    kinds[n // 2], kinds[-1] = "k65", "front_mid_back"
    reps = _run_batch(ctx, kinds, [[1] * n], min_tracked=2, min_disparity=2.0)
    assert reps[n // 2]["result"] == K.TRACKED and reps[-1]["n_after"] == 47 and reps[2]["n_after"] == 3 and reps[0]["result"] == K.FAILURE
    reps = _run_batch(ctx, ["short", "long"], [[1, 2]], cap=128)           # "short" offers 99 points, "long" 129 > cap_pts
    assert [r["result"] for r in reps] == [K.INACTIVE, K.INACTIVE]
    ctx.klt_reserve(2, 128)
    ctx.klt_first_frame([dict(slot=0, cam=Kc.pinhole(W, H), px=_kind_px(k)) for k in ("short", "long")])
    reps = ctx.klt_fetch()
    assert [(r["result"], r["n_before"], r["n_after"]) for r in reps] == [(K.FAILURE, 99, 0), (K.DROPPED, 129, 0)]
    assert all(len(ctx.klt_fetch_tracks(s)["px_ref"]) == 0 for s in range(2))


# ---- the first frame from the detector's device records ---------------------------------------------------------------------------------
def _device_buffer(data):
    """device memory holding `data` that the library's d_ pointers can reach: HBM through torch on a GPU, a host array on the emulation build"""
    import torch
    a = np.ascontiguousarray(data).view(np.uint8).ravel().copy()
    if torch.cuda.is_available():
        t = torch.from_numpy(a).cuda()
        torch.cuda.synchronize()
        return t, t.data_ptr(), lambda: t.cpu().numpy()
    return a, a.ctypes.data, lambda: a.copy()


def test_first_frame_from_detected_corners(ctx):
    w, h = 320, 240
    ref, cur = Kc.texture(w, h, seed=9, sigma=1.6), Kc.texture(w, h, seed=9, sigma=1.6, shift=(2.4, 1.1))
    ctx.config_pyramids(2, w, h, 3)
    ctx.build_pyramid(0, ref)
    ctx.build_pyramid(1, cur)
    cells = 13 * 10
    corners = ctx.detect_fast(0, 1)[0]
    assert 100 < len(corners) <= cells, len(corners)
    k_rec, p_rec, read_rec = _device_buffer(np.zeros(cells * 16, np.uint8))
    k_cnt, p_cnt, read_cnt = _device_buffer(np.zeros(1, np.int32))
    ctx.detect_fast_dev(0, 1, p_rec, p_cnt)                                # enqueue only: the first frame reads the records on the device
    k100, p100, _ = _device_buffer(np.array([100], np.int32))
    k99, p99, _ = _device_buffer(np.array([99], np.int32))
    cam = Kc.cam_for(w, h)
    px = np.stack([corners["x"], corners["y"]], axis=1).astype(np.float32)
    extra_px = np.array([[40.5, 50.25], [60.0, 55.5], [79.5, 60.75]], dtype=np.float32)            # endpoint, midpoint, endpoint
    ends = K.bearing(cam, extra_px[[0, 2]])
    extra_f = np.stack([ends[0], (ends[0] + ends[1]) / 2.0, ends[1]])    # the midpoint's bearing is no cam2world result
    pin = Kc.pinhole(w, h)
    frames = [dict(slot=0, cam=pin, d_corners=p_rec, d_count=p100), dict(slot=0, cam=pin, d_corners=p_rec, d_count=p99),
              dict(slot=0, cam=pin, d_corners=p_rec, d_count=p_cnt, extra_px=extra_px, extra_f=extra_f),
              dict(slot=0, cam=pin, px=px, extra_px=extra_px, extra_f=extra_f), None, dict(slot=0, cam=pin, px=px[:100], extra_px=extra_px[:1], extra_f=extra_f[:1])]
    cap = len(corners) + 3
    ctx.klt_reserve(len(frames), cap)
    ctx.klt_first_frame(frames)
    reps = ctx.klt_fetch()
    assert int(read_cnt().view(np.int32)[0]) == len(corners)
    want = [K.first_frame(cam, px[:100]), K.first_frame(cam, px[:99]), K.first_frame(cam, px, extra_px, extra_f), K.first_frame(cam, px, extra_px, extra_f), None,
            K.first_frame(cam, px[:100], extra_px[:1], extra_f[:1])]
    assert [r["result"] for r in reps] == [K.FIRST, K.FAILURE, K.FIRST, K.FIRST, K.INACTIVE, K.FIRST]
    for s, wv in enumerate(want):
        if wv is not None:
            assert _same_report(reps[s], wv[1]) and _same_lists(ctx.klt_fetch_tracks(s), wv[0], second=False), s
    assert _same(ctx.klt_fetch_tracks(2)["f_ref"][-2], extra_f[1])
    ctx.klt_second_frame([1, 1, 1, None, 1, None], 40, 2.0)
    reps = ctx.klt_fetch()
    lists, rep, tr = K.second_frame(want[2][0], cam, ref, cur, 0, 40, 2.0)
    assert rep["result"] == K.TRACKED and tr["status"].sum() >= 100
    assert _same_report(reps[2], rep) and _same_lists(ctx.klt_fetch_tracks(2), lists)
    assert reps[1]["result"] == reps[4]["result"] == K.INACTIVE and reps[3]["result"] == K.FIRST and reps[0]["result"] == K.TRACKED
    dev = ctx.klt_tracks_dev()
    assert dev["streams"] == len(frames) and dev["cap_pts"] == cap and all(dev[k] for k in ("px_ref", "px_cur", "f_ref", "f_cur", "disparity", "count"))


def test_sequence_bootstrap_plays_until_tracked(ctx):
    """sequence.klt_bootstrap on the synthetic sequence: first frame, then a second frame per image until the disparity gate passes"""
    import importlib
    seqm = importlib.import_module("pl-svo_amd.sequence")
    seq = seqm.make_sequence(7, 12, 320, 240, 120, 30, total=0.35)
    det = dict(fast_threshold=7, detection_threshold=2.0)
    backend = seqm.HipBackend(ctx)
    reports, tracks = seqm.klt_bootstrap(backend, seq["images"][:6], seq["cam"], init_min_disparity=10.0, detect=det)
    corners = backend.detect_corners(0, **det)
    cam = tuple(seq["cam"][:4])
    lists, rep = K.first_frame(cam, np.stack([corners["x"], corners["y"]], axis=1))
    assert rep["result"] == K.FIRST and _same_report(reports[0], rep)
    for k, got in enumerate(reports[1:], start=1):
        lists, rep, _ = K.second_frame(lists, cam, seq["images"][0], seq["images"][k], rep["n_calls"], 40, 10.0)
        assert _same_report(got, rep), k
    assert [r["result"] for r in reports[1:]] == [K.NO_KEYFRAME] * (len(reports) - 2) + [K.TRACKED] and 3 <= len(reports) <= 6
    assert _same_lists(tracks, lists) and len(tracks["px_ref"]) >= 100


# ---- every error return ------------------------------------------------------------------------------------------------------------------
def test_rejected_arguments_return_their_code_and_write_nothing(ctx):
    P = Kc.P
    L = ctx.L
    fresh = P.capi.Context(0)
    try:
        cfg = A.klt_cfg(1, 128)
        assert L.plsvo_klt_reserve(fresh.h, C.byref(cfg)) == E_STATE                               # pyramids not configured
        fresh.config_pyramids(2, W, H, 1)
        rep, tr, sec, par, fst = A.KltReport(), A.KltTracks(), (A.KltSecond * 1)(), A.KltParams(40, 0, 40.0), (A.KltFirst * 1)()
        assert L.plsvo_klt_first_frame(fresh.h, 1, fst) == E_STATE and L.plsvo_klt_second_frame(fresh.h, 1, sec, C.byref(par)) == E_STATE
        assert L.plsvo_klt_fetch(fresh.h, 1, C.byref(rep)) == E_STATE and L.plsvo_klt_fetch_tracks(fresh.h, 0, C.byref(tr)) == E_STATE
        assert L.plsvo_klt_tracks_dev(fresh.h, C.byref(tr)) == E_STATE and L.plsvo_klt_download_level(fresh.h, 0, 0, 1, None) == E_STATE
    finally:
        fresh.close()
    _load(ctx, list(_views()))
    assert L.plsvo_klt_reserve(ctx.h, None) == E_INVALID
    for kw in (dict(streams=0), dict(cap_pts=0), dict(win=21), dict(win=31), dict(max_level=-1), dict(max_level=5), dict(max_iter=0), dict(max_iter=256),
               dict(eps=-1.0), dict(eps=float("nan")), dict(min_eig=-1e-4), dict(min_eig=float("inf"))):
        cfg = A.klt_cfg(**dict(dict(streams=1, cap_pts=128), **kw))
        assert L.plsvo_klt_reserve(ctx.h, C.byref(cfg)) == E_INVALID, kw
        assert b"klt_reserve" in L.plsvo_hip_last_error(ctx.h)
    reps = _run_batch(ctx, ["k40", "k3"], [[1, 1]])
    before = (reps, [ctx.klt_fetch_tracks(s) for s in range(2)])
    pin, px = Kc.pinhole(W, H), _kind_px("k40")
    pxp = px.ctypes.data_as(A.c_float_p)

    def first(n=2, null=False, **kw):
        arr = (A.KltFirst * 2)()
        f = dict(dict(active=1, slot=0, cam=pin, n_host=100, host_px=pxp), **kw)
        for k, v in f.items():
            setattr(arr[1], k, v)
        return L.plsvo_klt_first_frame(ctx.h, n, None if null else arr)

    bad_cam = [A.Pinhole(pin.fx, pin.fy, pin.cx, pin.cy, W + 1, H), A.Pinhole(0.0, pin.fy, pin.cx, pin.cy, W, H), A.Pinhole(pin.fx, float("nan"), pin.cx, pin.cy, W, H)]
    for kw in (dict(n=1), dict(n=3), dict(null=True), dict(slot=-1), dict(slot=3), dict(n_host=-1), dict(host_px=None), dict(n_extra=-2), dict(n_extra=1),
               dict(n_extra=1, extra_px=pxp), dict(d_corners=8, d_count=None), *[dict(cam=c) for c in bad_cam]):
        assert first(**kw) == E_INVALID, kw
        assert b"klt_first_frame" in L.plsvo_hip_last_error(ctx.h)

    def second(n=2, null=False, params=True, mt=40, md=40.0, slot=1):
        arr = (A.KltSecond * 2)()
        arr[1].active, arr[1].cur_slot = 1, slot
        pr = A.KltParams(mt, 0, md)
        return L.plsvo_klt_second_frame(ctx.h, n, None if null else arr, C.byref(pr) if params else None)

    for kw in (dict(n=1), dict(null=True), dict(params=False), dict(mt=-1), dict(md=float("nan")), dict(md=float("inf")), dict(slot=-1), dict(slot=3)):
        assert second(**kw) == E_INVALID, kw
    rep2 = (A.KltReport * 2)()
    assert L.plsvo_klt_fetch(ctx.h, 1, rep2) == E_INVALID and L.plsvo_klt_fetch(ctx.h, 2, None) == E_INVALID
    tr = A.KltTracks()
    assert L.plsvo_klt_fetch_tracks(ctx.h, -1, C.byref(tr)) == E_INVALID and L.plsvo_klt_fetch_tracks(ctx.h, 2, C.byref(tr)) == E_INVALID
    assert L.plsvo_klt_fetch_tracks(ctx.h, 0, None) == E_INVALID and L.plsvo_klt_tracks_dev(ctx.h, None) == E_INVALID
    buf = np.full(W * H, 0x5A, np.uint8)
    u8 = buf.ctypes.data_as(A.c_u8_p)
    for a in ((-1, 0, 1, u8), (2, 0, 1, u8), (0, 2, 1, u8), (0, 0, 0, u8), (0, 0, 2, u8), (0, 0, 1, None)):
        assert L.plsvo_klt_download_level(ctx.h, *a) == E_INVALID, a
    # the stateless diagnostic
    pts = np.full((2, 2), 50.0, np.float32)
    nxt, st, ex, it = np.full((2, 2), 7.0, np.float32), np.full(2, 0x5A, np.uint8), np.full(10, 0x5A, np.uint8), np.full(10, 0x5A, np.uint8)
    fp, up = A.c_float_p, A.c_u8_p

    def points(cfg=A.klt_cfg(), ref=0, cur=1, n=2, prev=pts, nin=pts, nout=nxt, status=st, ec=ex, iters=it):
        p = lambda a, t: None if a is None else a.ctypes.data_as(t)
        return L.plsvo_klt_track_points(ctx.h, None if cfg is None else C.byref(cfg), ref, cur, n, p(prev, fp), p(nin, fp), p(nout, fp), p(status, up), p(ec, up), p(iters, up))

    for kw in (dict(cfg=None), dict(cfg=A.klt_cfg(win=15)), dict(cfg=A.klt_cfg(max_level=7)), dict(ref=-1), dict(ref=3), dict(cur=3), dict(n=-1), dict(prev=None),
               dict(nin=None), dict(nout=None), dict(status=None), dict(ec=None), dict(iters=None)):
        assert points(**kw) == E_INVALID, kw
    assert points(n=0) == 0
    assert np.all(buf == 0x5A) and np.all(nxt == 7.0) and np.all(st == 0x5A) and np.all(ex == 0x5A) and np.all(it == 0x5A)
    # nothing was written: the reports and the lists are what they were
    after = (ctx.klt_fetch(), [ctx.klt_fetch_tracks(s) for s in range(2)])
    assert before[0] == after[0] and all(_same(before[1][s][k], after[1][s][k]) for s in range(2) for k in before[1][s])
    # the pyramids reconfigured behind the reserve
    ctx.config_pyramids(3, W + 16, H, 1)
    assert second() == E_STATE and first() == E_STATE
    assert b"reconfigured" in L.plsvo_hip_last_error(ctx.h)
