"""Rectification of raw distorted frames into pyramid slots on the device (plsvo_hip_config_rectify, plsvo_hip_rectify_build_pyramid,
plsvo_hip_rectify_build_pyramids_dev) against the NumPy restatement of vk::PinholeCamera::undistortImage (tests/np_rectify.py): level 0
bit for bit, levels 1.. equal to the oracle's half-sampler on the NumPy-rectified image, the batched form's strides and slot range, every
rejected argument, and the tiled mirror the one-wave-per-frame alignment reads.  Images stay at <= 160 x 120 and a few slots so that the
emulated run (tests/test_emu_parity.py) takes them too; the name of the one 640 x 480 x 4096-slot check contains `full_size`."""
import numpy as np
import pytest

import helpers as Hh
import np_rectify as R

pytestmark = pytest.mark.gpu

MAX_MAPS = 8   # PLSVO_MAX_RECTIFY_MAPS (include/plsvo_hip.h)

W, H = 160, 120
CAMS = {
    "barrel": dict(width=W, height=H, fx=95.3, fy=96.1, cx=79.6, cy=60.2, d=[-0.28340811, 0.07395907, 1.9359e-4, 1.76187114e-5]),
    "strong_barrel_k3": dict(width=W, height=H, fx=90.0, fy=90.5, cx=80.4, cy=59.3, d=[-0.45, 0.22, 0.0, 0.0, -0.05]),
    "pincushion_tangential": dict(width=W, height=H, fx=110.0, fy=109.0, cx=79.0, cy=61.0, d=[0.3, 0.1, 0.004, -0.006]),
}


def _cam(P, c):
    return P.abi.pinhole_radtan(c["width"], c["height"], c["fx"], c["fy"], c["cx"], c["cy"], c["d"])


def _device_bytes(host):
    """`host` (uint8 array) where the library's device pointers reach it: HBM through torch on a GPU box, the array itself on the host
    emulation build (whose device memory is host memory).  -> (keep-alive, pointer)"""
    import torch
    if torch.cuda.is_available():
        t = torch.from_numpy(host).cuda()
        torch.cuda.synchronize()
        return t, t.data_ptr()
    return host, host.ctypes.data


@pytest.fixture
def ctx(P):
    """a context of its own: every test configures maps, and a context holds PLSVO_MAX_RECTIFY_MAPS of them"""
    c = P.capi.Context(0)
    yield c
    c.close()


def _scene(seed, w=W, h=H):
    """a smooth synthetic scene with edges: a few discs and bars on a gradient"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = 40 + 120 * xx / w + 30 * np.sin(yy / 7.0)
    for _ in range(6):
        cx, cy, r = rng.uniform(0, w), rng.uniform(0, h), rng.uniform(5, 25)
        img = np.where((xx - cx) ** 2 + (yy - cy) ** 2 < r * r, rng.uniform(0, 255), img)
    return np.clip(img, 0, 255).astype(np.uint8)


def test_noise_frames_hit_every_fraction():
    xy, frac = R.rectify_map(CAMS["barrel"])
    assert len(np.unique(frac)) == 1024
    # the pincushion camera samples beyond the raw frame: pixels with every tap outside, and pixels with some taps outside
    xy, _ = R.rectify_map(CAMS["pincushion_tangential"])
    x0, y0 = xy[..., 0].astype(int), xy[..., 1].astype(int)
    assert ((x0 < -1) | (x0 >= W) | (y0 < -1) | (y0 >= H)).sum() > 100
    assert ((x0 == -1) | (x0 == W - 1) | (y0 == -1) | (y0 == H - 1)).sum() > 20


@pytest.mark.parametrize("flip", [False, True], ids=["upright", "flipped"])
@pytest.mark.parametrize("name", sorted(CAMS))
@pytest.mark.parametrize("kind", ["noise", "scene"])
def test_level0_equals_numpy_remap(P, ctx, name, flip, kind):
    c = CAMS[name]
    raw = np.random.default_rng(5).integers(0, 256, (H, W), dtype=np.uint8) if kind == "noise" else _scene(6)
    ctx.config_pyramids(2, W, H, 3)
    mid = ctx.config_rectify(_cam(P, c), flip_vertical=flip)
    ctx.rectify_build_pyramid(mid, 1, raw)
    got = ctx.download_level(1, 0)
    want = R.undistort(raw, c, flip=flip)
    assert np.array_equal(got, want), f"{(got != want).sum()} pixels differ"
    assert not np.array_equal(want, raw[::-1] if flip else raw)


def test_odd_size_uses_the_byte_tail(P, ctx):
    c = dict(width=157, height=93, fx=80.3, fy=81.1, cx=77.9, cy=46.2, d=[-0.2, 0.05, 0.002, -0.001, 0.001])
    raw = np.random.default_rng(8).integers(0, 256, (93, 157), dtype=np.uint8)
    ctx.config_pyramids(1, 157, 93, 2)
    for flip in (False, True):
        mid = ctx.config_rectify(_cam(P, c), flip_vertical=flip)
        ctx.rectify_build_pyramid(mid, 0, raw)
        assert np.array_equal(ctx.download_level(0, 0), R.undistort(raw, c, flip=flip))


def test_identity_branch_copies(P, ctx):
    """|d0| <= 1e-7: vikit copies the frame even though d1..d4 are not zero (flipped first when asked)"""
    c = dict(CAMS["barrel"], d=[0.0, 0.3, 0.01, -0.02, 0.1])
    raw = np.random.default_rng(9).integers(0, 256, (H, W), dtype=np.uint8)
    ctx.config_pyramids(2, W, H, 3)
    up, fl = ctx.config_rectify(_cam(P, c)), ctx.config_rectify(_cam(P, c), flip_vertical=True)
    ctx.rectify_build_pyramid(up, 0, raw)
    ctx.rectify_build_pyramid(fl, 1, raw)
    assert np.array_equal(ctx.download_level(0, 0), raw)
    assert np.array_equal(ctx.download_level(1, 0), raw[::-1])
    mid = ctx.config_rectify(_cam(P, dict(c, d=[2e-7] + c["d"][1:])))   # just past the threshold: the remap
    ctx.rectify_build_pyramid(mid, 0, raw)
    assert np.array_equal(ctx.download_level(0, 0), R.undistort(raw, dict(c, d=[2e-7] + c["d"][1:])))


@pytest.mark.parametrize("rounding", [0, 1])
def test_upper_levels_equal_the_half_sampler_of_the_numpy_image(P, ob, ctx, rounding):
    c = CAMS["strong_barrel_k3"]
    raw = _scene(11)
    nlev = 4
    ctx.config_pyramids(1, W, H, nlev)
    mid = ctx.config_rectify(_cam(P, c))
    ctx.rectify_build_pyramid(mid, 0, raw, rounding)
    want = ob.build_pyramid(R.undistort(raw, c), nlev, rounding)
    for l, (d, o) in enumerate(zip(ctx.download_pyramid(0), want)):
        assert np.array_equal(d, o), f"level {l}"


def test_batched_form_strides_pitch_and_slot_range(P, ob, ctx):
    c = CAMS["pincushion_tangential"]
    nlev, n_slots, first, n = 3, 6, 2, 3
    stride, pitch = W + 24, (H + 3) * (W + 24) + 40
    rng = np.random.default_rng(12)
    buf = rng.integers(0, 256, n * pitch, dtype=np.uint8)
    raws = [buf[k * pitch:k * pitch + H * stride].reshape(H, stride)[:, :W] for k in range(n)]
    keep, d_ptr = _device_bytes(buf.copy())
    ctx.config_pyramids(n_slots, W, H, nlev)
    filler = np.full((H, W), 201, dtype=np.uint8)
    for s in range(n_slots):
        ctx.build_pyramid(s, filler)
    before = [ctx.download_pyramid(s) for s in range(n_slots)]
    mid = ctx.config_rectify(_cam(P, c), flip_vertical=True)
    ctx.rectify_build_pyramids_dev(mid, first, n, d_ptr, stride, pitch, 1)
    ctx.synchronize()
    for s in range(n_slots):
        got = ctx.download_pyramid(s)
        if first <= s < first + n:
            want = ob.build_pyramid(R.undistort(raws[s - first], c, flip=True), nlev, 1)
            for l in range(nlev):
                assert np.array_equal(got[l], want[l]), (s, l)
        else:
            for l in range(nlev):
                assert np.array_equal(got[l], before[s][l]), f"slot {s} outside the range was written"


def test_every_error_is_rejected_and_writes_nothing(P, ctx):
    import ctypes as C
    L, Eh = ctx.L, P.abi
    c = CAMS["barrel"]
    raw = np.random.default_rng(13).integers(0, 256, (H, W), dtype=np.uint8)
    keep, d_ptr = _device_bytes(np.tile(raw.reshape(-1), 3))
    mid_out = C.c_int(-7)
    # before config_pyramids: no map can be made
    assert L.plsvo_hip_config_rectify(ctx.h, C.byref(_cam(P, c)), 0, C.byref(mid_out)) == Eh.E_STATE and mid_out.value == -7
    ctx.config_pyramids(4, W, H, 3)
    filler = np.full((H, W), 99, dtype=np.uint8)
    for s in range(4):
        ctx.build_pyramid(s, filler)
    before = [ctx.download_pyramid(s) for s in range(4)]
    bad_cams = [dict(c, fx=float("nan")), dict(c, d=[float("inf"), 0, 0, 0]), dict(c, fy=0.0), dict(c, width=W + 2), dict(c, height=H - 2),
                dict(c, width=4000, height=H)]
    for bc in bad_cams:
        assert L.plsvo_hip_config_rectify(ctx.h, C.byref(_cam(P, bc)), 0, C.byref(mid_out)) == Eh.E_INVALID and mid_out.value == -7, bc
    assert L.plsvo_hip_config_rectify(ctx.h, None, 0, C.byref(mid_out)) == Eh.E_INVALID
    mid = ctx.config_rectify(_cam(P, c))
    u8 = raw.ctypes.data_as(Eh.c_u8_p)
    calls = [
        lambda: L.plsvo_hip_rectify_build_pyramid(ctx.h, mid + 1, 0, u8, W, 0),            # unknown map
        lambda: L.plsvo_hip_rectify_build_pyramid(ctx.h, -1, 0, u8, W, 0),
        lambda: L.plsvo_hip_rectify_build_pyramid(ctx.h, MAX_MAPS, 0, u8, W, 0),
        lambda: L.plsvo_hip_rectify_build_pyramid(ctx.h, mid, 4, u8, W, 0),               # slot out of range
        lambda: L.plsvo_hip_rectify_build_pyramid(ctx.h, mid, -1, u8, W, 0),
        lambda: L.plsvo_hip_rectify_build_pyramid(ctx.h, mid, 0, u8, W - 1, 0),           # stride < width
        lambda: L.plsvo_hip_rectify_build_pyramid(ctx.h, mid, 0, None, W, 0),
        lambda: L.plsvo_hip_rectify_build_pyramids_dev(ctx.h, mid, 2, 3, C.c_void_p(d_ptr), W, W * H, 0),   # range past the last slot
        lambda: L.plsvo_hip_rectify_build_pyramids_dev(ctx.h, mid, -1, 2, C.c_void_p(d_ptr), W, W * H, 0),
        lambda: L.plsvo_hip_rectify_build_pyramids_dev(ctx.h, mid, 0, 0, C.c_void_p(d_ptr), W, W * H, 0),
        lambda: L.plsvo_hip_rectify_build_pyramids_dev(ctx.h, mid, 0, 2, None, W, W * H, 0),
        lambda: L.plsvo_hip_rectify_build_pyramids_dev(ctx.h, mid + 3, 0, 2, C.c_void_p(d_ptr), W, W * H, 0),
        lambda: L.plsvo_hip_rectify_build_pyramids_dev(ctx.h, mid, 0, 2, C.c_void_p(d_ptr), 7, W * H, 0),
    ]
    for k, call in enumerate(calls):
        assert call() == Eh.E_INVALID, k
    ctx.synchronize()
    for s in range(4):
        for d, o in zip(ctx.download_pyramid(s), before[s]):
            assert np.array_equal(d, o), f"a rejected call wrote into slot {s}"
    # the pyramid re-configured to another size: the map no longer fits it
    ctx.config_pyramids(4, W // 2, H // 2, 2)
    assert L.plsvo_hip_rectify_build_pyramid(ctx.h, mid, 0, u8, W, 0) == Eh.E_INVALID
    assert L.plsvo_hip_rectify_build_pyramids_dev(ctx.h, mid, 0, 1, C.c_void_p(d_ptr), W, W * H, 0) == Eh.E_INVALID
    ctx.synchronize()
    for s in range(4):
        for l in range(2):
            assert not ctx.download_level(s, l).any(), "a rejected call wrote into the re-configured slab"
    # back at the camera's size the map works again
    ctx.config_pyramids(4, W, H, 3)
    ctx.rectify_build_pyramid(mid, 3, raw)
    assert np.array_equal(ctx.download_level(3, 0), R.undistort(raw, c))
    # a context holds PLSVO_MAX_RECTIFY_MAPS maps
    n_more = MAX_MAPS - 1
    for _ in range(n_more):
        ctx.config_rectify(_cam(P, c))
    assert L.plsvo_hip_config_rectify(ctx.h, C.byref(_cam(P, c)), 0, C.byref(mid_out)) == Eh.E_CAPACITY and mid_out.value == -7


def test_tiled_mirror_is_fresh_after_rectification(P, ob, ctx):
    """The one-wave-per-frame alignment reads the TILED mirror of the slots.  A batch run on slots that rectify_build_pyramids_dev filled
    (over slots whose mirror held other, fresh, images) returns bit for bit what the same batch returns on the NumPy-rectified pyramids
    uploaded: poses, chi2, iterations, culls."""
    nlev, n = 3, 3
    c = dict(CAMS["barrel"], d=[-0.03, 0.01, 0.0002, -0.0001])
    cases = [Hh.make_case(ob, 400 + k, W, H, 24, 10, nlev, 2, 0) for k in range(n)]
    raws = []
    for st, ref, cur, job in cases:
        raws += [ref[0], cur[0]]
    buf = np.concatenate([r.reshape(-1) for r in raws])
    keep, d_ptr = _device_bytes(buf.copy())
    jobs = [P.align_job_from_stream(st, 2, 0, ref_slot=2 * k, cur_slot=2 * k + 1) for k, (st, _, _, _) in enumerate(cases)]

    def run():
        ctx.set_launch_shapes(align_threads=64)
        try:
            return ctx.sparse_align_batch(jobs)
        finally:
            ctx.set_launch_shapes(align_threads=0)

    ctx.config_pyramids(2 * n, W, H, nlev)
    for s in range(2 * n):                       # fresh mirrors of OTHER images
        ctx.build_pyramid(s, raws[(s + 1) % (2 * n)][::-1].copy())
    mid = ctx.config_rectify(_cam(P, c))
    ctx.rectify_build_pyramids_dev(mid, 0, 2 * n, d_ptr, W, W * H, 0)
    got = run()
    for s in range(2 * n):
        ctx.upload_pyramid(s, ob.build_pyramid(R.undistort(raws[s], c), nlev, 0))
    want = run()
    for g, w in zip(got, want):
        assert np.array_equal(g.T, w.T) and g.chi2 == w.chi2 and g.iters_per_level == w.iters_per_level
        assert g.n_meas == w.n_meas and g.status == w.status and np.array_equal(g.seg_alive, w.seg_alive)
    assert any(w.n_meas > 0 for w in want)


def test_full_size_rectification_of_4096_slots(P, ob, ctx):
    """640 x 480, 4096 slots in one batched call: spot checks of the first, a middle and the last slot against the NumPy path"""
    import torch
    Wf, Hf, n, nlev = 640, 480, 4096, 4
    c = dict(width=Wf, height=Hf, fx=458.654 * 640 / 752, fy=457.296, cx=367.215 * 640 / 752, cy=248.375, d=[-0.28340811, 0.07395907, 1.9359e-4, 1.76187114e-5])
    g = torch.Generator(device="cuda").manual_seed(21)
    raw = torch.randint(0, 256, (n, Hf, Wf), dtype=torch.uint8, device="cuda", generator=g)
    ctx.config_pyramids(n, Wf, Hf, nlev)
    mid = ctx.config_rectify(_cam(P, c))
    torch.cuda.synchronize()
    ctx.rectify_build_pyramids_dev(mid, 0, n, raw.data_ptr(), Wf, Wf * Hf, 0)
    ctx.synchronize()
    for s in (0, 1777, n - 1):
        want = ob.build_pyramid(R.undistort(raw[s].cpu().numpy(), c), nlev, 0)
        for l, (d, o) in enumerate(zip(ctx.download_pyramid(s), want)):
            assert np.array_equal(d, o), (s, l)
