"""Cases shared by tests/test_gpu_align_setup.py (MI355X) and tests/test_emu_align_setup.py (the same file run against the host
emulation build): the per-level set-up of the alignment kernel's throughput shapes (64 and 128 threads per frame, align_kernels.hip) --
the slot table and the 64-byte reference records -- against a NumPy restatement built from the job and the host's slot layout, with
inputs planted so that every placement of a record's window and every state of a slot-table entry occurs.

The restatement (restate below): a point's position at a level is (float)(px * 2^-level); it is live when 3 <= u < W - 3 and
3 <= v < H - 3 on the level's image.  A segment with a slot code owns N slots from its first one; sample n sits at the start point
times 2^-level plus n accumulated steps of (end - start) * 2^-level / (N - 1), in double, rounded to float per sample.  The record of a
live slot is seven rows of the eight reference-image bytes [vi - 3 + k][ui - 3 .. ui + 4], ui = floor(u), vi = floor(v), then the
fractions u - ui and v - vi as floats.  The border rule allows ui + 3 = W - 1, so the eighth byte of a row, column ui + 4, can be column
W: a byte beyond the image that no patch row reads (the patch is 7 x 7) and that the two image layouts pad differently; for such a
slot the restatement leaves the eighth byte of every row open (pad_open) and fixes the other 57 bytes and the fractions."""
import numpy as np

LEVELS = (3, 2, 1)
SIZES = ((326, 246), (320, 240))          # a width that is no multiple of 16 (partial tiles at every level) and one that is
SLOT_COUNTS = (1, 63, 64, 65, 128, 129)
N_PTS_MAIN = 128                          # a multiple of 64: the segments start at slot 128 whichever alignment the staged batch packs them with


def planted_positions(W, H, level):
    """(u, v) on the level's image: the four corners of the border rule (the first two with ui - 3 = 0, the second and fourth with
    ui + 4 = W: the padding column), ui + 4 = W - 1 (the last column of the image), and (ui - 3) & 15 = 13, 14, 15 (the window spans two
    tile columns) with (vi - 3) & 7 = 2 (it spans two tile rows)"""
    Wl, Hl = W >> level, H >> level
    out = [(3.25, 3.5), (Wl - 4 + 0.25, 3.5), (3.25, Hl - 4 + 0.5), (Wl - 4 + 0.25, Hl - 4 + 0.5), (Wl - 5 + 0.75, Hl // 2 + 0.125)]
    out += [(16 + 13 + 3 + k + 0.375, 13 + 0.625) for k in range(3)]
    return out


def make_scene(P, ob, W, H, seed):
    """one reference / current image pair and its jobs: 'main' (128 points, the first 24 planted; 12 segments: two dead on entry, one
    whose start point is inside the border at levels 3 and 2, one with N = 2 samples at level 1) and one job of n points and no
    segment for every n in SLOT_COUNTS (n_slots = n at every level)"""
    S = P.synth
    st = S.make_align_stream(seed, W, H, 129, 12, max_level=3, motion_scale=0.4)
    imgs = S.render_streams([st]).numpy()
    ref, cur = ob.build_pyramid(imgs[0, 0], 4), ob.build_pyramid(imgs[0, 1], 4)

    def lift(px):   # the stream's own lift: the 3-D point (reference frame) of a reference pixel on the scene's plane
        _, rays = S._bearing(st.cam, np.asarray(px, float).reshape(-1, 2))
        return S._on_plane(st.plane_n, st.plane_d, rays)

    px = st.pt_px.copy()
    k = 1                                                   # (point 0 stays an ordinary interior point: the one-point job)
    for level in LEVELS:
        for (u, v) in planted_positions(W, H, level):
            px[k] = [u * (1 << level), v * (1 << level)]    # exact: the level's position is this times a power of two
            k += 1
    xyz = lift(px)
    spx, epx = st.seg_spx.copy(), st.seg_epx.copy()
    spx[2] = [9.0, 100.0]                                   # int(9 / 8) = 1, int(9 / 4) = 2: no slots at levels 3 and 2; 4 at level 1: slots
    spx[3], epx[3] = [100.0, 60.0], [156.0, 60.0]           # horizontal, 56 px: n0 = 3 samples, N = 1 + 2 / 2 = 2 at level 1 (1 above)
    alive_in = np.ones(12, np.uint8)
    alive_in[[0, 1]] = 0
    seg_p, seg_q = lift(spx), lift(epx)
    seg_len = np.linalg.norm(epx - spx, axis=1)

    def job(n_pts, with_segs, hi=3, lo=1):
        sl = slice(0, 12 if with_segs else 0)
        return P.abi.AlignJob(st.cam, hi, lo, 30, 1e-6, st.T_init, px[:n_pts], xyz[:n_pts], spx[sl], epx[sl], seg_len[sl], seg_p[sl], seg_q[sl],
                              seg_alive_in=alive_in[sl] if with_segs else None)
    makers = {"main": lambda hi=3, lo=1: job(N_PTS_MAIN, True, hi, lo)}
    for n in SLOT_COUNTS:
        makers[f"pts{n}"] = (lambda hi=3, lo=1, n=n: job(n, False, hi, lo))
    return dict(W=W, H=H, st=st, ref=ref, cur=cur, makers=makers, levels=LEVELS, n_levels=4)


def make_long_scene(P, ob):
    """the 1920 x 1080 case of tests/test_gpu_tail_split.py with 64 points: lines of more than 64 samples at level 0 (a two-pass level)"""
    S = P.synth
    W, H = 1920, 1080
    st = S.make_align_stream(41, W, H, 64, 6, max_level=1, motion_scale=0.5, seg_len_range=(1150.0, 1800.0))
    imgs = S.render_streams([st]).numpy()
    ref, cur = ob.build_pyramid(imgs[0, 0], 3), ob.build_pyramid(imgs[0, 1], 3)
    makers = {"long": lambda hi=1, lo=0: P.align_job_from_stream(st, hi, lo, n_iter=10)}
    return dict(W=W, H=H, st=st, ref=ref, cur=cur, makers=makers, levels=(1, 0), n_levels=3)


def restate(P, job, level, ref_level):
    """the slot table and the records of one job at one level from the job's arrays, the host's slot layout and the reference image of
    the level: dict(n_slots, live [n], kind [n] (0 point, 1 segment sample), uv float32 [n, 2], rec uint8 [n, 64], pad_open [n], first, N)"""
    first, N, n_slots, long_lines, _ = P.capi.align_slot_layout(job, level)
    Hl, Wl = ref_level.shape
    assert (Wl, Hl) == (int(job.c.cam.width) >> level, int(job.c.cam.height) >> level)
    scale = 1.0 / (1 << level)
    live = np.zeros(n_slots, bool)
    kind = np.zeros(n_slots, np.int8)
    uv = np.zeros((n_slots, 2), np.float32)
    for f in range(job.n_pts):
        u, v = np.float32(job.pt_px[f, 0] * scale), np.float32(job.pt_px[f, 1] * scale)
        uv[f] = (u, v)
        live[f] = bool(u >= np.float32(3.0) and v >= np.float32(3.0) and u < np.float32(Wl - 3) and v < np.float32(Hl - 3))
    with np.errstate(divide="ignore", invalid="ignore"):
        for s in range(job.n_seg):
            if first[s] < 0:
                continue
            n = int(N[s])
            sx, sy = job.seg_spx[s]
            incx = np.float64(job.seg_epx[s, 0] - sx) * scale / np.float64(n - 1)
            incy = np.float64(job.seg_epx[s, 1] - sy) * scale / np.float64(n - 1)
            x, y = np.float64(sx * scale), np.float64(sy * scale)
            for k in range(n):
                p = int(first[s]) + k
                uv[p] = (np.float32(x), np.float32(y))
                live[p], kind[p] = True, 1
                x, y = x + incx, y + incy
    rec = np.zeros((n_slots, 64), np.uint8)
    pad_open = np.zeros(n_slots, bool)
    for p in np.nonzero(live)[0]:
        u, v = uv[p]
        ui, vi = int(np.floor(u)), int(np.floor(v))
        rows = np.zeros((7, 8), np.uint8)
        width = 8 if ui + 4 <= Wl - 1 else 7
        pad_open[p] = width == 7
        rows[:, :width] = ref_level[vi - 3:vi + 4, ui - 3:ui - 3 + width]
        rec[p, :56] = rows.reshape(-1)
        rec[p, 56:] = np.array([u - np.floor(u), v - np.floor(v)], np.float32).view(np.uint8)
    return dict(n_slots=n_slots, live=live, kind=kind, uv=uv, rec=rec, pad_open=pad_open, first=first, N=N, long_lines=long_lines)


def load_scene(ctx, scene):
    ctx.config_pyramids(2, scene["W"], scene["H"], scene["n_levels"])
    ctx.upload_pyramid(0, scene["ref"])
    ctx.upload_pyramid(1, scene["cur"])


def same_result(a, b):
    """two alignment results of one job, bit for bit (bytes: NaN payloads and signed zeros count)"""
    return (a.T.tobytes() == b.T.tobytes() and a.H.tobytes() == b.H.tobytes() and np.float64(a.chi2).tobytes() == np.float64(b.chi2).tobytes()
            and a.n_meas == b.n_meas and a.iters_per_level == b.iters_per_level and a.status == b.status and np.array_equal(a.seg_alive, b.seg_alive))
