"""Structure optimiser on the device, path by path: structopt_kernel and the diagnostic view of its 3x3 solve (plsvo_structure_solve3: the
kernel's own __device__ ldlt_solve3, one lane per system) against the CPU oracle, BIT FOR BIT with equal_nan, on the directed inputs of
tests/structopt_cases.py.  tests/test_structopt_paths.py shows on the CPU that those inputs reach every pivot order, tie, cutoff and
tolerance branch of the solve and every exit of Point::optimize / LineSeg::optimize, and that the oracle equals an independent restatement
on them.  The device's 3x3 solve implements Eigen 3.2's zero-pivot rule only, so the oracle is pinned to flavour 320 here."""
import ctypes as C

import numpy as np
import pytest

import structopt_cases as sc

pytestmark = pytest.mark.gpu
KEYS = ("pt_iters", "seg_iters", "pt_pos", "seg_spos", "seg_epos")


@pytest.fixture(autouse=True)
def flavour320(ob):
    prev = ob.set_ldlt_flavour(320)
    yield
    ob.set_ldlt_flavour(prev)


@pytest.fixture(scope="module")
def solver_ref(ob):
    """names, A, b and the oracle's x of every solver system (flavour 320); computed once, never modified"""
    prev = ob.set_ldlt_flavour(320)
    names, A, b = sc.solver_arrays()
    x = np.stack([ob.ldlt_solve3(A[i], b[i]) for i in range(len(names))])
    ob.set_ldlt_flavour(prev)
    return names, A, b, x


@pytest.fixture(scope="module")
def geometry_ref(P, ob):
    """the oracle's results of the geometry batch at 5 + 5 iterations; computed once, never modified"""
    prev = ob.set_ldlt_flavour(320)
    r = ob.structure_optimize(P.structopt_job_from_batch(sc.geometry_batch()))
    ob.set_ldlt_flavour(prev)
    return r


def _same(rd, ro, what):
    for k in KEYS:
        bad = [i for i in range(len(ro[k])) if not np.array_equal(rd[k][i], ro[k][i], equal_nan=True)]
        assert not bad, (what, k, bad[:8], rd[k][bad[0]], ro[k][bad[0]])


def test_device_solve_equals_the_oracle_on_every_system(gpu_ctx, solver_ref):
    names, A, b, xo = solver_ref
    xd = gpu_ctx.structure_solve3(A, b)                        # all of them in one launch
    bad = [names[i] for i in range(len(names)) if not np.array_equal(xd[i], xo[i], equal_nan=True)]
    assert not bad, [(n, xd[names.index(n)], xo[names.index(n)]) for n in bad[:6]]


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_device_solve_at_the_wave_edges(gpu_ctx, solver_ref, n):
    """one lane short of a wave, a full wave, one lane into the second; the systems rotate so that every lane position sees another branch"""
    names, A, b, xo = solver_ref
    idx = (np.arange(n) * 7 + n) % len(names)
    xd = gpu_ctx.structure_solve3(A[idx], b[idx])
    assert xd.shape == (n, 3)
    bad = [(int(k), names[i]) for k, i in enumerate(idx) if not np.array_equal(xd[k], xo[i], equal_nan=True)]
    assert not bad, bad[:6]


def test_device_solve_reads_the_lower_triangle_and_checks_its_arguments(P, gpu_ctx, solver_ref):
    names, A, b, xo = solver_ref
    U = np.tril(A) + np.triu(np.full((3, 3), 12345.0), 1)
    assert np.array_equal(gpu_ctx.structure_solve3(U, b), xo, equal_nan=True)
    assert gpu_ctx.structure_solve3(np.zeros((0, 3, 3)), np.zeros((0, 3))).shape == (0, 3)
    dp = C.POINTER(C.c_double)
    x = np.zeros(3)
    assert gpu_ctx.L.plsvo_structure_solve3(gpu_ctx.h, -1, A.ctypes.data_as(dp), b.ctypes.data_as(dp), x.ctypes.data_as(dp)) == P.abi.E_INVALID
    assert b"structure_solve3" in gpu_ctx.L.plsvo_hip_last_error(gpu_ctx.h)
    assert gpu_ctx.L.plsvo_structure_solve3(gpu_ctx.h, 1, None, b.ctypes.data_as(dp), x.ctypes.data_as(dp)) == P.abi.E_INVALID
    assert gpu_ctx.L.plsvo_structure_solve3(gpu_ctx.h, 1, A.ctypes.data_as(dp), b.ctypes.data_as(dp), None) == P.abi.E_INVALID


@pytest.mark.parametrize("n_iter", sc.ITER_VARIANTS, ids=lambda v: "iters%d_%d" % v)
def test_device_equals_the_oracle_on_every_geometry_case(P, ob, gpu_ctx, n_iter):
    job = P.structopt_job_from_batch(sc.geometry_batch(), *n_iter)
    _same(gpu_ctx.structure_optimize(job), ob.structure_optimize(job), n_iter)


@pytest.mark.parametrize("n_pts,n_seg", sc.LAYOUT_SIZES)
def test_device_equals_the_oracle_at_every_batch_layout(P, ob, gpu_ctx, n_pts, n_seg):
    job = P.structopt_job_from_batch(sc.layout(n_pts, n_seg), 5, 4)
    _same(gpu_ctx.structure_optimize(job), ob.structure_optimize(job), (n_pts, n_seg))


def test_device_results_are_the_same_alone_batched_and_permuted(P, gpu_ctx, geometry_ref):
    rb = gpu_ctx.structure_optimize(P.structopt_job_from_batch(sc.geometry_batch()))
    _same(rb, geometry_ref, "batched")
    for i, p in enumerate(sc.POINTS):
        r1 = gpu_ctx.structure_optimize(P.structopt_job_from_batch(sc.batch([p], [])))
        assert r1["pt_iters"][0] == rb["pt_iters"][i] and np.array_equal(r1["pt_pos"][0], rb["pt_pos"][i], equal_nan=True), p["name"]
    for i, g in enumerate(sc.SEGMENTS):
        r1 = gpu_ctx.structure_optimize(P.structopt_job_from_batch(sc.batch([], [g])))
        assert r1["seg_iters"][0] == rb["seg_iters"][i] and np.array_equal(r1["seg_spos"][0], rb["seg_spos"][i], equal_nan=True), g["name"]
        assert np.array_equal(r1["seg_epos"][0], rb["seg_epos"][i], equal_nan=True), g["name"]
    for seed in (5, 6):
        dp, po, so = sc.permuted(sc.POINTS, sc.SEGMENTS, seed)
        rp = gpu_ctx.structure_optimize(P.structopt_job_from_batch(dp))
        _same(rp, dict(pt_iters=rb["pt_iters"][po], pt_pos=rb["pt_pos"][po], seg_iters=rb["seg_iters"][so], seg_spos=rb["seg_spos"][so],
                       seg_epos=rb["seg_epos"][so]), ("permuted", seed))


def test_device_reports_rest_with_a_nan_written_like_the_reference(P, ob, gpu_ctx):
    """b all NaN, A finite, the depth column pivoted first, the other two D entries zeroed: dp = 0 except a NaN on the depth axis.  With the
    depth on world z or y, dp[0] = 0 passes isnan(dp[0]) and norm_max passes over the NaN: one evaluation, the NaN written (reference
    src/feature3D_impl.cpp:65, :88); with the depth on world x the step is rolled back.  Points, and either end of a segment."""
    pts = [sc.NAMED[n] for n in ("shallow_f2_zero", "shallow_y_f2_zero", "shallow_nan_bearing", "shallow_x_f2_zero")]
    segs = [g for g in sc.SEGMENTS if g["name"] in ("shallow_f2_zero+off_axis_z", "off_axis_z+shallow_f2_zero", "shallow_f2_zero+shallow_nan_bearing")]
    assert len(segs) == 3
    job = P.structopt_job_from_batch(sc.batch(pts, segs))
    rd, ro = gpu_ctx.structure_optimize(job), ob.structure_optimize(job)
    _same(rd, ro, "nan written at rest")
    assert list(rd["pt_iters"]) == [1, 1, 1, 1] and list(rd["seg_iters"]) == [1, 1, 1]
    assert np.array_equal(np.isnan(rd["pt_pos"]), [[False, False, True], [False, True, False], [False, False, True], [False, False, False]])
    assert np.array_equal(rd["pt_pos"][3], pts[3]["pos"])
    assert [bool(np.isnan(rd["seg_spos"][k]).any()) for k in range(3)] == [True, False, True]
    assert [bool(np.isnan(rd["seg_epos"][k]).any()) for k in range(3)] == [False, True, True]


def test_null_optional_outputs(P, gpu_ctx, geometry_ref):
    """any output pointer may be NULL: the others are written as before, and nothing else is touched"""
    job = P.structopt_job_from_batch(sc.geometry_batch())
    for drop in KEYS + (KEYS,):
        drop = (drop,) if isinstance(drop, str) else drop
        out, bufs = job.make_out()
        for k in bufs:
            bufs[k][...] = -7
        for k in drop:
            setattr(out, k, None)
        assert gpu_ctx.L.plsvo_structure_optimize(gpu_ctx.h, C.byref(job.c), C.byref(out)) == 0
        for k in KEYS:
            if k in drop:
                assert np.all(bufs[k] == -7), (drop, k)
            else:
                assert np.array_equal(bufs[k][:len(geometry_ref[k])], geometry_ref[k], equal_nan=True), (drop, k)


def test_malformed_offset_tables_are_rejected_before_any_launch(P, gpu_ctx, geometry_ref):
    """pt_obs_off / seg_obs_off that do not start at 0, hold a negative entry or decrease: PLSVO_E_INVALID from the argument check (nothing
    is uploaded or launched; the last entry of each of these tables is the valid one, which is all the check used to look at)"""
    d = sc.geometry_batch()

    def rejected(key, edit):
        bad = dict(d)
        bad[key] = d[key].copy()
        edit(bad[key])
        job = P.structopt_job_from_batch(bad)
        out, bufs = job.make_out()
        for k in bufs:
            bufs[k][...] = -7
        rc = gpu_ctx.L.plsvo_structure_optimize(gpu_ctx.h, C.byref(job.c), C.byref(out))
        msg = (gpu_ctx.L.plsvo_hip_last_error(gpu_ctx.h) or b"").decode()
        assert rc == P.abi.E_INVALID and "structure_optimize" in msg and "offsets" in msg, (key, rc, msg)
        assert all(np.all(bufs[k] == -7) for k in bufs), key

    for key in ("pt_obs_off", "seg_obs_off"):
        n = len(d[key]) - 1
        assert n >= 8 and d[key][3] > 0
        rejected(key, lambda o: o.__setitem__(0, 1))                       # does not start at 0
        rejected(key, lambda o: o.__setitem__(0, -1))                      # negative first entry
        rejected(key, lambda o: o.__setitem__(3, -2))                      # negative entry inside (also a decrease)
        rejected(key, lambda o: o.__setitem__(3, int(o[-1]) + 5))          # rises past the end, then decreases
        rejected(key, lambda o: o.__setitem__(n - 1, int(o[n - 2]) - 1))   # decreases by one near the end
        rejected(key, lambda o: o.__setitem__(n, int(o[n - 1]) - 1))       # the last entry below the one before it
    # the context is still usable, and a table of equal entries (landmarks without observations) is fine
    _same(gpu_ctx.structure_optimize(P.structopt_job_from_batch(d)), geometry_ref, "after the rejections")
    e = dict(d, pt_obs_off=np.zeros_like(d["pt_obs_off"]), seg_obs_off=np.zeros_like(d["seg_obs_off"]))
    r = gpu_ctx.structure_optimize(P.structopt_job_from_batch(e))
    assert np.array_equal(r["pt_pos"], d["pt_pos"], equal_nan=True) and np.all(r["pt_iters"] == 1) and np.all(r["seg_iters"] == 1)
