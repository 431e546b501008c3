"""Per-level set-up of the alignment kernel's throughput shapes (64 and 128 threads per frame, align_kernels.hip): the slot table and the
64-byte reference records, read back through plsvo_align_fetch_records after a one-level run, equal a NumPy restatement
(tests/align_setup_cases.py) byte for byte -- on inputs planted so that every window placement and every slot-table state occurs, which
the tally test asserts from the restatement alone --, and the whole run on the same jobs follows the oracle, equals itself batched and
single, and equals itself with the launch tail split.  tests/test_emu_align_setup.py runs the small cases on the host emulation build."""
import numpy as np
import pytest

import align_setup_cases as A
import helpers as Hh
import tail_split_cases as C


@pytest.fixture(scope="module")
def scenes(P, ob):
    return [A.make_scene(P, ob, W, H, 8100 + k) for k, (W, H) in enumerate(A.SIZES)]


@pytest.fixture(scope="module")
def long_scene(P, ob):
    return A.make_long_scene(P, ob)


@pytest.fixture(scope="module")
def oracle_runs(ob, scenes):
    """the oracle's run of every small job, levels 3..1, once for both launch shapes"""
    return [{name: ob.sparse_align(mk(), sc["ref"], sc["cur"], max_log=200) for name, mk in sc["makers"].items()} for sc in scenes]


def test_the_planted_inputs_contain_every_placement_and_state(P, ob, scenes):
    """from the restatement alone (no device): every slot count, window placement and slot-table state the set-up can meet is present"""
    for sc in scenes:
        seen = dict(x0=0, pad=0, lastcol=0, tilecol=set(), tilerow=0, corners=set(), counts=set(), hole3_live1=0, dead=0, code_m1=0, n2=0)
        main = sc["makers"]["main"]()
        per_level = {l: A.restate(P, main, l, sc["ref"][l]) for l in A.LEVELS}
        for l, r in per_level.items():
            Wl, Hl = sc["W"] >> l, sc["H"] >> l
            for p in np.nonzero(r["live"] & (r["kind"] == 0))[0]:
                ui, vi = int(np.floor(r["uv"][p, 0])), int(np.floor(r["uv"][p, 1]))
                seen["x0"] += ui - 3 == 0
                seen["pad"] += ui + 4 == Wl            # the border rule's last position: the eighth byte is the padding column
                seen["lastcol"] += ui + 4 == Wl - 1    # the eighth byte is the last column of the image
                if (ui - 3) & 15 >= 13:
                    seen["tilecol"].add((ui - 3) & 15)
                seen["tilerow"] += (vi - 3) & 7 >= 2
                if ui in (3, Wl - 4) and vi in (3, Hl - 4):
                    seen["corners"].add((l, ui == 3, vi == 3))
            assert r["pad_open"].sum() == sum(int(np.floor(u)) + 4 == Wl for u in r["uv"][r["live"], 0])
        seen["hole3_live1"] = int((~per_level[3]["live"][:main.n_pts] & per_level[1]["live"][:main.n_pts]).sum())
        seen["dead"] = int(sum(per_level[1]["first"][s] < 0 for s in (0, 1)))
        seen["code_m1"] = int(per_level[3]["first"][2] < 0 and per_level[2]["first"][2] < 0 and per_level[1]["first"][2] >= 0)
        seen["n2"] = int(per_level[1]["N"][3] == 2)
        for n in A.SLOT_COUNTS:
            seen["counts"] |= {A.restate(P, sc["makers"][f"pts{n}"](), l, sc["ref"][l])["n_slots"] for l in A.LEVELS}
        assert seen["x0"] >= 3 and seen["pad"] >= 3 and seen["lastcol"] >= 3 and seen["tilecol"] == {13, 14, 15} and seen["tilerow"] >= 3, seen
        assert len(seen["corners"]) == 12, seen                     # four corners at each of the three levels
        assert seen["counts"] == set(A.SLOT_COUNTS), seen
        assert seen["hole3_live1"] >= 4 and seen["dead"] == 2 and seen["code_m1"] == 1 and seen["n2"] == 1, seen
        assert per_level[1]["n_slots"] > 129 and (per_level[1]["kind"] == 1).sum() > 0 and not per_level[3]["live"].all()   # samples; holes


def test_the_long_line_case_has_a_line_of_more_than_64_samples(P, ob, long_scene):
    r = A.restate(P, long_scene["makers"]["long"](), 0, long_scene["ref"][0])
    assert r["long_lines"] and int(r["N"].max()) > 64


def check_records(P, ctx, scene, threads):
    """every job of the scene, one level at a time: fetched records and positions against the restatement"""
    A.load_scene(ctx, scene)
    ctx.set_launch_shapes(align_threads=threads)
    checked = 0
    for name, mk in scene["makers"].items():
        for level in scene["levels"]:
            job = mk(level, level)
            want = A.restate(P, job, level, ctx.download_level(0, level))
            ctx.sparse_align(job)
            rec, uv = ctx.align_fetch_records(0, want["n_slots"])
            live = want["live"]
            w = (name, threads, level)
            assert np.array_equal(uv[live].view(np.uint32), want["uv"][live].view(np.uint32)), w          # bit for bit
            keep = np.ones(64, bool)
            closed, opened = live & ~want["pad_open"], live & want["pad_open"]
            assert np.array_equal(rec[closed], want["rec"][closed]), (w, np.nonzero((rec != want["rec"]).any(axis=1) & closed)[0][:8])
            keep[7:56:8] = False                                                                           # the padding column of the seven rows
            assert np.array_equal(rec[opened][:, keep], want["rec"][opened][:, keep]), w
            checked += int(live.sum())
    return checked


@pytest.mark.gpu
@pytest.mark.parametrize("threads", [64, 128])
def test_records_and_positions_equal_the_restatement(P, ob, scenes, threads):
    ctx = P.capi.Context(0)
    try:
        for sc in scenes:
            assert check_records(P, ctx, sc, threads) > 1000
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("threads", [64, 128])
def test_records_of_a_two_pass_level_full_size(P, ob, long_scene, threads):
    ctx = P.capi.Context(0)
    try:
        assert check_records(P, ctx, long_scene, threads) > 200
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("threads", [64, 128])
def test_whole_run_follows_the_oracle_and_batch_equals_single(P, ob, scenes, oracle_runs, threads):
    """levels 3..1 of every job: the per-iteration trace against the oracle's as the border test of tests/test_gpu_parity.py compares it,
    the pose, the segment flags; and the batch of all of a scene's jobs equals the single runs bit for bit"""
    ctx = P.capi.Context(0)
    try:
        ctx.set_launch_shapes(align_threads=threads)
        for sc, runs in zip(scenes, oracle_runs):
            A.load_scene(ctx, sc)
            jobs = {name: mk() for name, mk in sc["makers"].items()}
            ctx.align_set_trace(200)
            single = {}
            for name, job in jobs.items():
                ro, lo = runs[name]
                single[name] = rd = ctx.sparse_align(job)
                ld = ctx.align_fetch_trace(0)
                n, worst = Hh.compare_align_logs(lo, ld)            # asserts n_meas equality per shared iteration
                print(f"{sc['W']}x{sc['H']} T={threads} {name}: {n} shared iterations, worst {worst}")
                assert np.array_equal(rd.seg_alive, ro.seg_alive), name
                if job.n_pts + job.n_seg < 3:
                    # FEWER THAN THREE PATCHES: every pixel of a patch shares the patch's 2 x 6 projection Jacobian, so H has rank 2 per
                    # patch and is singular below three -- the step is whatever the LDLT makes of rounding noise (measured on the one-point
                    # job: the steps of the oracle and of the device differ by 1.4e-3 from the second iteration on, in this build and in
                    # its parent alike), and no summation order but the oracle's own reproduces it.  What IS defined is compared at the
                    # same tolerances: the first iteration, whose pose is the input's -- H, Jres, chi2 -- and n_meas at every iteration.
                    n1, first = Hh.compare_align_logs(lo[:1], ld[:1])
                    assert n1 == 1 and first["H"] < 1e-6 and first["chi2"] < 1e-4, (name, first)
                    continue
                assert n >= 3 and worst["H"] < 1e-6 and worst["chi2"] < 1e-4, (name, worst)
                assert Hh.pose_close(Hh.frame_pose(rd.T, sc["st"]), Hh.frame_pose(ro.T, sc["st"]))[2], name
            ctx.align_set_trace(0)
            batch = ctx.sparse_align_batch(list(jobs.values()))
            again = {name: ctx.sparse_align(job) for name, job in jobs.items()}   # (untraced singles: the same launch path as the batch)
            for (name, _), rb in zip(jobs.items(), batch):
                assert A.same_result(rb, again[name]) and A.same_result(rb, single[name]), name
    finally:
        ctx.close()


@pytest.mark.gpu
def test_tail_split_on_equals_off_on_the_same_jobs(P, ob, scenes):
    """the scene's jobs as one launch of the one-wave-per-frame shape with the split's thresholds lowered (tail_split_cases.make_ctx): every
    frame a coarse and a fine part, and half of them; every reported value equals the unsplit launch's"""
    for sc in scenes:
        jobs = [mk() for mk in sc["makers"].values()]
        for tail in (len(jobs), len(jobs) // 2):
            ctx = C.make_ctx(P, PLSVO_ALIGN_REORDER_MIN=4, PLSVO_ALIGN_TAIL_MIN=4, PLSVO_ALIGN_TAIL_FRAMES=tail)
            try:
                A.load_scene(ctx, sc)
                ctx.set_launch_shapes(align_threads=64)
                C.compare_split_on_off(ctx, jobs, tail, reruns=2)
            finally:
                ctx.close()


@pytest.mark.gpu
def test_fetch_records_rejects_what_it_cannot_serve(P, ob, scenes):
    sc = scenes[1]
    ctx = P.capi.Context(0)
    try:
        A.load_scene(ctx, sc)
        job = sc["makers"]["main"](1, 1)
        buf, uv = np.zeros((4, 64), np.uint8), np.zeros((4, 2), np.float32)
        call = lambda j, n: ctx.L.plsvo_align_fetch_records(ctx.h, j, n, buf.ctypes.data, uv.ctypes.data)
        ctx.align_stage([job])
        assert call(0, 4) == P.abi.E_STATE                         # staged, not run
        ctx.set_launch_shapes(align_threads=64)
        ctx.align_run()
        assert call(0, 4) == 0 and call(1, 4) == P.abi.E_INVALID and call(-1, 4) == P.abi.E_INVALID and call(0, -1) == P.abi.E_INVALID
        assert call(0, 1 << 20) == P.abi.E_INVALID                 # beyond the job's allocation
        assert ctx.L.plsvo_align_fetch_records(ctx.h, 0, 4, None, uv.ctypes.data) == P.abi.E_INVALID
        ctx.set_launch_shapes(align_threads=256)
        ctx.align_run()
        assert call(0, 4) == P.abi.E_STATE                         # a latency shape keeps float rows, not records
    finally:
        ctx.close()
