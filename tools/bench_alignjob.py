"""Cost of building the next frame's alignment job on the device (plsvo_candidates_align_build / _compose) beside the
host-fed path it replaces, and what the capacity layout of the built batch costs the alignment launch.  Needs an MI355X; prints one JSON
object and writes it to --out.

  The resident table sizes of tools/bench_structsel.py (12 keyframes of 200 + 80 features, 400 + 150 landmarks, 64 distinct streams
  repeated), 4096 streams, the resident frame step's shape.  A frame = run -> a constructed match that finds every filed candidate at its
  projection -> select -> resident pose optimisation: the frame step's hundred or so features per stream.  Per frame, in alternating order:
    resident   build_launch     map_align_job_kernel by its hipEvent pair (PLSVO_K_ALIGN_INIT; the counting sort of the launch order follows it)
               build_call       plsvo_candidates_align_build, records included, enqueue to completion on the host clock
               compose_launch   map_align_pose_kernel by its hipEvent pair
    host path  select_fetch     plsvo_candidates_select_fetch
               pose_fetch       plsvo_candidates_pose_fetch (poses and keep masks)
               numpy_job        f * ||pos - ref_pos|| per kept feature, the segment lengths, T0: NumPy, per stream, on the caller's positions
               align_stage      plsvo_align_stage (the slot layout per job and level on one host thread, one upload)
               host_total       the four together
    launch     align_built      the alignment launch of the built batch (PLSVO_K_ALIGN_LEVEL), its first launch: the initial order
               align_staged     the same launch of a host-staged batch of IDENTICAL content (the built jobs fetched back and staged)
  The whole leg runs for slot_cap = the batch's true maximum and for a generous slot_cap (--slot-cap), and once more in a context created
  with PLSVO_ALIGN_NO_LPT=1, where both batches launch in batch order (order = nullptr).  align_lds_bytes / align_threads: what pick_align_config
  asks for, from the library (plsvo_align_launch_shape), for each of the two batches.
  Reported as mean (min - max) over --reps frames; one more frame runs first and is left out (it pays the allocations).

usage: python tools/bench_alignjob.py [--reps 6] [--streams 4096] [--slot-cap 1024] [--out profiles/alignjob_bench.json]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench_candidates as B   # noqa: E402
import bench_insert as BI      # noqa: E402
from bench_structsel import found_everywhere   # noqa: E402

MAX_LEVEL, MIN_LEVEL, N_PYR = 3, 1, 4
CAP_PTS, CAP_SEG = 128, 112


def stats(v, scale=1.0, digits=3):
    return {"mean": round(scale * float(np.mean(v)), digits), "min": round(scale * min(v), digits), "max": round(scale * max(v), digits)}


def numpy_job(P, m, sel, po, ref_slot, cur_slot):
    """the job the harness gathers on the host (sequence.py, step 1) from the fetched selection, the fetched masks and its own positions"""
    cam, t = B.CAM, m.t
    T_inv = P.synth.se3_inv(po.T)
    ref = T_inv[4:]

    def scaled(px, pos):
        r = np.stack([(px[:, 0] - cam[2]) / cam[0], (px[:, 1] - cam[3]) / cam[1], np.ones(len(px))], axis=1)
        return r / np.linalg.norm(r, axis=1, keepdims=True) * np.linalg.norm(pos - ref, axis=1)[:, None]
    pk, sk = po.pt_keep.astype(bool), po.seg_keep.astype(bool)
    px, lm = sel["pt_px"][pk], sel["pt_lm"][pk]
    s4, slm = sel["seg_px"].reshape(-1, 4), sel["seg_lm"]
    return P.abi.AlignJob(cam, MAX_LEVEL, MIN_LEVEL, 30, 1e-6, P.synth.se3_mul(po.T, T_inv), px, scaled(px, t["pt_pos"][lm]), s4[:, :2], s4[:, 2:],
                          np.linalg.norm(s4[:, 2:] - s4[:, :2], axis=1), scaled(s4[:, :2], t["seg_spos"][slm]) * sk[:, None], scaled(s4[:, 2:], t["seg_epos"][slm]) * sk[:, None],
                          sk.astype(np.uint8), ref_slot=ref_slot, cur_slot=cur_slot)


def leg(P, ctx, pool, n, reps, slot_cap):
    abi = P.abi
    maps, frames = [pool[i % len(pool)][0] for i in range(n)], [pool[i % len(pool)][1] for i in range(n)]
    ctx.candidates_reserve()
    ctx.candidates_stage(maps, B.CAM, 30, 40, 8, 3, 10)
    ctx.candidates_align_reserve(MAX_LEVEL, MIN_LEVEL, CAP_PTS, CAP_SEG, slot_cap)
    ctx.set_profiling(True)
    names = ("build_launch", "build_call", "compose_launch", "select_fetch", "pose_fetch", "numpy_job", "align_stage", "host_total", "align_built", "align_staged")
    res = {k: [] for k in names}
    jobs_dev = [dict(ref_slot=B.N_KF - 1, cur_slot=B.N_KF)] * n
    info = {}

    def launch_ms(family, count):
        ms, cnt = ctx.kernel_time(family)
        assert cnt == count, (family, cnt, count)
        return ms

    def run_ms():
        ctx.reset_profiling()
        ctx.align_run()
        ctx.synchronize()
        return launch_ms(abi.K_ALIGN_LEVEL, 1)

    def resident():
        ctx.reset_profiling()
        t0 = time.perf_counter()
        ctx.candidates_align_build(jobs_dev)
        ctx.synchronize()
        res["build_call"].append(time.perf_counter() - t0)
        res["build_launch"].append(launch_ms(abi.K_ALIGN_INIT, 1))
        info["shape_built"] = ctx.align_launch_shape()
        res["align_built"].append(run_ms())
        ctx.reset_profiling()
        ctx.candidates_align_compose()
        ctx.synchronize()
        res["compose_launch"].append(launch_ms(abi.K_ALIGN_INIT, 1))

    def host():
        t0 = time.perf_counter()
        sels = ctx.candidates_select_fetch()
        t1 = time.perf_counter()
        po = ctx.candidates_pose_fetch([(s["n_matches"], s["n_ls_matches"]) for s in sels])
        t2 = time.perf_counter()
        jobs = [numpy_job(P, m, s, p, B.N_KF - 1, B.N_KF) for m, s, p in zip(maps, sels, po)]
        t3 = time.perf_counter()
        ctx.align_stage(jobs)
        ctx.synchronize()
        t4 = time.perf_counter()
        for name, dt in (("select_fetch", t1 - t0), ("pose_fetch", t2 - t1), ("numpy_job", t3 - t2), ("align_stage", t4 - t3), ("host_total", t4 - t0)):
            res[name].append(dt)

    def staged_identical():
        """the built jobs of the distinct streams fetched back and staged by the host: the same content in the staged layout"""
        ctx.candidates_align_build(jobs_dev)
        got = [ctx.candidates_align_fetch_job(k) for k in range(min(n, len(pool)))]
        info["max_slots"] = int(max(int(g["n_slots"].max()) for g in got))
        info["features"] = {"points": round(float(np.mean([g["n_pts"] for g in got])), 1), "segments": round(float(np.mean([g["n_seg"] for g in got])), 1),
                            "segments_alive": round(float(np.mean([int(g["seg_alive_in"].sum()) for g in got])), 1),
                            "patches_over_levels": round(float(np.mean([g["n_patches"] for g in got])), 1)}
        info["no_room"] = int(sum(r["status"] != abi.ALIGN_JOB_OK for r in ctx.candidates_align_fetch()))
        host_jobs = [abi.AlignJob(B.CAM, MAX_LEVEL, MIN_LEVEL, 30, 1e-6, g["T0"], g["pt_px"], g["pt_xyz_ref"], g["seg_spx"], g["seg_epx"], g["seg_len"], g["seg_p_ref"],
                                  g["seg_q_ref"], g["seg_alive_in"], ref_slot=B.N_KF - 1, cur_slot=B.N_KF) for g in got]
        ctx.align_stage([host_jobs[i % len(host_jobs)] for i in range(n)])
        info["shape_staged"] = ctx.align_launch_shape()
        return run_ms()

    for k in range(reps + 1):                          # the first frame pays the allocations and is left out
        ctx.candidates_run(frames)
        ctx.candidates_set_match([found_everywhere(c) for c in ctx.candidates_fetch()])
        ctx.candidates_select(max_fts=120, max_fts_segs=100)
        ctx.candidates_pose_optimize()
        ctx.synchronize()
        for which in (("resident", "host", "staged") if k % 2 else ("staged", "host", "resident")):
            if which == "resident":
                resident()
            elif which == "host":
                host()
            else:
                res["align_staged"].append(staged_identical())
        print(f"bench_alignjob: slot_cap {slot_cap}, {n} streams, frame {k} of {reps}", file=sys.stderr, flush=True)
    ctx.set_profiling(False)
    out = {name + "_ms": stats(v[1:], 1.0 if name.endswith("_launch") or name.startswith("align_b") or name == "align_staged" else 1e3) for name, v in res.items()}
    (t, lds_built), (t_staged, lds_staged) = info.pop("shape_built"), info.pop("shape_staged")
    assert t == t_staged
    out.update(info)
    out["slot_cap"] = slot_cap
    out["align_threads"] = t
    out["align_lds_bytes"] = {"built": lds_built, "staged": lds_staged}
    out["built_inside_staged_spread"] = bool(out["align_staged_ms"]["min"] <= out["align_built_ms"]["mean"] <= out["align_staged_ms"]["max"])
    out["frames"] = reps
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--slot-cap", type=int, default=1024)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_alignjob.py: no GPU (a timing needs the MI355X)")
    P = importlib.import_module("pl-svo_amd")
    res = {"what": f"tools/bench_alignjob.py: the next frame's alignment job built on the device on the workload of tools/bench_structsel.py ({B.N_KF} keyframes of "
                   f"{B.F_PT} + {B.F_SEG} features, {B.N_PT} + {B.N_SEG} landmarks), levels {MAX_LEVEL}..{MIN_LEVEL}, cap_pts {CAP_PTS}, cap_seg {CAP_SEG}; beside it select_fetch + "
                   "pose_fetch + the NumPy job + plsvo_align_stage",
           "device": torch.cuda.get_device_name(0), "gcn_arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", ""), "reps": args.reps, "streams": args.streams}
    rng = np.random.default_rng(2024)
    pool = [BI.make_stream(P, rng) for _ in range(64)]
    textures = [B._texture(rng) for _ in range(B.N_KF + 1)]

    def context(no_lpt=False):
        old = os.environ.pop("PLSVO_ALIGN_NO_LPT", None)
        if no_lpt:
            os.environ["PLSVO_ALIGN_NO_LPT"] = "1"
        try:
            c = P.capi.Context(0)
        finally:
            os.environ.pop("PLSVO_ALIGN_NO_LPT", None)
            if old is not None:
                os.environ["PLSVO_ALIGN_NO_LPT"] = old
        c.config_pyramids(B.N_KF + 1, B.CAM[4], B.CAM[5], N_PYR)
        for s, img in enumerate(textures):
            c.build_pyramid(s, img)
        return c
    ctx = context()
    try:
        cus = ctx.device_info()[1]
        probe = leg(P, ctx, pool, min(args.streams, max(192, cus // 2 + 64)), 1, args.slot_cap)      # the batch's true maximum under the large batch's layout (the streams repeat: the first 64 hold every one)
        true_max = probe["max_slots"]
        res["slot_cap_true_max"] = leg(P, ctx, pool, args.streams, args.reps, true_max)
        res["slot_cap_generous"] = leg(P, ctx, pool, args.streams, args.reps, args.slot_cap)
    finally:
        ctx.close()
    ctx = context(no_lpt=True)
    try:
        res["batch_order_slot_cap_true_max"] = leg(P, ctx, pool, args.streams, args.reps, true_max)
    finally:
        ctx.close()
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
