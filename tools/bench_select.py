"""Cost of the cell selection of the map candidates (plsvo_candidates_select).  Needs an MI355X; prints one JSON object and writes it
to --out.

  The workload of tools/bench_candidates.py (4096 and 32768 streams; 12 keyframes of 200 + 80 features, 10 in the overlap list, 400 + 150
  landmarks, 8 + 4 map candidates, 320 x 240 images, 64 distinct streams repeated), brought under the selection's preconditions: a
  candidate is listed once and belongs to no keyframe.  A frame = run -> resident match -> select on the resident tables; the selection
  changes them, so the frames of a leg are consecutive frames of one map, not repeats of one.  Per shape: the select launch with its
  re-arm (the event bytes, the cells' winner words) by a hipEvent pair on the stream (PLSVO_K_SELECT) around EACH call -- median, min
  and max over --reps calls -- beside the candidate launch and the resident match of the same frames (means), and the select call with
  the wait on the host clock.  With --frame-step-ms (the resident frame step's time per 4096 streams, `frame_chain` of the same
  session's bench.py --full) the launch's share of it is added, with the min - max of the calls.

usage: python tools/bench_select.py [--reps 7] [--streams 4096,32768] [--frame-step-ms X] [--launch-only] [--out profiles/select_bench.json]"""
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


def make_stream(P, rng):
    job, frame = B.make_stream(P, rng)
    for name, n in (("pt", B.N_PT), ("seg", B.N_SEG)):
        cand = job.t[name + "_cand"]
        cand[:] = rng.permutation(n)[:len(cand)]
        lm = job.t["kf_" + name + "_lm"]
        lm[np.isin(lm, cand)] = -1
        job.t[name + "_type"][cand] = P.abi.LM_CANDIDATE
    return job, frame


def leg(P, ctx, pool, n, reps, launch_only=False):
    abi = P.abi
    maps, frames = [pool[i % len(pool)][0] for i in range(n)], [pool[i % len(pool)][1] for i in range(n)]
    ctx.candidates_stage(maps, B.CAM, 30, 40, 8, 3, 10)
    ctx.set_profiling(True)

    def frame():
        ctx.candidates_run(frames)
        ctx.candidates_match()
        ctx.synchronize()
        ctx.reset_profiling()
        t0 = time.perf_counter()
        ctx.candidates_select(max_fts=120, max_fts_segs=100)
        ctx.synchronize()
        t = time.perf_counter() - t0
        ms, k = ctx.kernel_time(abi.K_SELECT)
        assert k == 1
        return ms, t
    frame()                                           # the first frame pays the allocations and the cell orders' upload
    launch, call = zip(*[frame() for _ in range(reps)])
    ctx.reset_profiling()
    ctx.candidates_run(frames); ctx.candidates_match(); ctx.synchronize()
    c_ms, c_n = ctx.kernel_time(abi.K_CANDIDATES)
    m_ms, m_n = ctx.kernel_time(abi.K_MATCH)
    ctx.candidates_select(max_fts=120, max_fts_segs=100)
    ctx.set_profiling(False)
    if launch_only:                                   # a timing build that returns early leaves no result to fetch
        return {"select_launch_ms": {"median": round(float(np.median(launch)), 4), "min": round(min(launch), 4), "max": round(max(launch), 4)}, "frames": reps + 2}
    sel = ctx.candidates_select_fetch()[:len(pool)]
    q = ctx.candidates_fetch_quality()[:len(pool)]
    return {"select_launch_ms": {"median": round(float(np.median(launch)), 4), "min": round(min(launch), 4), "max": round(max(launch), 4)},
            "select_call_and_wait_ms": {"median": round(1e3 * float(np.median(call)), 3), "min": round(1e3 * min(call), 3), "max": round(1e3 * max(call), 3)},
            "candidates_launch_ms": round(c_ms / max(c_n, 1), 4), "match_launch_ms": round(m_ms / max(m_n, 1), 4), "frames": reps + 2,
            "last_frame": {"mean_n_matches": float(np.mean([s["n_matches"] for s in sel])), "mean_n_ls_matches": float(np.mean([s["n_ls_matches"] for s in sel])),
                           "mean_n_trials": float(np.mean([s["n_trials"] for s in sel])),
                           "mean_deleted_landmarks": float(np.mean([(v["pt_type"] == 0).sum() + (v["seg_type"] == 0).sum() for v in q]))}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--streams", default="4096,32768")
    ap.add_argument("--frame-step-ms", type=float, default=None, help="resident frame step per 4096 streams, same session's bench.py --full")
    ap.add_argument("--launch-only", action="store_true", help="time the launch and fetch nothing (phase-timing builds, tools/patches/select_phase_timing.patch)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_select.py: no GPU (a timing needs the MI355X)")
    P = importlib.import_module("pl-svo_amd")
    res = {"what": f"tools/bench_select.py: plsvo_candidates_select on the workload of tools/bench_candidates.py ({B.N_KF} keyframes of {B.F_PT} + {B.F_SEG} features, "
                   f"{B.N_OV} in the overlap list, {B.N_PT} + {B.N_SEG} landmarks); the launch with its re-arm, hipEvent pair per call",
           "device": torch.cuda.get_device_name(0), "gcn_arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", ""), "reps": args.reps, "batched": {}}
    rng = np.random.default_rng(2024)
    pool = [make_stream(P, rng) for _ in range(64)]
    ctx = P.capi.Context(0)
    try:
        ctx.config_pyramids(B.N_KF + 1, B.CAM[4], B.CAM[5], 3)
        for s in range(B.N_KF + 1):
            ctx.build_pyramid(s, B._texture(rng))
        for n in [int(s) for s in args.streams.split(",") if s]:
            res["batched"][str(n)] = leg(P, ctx, pool, n, args.reps, args.launch_only)
    finally:
        ctx.close()
    if args.frame_step_ms is not None:
        res["frame_step_ms_per_4096_streams"] = args.frame_step_ms
        v = res["batched"].get("4096")
        if v:
            v["select_launch_over_frame_step"] = {k: round(x / args.frame_step_ms, 4) for k, x in v["select_launch_ms"].items()}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
