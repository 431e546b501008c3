"""Cost of appending new candidate landmarks to the resident map tables (plsvo_candidates_add) beside the restage it replaces.  Needs an
MI355X; prints one JSON object and writes it to --out.

  The workload of tools/bench_insert.py (tools/bench_select.py's 12 keyframes of 200 + 80 features, 400 + 150 landmarks, 64 distinct
  streams repeated, under the insertion's preconditions).  Each step adds a fixed number of points and segments to EVERY stream (--adds
  "points,segments"; several shapes separated by ';'), each observed in one keyframe of the table.  Per shape, as median (min - max) of
  --reps consecutive adds behind one untimed first add (which pays the allocations): the launch by a hipEvent pair on the stream
  (PLSVO_K_NEWCAND), and the whole call of the C entry point -- its checks, packing the records into one blob, their copy, the launch --
  plus a wait on the host clock; the Python binding's own conversion of 15 arrays per stream into ctypes (candidates_add_records) is timed
  apart, because a C or C++ host does not pay it.  Beside them, in
  the same session, the restage of the SAME tables that the add replaces: plsvo_candidates_fetch_quality, plsvo_candidates_stage,
  plsvo_candidates_set_quality through the same binding on the host clock (the tables are fetched and packed into jobs outside the timed
  region).  With --frame-step-ms (the resident frame step per 4096 streams, `frame_chain` of the same session's bench.py --full) the add's
  share of it is added.

usage: python tools/bench_newcand.py [--reps 7] [--streams 4096] [--adds "2,1;16,8"] [--frame-step-ms X] [--out profiles/newcand_bench.json]"""
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


def make_records(rng, n_pt, n_seg):
    """the records of one stream's new landmarks: positions in front of the camera, one observation each in a keyframe of the table"""
    w, h = B.CAM[4], B.CAM[5]

    def obs(k):
        px = np.stack([rng.uniform(10, w - 10, k), rng.uniform(10, h - 10, k)], 1)
        f = np.stack([(px[:, 0] - B.CAM[2]) / B.CAM[0], (px[:, 1] - B.CAM[3]) / B.CAM[1], np.ones(k)], 1)
        return px, f / np.linalg.norm(f, axis=1, keepdims=True)
    d = {}
    if n_pt:
        px, f = obs(n_pt)
        d.update(pt_pos=f * rng.uniform(2.0, 6.0, (n_pt, 1)), pt_obs_kf=rng.integers(0, B.N_KF, n_pt), pt_obs_px=px, pt_obs_f=f, pt_obs_level=rng.integers(0, 3, n_pt),
                 pt_obs_type=np.zeros(n_pt, np.uint8), pt_obs_grad=np.tile([1.0, 0.0], (n_pt, 1)))
    if n_seg:
        (spx, sf), (epx, ef) = obs(n_seg), obs(n_seg)
        z = rng.uniform(2.0, 6.0, (n_seg, 1))
        d.update(seg_spos=sf * z, seg_epos=ef * z, seg_obs_kf=rng.integers(0, B.N_KF, n_seg), seg_obs_spx=spx, seg_obs_epx=epx, seg_obs_sf=sf, seg_obs_ef=ef,
                 seg_obs_level=rng.integers(0, 3, n_seg))
    return d or None


def leg(P, ctx, pool, n, reps, n_pt, n_seg, rng):
    abi = P.abi
    maps = [pool[i % len(pool)][0] for i in range(n)]
    steps = reps + 1
    ctx.candidates_reserve(extra_pt_obs=steps * n_pt, extra_seg_obs=steps * n_seg)
    ctx.candidates_reserve_landmarks(extra_pt=steps * n_pt, extra_seg=steps * n_seg)
    ctx.candidates_stage(maps, B.CAM, 30, 40, 8, 3, 10)
    recs = [make_records(rng, n_pt, n_seg) for _ in pool]
    new = [recs[i % len(recs)] for i in range(n)]
    ctx.set_profiling(True)

    def add():
        ctx.synchronize()
        ctx.reset_profiling()
        t0 = time.perf_counter()
        batch = ctx.candidates_add_records(new)       # the Python binding's own work: 15 arrays per stream into ctypes
        t1 = time.perf_counter()
        ctx.candidates_add(batch)                     # the C entry point: checks, packing into one blob, its copy, the launch
        ctx.synchronize()
        t2 = time.perf_counter()
        ms, k = ctx.kernel_time(abi.K_NEWCAND)
        assert k == 1
        return ms, t2 - t1, t1 - t0
    add()                                             # the first add pays the allocations
    launch, call, pack = zip(*[add() for _ in range(reps)])
    ctx.set_profiling(False)
    rep = ctx.candidates_add_fetch()[:len(pool)]
    # the restage of the same tables
    tables = ctx.candidates_fetch_map(streams=range(len(pool)))[:len(pool)]      # (the replicas hold the same tables)
    jobs = [abi.CandidateMapJob(**t) for t in tables]
    again = [jobs[i % len(jobs)] for i in range(n)]
    ctx.candidates_reserve()
    ctx.candidates_reserve_landmarks()
    restage = []
    for _ in range(reps):
        ctx.synchronize()
        t0 = time.perf_counter()
        q = ctx.candidates_fetch_quality()
        ctx.candidates_stage(again, B.CAM, 30, 40, 8, 3, 10)
        ctx.candidates_set_quality([dict(pt_n_failed=v["pt_n_failed"], pt_n_succeeded=v["pt_n_succeeded"], seg_n_failed=v["seg_n_failed"], seg_n_succeeded=v["seg_n_succeeded"]) for v in q])
        ctx.synchronize()
        restage.append(time.perf_counter() - t0)
    bytes_per_stream = n_pt * (24 + 4 + 16 + 24 + 4 + 1 + 16) + n_seg * (48 + 4 + 32 + 48 + 4)
    return {"added_per_stream": {"points": n_pt, "segments": n_seg}, "record_bytes_per_stream": bytes_per_stream, "adds": steps,
            "add_launch_ms": BI.stats(launch), "add_call_and_wait_ms": BI.stats(call, 1e3, 3), "binding_pack_ms": BI.stats(pack, 1e3, 2), "restage_ms": BI.stats(restage, 1e3, 2),
            "restage_over_add_call": round(float(np.median(restage)) / float(np.median(call)), 1),
            "last_add": {f: float(np.mean([r[f] for r in rep])) for f in ("first_pt", "first_seg", "n_pt", "n_seg", "n_pt_cand", "n_seg_cand", "n_pt_obs", "n_seg_obs")}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--adds", default="2,1", help='"points,segments" added per stream and step; several shapes separated by ;')
    ap.add_argument("--frame-step-ms", type=float, default=None, help="resident frame step per 4096 streams, same session's bench.py --full")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_newcand.py: no GPU (a timing needs the MI355X)")
    P = importlib.import_module("pl-svo_amd")
    res = {"what": f"tools/bench_newcand.py: plsvo_candidates_add on the workload of tools/bench_insert.py ({B.N_KF} keyframes of {B.F_PT} + {B.F_SEG} features, "
                   f"{B.N_PT} + {B.N_SEG} landmarks), a fixed number of new landmarks per stream and step; beside it the restage of the same tables",
           "device": torch.cuda.get_device_name(0), "gcn_arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", ""), "reps": args.reps,
           "streams": args.streams, "shapes": []}
    rng = np.random.default_rng(2025)
    pool = [BI.make_stream(P, rng) for _ in range(64)]
    ctx = P.capi.Context(0)
    try:
        for shape in [s for s in args.adds.split(";") if s]:
            n_pt, n_seg = [int(v) for v in shape.split(",")]
            res["shapes"].append(leg(P, ctx, pool, args.streams, args.reps, n_pt, n_seg, rng))
    finally:
        ctx.close()
    if args.frame_step_ms is not None:
        res["frame_step_ms_per_4096_streams"] = args.frame_step_ms
        if args.streams == 4096:
            for v in res["shapes"]:
                v["add_call_over_frame_step"] = {k: round(x / args.frame_step_ms, 4) for k, x in v["add_call_and_wait_ms"].items()}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
