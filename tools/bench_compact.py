"""Cost of the compaction of the resident map tables (plsvo_candidates_compact) beside the restage it replaces.  Needs an MI355X; prints
one JSON object and writes it to --out.

  The workload of tools/bench_insert.py (12 keyframes of 200 + 80 features, 400 + 150 landmarks, 64 distinct streams repeated) with about a
  quarter of the landmark rows deleted the way the selection and the insertion leave them: TYPE_DELETED, no keyframe feature, no candidate
  entry, the observation list left over.  An event = the tables staged afresh (not timed), then the compaction.  Per shape, as median
  (min - max) of --reps consecutive events behind an untimed first one: the launch by a hipEvent pair on the stream (PLSVO_K_INSERT) and
  the whole call with its read-back and the wait on the host clock.  Beside them, in the same session and on the same tables:
    * the restage the compaction replaces, phase by phase on the host clock: plsvo_candidates_fetch_map + _fetch_quality +
      _fetch_last_optim; the deleted rows dropped on the host (NumPy, per stream); plsvo_candidates_stage + _set_quality + _set_last_optim;
    * the resident frame step on those tables (run -> resident match -> select -> resident pose optimisation, one wait), which the
      compaction's launch is stated as a fraction of.

usage: python tools/bench_compact.py [--reps 7] [--streams 4096] [--out profiles/compact_bench.json]"""
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

DEAD_FRACTION = 0.25


def with_deleted_rows(P, rng, job):
    """the stream with a quarter of its non-candidate landmarks deleted: the type, and their features without a landmark"""
    t = dict(job.t)
    for name in ("pt", "seg"):
        typ = t[name + "_type"].copy()
        cand = np.zeros(len(typ), bool); cand[t[name + "_cand"]] = True
        dead = (rng.random(len(typ)) < DEAD_FRACTION) & ~cand
        typ[dead] = P.abi.LM_DELETED
        lm = t["kf_" + name + "_lm"].copy()
        held = lm >= 0
        lm[held & (typ[np.where(held, lm, 0)] == P.abi.LM_DELETED)] = -1
        t[name + "_type"], t["kf_" + name + "_lm"] = typ, lm
    return P.abi.CandidateMapJob(**t)


def drop_deleted(P, t, q, k):
    """the restage's host step on one stream's fetched tables, quality and keys: the compaction in NumPy"""
    t, q, k = dict(t), dict(q), dict(k)
    for name in ("pt", "seg"):
        typ = t[name + "_type"]
        live = typ != P.abi.LM_DELETED
        remap = np.where(live, np.cumsum(live) - 1, -1).astype(np.int32)
        off = t[name + "_obs_off"]
        keep = np.repeat(live, np.diff(off))
        for f in [f for f in t if f.startswith(name + "_obs_") and f != name + "_obs_off"]:
            t[f] = t[f][keep]
        t[name + "_obs_off"] = np.concatenate([[0], np.cumsum(np.diff(off)[live])]).astype(np.int32)
        for f in ((name + "_pos",) if name == "pt" else ("seg_spos", "seg_epos")) + (name + "_type",):
            t[f] = t[f][live]
        lm = t["kf_" + name + "_lm"]
        t["kf_" + name + "_lm"] = np.where(lm >= 0, remap[np.maximum(lm, 0)], -1).astype(np.int32)
        c = remap[t[name + "_cand"]]
        t[name + "_cand"] = c[c >= 0]
        for f in (name + "_n_failed", name + "_n_succeeded"):
            q[f] = q[f][live]
        k[name + "_last_optim"] = k[name + "_last_optim"][live]
    return t, q, k


def leg(P, ctx, pool, n, reps):
    abi = P.abi
    maps, frames = [pool[i % len(pool)][0] for i in range(n)], [pool[i % len(pool)][1] for i in range(n)]
    keys = [dict(pt_last_optim=np.arange(m.n_pt, dtype=np.int32) + 1, seg_last_optim=np.arange(m.n_seg, dtype=np.int32) + 1) for m in maps]

    def stage(m, quality=None, last=None):
        ctx.candidates_stage(m, B.CAM, 30, 40, 8, 3, 10)
        if quality is not None:
            ctx.candidates_set_quality(quality)
        ctx.candidates_set_last_optim(keys if last is None else last)
    ctx.candidates_reserve(**BI.RESERVE)
    ctx.candidates_reserve_landmarks(extra_pt=64, extra_seg=64)
    ctx.set_profiling(True)

    def event():
        stage(maps)
        ctx.synchronize()
        ctx.reset_profiling()
        t0 = time.perf_counter()
        ctx.candidates_compact([1] * n)
        ctx.synchronize()
        t = time.perf_counter() - t0
        ms, k = ctx.kernel_time(abi.K_INSERT)
        assert k == 1
        return ms, t
    event()                                           # the first event pays the allocations
    launch, call = zip(*[event() for _ in range(reps)])
    rep = ctx.candidates_compact_fetch(remap=False)[:len(pool)]
    # the resident frame step on the compacted tables
    step = []
    for _ in range(reps + 1):
        ctx.synchronize()
        t0 = time.perf_counter()
        ctx.candidates_run(frames)
        ctx.candidates_match()
        ctx.candidates_select(max_fts=120, max_fts_segs=100)
        ctx.candidates_pose_optimize()
        ctx.synchronize()
        step.append(time.perf_counter() - t0)
    ctx.set_profiling(False)
    # the restage of the same tables
    fetch, host, restage = [], [], []
    for r in range(reps + 1):
        stage(maps)
        ctx.synchronize()
        t0 = time.perf_counter()
        tables, q, k = ctx.candidates_fetch_map(), ctx.candidates_fetch_quality(), ctx.candidates_fetch_last_optim()
        t1 = time.perf_counter()
        dropped = [drop_deleted(P, a, b, c) for a, b, c in zip(tables, q, k)]
        jobs = [abi.CandidateMapJob(**d[0]) for d in dropped]
        t2 = time.perf_counter()
        stage(jobs, [{f: d[1][f] for f in ("pt_n_failed", "pt_n_succeeded", "seg_n_failed", "seg_n_succeeded")} for d in dropped], [d[2] for d in dropped])
        ctx.synchronize()
        t3 = time.perf_counter()
        if r:
            fetch.append(t1 - t0); host.append(t2 - t1); restage.append(t3 - t2)
    total = [a + b + c for a, b, c in zip(fetch, host, restage)]
    device_only = [a + c for a, c in zip(fetch, restage)]
    same = all(int(jobs[i].n_pt) == rep[i]["n_pt_after"] and int(jobs[i].n_seg) == rep[i]["n_seg_after"] for i in range(len(pool)))
    return {"compact_launch_ms": BI.stats(launch), "compact_call_and_wait_ms": BI.stats(call, 1e3, 3), "frame_step_ms": BI.stats(step[1:], 1e3, 3),
            "restage_ms": {"fetch": BI.stats(fetch, 1e3, 2), "drop_on_host": BI.stats(host, 1e3, 2), "stage_and_set": BI.stats(restage, 1e3, 2), "total": BI.stats(total, 1e3, 2),
                           "without_the_host_step": BI.stats(device_only, 1e3, 2)},
            "launch_over_frame_step": round(float(np.median(launch)) / (1e3 * float(np.median(step[1:]))), 4),
            "call_below_restage_minimum": bool(1e3 * max(call) < 1e3 * min(device_only)),
            "restage_counts_equal_the_compaction": bool(same), "events": reps + 1,
            "mean_rows": {f: float(np.mean([r[f] for r in rep])) for f in ("n_pt_before", "n_pt_after", "n_seg_before", "n_seg_after", "n_pt_obs_before", "n_pt_obs_after",
                                                                           "n_seg_obs_before", "n_seg_obs_after")}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--streams", default="4096")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_compact.py: no GPU (a timing needs the MI355X)")
    P = importlib.import_module("pl-svo_amd")
    res = {"what": f"tools/bench_compact.py: plsvo_candidates_compact on the workload of tools/bench_insert.py ({B.N_KF} keyframes of {B.F_PT} + {B.F_SEG} features, "
                   f"{B.N_PT} + {B.N_SEG} landmarks) with {DEAD_FRACTION:.0%} of the non-candidate rows deleted; beside it the restage of the same tables and a frame step on them",
           "device": torch.cuda.get_device_name(0), "gcn_arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", ""), "reps": args.reps, "batched": {}}
    rng = np.random.default_rng(2024)
    pool = []
    for _ in range(64):
        job, frame = BI.make_stream(P, rng)
        pool.append((with_deleted_rows(P, rng, job), frame))
    ctx = P.capi.Context(0)
    try:
        ctx.config_pyramids(B.N_KF + 1, B.CAM[4], B.CAM[5], 3)
        for s in range(B.N_KF + 1):
            ctx.build_pyramid(s, B._texture(rng))
        for n in [int(s) for s in args.streams.split(",") if s]:
            res["batched"][str(n)] = leg(P, ctx, pool, n, args.reps)
    finally:
        ctx.close()
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
