"""Cost of the keyframe insertion into the resident map tables (plsvo_candidates_insert_keyframe) beside the restage it replaces.  Needs an
MI355X; prints one JSON object and writes it to --out.

  The workload of tools/bench_select.py (12 keyframes of 200 + 80 features, 400 + 150 landmarks, 10 in the overlap list, 64 distinct
  streams repeated), brought under the insertion's preconditions (make_stream below): a keyframe's features are the landmarks observed in
  it, a candidate has one observation, a deleted landmark no feature.  A keyframe = run -> resident match -> select -> resident pose optimisation -> insert, with the first row removed, so
  the table keeps its twelve keyframes; the insertion changes the tables, so the keyframes of a leg are consecutive keyframes of one map.
  Per shape, as median (min - max) of --reps consecutive keyframes: the launch that changes the tables by a hipEvent pair on the stream
  (PLSVO_K_INSERT), and the whole call with its planning launch, its read-back and the wait on the host clock.  Beside them, in the same
  session, the restage of the SAME tables that the insertion replaces: plsvo_candidates_fetch_quality, plsvo_candidates_stage,
  plsvo_candidates_set_quality on the host clock (the tables are fetched and packed into jobs outside the timed region).  The extra
  device memory of the reserve is computed from the element sizes.  With --frame-step-ms (the resident frame step per 4096 streams,
  `frame_chain` of the same session's bench.py --full) the insertion's share of it is added.

usage: python tools/bench_insert.py [--reps 7] [--streams 4096,32768] [--frame-step-ms X] [--out profiles/insert_bench.json]"""
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
import bench_select as BS      # noqa: E402

RESERVE = dict(extra_kf=1, extra_kf_pt=200, extra_kf_seg=160, extra_pt_obs=1000, extra_seg_obs=800)


def make_stream(P, rng):
    """a stream of tools/bench_select.py whose feature lists follow its observation lists: every non-candidate, non-deleted landmark is a
    feature of exactly the keyframes that observe it (once per observation), the lists shuffled and filled up to 200 + 80 entries with
    features without a landmark; a candidate keeps its first observation only"""
    job, frame = BS.make_stream(P, rng)
    t = dict(job.t)
    for name, n_ftr in (("pt", B.F_PT), ("seg", B.F_SEG)):
        off, kf, typ, cand = t[name + "_obs_off"], t[name + "_obs_kf"], t[name + "_type"], t[name + "_cand"]
        n = len(typ)
        lm_of = np.repeat(np.arange(n), np.diff(off))
        keep = np.ones(len(kf), bool)
        is_cand = np.zeros(n, bool); is_cand[cand] = True
        keep[is_cand[lm_of]] = False
        keep[off[:-1][is_cand]] = True                                  # the original feature
        for f in [f for f in t if f.startswith(name + "_obs_") and f != name + "_obs_off"]:
            t[f] = t[f][keep]
        lm_of, kf = lm_of[keep], kf[keep]
        t[name + "_obs_off"] = np.concatenate([[0], np.cumsum(np.bincount(lm_of, minlength=n))]).astype(np.int32)
        holds = ~is_cand[lm_of] & (typ[lm_of] != P.abi.LM_DELETED)
        lists = []
        for k in range(B.N_KF):
            l = lm_of[holds & (kf == k)].astype(np.int32)
            l = np.concatenate([l, np.full(max(n_ftr - len(l), 0), -1, np.int32)])
            rng.shuffle(l)
            lists.append(l)
        t["kf_" + name + "_off"] = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int32)
        t["kf_" + name + "_lm"] = np.concatenate(lists)
    return P.abi.CandidateMapJob(**t), frame


def reserve_bytes(r):
    """device bytes per stream the reserve adds to the resident tables (the insertion's staging rows add as much again for the arrays that shift)"""
    kf = r["extra_kf"] * (7 * 8 + 3 * 8 + 2 * 4 + 7 * 8 + 4)
    lists = 4 * (r["extra_kf_pt"] + r["extra_kf_seg"])
    obs = r["extra_pt_obs"] * (4 + 16 + 24 + 4 + 1 + 16) + r["extra_seg_obs"] * (4 + 16 + 16 + 24 + 24 + 4)
    return dict(tables=kf + lists + obs, staging=lists + obs + r["extra_kf"] * 8)


def stats(v, scale=1.0, digits=4):
    return {"median": round(scale * float(np.median(v)), digits), "min": round(scale * min(v), digits), "max": round(scale * max(v), digits)}


def leg(P, ctx, pool, n, reps):
    abi = P.abi
    maps, frames = [pool[i % len(pool)][0] for i in range(n)], [pool[i % len(pool)][1] for i in range(n)]
    ctx.candidates_reserve(**RESERVE)
    ctx.candidates_stage(maps, B.CAM, 30, 40, 8, 3, 10)
    ctx.set_profiling(True)
    ins = [dict(remove_kf=0, kf_slot=B.N_KF)] * n      # the resident pose and masks: nothing but the records travels

    def keyframe():
        ctx.candidates_run(frames)
        ctx.candidates_match()
        ctx.candidates_select(max_fts=120, max_fts_segs=100)
        ctx.candidates_pose_optimize()
        ctx.synchronize()
        ctx.reset_profiling()
        t0 = time.perf_counter()
        ctx.candidates_insert_keyframe(ins)
        ctx.synchronize()
        t = time.perf_counter() - t0
        ms, k = ctx.kernel_time(abi.K_INSERT)
        assert k == 1
        return ms, t
    keyframe()                                        # the first keyframe pays the allocations
    launch, call = zip(*[keyframe() for _ in range(reps)])
    ctx.set_profiling(False)
    rep = ctx.candidates_insert_fetch()[:len(pool)]
    # the restage of the same tables
    tables = ctx.candidates_fetch_map(streams=range(len(pool)))[:len(pool)]      # (the replicas hold the same tables)
    jobs = [abi.CandidateMapJob(**t) for t in tables]
    again = [jobs[i % len(jobs)] for i in range(n)]
    ctx.candidates_reserve()
    restage = []
    for _ in range(reps):
        ctx.synchronize()
        t0 = time.perf_counter()
        q = ctx.candidates_fetch_quality()
        ctx.candidates_stage(again, B.CAM, 30, 40, 8, 3, 10)
        ctx.candidates_set_quality([dict(pt_n_failed=v["pt_n_failed"], pt_n_succeeded=v["pt_n_succeeded"], seg_n_failed=v["seg_n_failed"], seg_n_succeeded=v["seg_n_succeeded"]) for v in q])
        ctx.synchronize()
        restage.append(time.perf_counter() - t0)
    out = {"insert_launch_ms": stats(launch), "insert_call_and_wait_ms": stats(call, 1e3, 3), "restage_ms": stats(restage, 1e3, 2), "keyframes": reps + 1,
           "restage_over_insert_call": round(float(np.median(restage)) / float(np.median(call)), 1),
           "first_keyframe_tables": {f: float(np.mean([getattr(m, "t")[a].size for m, _ in pool])) for f, a in (("n_kf_pt", "kf_pt_lm"), ("n_kf_seg", "kf_seg_lm"), ("n_pt_obs", "pt_obs_kf"),
                                                                                                             ("n_seg_obs", "seg_obs_kf"))},
           "last_keyframe": {f: float(np.mean([r[f] for r in rep])) for f in ("n_kf", "n_kf_pt", "n_kf_seg", "n_pt_obs", "n_seg_obs", "n_joined_pt", "n_deleted_pt", "n_deleted_seg")}}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--streams", default="4096,32768")
    ap.add_argument("--frame-step-ms", type=float, default=None, help="resident frame step per 4096 streams, same session's bench.py --full")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_insert.py: no GPU (a timing needs the MI355X)")
    P = importlib.import_module("pl-svo_amd")
    res = {"what": f"tools/bench_insert.py: plsvo_candidates_insert_keyframe on the workload of tools/bench_select.py ({B.N_KF} keyframes of {B.F_PT} + {B.F_SEG} features, "
                   f"{B.N_PT} + {B.N_SEG} landmarks), the first row removed at every keyframe; beside it the restage of the same tables",
           "device": torch.cuda.get_device_name(0), "gcn_arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", ""), "reps": args.reps,
           "reserve": RESERVE, "reserve_bytes_per_stream": reserve_bytes(RESERVE), "batched": {}}
    rng = np.random.default_rng(2024)
    pool = [make_stream(P, rng) for _ in range(64)]
    ctx = P.capi.Context(0)
    try:
        ctx.config_pyramids(B.N_KF + 1, B.CAM[4], B.CAM[5], 3)
        for s in range(B.N_KF + 1):
            ctx.build_pyramid(s, B._texture(rng))
        for n in [int(s) for s in args.streams.split(",") if s]:
            res["batched"][str(n)] = leg(P, ctx, pool, n, args.reps)
    finally:
        ctx.close()
    if args.frame_step_ms is not None:
        res["frame_step_ms_per_4096_streams"] = args.frame_step_ms
        v = res["batched"].get("4096")
        if v:
            v["insert_call_over_frame_step"] = {k: round(x / args.frame_step_ms, 4) for k, x in v["insert_call_and_wait_ms"].items()}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
