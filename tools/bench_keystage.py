"""Cost of the keyframe stage on the resident map tables (plsvo_candidates_run_close, plsvo_candidates_keyframe_decide and the upkeep of the
key-point table) beside the synchronous host-fed path it replaces.  Needs an MI355X; prints one JSON object and writes it to --out.

  The resident table sizes of tools/bench_select.py (12 keyframes of 200 + 80 features, 400 + 150 landmarks, 64 distinct streams repeated)
  in tools/bench_insert.py's variant of its streams, whose keyframe features follow the observation lists: a feature's px is looked up
  in its landmark's observations, so the key points need that precondition.  4096 streams, the resident frame step's shape.  A frame = run_close (the overlap list from the live key-point table, max_n_kfs 10) -> a
  constructed match that finds every filed candidate at its projection -> select -> resident pose optimisation.  Per frame:
    resident   close_launch    the launch plsvo_candidates_run_close puts ahead of the candidate launch, by its hipEvent pair
               upkeep_launch   the key-point upkeep behind plsvo_candidates_select, by its hipEvent pair
               insert_upkeep_launch   the key-point upkeep behind plsvo_candidates_insert_keyframe (rows close up over the removed
                               keyframe 0, lost holders replaced, the new row from the resident decision), by its hipEvent pair, in
                               keyframes of their own (run_close -> resident match -> select -> pose optimisation -> decision ->
                               insertion, bench_insert.py's reserve); insert_launch: the insertion's own launch beside it
               decide_call     plsvo_candidates_keyframe_decide + plsvo_candidates_decide_fetch (the 56-byte records alone), enqueue to
                               results on the host clock; decide_launch: of that, the launch by its hipEvent pair
    host path  pose_fetch      plsvo_candidates_pose_fetch (poses and keep masks)
               close           plsvo_close_keyframes on the caller's keyframe table (kf_T, five key-point positions per keyframe: the
                               upload) -- synchronous
               select_fetch    plsvo_candidates_select_fetch (the selection's features) and the gather of their landmark positions
               decide          plsvo_keyframe_decide on the gathered arrays -- synchronous
               host_total      the four together
  Every leg goes through the Python wrapper on both sides.  Reported as median (min - max) over --reps frames; one more frame runs first
  and is left out (it pays the allocations).

usage: python tools/bench_keystage.py [--reps 7] [--streams 4096] [--out profiles/keystage_bench.json]"""
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

MAX_N_KFS = 10


def stats(v, scale=1.0, digits=3):
    return {"median": round(scale * float(np.median(v)), digits), "min": round(scale * min(v), digits), "max": round(scale * max(v), digits)}


def leg(P, ctx, pool, n, reps):
    abi = P.abi
    maps = [pool[i % len(pool)][0] for i in range(n)]
    frames = [abi.CandidateFrameJob(list(pool[i % len(pool)][1].c.T_f_w), (), cur_slot=pool[i % len(pool)][1].c.cur_slot) for i in range(n)]
    ctx.candidates_reserve()
    ctx.candidates_stage(maps, B.CAM, 30, 40, 8, 3, 10)
    ctx.candidates_set_keypts()
    tables = ctx.candidates_fetch_keypts()
    # the host path's own keyframe table: kf_T and the key points' positions as the caller would keep them
    host_kf = []
    for m, tab in zip(maps, tables):
        t = m.t
        kp, kv = np.zeros((m.n_kf, 5, 3)), np.zeros((m.n_kf, 5), np.uint8)
        for k in range(m.n_kf):
            for s in range(5):
                h = tab[k][s]
                lm = t["kf_pt_lm"][t["kf_pt_off"][k] + h] if h >= 0 else -1
                if lm >= 0:
                    kp[k, s], kv[k, s] = t["pt_pos"][lm], 1
        host_kf.append((kp, kv))
    ctx.set_profiling(True)
    res = dict(close_launch=[], upkeep_launch=[], decide_call=[], decide_launch=[], pose_fetch=[], close=[], select_fetch=[], decide=[], host_total=[])
    n_close, agree = [], True
    T_last = [list(f.c.T_f_w) for f in frames]

    def launch_ms(family, count):
        ms, cnt = ctx.kernel_time(family)
        assert cnt == count, (family, cnt, count)
        return ms

    def resident():
        ctx.reset_profiling()
        t0 = time.perf_counter()
        ctx.candidates_keyframe_decide([dict(T_last_w=T) for T in T_last])
        out = ctx.candidates_decide_fetch(deltas=False)
        res["decide_call"].append(time.perf_counter() - t0)
        res["decide_launch"].append(launch_ms(abi.K_KEYFRAME, 1))
        return out

    def host(counts):
        t0 = time.perf_counter()
        po = ctx.candidates_pose_fetch(counts)
        t1 = time.perf_counter()
        close = ctx.close_keyframes([abi.CloseKeyframesJob(B.CAM, f.c.T_f_w, m.t["kf_T"], kp, kv, MAX_N_KFS) for f, m, (kp, kv) in zip(frames, maps, host_kf)])
        t2 = time.perf_counter()
        sels = ctx.candidates_select_fetch()
        jobs = []
        for m, s, p, c, T in zip(maps, sels, po, close, T_last):
            t = m.t
            jobs.append(abi.KeyframeDecideJob(B.CAM, p.T, T, s["pt_px"], t["pt_pos"][s["pt_lm"]], p.pt_keep, t["seg_spos"][s["seg_lm"]], t["seg_epos"][s["seg_lm"]], p.seg_keep,
                                              t["kf_T"], c["close_idx"][:c["n_overlap"]], [-1] * 5))
        t3 = time.perf_counter()
        out = ctx.keyframe_decide(jobs)
        t4 = time.perf_counter()
        for name, dt in (("pose_fetch", t1 - t0), ("close", t2 - t1), ("select_fetch", t3 - t2), ("decide", t4 - t3), ("host_total", t4 - t0)):
            res[name].append(dt)
        return close, out

    for k in range(reps + 1):                          # the first frame pays the allocations and is left out
        ctx.reset_profiling()
        ctx.candidates_run_close(frames, MAX_N_KFS)
        ctx.synchronize()
        res["close_launch"].append(launch_ms(abi.K_KEYFRAME, 1))
        ctx.candidates_set_match([found_everywhere(c) for c in ctx.candidates_fetch()])
        ctx.reset_profiling()
        ctx.candidates_select(max_fts=120, max_fts_segs=100)
        ctx.synchronize()
        res["upkeep_launch"].append(launch_ms(abi.K_KEYFRAME, 1))
        ctx.candidates_pose_optimize()
        sels = ctx.candidates_select_fetch()
        counts = [(s["n_matches"], s["n_ls_matches"]) for s in sels]
        ctx.synchronize()
        for which in (("resident", "host") if k % 2 else ("host", "resident")):
            if which == "resident":
                dev = resident()
            else:
                close, ref = host(counts)
        # (the positions have not moved and the table is the one the host copy was made from: the two paths must agree)
        for d, r in zip(dev, ref):
            agree = agree and all(np.asarray(d[f]).tobytes() == np.asarray(r[f]).tobytes() for f in ("depth_mean", "depth_min", "need_new_kf", "blocking", "furthest_kf", "n_depth"))
            agree = agree and np.array_equal(d["key_pts"], r["key_pts"])
        dc = ctx.candidates_close_fetch()
        agree = agree and all(np.array_equal(a["close_idx"], b["close_idx"]) for a, b in zip(dc, close))
        n_close.append(float(np.mean([c["n_close"] for c in dc])))
    ctx.set_profiling(False)
    out = {name + "_ms": stats(v[1:], 1.0 if name.endswith("_launch") else 1e3) for name, v in res.items()}
    out["resident_median_below_host_minimum"] = bool(out["decide_call_ms"]["median"] + out["close_launch_ms"]["median"] < out["host_total_ms"]["min"])
    out["paths_agree"] = bool(agree)
    out["close_keyframes_per_stream"] = round(float(np.mean(n_close)), 2)
    out["frames"] = reps
    return out


def insert_leg(P, ctx, pool, n, reps):
    """the upkeep launch behind the insertion, table live: every keyframe removes row 0 and appends the frame"""
    abi = P.abi
    maps = [pool[i % len(pool)][0] for i in range(n)]
    frames = [abi.CandidateFrameJob(list(pool[i % len(pool)][1].c.T_f_w), (), cur_slot=pool[i % len(pool)][1].c.cur_slot) for i in range(n)]
    ctx.candidates_reserve(**BI.RESERVE)
    ctx.candidates_stage(maps, B.CAM, 30, 40, 8, 3, 10)
    ctx.candidates_reserve()
    ctx.candidates_set_keypts()
    ctx.set_profiling(True)
    ins = [dict(remove_kf=0, kf_slot=B.N_KF)] * n
    decides = [dict(T_last_w=list(f.c.T_f_w)) for f in frames]
    upkeep, insert = [], []
    for _ in range(reps + 1):
        ctx.candidates_run_close(frames, MAX_N_KFS)
        ctx.candidates_match()
        ctx.candidates_select(max_fts=120, max_fts_segs=100)
        ctx.candidates_pose_optimize()
        ctx.candidates_keyframe_decide(decides)
        ctx.synchronize()
        ctx.reset_profiling()
        ctx.candidates_insert_keyframe(ins)
        ctx.synchronize()
        for family, to in ((abi.K_KEYFRAME, upkeep), (abi.K_INSERT, insert)):
            ms, cnt = ctx.kernel_time(family)
            assert cnt == 1, (family, cnt)
            to.append(ms)
    ctx.set_profiling(False)
    rep = ctx.candidates_insert_fetch()[:len(pool)]
    return {"insert_upkeep_launch_ms": stats(upkeep[1:]), "insert_launch_ms": stats(insert[1:]), "keyframes": reps,
            "last_keyframe_deleted_pt_per_stream": round(float(np.mean([r["n_deleted_pt"] for r in rep])), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--streams", default="4096")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_keystage.py: no GPU (a timing needs the MI355X)")
    P = importlib.import_module("pl-svo_amd")
    res = {"what": f"tools/bench_keystage.py: the keyframe stage on the resident tables on the workload of tools/bench_insert.py ({B.N_KF} keyframes of {B.F_PT} + {B.F_SEG} "
                   f"features, {B.N_PT} + {B.N_SEG} landmarks), max_n_kfs {MAX_N_KFS}; beside it pose_fetch + plsvo_close_keyframes + select_fetch + plsvo_keyframe_decide",
           "device": torch.cuda.get_device_name(0), "gcn_arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", ""), "reps": args.reps, "batched": {}}
    rng = np.random.default_rng(2024)
    pool = [BI.make_stream(P, rng) for _ in range(64)]
    ctx = P.capi.Context(0)
    try:
        ctx.config_pyramids(B.N_KF + 1, B.CAM[4], B.CAM[5], 3)
        for s in range(B.N_KF + 1):
            ctx.build_pyramid(s, B._texture(rng))
        for n in [int(s) for s in args.streams.split(",") if s]:
            res["batched"][str(n)] = leg(P, ctx, pool, n, args.reps)
            res["batched"][str(n)].update(insert_leg(P, ctx, pool, n, args.reps))
    finally:
        ctx.close()
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
