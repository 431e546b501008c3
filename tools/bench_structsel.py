"""Cost of the structure optimisation on the resident map tables (plsvo_candidates_optimize_structure) beside the host-fed path it
replaces.  Needs an MI355X; prints one JSON object and writes it to --out.

  The workload of tools/bench_insert.py (12 keyframes of 200 + 80 features, 400 + 150 landmarks, 64 distinct streams repeated) at the
  resident frame step's shape, 4096 streams: a frame = run -> a constructed match that finds every filed candidate at its projection
  (plsvo_candidates_set_match) -> select -> resident pose optimisation, which leaves a feature in every occupied cell -- the frame step's
  hundred or so -- with their keep masks on the device; the caps are the reference's 20 + 20, five
  iterations each.  Behind every frame, in the same session and in alternating order:
    resident   plsvo_candidates_optimize_structure with the resident masks, enqueue to completion on the host clock, and its launch by a
               hipEvent pair on the stream (PLSVO_K_STRUCTOPT)
    host path  plsvo_candidates_fetch_map of every stream, the choice of the 20 + 20 least recently refined kept landmarks and the gather
               of their observation lists in NumPy, plsvo_structure_optimize on the gathered job, plsvo_candidates_set_positions -- each
               leg on the host clock (fetch_map's leg includes the Python wrapper's buffers; the selection and the masks the path needs
               as well are fetched outside the timed region)
  Reported as mean (min - max) over --reps frames.

usage: python tools/bench_structsel.py [--reps 5] [--streams 4096] [--out profiles/structsel_bench.json]"""
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

CAPS = dict(max_n_pts=20, n_iter_pts=5, max_n_segs=20, n_iter_segs=5)


def stats(v, scale=1.0, digits=3):
    return {"mean": round(scale * float(np.mean(v)), digits), "min": round(scale * min(v), digits), "max": round(scale * max(v), digits)}


def gather(P, tables, sels, masks, keys, frame_id):
    """the host's half of the path: per stream the 20 + 20 kept landmarks with the smallest keys (ties to the earlier feature), their
    observation lists flattened into one plsvo_structure_optimize job; -> (job, per stream (point rows, segment rows))"""
    T, chosen = [], []
    cols = dict(pt_pos=[], pt_off=[0], pt_fr=[], pt_f=[], seg_spos=[], seg_epos=[], seg_off=[0], seg_fr=[], seg_sf=[], seg_ef=[])
    base = 0
    for t, sel, m, key in zip(tables, sels, masks, keys):
        rows = []
        for name, keep, cap in (("pt", m[0], CAPS["max_n_pts"]), ("seg", m[1], CAPS["max_n_segs"])):
            lm = sel[name + "_lm"][keep.astype(bool)]
            lm = lm[np.sort(np.argsort(key[name][lm], kind="stable")[:cap])]
            lm = lm[np.sort(np.unique(lm, return_index=True)[1])]       # (a doubly won segment is gathered once here: the host path's job lists a landmark once)
            off = t[name + "_obs_off"]
            idx = np.concatenate([np.arange(off[i], off[i + 1]) for i in lm]) if len(lm) else np.zeros(0, np.int64)
            cols[name + "_off"] += list(cols[name + "_off"][-1] + np.cumsum(off[lm + 1] - off[lm]))
            cols[name + "_fr"].append(t[name + "_obs_kf"][idx] + base)
            if name == "pt":
                cols["pt_pos"].append(t["pt_pos"][lm]); cols["pt_f"].append(t["pt_obs_f"][idx])
            else:
                cols["seg_spos"].append(t["seg_spos"][lm]); cols["seg_epos"].append(t["seg_epos"][lm])
                cols["seg_sf"].append(t["seg_obs_sf"][idx]); cols["seg_ef"].append(t["seg_obs_ef"][idx])
            key[name][lm] = frame_id
            rows.append(lm.astype(np.int32))
        T.append(t["kf_T"])
        base += len(t["kf_T"])
        chosen.append(rows)
    cat = lambda k, w: np.concatenate(cols[k]).reshape(-1, w) if cols[k] else np.zeros((0, w))
    job = P.abi.StructOptJob(np.concatenate(T), cat("pt_pos", 3), cols["pt_off"], np.concatenate(cols["pt_fr"]), cat("pt_f", 3), cat("seg_spos", 3), cat("seg_epos", 3),
                             cols["seg_off"], np.concatenate(cols["seg_fr"]), cat("seg_sf", 3), cat("seg_ef", 3), CAPS["n_iter_pts"], CAPS["n_iter_segs"])
    return job, chosen


def found_everywhere(c):
    """a constructed match of every filed candidate at its projection (plsvo_cand_match_out's layout: points, segment starts, segment ends):
    the frame then has a feature in every occupied cell, the resident frame step's hundred or so, and the pose optimiser keeps them"""
    px = np.concatenate([c["pt_px"].reshape(-1, 2), c["seg_px"].reshape(-1, 4)[:, :2], c["seg_px"].reshape(-1, 4)[:, 2:]])
    return dict(found=np.ones(len(px), np.uint8), px=px, search_level=np.zeros(len(px), np.int32))


def leg(P, ctx, pool, n, reps):
    abi = P.abi
    maps, frames = [pool[i % len(pool)][0] for i in range(n)], [pool[i % len(pool)][1] for i in range(n)]
    ctx.candidates_reserve()
    ctx.candidates_stage(maps, B.CAM, 30, 40, 8, 3, 10)
    ctx.set_profiling(True)
    keys = [dict(pt=np.zeros(m.n_pt, np.int64), seg=np.zeros(m.n_seg, np.int64)) for m in maps]      # the host path's own last_structure_optim_
    res = dict(resident_call=[], resident_launch=[], fetch_map=[], gather=[], structure_optimize=[], set_positions=[], host_total=[])
    feats, sel_n = [], []

    def resident(k):
        ctx.reset_profiling()
        t0 = time.perf_counter()
        ctx.candidates_optimize_structure([dict(frame_id=k)] * n, **CAPS)
        ctx.synchronize()
        res["resident_call"].append(time.perf_counter() - t0)
        ms, cnt = ctx.kernel_time(abi.K_STRUCTOPT)
        assert cnt == 1
        res["resident_launch"].append(ms)

    def host(k, sels, masks):
        t0 = time.perf_counter()
        tables = ctx.candidates_fetch_map()
        t1 = time.perf_counter()
        job, chosen = gather(P, tables, sels, masks, keys, k)
        t2 = time.perf_counter()
        out = ctx.structure_optimize(job)
        t3 = time.perf_counter()
        ap = asg = 0
        moved = []
        for rows in chosen:
            moved.append(dict(pt_idx=rows[0], pt_pos=out["pt_pos"][ap:ap + len(rows[0])], seg_idx=rows[1], seg_spos=out["seg_spos"][asg:asg + len(rows[1])],
                              seg_epos=out["seg_epos"][asg:asg + len(rows[1])]))
            ap += len(rows[0]); asg += len(rows[1])
        ctx.candidates_set_positions(moved)
        ctx.synchronize()
        t4 = time.perf_counter()
        for name, dt in (("fetch_map", t1 - t0), ("gather", t2 - t1), ("structure_optimize", t3 - t2), ("set_positions", t4 - t3), ("host_total", t4 - t0)):
            res[name].append(dt)

    for k in range(reps + 1):                          # the first frame pays the allocations and is left out
        ctx.candidates_run(frames)
        ctx.candidates_set_match([found_everywhere(c) for c in ctx.candidates_fetch()])
        ctx.candidates_select(max_fts=120, max_fts_segs=100)
        ctx.candidates_pose_optimize()
        sels = ctx.candidates_select_fetch()
        po = ctx.candidates_pose_fetch([(s["n_matches"], s["n_ls_matches"]) for s in sels])
        masks = [(p.pt_keep, p.seg_keep) for p in po]
        ctx.synchronize()
        for which in (("resident", "host") if k % 2 else ("host", "resident")):
            resident(k + 1) if which == "resident" else host(k + 1, sels, masks)
        feats.append((np.mean([int(m[0].sum()) for m in masks]), np.mean([int(m[1].sum()) for m in masks])))
        rep = ctx.candidates_structure_fetch()
        sel_n.append((np.mean([r["n_sel_pt"] for r in rep]), np.mean([r["n_sel_seg"] for r in rep])))
    ctx.set_profiling(False)
    out = {name + ("_ms"): stats(v[1:], 1.0 if name == "resident_launch" else 1e3) for name, v in res.items()}
    out["host_total_over_resident_call"] = round(float(np.mean(res["host_total"][1:])) / float(np.mean(res["resident_call"][1:])), 1)
    out["kept_features_per_stream"] = {"points": round(float(np.mean([f[0] for f in feats])), 1), "segments": round(float(np.mean([f[1] for f in feats])), 1)}
    out["selected_per_stream"] = {"points": round(float(np.mean([f[0] for f in sel_n])), 1), "segments": round(float(np.mean([f[1] for f in sel_n])), 1)}
    out["frames"] = reps
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--streams", default="4096")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_structsel.py: no GPU (a timing needs the MI355X)")
    P = importlib.import_module("pl-svo_amd")
    res = {"what": f"tools/bench_structsel.py: plsvo_candidates_optimize_structure on the workload of tools/bench_insert.py ({B.N_KF} keyframes of {B.F_PT} + {B.F_SEG} features, "
                   f"{B.N_PT} + {B.N_SEG} landmarks), caps {CAPS}; beside it fetch_map + NumPy gather + plsvo_structure_optimize + set_positions",
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
    finally:
        ctx.close()
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
