"""Cost of relocalisation's device pieces beside the host-fed paths they replace.  Needs an MI355X; prints one JSON
object and writes it to --out, and a table to --md.

  The resident table sizes of tools/bench_alignjob.py (12 keyframes of 200 + 80 features, 400 + 150 landmarks, 64 distinct streams
  repeated), 4096 streams.  A frame = run -> a constructed match that finds every filed candidate -> select -> resident pose
  optimisation.  Per frame, in alternating order:
    resident   kf_build_launch       map_align_kf_job_kernel from a given keyframe row by its hipEvent pair (PLSVO_K_ALIGN_INIT)
               kf_build_call         plsvo_candidates_align_build_kf, records included, enqueue to completion on the host clock
               closest_build_launch  the same launch with PLSVO_ALIGN_REF_CLOSEST (the wave picks the row from the live key-point table)
               closest_build_call
               gate_launch           map_track_gate_kernel by its hipEvent pair (PLSVO_K_KEYFRAME)
               gate_call             plsvo_candidates_track_gate + plsvo_candidates_gate_fetch on the host clock (the harness's wait)
    host path  map_fetch             plsvo_candidates_fetch_map of every stream
               numpy_job             the keyframe's job per stream from the fetched tables on the host (sequence.align_kf_job_host)
               align_stage           plsvo_align_stage
               host_total            the three together
               gate_fetches          plsvo_candidates_select_fetch + _pose_fetch, which the comparisons in Python need
  Reported as mean (min - max) over --reps frames; one more frame runs first and is left out (it pays the allocations).

usage: python tools/bench_reloc.py [--reps 4] [--streams 4096] [--out profiles/reloc_bench.json] [--md profiles/reloc_resident.md]"""
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
from bench_alignjob import CAP_PTS, CAP_SEG, MAX_LEVEL, MIN_LEVEL, N_PYR, stats   # noqa: E402
from bench_structsel import found_everywhere   # noqa: E402

CAP_KF_PTS, CAP_KF_SEG = 224, 112                      # a keyframe's features (200 + 80), kept or not


def leg(P, ctx, pool, n, reps, slot_cap):
    abi = P.abi
    maps, frames = [pool[i % len(pool)][0] for i in range(n)], [pool[i % len(pool)][1] for i in range(n)]
    ctx.candidates_reserve()
    ctx.candidates_stage(maps, B.CAM, 30, 40, 8, 3, 10)
    ctx.candidates_set_keypts()
    ctx.candidates_align_reserve(MAX_LEVEL, MIN_LEVEL, CAP_KF_PTS, CAP_KF_SEG, slot_cap)
    ctx.set_profiling(True)
    names = ("kf_build_launch", "kf_build_call", "closest_build_launch", "closest_build_call", "gate_launch", "gate_call", "map_fetch", "numpy_job", "align_stage",
             "host_total", "gate_fetches")
    res = {k: [] for k in names}
    ident = [0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]
    row = B.N_KF - 1
    jobs_row = [dict(ref_kf=row, cur_slot=B.N_KF, T_init=ident)] * n
    jobs_closest = [dict(cur_slot=B.N_KF, T_init=ident, T_last=list(f.c.T_f_w)) for f in frames]
    gate = [dict(T_reset=ident, num_obs_last=(100, 50))] * n
    info = {}

    def launch_ms(family, count):
        ms, cnt = ctx.kernel_time(family)
        assert cnt == count, (family, cnt, count)
        return ms

    def build(jobs, tag):
        ctx.reset_profiling()
        t0 = time.perf_counter()
        ctx.candidates_align_build_kf(jobs)
        ctx.synchronize()
        res[tag + "_call"].append(time.perf_counter() - t0)
        res[tag + "_launch"].append(launch_ms(abi.K_ALIGN_INIT, 1))

    def resident():
        build(jobs_row, "kf_build")
        rep = ctx.candidates_align_fetch()
        info["no_room"] = int(sum(r["status"] != abi.ALIGN_JOB_OK for r in rep))
        info["features"] = {"points": round(float(np.mean([r["n_pts"] for r in rep])), 1), "segments": round(float(np.mean([r["n_seg"] for r in rep])), 1)}
        build(jobs_closest, "closest_build")
        info["closest_none"] = int(sum(r["status"] == abi.ALIGN_JOB_NO_KEYFRAME for r in ctx.candidates_align_fetch()))
        ctx.reset_profiling()
        t0 = time.perf_counter()
        ctx.candidates_track_gate(gate)
        ctx.candidates_gate_fetch()
        res["gate_call"].append(time.perf_counter() - t0)
        res["gate_launch"].append(launch_ms(abi.K_KEYFRAME, 1))

    def host():
        t0 = time.perf_counter()
        tabs = ctx.candidates_fetch_map()
        t1 = time.perf_counter()
        jobs = [P.sequence.align_kf_job_host(B.CAM, MAX_LEVEL, MIN_LEVEL, t, row, ident, B.N_KF) for t in tabs]
        t2 = time.perf_counter()
        ctx.align_stage(jobs)
        ctx.synchronize()
        t3 = time.perf_counter()
        sels = ctx.candidates_select_fetch()
        ctx.candidates_pose_fetch([(s["n_matches"], s["n_ls_matches"]) for s in sels])
        t4 = time.perf_counter()
        for name, dt in (("map_fetch", t1 - t0), ("numpy_job", t2 - t1), ("align_stage", t3 - t2), ("host_total", t3 - t0), ("gate_fetches", t4 - t3)):
            res[name].append(dt)

    for k in range(reps + 1):                          # the first frame pays the allocations and is left out
        ctx.candidates_run(frames)
        ctx.candidates_set_match([found_everywhere(c) for c in ctx.candidates_fetch()])
        ctx.candidates_select(max_fts=120, max_fts_segs=100)
        ctx.candidates_pose_optimize()
        ctx.synchronize()
        for which in (("resident", "host") if k % 2 else ("host", "resident")):
            resident() if which == "resident" else host()
        print(f"bench_reloc: {n} streams, frame {k} of {reps}", file=sys.stderr, flush=True)
    ctx.set_profiling(False)
    out = {name + "_ms": stats(v[1:], 1.0 if name.endswith("_launch") else 1e3) for name, v in res.items()}
    out.update(info)
    out["slot_cap"] = slot_cap
    out["frames"] = reps
    return out


def table(res):
    r = res["leg"]
    f = lambda k: "{mean} ({min} - {max})".format(**r[k + "_ms"])
    lines = ["# Relocalisation on the resident map: measured times", "",
             f"`tools/bench_reloc.py`, {res['device']} ({res['gcn_arch']}), {res['streams']} streams, {r['frames']} alternated frames in one session; mean (min - max), ms.",
             f"Keyframe row {B.N_KF - 1} of {B.N_KF}: {r['features']['points']} kept points and {r['features']['segments']} segment features per stream; no-room streams: {r['no_room']}; "
             f"streams without a close keyframe: {r['closest_none']}.", "",
             "| step | ms |", "|---|---|"]
    for k, what in (("kf_build_launch", "`map_align_kf_job_kernel`, a given row (launch)"), ("kf_build_call", "`plsvo_candidates_align_build_kf`, a given row (call to completion)"),
                    ("closest_build_launch", "`map_align_kf_job_kernel`, closest keyframe (launch)"), ("closest_build_call", "`plsvo_candidates_align_build_kf`, closest keyframe (call to completion)"),
                    ("map_fetch", "host path: `plsvo_candidates_fetch_map`"), ("numpy_job", "host path: `sequence.align_kf_job_host` per stream"), ("align_stage", "host path: `plsvo_align_stage`"),
                    ("host_total", "host path: total"), ("gate_launch", "`map_track_gate_kernel` (launch)"), ("gate_call", "`plsvo_candidates_track_gate` + `_gate_fetch` (call)"),
                    ("gate_fetches", "host path: `_select_fetch` + `_pose_fetch`")):
        lines.append(f"| {what} | {f(k)} |")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--slot-cap", type=int, default=1024)
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_reloc.py: no GPU (a timing needs the MI355X)")
    P = importlib.import_module("pl-svo_amd")
    res = {"what": "tools/bench_reloc.py: the alignment job from a resident keyframe and the tracking gates beside the host-fed paths they replace",
           "device": torch.cuda.get_device_name(0), "gcn_arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", ""), "reps": args.reps, "streams": args.streams}
    rng = np.random.default_rng(2024)
    pool = [BI.make_stream(P, rng) for _ in range(64)]
    textures = [B._texture(rng) for _ in range(B.N_KF + 1)]
    ctx = P.capi.Context(0)
    try:
        ctx.config_pyramids(B.N_KF + 1, B.CAM[4], B.CAM[5], N_PYR)
        for s, img in enumerate(textures):
            ctx.build_pyramid(s, img)
        res["leg"] = leg(P, ctx, pool, args.streams, args.reps, args.slot_cap)
    finally:
        ctx.close()
    text = json.dumps(res)
    print(text)
    for path, body in ((args.out, text + "\n"), (args.md, table(res))):
        if path:
            with open(path, "w") as fh:
                fh.write(body)


if __name__ == "__main__":
    main()
