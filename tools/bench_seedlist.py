"""Cost of the resident seed lists' hand-over (plsvo_seeds_*) beside the host path of the same tree.  Needs an MI355X; prints one JSON object
and writes it to --out.

  The workload and preconditions of tools/bench_newcand.py (tools/bench_insert.py's streams: 12 keyframes of 200 + 80 features, 400 + 150
  landmarks, 64 distinct streams repeated), 200 point + 80 line seeds per stream in random keyframes of its table, textured frames in the
  pyramid slots.  Per load (--loads "points,segments" converged per stream and step; several separated by ';'), as median (min - max) of
  --reps consecutive steps behind one untimed first step (which pays the allocations):
   (a) the resident hand-over, driven with constructed rows (plsvo_seeds_commit_rows) so that the converged counts are exact: the commit
       launch by a hipEvent pair on the stream (counted under PLSVO_K_NEWCAND), and plsvo_seeds_update_fetch -- the frame's one wait: the
       96-byte reports and the refresh of the host's mirrors -- on the host clock.  The diagnostic's own per-stream copies are not timed.
   (b) the host path: plsvo_candidates_add call plus wait for the SAME records on a fresh stage of the same tables; the Python binding's
       packing apart, as tools/bench_newcand.py reports it.
   (c) the whole update step at 200 + 80 seeds per stream: plsvo_seeds_update -> plsvo_seeds_update_fetch on the host clock, against
       plsvo_update_seeds (upload, launch, download: one call for the whole batch) plus plsvo_candidates_add of what converged.
  Every timed region is the C entry points alone, called on prepared ctypes arrays; what the Python binding adds is reported apart.
  With --frame-step-ms (the resident frame step per 4096 streams, `frame_chain` of the same session's bench.py --full) the shares are added.

usage: python tools/bench_seedlist.py [--reps 7] [--streams 4096] [--loads "3,0;7,3;25,10"] [--frame-step-ms X] [--out profiles/seedlist_bench.json]"""
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


def raw_fetch(P, ctx, n, outs):
    """plsvo_seeds_update_fetch itself, into a prepared array: the C call, without the binding's conversion of the reports into dicts"""
    rc = ctx.L.plsvo_seeds_update_fetch(ctx.h, n, outs)
    assert rc == 0, rc


def frames_array(P, frames):
    """the records of plsvo_seeds_update packed once (host poses), as capi.Context.seeds_update packs them on every call"""
    import ctypes as C
    arr = (P.abi.SeedFrame * len(frames))()
    for a, f in zip(arr, frames):
        a.active, a.cur_slot, a.pose_source = 1, int(f["cur_slot"]), P.abi.INSERT_POSE_HOST
        a.T_f_w = (C.c_double * 7)(*[float(v) for v in f["T_f_w"]])
    return arr


N_SP, N_SS = 200, 80
f32 = np.float32


def make_seeds(rng):
    """one stream's seed lists as capi.Context.seeds_stage takes them: features anywhere in the image of a random keyframe of the table"""
    w, h = B.CAM[4], B.CAM[5]

    def obs(k):
        px = np.stack([rng.uniform(20, w - 20, k), rng.uniform(20, h - 20, k)], 1)
        f = np.stack([(px[:, 0] - B.CAM[2]) / B.CAM[0], (px[:, 1] - B.CAM[3]) / B.CAM[1], np.ones(k)], 1)
        return px, f / np.linalg.norm(f, axis=1, keepdims=True)
    zr = f32(1.0 / 2.0)
    par = lambda k: dict(a=np.full(k, 10, f32), b=np.full(k, 10, f32), mu=np.full(k, 1.0 / 4.0, f32), z_range=np.full(k, zr, f32), sigma2=np.full(k, zr * zr / f32(36), f32))
    px, f = obs(N_SP)
    p = par(N_SP)
    d = dict(batch_counter=0, pt_ref_kf=rng.integers(0, B.N_KF, N_SP), pt_batch_id=np.zeros(N_SP, np.int32), pt_px=px, pt_f=f, pt_level=rng.integers(0, 3, N_SP),
             pt_type=np.zeros(N_SP, np.uint8), pt_grad=np.tile([1.0, 0.0], (N_SP, 1)), pt_a=p["a"], pt_b=p["b"], pt_mu=p["mu"], pt_z_range=p["z_range"], pt_sigma2=p["sigma2"])
    (spx, sf), (epx, ef) = obs(N_SS), obs(N_SS)
    mid = sf + ef
    q = par(N_SS)
    d.update(seg_ref_kf=rng.integers(0, B.N_KF, N_SS), seg_batch_id=np.zeros(N_SS, np.int32), seg_px=(spx + epx) / 2, seg_f=mid / np.linalg.norm(mid, axis=1, keepdims=True), seg_sf=sf,
             seg_ef=ef, seg_spx=spx, seg_epx=epx, seg_level=rng.integers(0, 3, N_SS), seg_a=q["a"], seg_b=q["b"], seg_mu_s=q["mu"], seg_mu_e=q["mu"], seg_z_range_s=q["z_range"],
             seg_z_range_e=q["z_range"], seg_sigma2_s=q["sigma2"], seg_sigma2_e=q["sigma2"])
    return d


def rows_and_records(sd, at_pt, at_seg, c_pt, c_seg, xyz):
    """constructed rows for the lists as they stand (the first at_pt / at_seg seeds have left): the first c_pt / c_seg rows converge, the
    others are updated with their own parameters; and the same hand-over as plsvo_cand_new records"""
    P, S = slice(at_pt, N_SP), slice(at_seg, N_SS)
    npt, nsg = N_SP - at_pt, N_SS - at_seg
    st_p, st_s = np.full(npt, 2, np.int32), np.full(nsg, 2, np.int32)
    st_p[:c_pt] = 3; st_s[:c_seg] = 3
    rows = dict(pt_status=st_p, pt_a=sd["pt_a"][P], pt_b=sd["pt_b"][P], pt_mu=sd["pt_mu"][P], pt_sigma2=sd["pt_sigma2"][P], pt_xyz_world=xyz[:npt],
                seg_status=st_s, seg_a=sd["seg_a"][S], seg_b=sd["seg_b"][S], seg_mu_s=sd["seg_mu_s"][S], seg_mu_e=sd["seg_mu_e"][S], seg_sigma2_s=sd["seg_sigma2_s"][S],
                seg_sigma2_e=sd["seg_sigma2_e"][S], seg_xyz_world_s=xyz[:nsg], seg_xyz_world_e=xyz[nsg:2 * nsg] if nsg else xyz[:0])
    Pc, Sc = slice(at_pt, at_pt + c_pt), slice(at_seg, at_seg + c_seg)
    rec = {}
    if c_pt:
        rec.update(pt_pos=xyz[:c_pt], pt_obs_kf=sd["pt_ref_kf"][Pc], pt_obs_px=sd["pt_px"][Pc], pt_obs_f=sd["pt_f"][Pc], pt_obs_level=sd["pt_level"][Pc], pt_obs_type=sd["pt_type"][Pc],
                   pt_obs_grad=sd["pt_grad"][Pc])
    if c_seg:
        rec.update(seg_spos=xyz[:c_seg], seg_epos=xyz[nsg:nsg + c_seg], seg_obs_kf=sd["seg_ref_kf"][Sc], seg_obs_spx=sd["seg_spx"][Sc], seg_obs_epx=sd["seg_epx"][Sc],
                   seg_obs_sf=sd["seg_sf"][Sc], seg_obs_ef=sd["seg_ef"][Sc], seg_obs_level=sd["seg_level"][Sc])
    return rows, (rec or None)


def stage(ctx, maps, seeds, steps, c_pt, c_seg, with_seeds=True):
    ctx.candidates_reserve(extra_pt_obs=steps * c_pt, extra_seg_obs=steps * c_seg)
    ctx.candidates_reserve_landmarks(extra_pt=steps * c_pt, extra_seg=steps * c_seg)
    ctx.candidates_stage(maps, B.CAM, 30, 40, 8, 3, 10)
    if with_seeds:
        ctx.seeds_reserve()
        ctx.seeds_stage(seeds, B.CAM, max_n_kfs=1 << 30)


def handover_leg(P, ctx, pool, seed_pool, n, reps, c_pt, c_seg, rng):
    abi = P.abi
    maps = [pool[i % len(pool)][0] for i in range(n)]
    seeds = [seed_pool[i % len(seed_pool)] for i in range(n)]
    steps = reps + 1
    assert steps * c_pt <= N_SP and steps * c_seg <= N_SS
    xyz = rng.uniform(-3.0, 3.0, (2 * N_SP, 3)) + [0.0, 0.0, 6.0]
    per_step = [[rows_and_records(sd, k * c_pt, k * c_seg, c_pt, c_seg, xyz) for sd in seed_pool] for k in range(steps)]
    # (a) resident
    stage(ctx, maps, seeds, steps, c_pt, c_seg)
    ctx.set_profiling(True)
    launch, fetch = [], []
    for k in range(steps):
        rows = [per_step[k][i % len(seed_pool)][0] for i in range(n)]
        ctx.synchronize()
        ctx.reset_profiling()
        ctx.seeds_commit_rows(rows)                   # (diagnostic: its per-stream copies are not part of what is measured)
        outs = (abi.SeedReport * n)()
        t0 = time.perf_counter()
        raw_fetch(P, ctx, n, outs)                    # the C call: the reports' copy, the wait, the mirrors
        t1 = time.perf_counter()
        rep = ctx.seeds_update_fetch()                # (again through the binding, for the dicts and its own mirrors: the report is kept)
        ms, cnt = ctx.kernel_time(abi.K_NEWCAND)
        assert cnt == 1 and all(r["pt"][3] == c_pt and r["seg"][3] == c_seg and not r["no_room"] for r in rep[:len(seed_pool)])
        launch.append(ms); fetch.append(t1 - t0)
    ctx.set_profiling(False)
    # (b) the host path of the same tree: the same records through plsvo_candidates_add
    stage(ctx, maps, seeds, steps, c_pt, c_seg, with_seeds=False)
    call, pack = [], []
    for k in range(steps):
        new = [per_step[k][i % len(seed_pool)][1] for i in range(n)]
        ctx.synchronize()
        t0 = time.perf_counter()
        batch = ctx.candidates_add_records(new)
        t1 = time.perf_counter()
        ctx.candidates_add(batch)
        ctx.synchronize()
        t2 = time.perf_counter()
        call.append(t2 - t1); pack.append(t1 - t0)
    return {"converged_per_stream": {"points": c_pt, "segments": c_seg}, "steps": steps, "commit_launch_ms": BI.stats(launch[1:]),
            "update_fetch_call_ms": BI.stats(fetch[1:], 1e3, 3), "resident_launch_plus_fetch_ms": BI.stats([a + 1e3 * b for a, b in zip(launch[1:], fetch[1:])], 1.0, 3),
            "host_add_call_and_wait_ms": BI.stats(call[1:], 1e3, 3), "host_binding_pack_ms": BI.stats(pack[1:], 1e3, 2),
            "resident_median_below_host_minimum": bool(np.median([a + 1e3 * b for a, b in zip(launch[1:], fetch[1:])]) < 1e3 * min(call[1:]))}


def update_leg(P, ctx, pool, seed_pool, n, reps, rng):
    abi = P.abi
    maps = [pool[i % len(pool)][0] for i in range(n)]
    seeds = [seed_pool[i % len(seed_pool)] for i in range(n)]
    steps = reps + 1
    frames = [dict(cur_slot=B.N_KF, T_f_w=list(pool[i % len(pool)][1].c.T_f_w)) for i in range(n)]
    stage(ctx, maps, seeds, steps, N_SP, N_SS)
    res_t, hist = [], None
    farr, outs = frames_array(P, frames), (abi.SeedReport * n)()
    for k in range(steps):
        ctx.synchronize()
        t0 = time.perf_counter()
        rc = ctx.L.plsvo_seeds_update(ctx.h, n, farr)   # the two C calls (the binding's packing of frames and reports is not part of them)
        raw_fetch(P, ctx, n, outs)
        res_t.append(time.perf_counter() - t0)
        assert rc == 0, rc
        rep = ctx.seeds_update_fetch()
        if k == 0:
            hist = {"pt": np.sum([r["pt"] for r in rep], 0).tolist(), "seg": np.sum([r["seg"] for r in rep], 0).tolist()}
    # the host path: one plsvo_update_seeds for the whole batch (frame table: every stream's keyframes, then its new frame), the lists kept by the caller
    stage(ctx, maps, seeds, steps, N_SP, N_SS, with_seeds=False)
    nf = B.N_KF + 1
    frame_T = np.concatenate([np.concatenate([np.asarray(maps[i].t["kf_T"]).reshape(-1, 7), np.asarray(frames[i]["T_f_w"])[None]]) for i in range(n)])
    frame_slot = np.tile(np.arange(nf, dtype=np.int32), n)
    cat = lambda f: np.concatenate([s[f] for s in seeds])
    base_p, base_s = np.repeat(np.arange(n) * nf, N_SP), np.repeat(np.arange(n) * nf, N_SS)
    pt = dict(ref_frame=base_p + cat("pt_ref_kf"), cur_frame=base_p + B.N_KF, px=cat("pt_px"), f=cat("pt_f"), level=cat("pt_level"), type=cat("pt_type"), grad=cat("pt_grad"),
              **{k: cat("pt_" + k) for k in ("a", "b", "mu", "z_range", "sigma2")})
    seg = dict(ref_frame=base_s + cat("seg_ref_kf"), cur_frame=base_s + B.N_KF, px=cat("seg_px"), f=cat("seg_f"), sf=cat("seg_sf"), ef=cat("seg_ef"), level=cat("seg_level"),
               **{k: cat("seg_" + k) for k in ("a", "b", "mu_s", "mu_e", "z_range_s", "z_range_e", "sigma2_s", "sigma2_e")})
    job = abi.SeedsJob(B.CAM, frame_T, frame_slot, pt, seg)
    host_t, add_t = [], []
    import ctypes as C
    out, bufs = job.make_out()
    for k in range(steps):
        ctx.synchronize()
        t0 = time.perf_counter()
        rc = ctx.L.plsvo_update_seeds(ctx.h, C.byref(job.c), C.byref(out))   # the C call into prepared buffers: upload, launch, download
        t1 = time.perf_counter()
        host_t.append(t1 - t0)
        assert rc == 0, rc
        r = job.trim(bufs)
        if k == 0:                                    # what converged is added once (later steps of the unchanged job would add it again)
            cp, cs = (r["pt_status"] == 3).reshape(n, N_SP), (r["seg_status"] == 3).reshape(n, N_SS)
            new = []
            for i in range(n):
                jp, js = np.nonzero(cp[i])[0], np.nonzero(cs[i])[0]
                d, sd = {}, seeds[i]
                if len(jp):
                    d.update(pt_pos=r["pt_xyz_world"].reshape(n, N_SP, 3)[i][jp], pt_obs_kf=sd["pt_ref_kf"][jp], pt_obs_px=sd["pt_px"][jp], pt_obs_f=sd["pt_f"][jp],
                             pt_obs_level=sd["pt_level"][jp], pt_obs_type=sd["pt_type"][jp], pt_obs_grad=sd["pt_grad"][jp])
                if len(js):
                    d.update(seg_spos=r["seg_xyz_world_s"].reshape(n, N_SS, 3)[i][js], seg_epos=r["seg_xyz_world_e"].reshape(n, N_SS, 3)[i][js], seg_obs_kf=sd["seg_ref_kf"][js],
                             seg_obs_spx=sd["seg_spx"][js], seg_obs_epx=sd["seg_epx"][js], seg_obs_sf=sd["seg_sf"][js], seg_obs_ef=sd["seg_ef"][js], seg_obs_level=sd["seg_level"][js])
                new.append(d or None)
            batch = ctx.candidates_add_records(new)
            t2 = time.perf_counter()
            ctx.candidates_add(batch)
            ctx.synchronize()
            add_t = [time.perf_counter() - t2]
    return {"seeds_per_stream": {"points": N_SP, "segments": N_SS}, "steps": steps, "first_step_status_counts": hist,
            "resident_update_and_fetch_ms": BI.stats(res_t[1:], 1e3, 3), "host_update_seeds_call_ms": BI.stats(host_t[1:], 1e3, 3), "host_add_call_and_wait_ms_once": round(1e3 * add_t[0], 3),
            "note": "the resident lists shrink as seeds leave them; the host job is the staged lists at every step (its lists are the caller's, whose handling is not timed)",
            "resident_median_below_host_minimum": bool(np.median(res_t[1:]) < min(host_t[1:]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--loads", default="3,0;7,3;25,10", help='"points,segments" converged per stream and step; several loads separated by ;')
    ap.add_argument("--frame-step-ms", type=float, default=None, help="resident frame step per 4096 streams, same session's bench.py --full")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_seedlist.py: no GPU (a timing needs the MI355X)")
    P = importlib.import_module("pl-svo_amd")
    res = {"what": f"tools/bench_seedlist.py: the resident seed lists' hand-over and update step beside the host path of the same tree, on the workload of tools/bench_newcand.py "
                   f"({B.N_KF} keyframes of {B.F_PT} + {B.F_SEG} features, {B.N_PT} + {B.N_SEG} landmarks), {N_SP} + {N_SS} seeds per stream",
           "device": torch.cuda.get_device_name(0), "gcn_arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", ""), "reps": args.reps,
           "streams": args.streams, "handover": [], "update_step": None}
    rng = np.random.default_rng(2026)
    pool = [BI.make_stream(P, rng) for _ in range(64)]
    seed_pool = [make_seeds(rng) for _ in range(64)]
    ctx = P.capi.Context(0)
    try:
        ctx.config_pyramids(B.N_KF + 1, B.CAM[4], B.CAM[5], 3)
        for slot in range(B.N_KF + 1):
            ctx.build_pyramid(slot, B._texture(rng), 0)
        for load in [s for s in args.loads.split(";") if s]:
            c_pt, c_seg = [int(v) for v in load.split(",")]
            res["handover"].append(handover_leg(P, ctx, pool, seed_pool, args.streams, args.reps, c_pt, c_seg, rng))
        res["update_step"] = update_leg(P, ctx, pool, seed_pool, args.streams, args.reps, rng)
    finally:
        ctx.close()
    if args.frame_step_ms is not None:
        res["frame_step_ms_per_4096_streams"] = args.frame_step_ms
        if args.streams == 4096:
            for v in res["handover"]:
                v["resident_over_frame_step"] = {k: round(x / args.frame_step_ms, 4) for k, x in v["resident_launch_plus_fetch_ms"].items()}
            res["update_step"]["resident_over_frame_step"] = {k: round(x / args.frame_step_ms, 4) for k, x in res["update_step"]["resident_update_and_fetch_ms"].items()}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
