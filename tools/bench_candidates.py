"""Cost of the map-candidate stage (plsvo_candidates_stage / run / fetch and the resident match).  Needs an MI355X; prints one JSON
object and writes it to --out.

  4096 and 32768 streams; per stream a table of 12 keyframes of 200 point + 80 segment features, 10 of them in the overlap list,
  400 point and 150 segment landmarks with observation lists of 1 to 7 entries (mean 4), 8 + 4 map candidates; 320 x 240 images.
  The 64 distinct streams of a batch repeat; the device does not know.  Per shape: the staging call (tables packed and sent once), the
  run call with the wait for it, and the fetch on the host clock (median, min, max of --reps); the launch alone -- the re-arm of the
  first-visit words and the kernel -- by a hipEvent pair on the stream (PLSVO_K_CANDIDATES), and the resident match launch
  (PLSVO_K_MATCH), means of the same calls.  With --frame-step-ms (the resident frame step's time per 4096 streams from the same
  session's bench.py --full) the shares of it are added.

usage: python tools/bench_candidates.py [--reps 7] [--streams 4096,32768] [--frame-step-ms X] [--out profiles/candidates_bench.json]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_KF, N_OV, F_PT, F_SEG, N_PT, N_SEG, N_PT_CAND, N_SEG_CAND, MAX_OBS = 12, 10, 200, 80, 400, 150, 8, 4, 7
CAM = (256.0, 256.0, 160.0, 120.0, 320, 240)


def _rot(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _observe(T, pos):
    """pixels and unit bearings of world positions [n, 3] in the frame with pose T"""
    c = pos @ _rot(T[:4]).T + T[4:]
    px = np.stack([CAM[0] * c[:, 0] / c[:, 2] + CAM[2], CAM[1] * c[:, 1] / c[:, 2] + CAM[3]], 1)
    return px, c / np.linalg.norm(c, axis=1, keepdims=True)


def make_stream(P, rng):
    sy, abi = P.synth, P.abi
    pose = lambda r, t: np.asarray(sy.se3_exp(np.concatenate([rng.uniform(-t, t, 3), rng.uniform(-r, r, 3)])), float)
    kf_T = np.array([pose(0.12, 0.3) for _ in range(N_KF)])
    T = pose(0.08, 0.2)

    def world(n):                                    # in and a little around the view of a camera at the origin
        z = rng.uniform(2.0, 7.0, n)
        return np.stack([(rng.uniform(-40, 360, n) - CAM[2]) / CAM[0] * z, (rng.uniform(-30, 270, n) - CAM[3]) / CAM[1] * z, z], 1)

    def obs_lists(n):
        cnt = rng.integers(1, MAX_OBS + 1, n)
        off = np.zeros(n + 1, np.int32)
        off[1:] = np.cumsum(cnt)
        return off, np.repeat(np.arange(n), cnt), rng.integers(0, N_KF, off[-1]).astype(np.int32)

    pt_pos, s_pos = world(N_PT), world(N_SEG)
    e_pos = s_pos + rng.uniform(-0.5, 0.5, (N_SEG, 3)) * [1, 1, 0.4]
    po_off, po_lm, po_kf = obs_lists(N_PT)
    so_off, so_lm, so_kf = obs_lists(N_SEG)
    po_px, po_f = np.zeros((len(po_kf), 2)), np.zeros((len(po_kf), 3))
    so = {k: np.zeros((len(so_kf), 2 if "px" in k else 3)) for k in ("spx", "epx", "sf", "ef")}
    for k in range(N_KF):
        m = po_kf == k
        po_px[m], po_f[m] = _observe(kf_T[k], pt_pos[po_lm[m]])
        m = so_kf == k
        so["spx"][m], so["sf"][m] = _observe(kf_T[k], s_pos[so_lm[m]])
        so["epx"][m], so["ef"][m] = _observe(kf_T[k], e_pos[so_lm[m]])
    types = lambda n: rng.choice(4, n, p=[0.05, 0.25, 0.3, 0.4]).astype(np.int32)
    lists = lambda per, n: np.where(rng.random(N_KF * per) < 0.1, -1, rng.integers(0, n, N_KF * per)).astype(np.int32)
    ang = rng.uniform(0, 6.28, len(po_kf))
    job = abi.CandidateMapJob(
        kf_T=kf_T, kf_slot=np.arange(N_KF), kf_pt_off=np.arange(N_KF + 1) * F_PT, kf_pt_lm=lists(F_PT, N_PT), kf_seg_off=np.arange(N_KF + 1) * F_SEG,
        kf_seg_lm=lists(F_SEG, N_SEG), pt_pos=pt_pos, pt_type=types(N_PT), pt_obs_off=po_off, pt_obs_kf=po_kf, pt_obs_px=po_px, pt_obs_f=po_f,
        pt_obs_level=rng.integers(0, 3, len(po_kf)), pt_obs_type=(rng.random(len(po_kf)) < 0.2), pt_obs_grad=np.stack([np.cos(ang), np.sin(ang)], 1),
        seg_spos=s_pos, seg_epos=e_pos, seg_type=types(N_SEG), seg_obs_off=so_off, seg_obs_kf=so_kf, seg_obs_spx=so["spx"], seg_obs_epx=so["epx"],
        seg_obs_sf=so["sf"], seg_obs_ef=so["ef"], seg_obs_level=rng.integers(0, 3, len(so_kf)),
        pt_cand=rng.integers(0, N_PT, N_PT_CAND), seg_cand=rng.integers(0, N_SEG, N_SEG_CAND))
    return job, abi.CandidateFrameJob(T, rng.permutation(N_KF)[:N_OV], cur_slot=N_KF)


def _texture(rng, w=CAM[4], h=CAM[5]):
    img = np.kron(rng.integers(0, 256, (h // 8 + 2, w // 8 + 2)).astype(np.float64), np.ones((8, 8)))
    k = np.ones(7) / 7.0
    img = np.apply_along_axis(lambda r: np.convolve(r, k, mode="same"), 1, img)
    img = np.apply_along_axis(lambda c: np.convolve(c, k, mode="same"), 0, img)
    return np.clip(img[4:h + 4, 4:w + 4], 0, 255).astype(np.uint8)


def _stats(ts, n):
    t = float(np.median(ts))
    return {"ms_median": round(1e3 * t, 3), "ms_min": round(1e3 * min(ts), 3), "ms_max": round(1e3 * max(ts), 3), "streams_per_s": round(n / t, 1)}


def leg(P, ctx, pool, n, reps):
    abi = P.abi
    maps, frames = [pool[i % len(pool)][0] for i in range(n)], [pool[i % len(pool)][1] for i in range(n)]
    t_stage, t_run, t_fetch, t_match = [], [], [], []
    for _ in range(min(reps, 3)):                    # the tables travel at keyframes only: three calls are enough to see the spread
        t0 = time.perf_counter()
        ctx.candidates_stage(maps, CAM, 30, 40, 8, 3, 10)
        ctx.synchronize()
        t_stage.append(time.perf_counter() - t0)
    ctx.candidates_run(frames)
    res = ctx.candidates_fetch()
    ctx.candidates_match()
    ctx.synchronize()
    ctx.set_profiling(True)
    ctx.reset_profiling()
    for _ in range(reps):
        t0 = time.perf_counter()
        ctx.candidates_run(frames)
        ctx.synchronize()
        t_run.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        ctx.candidates_match()
        ctx.synchronize()
        t_match.append(time.perf_counter() - t0)
    k_ms, k_n = ctx.kernel_time(abi.K_CANDIDATES)
    m_ms, m_n = ctx.kernel_time(abi.K_MATCH)
    ctx.set_profiling(False)
    for _ in range(min(reps, 3)):
        t0 = time.perf_counter()
        ctx.candidates_fetch()
        t_fetch.append(time.perf_counter() - t0)
    return {"stage": _stats(t_stage, n), "run_and_wait": _stats(t_run, n), "match_and_wait": _stats(t_match, n), "fetch": _stats(t_fetch, n),
            "launch_ms": round(k_ms / max(k_n, 1), 4), "match_launch_ms": round(m_ms / max(m_n, 1), 4),
            "mean_filed_pt": float(np.mean([r["n_filed_pt"] for r in res[:len(pool)]])), "mean_filed_seg": float(np.mean([r["n_filed_seg"] for r in res[:len(pool)]])),
            "mean_active_pt": float(np.mean([r["pt_active"].sum() for r in res[:len(pool)]]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--streams", default="4096,32768")
    ap.add_argument("--frame-step-ms", type=float, default=None, help="resident frame step per 4096 streams, same session's bench.py --full")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_candidates.py: no GPU (a timing needs the MI355X)")
    P = importlib.import_module("pl-svo_amd")
    res = {"what": f"tools/bench_candidates.py: plsvo_candidates_stage / run / fetch / match ({N_KF} keyframes of {F_PT} + {F_SEG} features, {N_OV} in the "
                   f"overlap list, {N_PT} + {N_SEG} landmarks, observation lists of 1..{MAX_OBS})",
           "device": torch.cuda.get_device_name(0), "reps": args.reps, "batched": {}}
    rng = np.random.default_rng(2024)
    pool = [make_stream(P, rng) for _ in range(64)]
    ctx = P.capi.Context(0)
    try:
        ctx.config_pyramids(N_KF + 1, CAM[4], CAM[5], 3)
        for s in range(N_KF + 1):
            ctx.build_pyramid(s, _texture(rng))
        for n in [int(s) for s in args.streams.split(",") if s]:
            res["batched"][str(n)] = leg(P, ctx, pool, n, args.reps)
    finally:
        ctx.close()
    if args.frame_step_ms is not None:
        res["frame_step_ms_per_4096_streams"] = args.frame_step_ms
        v = res["batched"].get("4096")
        if v:
            v["launch_over_frame_step"] = round(v["launch_ms"] / args.frame_step_ms, 4)
            v["launch_and_match_over_frame_step"] = round((v["launch_ms"] + v["match_launch_ms"]) / args.frame_step_ms, 4)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
