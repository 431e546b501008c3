"""Cost of the keyframe stage (plsvo_close_keyframes, plsvo_keyframe_decide) per call.  Needs an MI355X; prints one JSON object and
writes it to --out.

  4096 and 32768 streams of 200 points + 80 segments with a table of 10 and of 64 keyframes (every keyframe in the overlap list of the
  decide call).  A call is what the C ABI does for host arrays: pack, one copy to the device, one launch, one copy back; the host clock
  runs around the whole call (median, min and max of --reps calls); kernel_ms is the launch alone, a hipEvent pair on the stream around it
  (PLSVO_K_KEYFRAME, mean of the same calls).  The 64 distinct streams of a batch repeat; the device does not know.
  With --frame-step-ms (the resident frame step's time per 4096 streams from the same run of bench.py --full) the share of it is added.

usage: python tools/bench_keyframe.py [--reps 7] [--streams 4096,32768] [--keyframes 10,64] [--frame-step-ms X] [--out profiles/keyframe_bench.json]"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_PT, N_SEG = 200, 80
CAM = (315.5, 315.5, 376.0, 240.0, 752, 480)


def make_stream(P, rng, n_kf):
    """one stream: a frame of N_PT + N_SEG landmarks in view, n_kf keyframes around it (all overlapping), the job pair"""
    sy, abi = P.synth, P.abi
    T = sy.se3_exp(np.concatenate([rng.uniform(-0.5, 0.5, 3), rng.uniform(-0.3, 0.3, 3)]))
    Ti = sy.se3_inv(T)

    def in_view(n):
        px = np.stack([rng.uniform(0, CAM[4], n), rng.uniform(0, CAM[5], n)], 1)
        z = rng.uniform(1.0, 6.0, n)
        f = np.stack([(px[:, 0] - CAM[2]) / CAM[0] * z, (px[:, 1] - CAM[3]) / CAM[1] * z, z], 1)
        return np.array([sy.se3_act(Ti, p) for p in f]).reshape(-1, 3), px
    pos, px = in_view(N_PT)
    sp, ep = in_view(N_SEG)[0], in_view(N_SEG)[0]
    kf_T = np.array([sy.se3_mul(sy.se3_exp(np.concatenate([rng.uniform(-0.6, 0.6, 3), rng.uniform(-0.2, 0.2, 3)])), T) for _ in range(n_kf)])
    kp = in_view(5 * n_kf)[0].reshape(n_kf, 5, 3)
    T_last = sy.se3_mul(sy.se3_exp(rng.uniform(-0.02, 0.02, 6)), T)
    close = abi.CloseKeyframesJob(CAM, T, kf_T, kp, np.ones((n_kf, 5), np.uint8), max_n_kfs=n_kf)
    decide = abi.KeyframeDecideJob(CAM, T, T_last, px, pos, None, sp, ep, None, kf_T, np.arange(n_kf), (-1,) * 5)
    return close, decide


def leg(P, ctx, n, n_kf, reps):
    abi = P.abi
    rng = np.random.default_rng(100 + n_kf)
    pool = [make_stream(P, rng, n_kf) for _ in range(64)]
    cj, dj = [pool[i % 64][0] for i in range(n)], [pool[i % 64][1] for i in range(n)]
    cin = (abi.CloseKfIn * n)(*[j.c for j in cj])
    cout = (abi.CloseKfOut * n)()
    idx, dist = np.zeros((n, n_kf), np.int32), np.zeros((n, n_kf))
    din = (abi.KfDecideIn * n)(*[j.c for j in dj])
    dout = (abi.KfDecideOut * n)()
    dt, dr = np.zeros((n, n_kf)), np.zeros((n, n_kf))
    for i in range(n):
        cout[i].close_idx, cout[i].close_dist = idx[i].ctypes.data_as(abi.c_i32_p), dist[i].ctypes.data_as(abi.c_double_p)
        dout[i].delta_t, dout[i].delta_r = dt[i].ctypes.data_as(abi.c_double_p), dr[i].ctypes.data_as(abi.c_double_p)
    calls = {"close_keyframes": lambda: ctx._chk(ctx.L.plsvo_close_keyframes(ctx.h, n, cin, cout)),
             "keyframe_decide": lambda: ctx._chk(ctx.L.plsvo_keyframe_decide(ctx.h, n, din, dout))}
    times = {k: [] for k in calls}
    for f in calls.values():
        f()
    kernel_ms = {}
    ctx.set_profiling(True)
    for k, f in calls.items():
        ctx.reset_profiling()
        for _ in range(reps):
            t0 = time.perf_counter()
            f()
            times[k].append(time.perf_counter() - t0)
        ms, launches = ctx.kernel_time(abi.K_KEYFRAME)
        kernel_ms[k] = ms / max(launches, 1)
    ctx.set_profiling(False)
    out = {}
    for k in calls:
        t = float(np.median(times[k]))
        out[k] = {"ms_median": round(1e3 * t, 3), "ms_min": round(1e3 * min(times[k]), 3), "ms_max": round(1e3 * max(times[k]), 3),
                  "streams_per_s": round(n / t, 1), "kernel_ms": round(kernel_ms[k], 4)}
    out["mean_n_close"] = float(np.mean([o.n_close for o in cout]))
    out["need_new_kf_fraction"] = float(np.mean([o.need_new_kf for o in dout]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--streams", default="4096,32768")
    ap.add_argument("--keyframes", default="10,64")
    ap.add_argument("--frame-step-ms", type=float, default=None, help="resident frame step per 4096 streams, same run of bench.py --full")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_keyframe.py: no GPU (a timing needs the MI355X)")
    P = importlib.import_module("pl-svo_amd")
    res = {"what": f"tools/bench_keyframe.py: plsvo_close_keyframes and plsvo_keyframe_decide per call, host arrays in and out "
                   f"({N_PT} points + {N_SEG} segments per stream, every keyframe in the overlap list)",
           "device": torch.cuda.get_device_name(0), "reps": args.reps, "batched": {}}
    ctx = P.capi.Context(0)
    try:
        for n in [int(s) for s in args.streams.split(",") if s]:
            for n_kf in [int(s) for s in args.keyframes.split(",") if s]:
                res["batched"][f"{n}x{n_kf}kf"] = leg(P, ctx, n, n_kf, args.reps)
    finally:
        ctx.close()
    if args.frame_step_ms is not None:
        res["frame_step_ms_per_4096_streams"] = args.frame_step_ms
        for key, v in res["batched"].items():
            if key.startswith("4096x"):
                v["calls_over_frame_step"] = round((v["close_keyframes"]["ms_median"] + v["keyframe_decide"]["ms_median"]) / args.frame_step_ms, 4)
                v["kernels_over_frame_step"] = round((v["close_keyframes"]["kernel_ms"] + v["keyframe_decide"]["kernel_ms"]) / args.frame_step_ms, 4)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
