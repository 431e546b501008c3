"""Cost of rectifying raw distorted frames on the device (plsvo_hip_rectify_build_pyramids_dev) against the pyramid build of frames that
arrive already rectified (plsvo_hip_build_pyramids_dev).  Needs an MI355X; prints one JSON object and writes it to --out.

  (a) batched build, 640x480, 4-image pyramid, 4096 and 32768 slots: time per call (host clock around a device synchronise, median of
      --reps calls, the two builders alternating), bytes the call must move / time, and that over the 8 TB/s HBM peak
  (b) bench.py's host-fed leg (pinned host frames -> PCIe -> pyramid -> align_run + poseopt_run, double-buffered) run as it is and with
      every pyramid build replaced by the rectifying one: does rectification stay hidden behind the PCIe bound?

usage: python tools/bench_rectify.py [--reps 7] [--slots 4096,32768] [--out profiles/rectify_bench.json]"""
import argparse
import importlib
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12
# EuRoC cam0's distortion (ASL MH_01_easy, the dataset app/run_pipeline.cpp names) on a 640x480 frame
CAM = dict(width=640, height=480, fx=458.654 * 640 / 752, fy=457.296, cx=367.215 * 640 / 752, cy=248.375,
           d=[-0.28340811, 0.07395907, 1.9359e-4, 1.76187114e-5])


def pyramid_bytes(W, H, nlev):
    """bytes one slot's half-sampler and tile launches must read + write after level 0 is in place (each level read once by the next
    level's half-sampler and once by its tile launch; every level written once row-major and once tiled)"""
    sizes = [(W >> l) * (H >> l) for l in range(nlev)]
    tiled = [((W >> l) + 15) // 16 * 16 * (((H >> l) + 7) // 8 * 8) for l in range(nlev)]
    return sum(sizes[:-1]) + sum(sizes[1:]) + sum(sizes) + sum(tiled)


def batched_leg(P, torch, n, reps, nlev=4):
    W, H = CAM["width"], CAM["height"]
    ctx = P.capi.Context(0)
    try:
        ctx.config_pyramids(n, W, H, nlev)
        mid = ctx.config_rectify(P.abi.pinhole_radtan(W, H, CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"], CAM["d"]))
        g = torch.Generator(device="cuda").manual_seed(5)
        raw = torch.randint(0, 256, (n, H, W), dtype=torch.uint8, device="cuda", generator=g)
        torch.cuda.synchronize()
        calls = {"build_pyramids_dev": lambda: ctx.build_pyramids_dev(0, n, raw.data_ptr(), W, W * H, 0),
                 "rectify_build_pyramids_dev": lambda: ctx.rectify_build_pyramids_dev(mid, 0, n, raw.data_ptr(), W, W * H, 0)}
        times = {k: [] for k in calls}
        for k, f in calls.items():   # warm-up
            f()
        ctx.synchronize()
        for _ in range(reps):
            for k, f in calls.items():
                t0 = time.perf_counter()
                f()
                ctx.synchronize()
                times[k].append(time.perf_counter() - t0)
        pyr = pyramid_bytes(W, H, nlev)
        # level 0: the copy reads and writes every pixel once; the remap reads every raw pixel once (its 2x2 gathers re-read them from
        # cache) and writes it once -- its map (4 B per pixel, shared by every slot) is counted once per call
        moved = {"build_pyramids_dev": n * (2 * W * H + pyr), "rectify_build_pyramids_dev": n * (2 * W * H + pyr) + 4 * W * H}
        out = {}
        for k in calls:
            t = float(np.median(times[k]))
            out[k] = {"ms_median": round(1e3 * t, 3), "ms_min": round(1e3 * min(times[k]), 3), "ms_max": round(1e3 * max(times[k]), 3),
                      "bytes": moved[k], "TBps": round(moved[k] / t / 1e12, 3), "fraction_of_8TBps": round(moved[k] / t / HBM_PEAK, 3),
                      "frames_per_s": round(n / t, 1)}
        out["rectify_over_plain"] = round(out["rectify_build_pyramids_dev"]["ms_median"] / out["build_pyramids_dev"]["ms_median"], 3)
        del raw
        return out
    finally:
        ctx.close()


def host_fed(P, torch, bench, reps, n_streams):
    """bench.host_fed_leg unchanged; its Context is swapped for one whose build_pyramids_dev rectifies (the map configured with the
    pyramids), so the timed loop, the copies and the launches are the same line for line"""
    base = P.capi.Context

    class Rectifying(base):
        def config_pyramids(self, n_slots, width, height, n_levels):
            super().config_pyramids(n_slots, width, height, n_levels)
            self._mid = self.config_rectify(P.abi.pinhole_radtan(width, height, CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"], CAM["d"]))

        def build_pyramids_dev(self, first_slot, n, d_ptr, stride_bytes, image_pitch_bytes, rounding=0):
            self.rectify_build_pyramids_dev(self._mid, first_slot, n, d_ptr, stride_bytes, image_pitch_bytes, rounding)

    capi_r = types.SimpleNamespace(**{k: getattr(P.capi, k) for k in dir(P.capi) if not k.startswith("__")})
    capi_r.Context = Rectifying
    P_r = types.SimpleNamespace(capi=capi_r, synth=P.synth, align_job_from_stream=P.align_job_from_stream,
                                poseopt_job_from_frame=P.poseopt_job_from_frame)
    cfg = bench.CONFIGS[2]
    streams = [P.synth.make_align_stream(s, cfg["W"], cfg["H"], cfg["pts"], cfg["seg"], max_level=cfg["maxl"]) for s in range(n_streams)]
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    runs = {"plain": [], "rectifying": []}
    for _ in range(reps):
        for k, PP in (("plain", P), ("rectifying", P_r)):
            with torch.cuda.stream(stream):
                runs[k].append(bench.host_fed_leg(PP, torch, dev, stream, streams, cfg, n_streams=n_streams))
    out = {}
    for k, rs in runs.items():
        fps = [r["frames_per_s"] for r in rs]
        out[k] = {"frames_per_s_median": float(np.median(fps)), "frames_per_s_runs": fps, "h2d_GBps_median": float(np.median([r["h2d_GBps"] for r in rs])),
                  "ms_per_step_median": float(np.median([r["ms_per_step"] for r in rs]))}
    out["rectifying_over_plain"] = round(out["rectifying"]["frames_per_s_median"] / out["plain"]["frames_per_s_median"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--slots", default="4096,32768")
    ap.add_argument("--host-fed-reps", type=int, default=3)
    ap.add_argument("--host-fed-streams", type=int, default=1024)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_rectify.py: no GPU (a timing needs the MI355X)")
    P = importlib.import_module("pl-svo_amd")
    bench = importlib.import_module("bench")
    res = {"what": "tools/bench_rectify.py: rectify_build_pyramids_dev vs build_pyramids_dev (640x480, 4 levels, EuRoC cam0 distortion "
                   "scaled to 640 wide), and bench.py's host-fed leg with raw frames",
           "device": torch.cuda.get_device_name(0), "batched": {}}
    for n in [int(s) for s in args.slots.split(",") if s]:
        res["batched"][str(n)] = batched_leg(P, torch, n, args.reps)
        torch.cuda.empty_cache()
    if args.host_fed_reps > 0:
        res["host_fed"] = host_fed(P, torch, bench, args.host_fed_reps, args.host_fed_streams)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
