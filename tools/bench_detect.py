"""Cost of FAST corner detection per grid cell on resident pyramid slots (plsvo_hip_detect_fast_dev) against the pyramid build of the
same batch (plsvo_hip_build_pyramids_dev), the bandwidth yardstick.  Needs an MI355X; prints one JSON object and writes it to --out.

  640x480 slots, 3 levels, cell 25, FAST threshold 20, detection threshold 20; 4096 and 32768 slots; the detector with an all-zero and
  with a half-set occupancy; the two detector legs and the pyramid build alternate in one process.  Per leg: time per call (host clock
  around a device synchronise; median, min and max of --reps calls), the bytes the call must read, n * sum_L W_L * H_L, over the time,
  and that over the 8 TB/s HBM peak.  A call is the detector launch plus the compaction launch.

usage: python tools/bench_detect.py [--reps 7] [--slots 4096,32768] [--image scene|noise] [--out profiles/detect_bench.json]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12
W, H, NLEV, CELL = 640, 480, 3, 25


def scene_batch(torch, n, kind):
    """n level-0 frames on the device: `noise` = independent uniform bytes (every pixel passes the early reject: the detector's worst
    case), `scene` = 64 synthetic frames of the alignment benchmark's textured plane (pl-svo_amd/synth.py), each shifted by a few pixels
    per slot so that no two slots hold the same bytes"""
    g = torch.Generator(device="cuda").manual_seed(5)
    if kind == "noise":
        return torch.randint(0, 256, (n, H, W), dtype=torch.uint8, device="cuda", generator=g)
    P = importlib.import_module("pl-svo_amd")
    streams = [P.synth.make_align_stream(s, W, H, 20, 4, 3) for s in range(64)]
    base = P.synth.render_streams(streams)[:, 0].contiguous().cuda()                  # [64, H, W] uint8
    out = torch.empty((n, H, W), dtype=torch.uint8, device="cuda")
    for i0 in range(0, n, 64):
        m = min(64, n - i0)
        out[i0:i0 + m] = torch.roll(base[:m], shifts=((i0 // 64) % 17, (i0 // 64) % 23), dims=(1, 2))
    return out


def leg(P, torch, n, reps, kind):
    ctx = P.capi.Context(0)
    try:
        ctx.config_pyramids(n, W, H, NLEV)
        raw = scene_batch(torch, n, kind)
        cols, rows = P.capi.detect_grid(W, H, CELL)
        cells = cols * rows
        corners = torch.zeros(n * cells * 16, dtype=torch.uint8, device="cuda")
        counts = torch.zeros(n, dtype=torch.int32, device="cuda")
        occ_half = torch.zeros((n, cells), dtype=torch.uint8, device="cuda")
        occ_half[:, ::2] = 1
        occ_zero = torch.zeros((n, cells), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        calls = {"build_pyramids_dev": lambda: ctx.build_pyramids_dev(0, n, raw.data_ptr(), W, W * H, 0),
                 "detect_fast_dev_occupancy_zero": lambda: ctx.detect_fast_dev(0, n, corners.data_ptr(), counts.data_ptr(), CELL, NLEV, 20, 20.0, occ_zero.data_ptr()),
                 "detect_fast_dev_occupancy_half": lambda: ctx.detect_fast_dev(0, n, corners.data_ptr(), counts.data_ptr(), CELL, NLEV, 20, 20.0, occ_half.data_ptr())}
        times = {k: [] for k in calls}
        found = {}
        for k, f in calls.items():   # warm-up (the first one fills the slots)
            f()
            ctx.synchronize()
            if k != "build_pyramids_dev":
                found[k] = float(counts.float().mean().item())
        for _ in range(reps):
            for k, f in calls.items():
                t0 = time.perf_counter()
                f()
                ctx.synchronize()
                times[k].append(time.perf_counter() - t0)
        read = n * sum((W >> l) * (H >> l) for l in range(NLEV))
        out = {}
        for k in calls:
            t = float(np.median(times[k]))
            out[k] = {"ms_median": round(1e3 * t, 3), "ms_min": round(1e3 * min(times[k]), 3), "ms_max": round(1e3 * max(times[k]), 3),
                      "slots_per_s": round(n / t, 1)}
            if k != "build_pyramids_dev":
                out[k].update(bytes_read=read, TBps=round(read / t / 1e12, 3), fraction_of_8TBps=round(read / t / HBM_PEAK, 4),
                              features_per_slot=round(found[k], 2),
                              over_build_pyramids_dev=round(t / float(np.median(times["build_pyramids_dev"])), 3))
        return out
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--slots", default="4096,32768")
    ap.add_argument("--image", default="scene", choices=["scene", "noise"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_detect.py: no GPU (a timing needs the MI355X)")
    P = importlib.import_module("pl-svo_amd")
    res = {"what": f"tools/bench_detect.py: detect_fast_dev vs build_pyramids_dev ({W}x{H}, {NLEV} levels, cell {CELL}, image {args.image}); "
                   "bytes_read = n * sum_L W_L * H_L", "device": torch.cuda.get_device_name(0), "reps": args.reps, "batched": {}}
    for n in [int(s) for s in args.slots.split(",") if s]:
        res["batched"][str(n)] = leg(P, torch, n, args.reps, args.image)
        torch.cuda.empty_cache()
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
