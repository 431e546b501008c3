"""Cost of the bootstrap's KLT second frame on resident streams (plsvo_klt_second_frame: the KLT pyramid of the current slot, the track of
every corner of the first keyframe, the list commit).  Needs an MI355X; prints one JSON object and writes it to --out.

  640x480 rendered views (the alignment benchmark's textured plane), 3 half-sampled levels for the detector; per stream a reference slot
  and a current slot whose view is the reference rolled by --shift pixels; the corners come from plsvo_hip_detect_fast_dev and never
  leave the device.  Every timed call is preceded by an untimed first frame, so each one tracks the same lists from next = prev.
  Per launch family: GPU time per call from the library's event pairs (PLSVO_K_HALFSAMPLE = the pyramid launches, PLSVO_K_MATCH = the
  track launch, PLSVO_K_NEWCAND = the commit launch), median (min - max) of --reps calls; the whole call by the host clock around a
  synchronise.  Iterations per point come from plsvo_klt_track_points on the lists of --sample streams.  bytes_* are the bytes the
  launches must move by their access pattern (no counter run): pyramid = level reads and writes; track = per point and level the 33 x 33
  source window plus 31 x 31 bytes per iteration; commit = the list entries read and written.

usage: python tools/bench_klt.py [--streams 4096] [--reps 7] [--shift 5,3] [--sample 8] [--out profiles/klt_bench.json]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, NLEV, CELL = 640, 480, 3, 25
DET = dict(cell_size=CELL, n_levels=NLEV, fast_threshold=7, detection_threshold=2.0)   # the synthetic plane is smooth: the sequence harness's thresholds


def scene_batch(torch, P, n):
    streams = [P.synth.make_align_stream(s, W, H, 20, 4, 3) for s in range(64)]
    base = P.synth.render_streams(streams)[:, 0].contiguous().cuda()
    out = torch.empty((n, H, W), dtype=torch.uint8, device="cuda")
    for i0 in range(0, n, 64):
        m = min(64, n - i0)
        out[i0:i0 + m] = torch.roll(base[:m], shifts=((i0 // 64) % 17, (i0 // 64) % 23), dims=(1, 2))
    return out


def stat(v):
    return {"median": round(float(np.median(v)), 3), "min": round(float(min(v)), 3), "max": round(float(max(v)), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shift", default="5,3")
    ap.add_argument("--sample", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_klt.py: no GPU (a timing needs the MI355X)")
    P = importlib.import_module("pl-svo_amd")
    A = P.abi
    n = args.streams
    sx, sy = [int(v) for v in args.shift.split(",")]
    ctx = P.capi.Context(0)
    ctx.config_pyramids(2 * n, W, H, NLEV)
    ref = scene_batch(torch, P, n)
    cur = torch.roll(ref, shifts=(sy, sx), dims=(1, 2)).contiguous()
    ctx.build_pyramids_dev(0, n, ref.data_ptr(), W, W * H, 0)
    ctx.build_pyramids_dev(n, n, cur.data_ptr(), W, W * H, 0)
    cols, rows = P.capi.detect_grid(W, H, CELL)
    cells = cols * rows
    corners = torch.zeros(n * cells * 16, dtype=torch.uint8, device="cuda")
    counts = torch.zeros(n, dtype=torch.int32, device="cuda")
    ctx.detect_fast_dev(0, n, corners.data_ptr(), counts.data_ptr(), **DET)
    ctx.synchronize()
    n_corners = counts.cpu().numpy()
    pin = A.Pinhole(400.0, 400.0, 319.5, 239.5, W, H)
    frames = [dict(slot=i, cam=pin, d_corners=corners.data_ptr() + i * cells * 16, d_count=counts.data_ptr() + 4 * i) for i in range(n)]
    cur_slots = [n + i for i in range(n)]
    ctx.klt_reserve(n, cells)
    sizes = P.capi.klt_levels(W, H)
    ctx.set_profiling(True)
    fam = {"pyramid": A.K_HALFSAMPLE, "track": A.K_MATCH, "commit": A.K_NEWCAND}
    ms = {k: [] for k in fam}
    wall = []
    for rep in range(args.reps + 1):                                       # the first round warms up
        ctx.klt_first_frame(frames)
        ctx.synchronize()
        ctx.reset_profiling()
        t0 = time.perf_counter()
        ctx.klt_second_frame(cur_slots, 40, 1.0)
        ctx.synchronize()
        t1 = time.perf_counter()
        if rep:
            wall.append(1e3 * (t1 - t0))
            for k, f in fam.items():
                ms[k].append(ctx.kernel_time(f)[0])
    reps = ctx.klt_fetch()
    n_after = np.array([r["n_after"] for r in reps])
    results = np.bincount([r["result"] for r in reps], minlength=6).tolist()
    # iterations per point and level on a sample of streams, through the diagnostic entry (the same kernel)
    iters, exits, pts = [], [], 0
    for s in range(min(args.sample, n)):
        ctx.klt_first_frame([frames[i] if i == s else None for i in range(n)])
        px = ctx.klt_fetch_tracks(s)["px_ref"]
        d = ctx.klt_track_points(s, n + s, px, px)
        iters.append(d["iters"][:, :len(sizes)].astype(np.int64))
        exits.append(d["exit"][:, :len(sizes)])
        pts += len(px)
    iters, exits = np.concatenate(iters), np.concatenate(exits)
    it_level = iters.mean(axis=0)
    total_pts = int(n_corners.sum())
    b_pyr = n * (sizes[0][0] * sizes[0][1] + sum(2 * w * h for w, h in sizes[1:-1]) + sizes[-1][0] * sizes[-1][1])
    b_track = int(total_pts * sum(33 * 33 + 31 * 31 * it_level[l] for l in range(len(sizes))))
    b_commit = int(total_pts * (1 + 8 + 8 + 24) + n_after.sum() * (8 + 8 + 24 + 24 + 8 + 8 + 8))
    t_med = {k: float(np.median(v)) for k, v in ms.items()}
    res = {"what": f"tools/bench_klt.py: plsvo_klt_second_frame on {n} streams of {W}x{H}, view shift ({sx}, {sy}) px, KLT levels {sizes}",
           "device": torch.cuda.get_device_name(0), "reps": args.reps, "streams": n,
           "corners_per_stream": {"mean": round(float(n_corners.mean()), 1), "min": int(n_corners.min()), "max": int(n_corners.max())},
           "points_tracked_per_call": total_pts, "kept_per_stream_mean": round(float(n_after.mean()), 1), "results_by_code": results,
           "ms_per_call": {"pyramid": stat(ms["pyramid"]), "track": stat(ms["track"]), "commit": stat(ms["commit"]), "whole_call_host_clock": stat(wall)},
           "us_per_stream": round(1e3 * float(np.median(wall)) / n, 2), "ns_per_point_track": round(1e6 * t_med["track"] / max(total_pts, 1), 1),
           "iterations_per_point": {"sample_points": pts, "per_level_mean": [round(float(v), 2) for v in it_level], "per_level_max": iters.max(axis=0).tolist(),
                                    "all_levels_mean": round(float(iters.sum(axis=1).mean()), 2),
                                    "exits_by_code_level0": np.bincount(exits[:, 0], minlength=7).tolist()},
           "bytes_by_access_pattern": {"pyramid": b_pyr, "track": b_track, "commit": b_commit},
           "GBps_by_access_pattern": {"pyramid": round(b_pyr / t_med["pyramid"] / 1e6, 1), "track": round(b_track / t_med["track"] / 1e6, 1),
                                      "commit": round(b_commit / t_med["commit"] / 1e6, 1)}}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
